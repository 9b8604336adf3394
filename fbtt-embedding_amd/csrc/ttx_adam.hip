// ttx_adam.hip -- one Adam / AdamW step over a short list of dense tensors: the cores of a TT module, or the weight of a dense
// group (include/ttx.h "fused Adam"; not in the reference).  gfx950, wave64.
//
// TT cores have no sparsity a lazy optimizer could use (a training batch touches nearly every slice), so the semantics are
// torch.optim.Adam's: every element steps every time.  The dense core gradients come from the existing TTX_OPTIM_DENSE routes;
// this file only applies them.
//
// Step and bias corrections -- MECHANISM: a one-thread launch in front (adam_step_kernel) reads the step counter, advances it and
// leaves the step's two factors, lr / (1 - beta1^t) and 1 / sqrt(1 - beta2^t) (computed in double), in the workspace; the
// element kernel behind it on the same stream reads the factors only, never the counter.  So no work-group can see a step another
// work-group of the same call has advanced, nothing is read back and nothing allocated: the call is capturable, and a replayed
// graph advances the counter as eager calls do.  Two launches per call.
//
// Element kernel: memory-bound, 16 bytes read and 12 written per element.  The call's tensors are cut into chunks of
// kAdamT * kAdamVec elements, numbered through all tensors; a work-group walks the chunks blockIdx.x, + gridDim.x, ... (grid
// capped at kAdamGridCap).  A full chunk of a tensor whose four pointers are 16-byte aligned moves as one float4 per thread and
// array; a tensor's last, partial chunk and every chunk of a misaligned tensor move as scalars, consecutive threads on consecutive
// elements.  Pointers, sizes and first chunks are HOST values that travel by value in the kernel arguments and are staged in LDS
// through constant subscripts (ttx_dense.hip DenseTabs: a run-time subscript into a by-value argument goes through scratch).
#include <math.h>

#include "ttx_internal.h"

namespace ttx {

constexpr int kAdamT = 256;          // threads per work-group
constexpr int kAdamVec = 4;          // floats per thread and chunk
constexpr int kAdamGridCap = 2048;   // work-groups per launch; the chunks beyond are walked grid-stride
constexpr int kAdamChunk = kAdamT * kAdamVec;
static_assert(TTX_ADAM_MAX_TENSORS <= kAdamT, "one thread stages one tensor");
static_assert(TTX_ADAM_MAX_TENSORS <= 32, "the aligned tensors are a 32-bit mask");

struct AdamTabs {
  float* w[TTX_ADAM_MAX_TENSORS];
  const float* g[TTX_ADAM_MAX_TENSORS];
  float* m[TTX_ADAM_MAX_TENSORS];
  float* v[TTX_ADAM_MAX_TENSORS];
  long long n[TTX_ADAM_MAX_TENSORS];      // elements; entries beyond ntensors are 0
  long long first[TTX_ADAM_MAX_TENSORS];  // the tensor's first chunk; entries beyond ntensors hold the total
};

// base^e for e >= 0 by squaring, in double
__device__ __forceinline__ double adam_ipow(double base, long long e) {
  double r = 1.0;
  while (e > 0) {
    if (e & 1) r *= base;
    base *= base;
    e >>= 1;
  }
  return r;
}

// t = *step + 1; factors[0] = lr / (1 - beta1^t), factors[1] = 1 / sqrt(1 - beta2^t); *step = t.  One thread.
__global__ void adam_step_kernel(int64_t* __restrict__ step, float* __restrict__ factors, float lr, float b1, float b2) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  long long t = (long long)*step + 1;
  t = t < 1 ? 1 : t;
  const double bc1 = 1.0 - adam_ipow((double)b1, t), bc2 = 1.0 - adam_ipow((double)b2, t);
  factors[0] = (float)((double)lr / bc1);
  factors[1] = (float)(1.0 / sqrt(bc2));
  *step = t;
}

// WD 0: no weight decay; 1: coupled (g += wd w); 2: decoupled (w *= 1 - lr wd first: AdamW).  a = lr / bc1, c = 1 / sqrt(bc2).
template <int WD>
__device__ __forceinline__ void adam_one(float& w, float g, float& m, float& v, float a, float c, float b1, float omb1, float b2,
                                         float omb2, float eps, float wd, float shrink) {
  if constexpr (WD == 2) w = w * shrink;
  if constexpr (WD == 1) g = fmaf(wd, w, g);
  m = fmaf(b1, m, omb1 * g);
  v = fmaf(b2, v, omb2 * g * g);
  w = w - a * m / (sqrtf(v) * c + eps);
}

template <int WD>
__global__ __launch_bounds__(kAdamT) void adam_apply_kernel(int nt, long long chunks, unsigned vecmask,
                                                            const float* __restrict__ factors, float b1, float omb1, float b2,
                                                            float omb2, float eps, float wd, float shrink, const AdamTabs tb) {
  __shared__ float* sw[TTX_ADAM_MAX_TENSORS];
  __shared__ const float* sg[TTX_ADAM_MAX_TENSORS];
  __shared__ float* sm[TTX_ADAM_MAX_TENSORS];
  __shared__ float* sv[TTX_ADAM_MAX_TENSORS];
  __shared__ long long sn[TTX_ADAM_MAX_TENSORS];
  __shared__ long long sf[TTX_ADAM_MAX_TENSORS];
  const int tid = threadIdx.x;
  {  // thread k picks tensor k's entries with constant subscripts
    float *pw = nullptr, *pm = nullptr, *pv = nullptr;
    const float* pg = nullptr;
    long long n = 0, f = 0;
#pragma unroll
    for (int k = 0; k < TTX_ADAM_MAX_TENSORS; ++k) {
      pw = tid == k ? tb.w[k] : pw;
      pg = tid == k ? tb.g[k] : pg;
      pm = tid == k ? tb.m[k] : pm;
      pv = tid == k ? tb.v[k] : pv;
      n = tid == k ? tb.n[k] : n;
      f = tid == k ? tb.first[k] : f;
    }
    if (tid < TTX_ADAM_MAX_TENSORS) {
      sw[tid] = pw; sg[tid] = pg; sm[tid] = pm; sv[tid] = pv; sn[tid] = n; sf[tid] = f;
    }
  }
  __syncthreads();
  const float a = factors[0], c = factors[1];
  for (long long ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
    int k = 0;  // the last tensor whose first chunk is <= ch (an empty tensor shares its first chunk with the next one)
    for (int j = 1; j < nt; ++j) k = sf[j] <= ch ? j : k;
    const long long n = sn[k], e0 = (ch - sf[k]) * kAdamChunk;
    float* __restrict__ w = sw[k];
    const float* __restrict__ g = sg[k];
    float* __restrict__ m = sm[k];
    float* __restrict__ v = sv[k];
    if (((vecmask >> k) & 1u) && e0 + kAdamChunk <= n) {  // (work-group uniform)
      const long long i = e0 + (long long)tid * kAdamVec;
      float4 W = *(const float4*)(w + i), M = *(const float4*)(m + i), V = *(const float4*)(v + i);
      const float4 G = *(const float4*)(g + i);
      adam_one<WD>(W.x, G.x, M.x, V.x, a, c, b1, omb1, b2, omb2, eps, wd, shrink);
      adam_one<WD>(W.y, G.y, M.y, V.y, a, c, b1, omb1, b2, omb2, eps, wd, shrink);
      adam_one<WD>(W.z, G.z, M.z, V.z, a, c, b1, omb1, b2, omb2, eps, wd, shrink);
      adam_one<WD>(W.w, G.w, M.w, V.w, a, c, b1, omb1, b2, omb2, eps, wd, shrink);
      *(float4*)(w + i) = W;
      *(float4*)(m + i) = M;
      *(float4*)(v + i) = V;
    } else {
#pragma unroll
      for (int u = 0; u < kAdamVec; ++u) {
        const long long i = e0 + (long long)u * kAdamT + tid;
        if (i < n) {
          float W = w[i], M = m[i], V = v[i];
          adam_one<WD>(W, g[i], M, V, a, c, b1, omb1, b2, omb2, eps, wd, shrink);
          w[i] = W;
          m[i] = M;
          v[i] = V;
        }
      }
    }
  }
}

}  // namespace ttx

using namespace ttx;

extern "C" {

size_t ttx_adam_apply_workspace_bytes(int32_t ntensors) {
  (void)ntensors;
  return 256 + 256;  // the step's two factors, behind the alignment slack
}

int ttx_adam_apply(int32_t ntensors, const int64_t* numel, float* const* w, const float* const* g, float* const* m,
                   float* const* v, int64_t* step, float lr, float beta1, float beta2, float eps, float weight_decay,
                   int32_t decoupled, void* workspace, size_t workspace_bytes, ttx_stream_t stream) {
  const char* what = "adam_apply";
  if (ntensors < 0 || ntensors > TTX_ADAM_MAX_TENSORS)
    TTX_FAIL(TTX_EINVAL, "%s: ntensors=%d outside [0, %d]", what, ntensors, TTX_ADAM_MAX_TENSORS);
  if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f))
    TTX_FAIL(TTX_EINVAL, "%s: betas (%g, %g) must lie in [0, 1)", what, (double)beta1, (double)beta2);
  if (!(eps >= 0.f)) TTX_FAIL(TTX_EINVAL, "%s: eps=%g must not be negative", what, (double)eps);
  if (ntensors > 0 && (!numel || !w || !g || !m || !v)) TTX_FAIL(TTX_EINVAL, "%s: numel / w / g / m / v is NULL", what);
  AdamTabs tb;
  memset(&tb, 0, sizeof(tb));
  long long chunks = 0;
  unsigned vecmask = 0;
  for (int k = 0; k < ntensors; ++k) {
    const int64_t n = numel[k];
    if (n < 0) TTX_FAIL(TTX_EINVAL, "%s: numel[%d]=%lld is negative", what, k, (long long)n);
    if (n >= (1ll << 40)) TTX_FAIL(TTX_EINVAL, "%s: numel[%d]=%lld must stay below 2^40", what, k, (long long)n);
    const uintptr_t all = (uintptr_t)w[k] | (uintptr_t)g[k] | (uintptr_t)m[k] | (uintptr_t)v[k];
    if (n > 0 && (!w[k] || !g[k] || !m[k] || !v[k])) TTX_FAIL(TTX_EINVAL, "%s: tensor %d: a pointer is NULL", what, k);
    if (all & 3) TTX_FAIL(TTX_EINVAL, "%s: tensor %d: every pointer must be 4-byte aligned", what, k);
    tb.w[k] = w[k]; tb.g[k] = g[k]; tb.m[k] = m[k]; tb.v[k] = v[k];
    tb.n[k] = n;
    tb.first[k] = chunks;
    if (!(all & 15)) vecmask |= 1u << k;
    chunks += (n + kAdamChunk - 1) / kAdamChunk;
  }
  for (int k = ntensors; k < TTX_ADAM_MAX_TENSORS; ++k) tb.first[k] = chunks;
  if (chunks == 0) return TTX_OK;  // nothing to step: no launch, the counter stays
  if (!step || (((uintptr_t)step) & 7)) TTX_FAIL(TTX_EINVAL, "%s: step is NULL or not 8-byte aligned", what);
  if (!workspace || workspace_bytes < ttx_adam_apply_workspace_bytes(ntensors))
    TTX_FAIL(TTX_EINVAL, "%s: workspace of %zu bytes, need %zu", what, workspace ? workspace_bytes : (size_t)0,
             ttx_adam_apply_workspace_bytes(ntensors));
  hipStream_t st = (hipStream_t)stream;
  float* factors = (float*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  hipLaunchKernelGGL(adam_step_kernel, dim3(1), dim3(kWave), 0, st, step, factors, lr, beta1, beta2);
  const unsigned blocks = (unsigned)(chunks < kAdamGridCap ? chunks : kAdamGridCap);
  const float omb1 = (float)(1.0 - (double)beta1), omb2 = (float)(1.0 - (double)beta2);
  const float shrink = (float)(1.0 - (double)lr * (double)weight_decay);
  const int mode = weight_decay == 0.f ? 0 : (decoupled ? 2 : 1);
#define TTX_ADAM_APPLY(WD)                                                                                                \
  hipLaunchKernelGGL(adam_apply_kernel<WD>, dim3(blocks), dim3(kAdamT), 0, st, (int)ntensors, chunks, vecmask,            \
                     (const float*)factors, beta1, omb1, beta2, omb2, eps, weight_decay, shrink, tb)
  if (mode == 0) TTX_ADAM_APPLY(0);
  else if (mode == 1) TTX_ADAM_APPLY(1);
  else TTX_ADAM_APPLY(2);
#undef TTX_ADAM_APPLY
  TTX_HIP(hipGetLastError());
  return TTX_OK;
}

}  // extern "C"

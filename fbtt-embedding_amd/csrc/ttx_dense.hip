// ttx_dense.hip -- bags over UNCOMPRESSED tables: the members of a mixed-cardinality module that are too small for a TT
// factorisation to pay (include/ttx.h "dense member tables"; not in the reference).  gfx950, wave64.
//
// One weight [R, D] holds the tables' rows one table after the other (table k: rows [row_base[k], row_base[k + 1])); the batch
// is the table-major form of the batched modules (bag b belongs to table b / B).  row_base and padding are HOST arrays that
// travel by value in the kernel arguments and are staged in LDS through constant subscripts (ttx_cache_vtables.hip KeyBases).
//
// Forward: one wave per bag on the lane layout of bag_max_pool_kernel (ttx_pool.hip): LPR lanes per row, 64 / LPR row groups,
// four slots of a group in flight.  A slot is padding when its index is negative or equals the table's padding value; any other
// index is clamped into the table.  Every output element has one writer.
//
// Backward: no float atomics, one writer per weight row, bit-identical from run to run.  (1) a key per lookup -- row + 1, or 0
// at padding -- with the value (bag << 32 | n); (2) the stable descending pair sort of ttx_cache.hip: a row's lookups become one
// run of the sorted order, in index order; (3) runs longer than kDenseSplit are cut, from the run's head, into chunks of
// kDenseSplit whose sums go to the workspace (dense_partial_kernel); (4) the lane group at a run's head sums the run -- its
// lookups in index order, or its chunks' sums in chunk order -- and applies the update once (dense_apply_kernel).  The
// contribution rows are grad_output's own rows, read where they lie.  Nothing is read back, nothing allocated: capturable.
//
// Every value array below is assigned on every path (ttx_rows.hip: the compiler otherwise moved such an array out of registers).
#include "ttx_internal.h"

namespace ttx {

constexpr int kDT = 256;                  // threads per work-group
constexpr int kDW = kDT / kWave;          // waves (forward: bags in flight) per work-group
constexpr int kDenseSplit = 32;           // lookups of one row that one lane group sums; longer lists are split
constexpr int kDenseFlight = 8;           // lookups of a list in flight per lane group
constexpr int kDenseBases = TTX_MAX_TABLES_MIXED + 1;
static_assert(kDenseBases <= kDT, "one thread stages one row base");

struct DenseTabs {
  int64_t base[kDenseBases];          // entries beyond num_tables repeat the total
  int64_t pad[TTX_MAX_TABLES_MIXED];  // -1: the table has no padding value
};

// sb[k] = tb.base[k], sp[k] = tb.pad[k]: thread k picks its entries with constant subscripts
__device__ __forceinline__ void stage_tabs(const DenseTabs& tb, int64_t* sb, int64_t* sp) {
  const int tid = threadIdx.x;
  int64_t b = 0, p = -1;
#pragma unroll
  for (int k = 0; k < kDenseBases; ++k) b = tid == k ? tb.base[k] : b;
#pragma unroll
  for (int k = 0; k < TTX_MAX_TABLES_MIXED; ++k) p = tid == k ? tb.pad[k] : p;
  if (tid < kDenseBases) sb[tid] = b;
  if (tid < TTX_MAX_TABLES_MIXED) sp[tid] = p;
}

template <int W>
__device__ __forceinline__ void dld(const float* p, float (&v)[W]) {
  if constexpr (W == 4) {
    const float4 t = *(const float4*)p;
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    v[0] = *p;
  }
}

template <int W>
__device__ __forceinline__ void dst(float* p, const float (&v)[W]) {
  if constexpr (W == 4) *(float4*)p = make_float4(v[0], v[1], v[2], v[3]);
  else *p = v[0];
}

template <int W>
__device__ __forceinline__ void dldi(const int* p, int (&v)[W]) {
  if constexpr (W == 4) {
    const int4 t = *(const int4*)p;
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    v[0] = *p;
  }
}

template <int W>
__device__ __forceinline__ void dsti(int* p, const int (&v)[W]) {
  if constexpr (W == 4) *(int4*)p = make_int4(v[0], v[1], v[2], v[3]);
  else *p = v[0];
}

__device__ __forceinline__ long long clamp_off(long long v, long long nnz) { return v < 0 ? 0 : (v > nnz ? nnz : v); }

// ------------------------------------------------------------------------------------------------------------ forward
// MODE 0 sum (weights optional), 1 mean (live[bag] = the bag's count of non-padding slots, its divisor), 2 max (strict > in
// position order within a group, the lower position on a tie between groups: the bag's first maximum; argmax -1 and output 0
// for a bag without a live slot).  W floats per lane (4: 16-byte loads, 1: the scalar path), DV = D / W column vectors; rows
// wider than LPR vectors are walked per column block.  A wave takes the bags bag, bag + waves of the grid, ...
template <int W, int MODE>
__global__ __launch_bounds__(kDT) void dense_fwd_kernel(long long nb, long long B, int DV, int lpr_log2, long long nnz,
                                                        const int64_t* __restrict__ indices,
                                                        const int64_t* __restrict__ offsets, const DenseTabs tb,
                                                        const float* __restrict__ psw, const float* __restrict__ weight,
                                                        float* __restrict__ out, int* __restrict__ live_out,
                                                        int* __restrict__ argmax) {
  __shared__ int64_t sb[kDenseBases];
  __shared__ int64_t sp[TTX_MAX_TABLES_MIXED];
  stage_tabs(tb, sb, sp);
  __syncthreads();
  const int lane = lane_id();
  const int LPR = 1 << lpr_log2, G = kWave >> lpr_log2;
  const int grp = lane >> lpr_log2, cl = lane & (LPR - 1);
  const size_t ld = (size_t)DV * W;
  for (long long bag = (long long)blockIdx.x * kDW + threadIdx.x / kWave; bag < nb; bag += (long long)gridDim.x * kDW) {
    const int t = (int)(bag / B);
    const long long base = sb[t], E = sb[t + 1] - base, pad = sp[t];
    const long long s = clamp_off(offsets[bag], nnz);
    long long e = clamp_off(offsets[bag + 1], nnz);
    e = e < s ? s : e;
    for (int c0 = 0; c0 < DV; c0 += LPR) {
      const int c = c0 + cl;
      const bool colok = c < DV;
      float m[W];
      int p[W];
      int cnt = 0;
#pragma unroll
      for (int k = 0; k < W; ++k) { m[k] = 0.f; p[k] = -1; }
      const float* wcol = weight + (size_t)(colok ? c : 0) * W;
      for (long long j = s + grp; j < e; j += 4 * G) {  // four slots of the group in flight
        float a[4][W], w[4];
        bool ok[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const long long jj = j + (long long)u * G;
          long long idx = -1;
          if (jj < e) idx = indices[jj];
          ok[u] = idx >= 0 && idx != pad;
          w[u] = 0.f;
#pragma unroll
          for (int k = 0; k < W; ++k) a[u][k] = 0.f;
          if (ok[u]) {
            const long long row = base + (idx < E ? idx : E - 1);
            if (colok) dld<W>(wcol + (size_t)row * ld, a[u]);
            w[u] = 1.f;
            if constexpr (MODE == 0)
              if (psw) w[u] = psw[jj];
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          cnt += ok[u] ? 1 : 0;
          if constexpr (MODE == 2) {
            const int pos = (int)(j + (long long)u * G);
#pragma unroll
            for (int k = 0; k < W; ++k)
              if (ok[u] && (p[k] < 0 || a[u][k] > m[k])) { m[k] = a[u][k]; p[k] = pos; }
          } else {
#pragma unroll
            for (int k = 0; k < W; ++k) m[k] = fmaf(w[u], a[u][k], m[k]);
          }
        }
      }
      for (int o = LPR; o < kWave; o <<= 1) {  // combine the row groups (wave-uniform: every lane takes part)
        cnt += __shfl_xor(cnt, o, kWave);
#pragma unroll
        for (int k = 0; k < W; ++k) {
          const float om = __shfl_xor(m[k], o, kWave);
          if constexpr (MODE == 2) {
            const int op = __shfl_xor(p[k], o, kWave);
            if (op >= 0 && (p[k] < 0 || om > m[k] || (om == m[k] && op < p[k]))) { m[k] = om; p[k] = op; }
          } else {
            m[k] += om;
          }
        }
      }
      if (grp == 0 && colok) {
        if constexpr (MODE == 1) {
          const float d = (float)(cnt > 1 ? cnt : 1);
#pragma unroll
          for (int k = 0; k < W; ++k) m[k] = m[k] / d;
        }
        if constexpr (MODE == 2) {
#pragma unroll
          for (int k = 0; k < W; ++k) m[k] = p[k] < 0 ? 0.f : m[k];
          dsti<W>(argmax + (size_t)bag * ld + (size_t)c * W, p);
        }
        dst<W>(out + (size_t)bag * ld + (size_t)c * W, m);
      }
      if constexpr (MODE == 1)
        if (lane == 0 && c0 == 0) live_out[bag] = cnt;
    }
  }
}

// ----------------------------------------------------------------------------------------------------------- backward
// keys[n] = row(n) + 1 for a live lookup, 0 at padding and for a position no bag covers; vals[n] = bag(n) << 32 | n.  The bag of
// position n: the last b with offsets[b] <= n (empty bags give equal entries, which the search steps over).
__global__ __launch_bounds__(kDT) void dense_keys_kernel(long long nnz, long long nb, long long B,
                                                         const int64_t* __restrict__ indices,
                                                         const int64_t* __restrict__ offsets, const DenseTabs tb,
                                                         int64_t* __restrict__ keys, int64_t* __restrict__ vals) {
  __shared__ int64_t sb[kDenseBases];
  __shared__ int64_t sp[TTX_MAX_TABLES_MIXED];
  stage_tabs(tb, sb, sp);
  __syncthreads();
  for (long long n = (long long)blockIdx.x * kDT + threadIdx.x; n < nnz; n += (long long)gridDim.x * kDT) {
    long long lo = 0, hi = nb;  // the first b in [0, nb] with offsets[b] > n (nb: none)
    while (lo < hi) {
      const long long mid = (lo + hi) >> 1;
      if (clamp_off(offsets[mid], nnz) > n) hi = mid;
      else lo = mid + 1;
    }
    const long long bag = lo - 1;
    long long key = 0;
    if (bag >= 0 && n < clamp_off(offsets[bag + 1], nnz)) {
      const int t = (int)(bag / B);
      const long long base = sb[t], E = sb[t + 1] - base, idx = indices[n];
      if (idx >= 0 && idx != sp[t]) key = base + (idx < E ? idx : E - 1) + 1;
    }
    keys[n] = key;
    vals[n] = ((bag < 0 ? 0 : bag) << 32) | n;
  }
}

// d_psw[n] = <grad_output[bag(n)], weight[row(n)]>, 0 at padding: one lane group per lookup, before the update touches weight
template <int W>
__global__ __launch_bounds__(kDT) void dense_psw_grad_kernel(long long nnz, int DV, int lpr_log2,
                                                             const int64_t* __restrict__ keys,
                                                             const int64_t* __restrict__ vals,
                                                             const float* __restrict__ d_out,
                                                             const float* __restrict__ weight, float* __restrict__ d_psw) {
  const int LPR = 1 << lpr_log2;
  const int cl = threadIdx.x & (LPR - 1);
  const long long n = ((long long)blockIdx.x * kDT + threadIdx.x) >> lpr_log2;
  const size_t ld = (size_t)DV * W;
  long long key = 0, bag = 0;
  if (n < nnz) {
    key = keys[n];
    bag = vals[n] >> 32;
  }
  float dot = 0.f;
  for (int c0 = 0; c0 < DV; c0 += LPR) {
    const int c = c0 + cl;
    float a[W], g[W];
#pragma unroll
    for (int k = 0; k < W; ++k) { a[k] = 0.f; g[k] = 0.f; }
    if (key > 0 && c < DV) {
      dld<W>(weight + (size_t)(key - 1) * ld + (size_t)c * W, a);
      dld<W>(d_out + (size_t)bag * ld + (size_t)c * W, g);
    }
#pragma unroll
    for (int k = 0; k < W; ++k) dot = fmaf(a[k], g[k], dot);
  }
  for (int o = 1; o < LPR; o <<= 1) dot += __shfl_xor(dot, o, kWave);  // (wave-uniform)
  if (n < nnz && cl == 0) d_psw[n] = dot;
}

// what the lookups at sorted positions [i, end) that belong to row key k add to columns c * W .. of the row's gradient, in
// position (= index) order, kDenseFlight lookups in flight: their keys and values are loaded side by side, then their gradient
// rows.  mode 0: the weight (1 without), 1: 1 / live[bag], 2: the columns the lookup won in its bag.
template <int W>
__device__ __forceinline__ void dense_list_sum(const int64_t* __restrict__ ks, const int64_t* __restrict__ vs, long long i,
                                               long long end, long long k, int c, size_t ld, int mode,
                                               const float* __restrict__ psw, const int* __restrict__ live,
                                               const int* __restrict__ argmax, const float* __restrict__ d_out,
                                               float (&acc)[W]) {
  for (long long j = i; j < end; j += kDenseFlight) {
    long long kk[kDenseFlight], vv[kDenseFlight];
    float d[kDenseFlight][W];
#pragma unroll
    for (int u = 0; u < kDenseFlight; ++u) {
      const long long jj = j + u;
      kk[u] = 0;  // (no row: keys of live lookups are positive)
      vv[u] = 0;
      if (jj < end) {
        kk[u] = ks[jj];
        vv[u] = vs[jj];
      }
    }
    bool more = true;
#pragma unroll
    for (int u = 0; u < kDenseFlight; ++u) {
      const bool ok = more && kk[u] == k;  // (a run is contiguous: nothing behind its end belongs to it)
      more = ok;
#pragma unroll
      for (int e = 0; e < W; ++e) d[u][e] = 0.f;
      if (ok) {
        const long long v = vv[u];
        const int n = (int)(v & 0x7fffffffll);
        const size_t at = (size_t)(v >> 32) * ld + (size_t)c * W;
        dld<W>(d_out + at, d[u]);
        if (mode == 2) {
          int am[W];
          dldi<W>(argmax + at, am);
#pragma unroll
          for (int e = 0; e < W; ++e) d[u][e] = am[e] == n ? d[u][e] : 0.f;
        } else if (mode == 1) {
          const int l = live[v >> 32];
          const float x = 1.f / (float)(l > 1 ? l : 1);
#pragma unroll
          for (int e = 0; e < W; ++e) d[u][e] *= x;
        } else if (psw) {
          const float x = psw[n];
#pragma unroll
          for (int e = 0; e < W; ++e) d[u][e] *= x;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kDenseFlight; ++u)
#pragma unroll
      for (int e = 0; e < W; ++e) acc[e] += d[u][e];
    if (!more) break;
  }
}

// the workspace row of the chunk that starts at sorted position j of a split run: chunks are kDenseSplit long except a run's
// last, so an aligned window of kDenseSplit positions holds the start of at most one full chunk and of at most one last chunk
__device__ __forceinline__ long long dense_slot(const int64_t* __restrict__ ks, long long j, long long k, long long nnz) {
  const bool full = j + kDenseSplit - 1 < nnz && ks[j + kDenseSplit - 1] == k;
  return 2 * (j / kDenseSplit) + (full ? 0 : 1);
}

// One lane group per sorted position; the groups at the chunk starts of runs LONGER than kDenseSplit sum their chunk into the
// workspace.  A position is a chunk start when it is the run's head or a multiple of kDenseSplit behind it (the head of a
// position deep in a run: binary search in the descending keys).
template <int W>
__global__ __launch_bounds__(kDT) void dense_partial_kernel(long long nnz, int DV, int lpr_log2,
                                                            const int64_t* __restrict__ ks, const int64_t* __restrict__ vs,
                                                            int mode, const float* __restrict__ psw,
                                                            const int* __restrict__ live, const int* __restrict__ argmax,
                                                            const float* __restrict__ d_out, float* __restrict__ part) {
  const int LPR = 1 << lpr_log2;
  const int cl = threadIdx.x & (LPR - 1);
  const long long i = ((long long)blockIdx.x * kDT + threadIdx.x) >> lpr_log2;
  if (i >= nnz) return;
  const long long k = ks[i];
  if (k == 0) return;
  const bool head = i == 0 || ks[i - 1] != k;
  if (head) {
    if (!(i + kDenseSplit < nnz && ks[i + kDenseSplit] == k)) return;  // the whole run is the apply kernel's
  } else {
    if (i < kDenseSplit || ks[i - kDenseSplit] != k) return;
    long long lo = 0, hi = i;  // the first position with ks <= k (descending order): the run's head
    while (lo < hi) {
      const long long mid = (lo + hi) >> 1;
      if (ks[mid] <= k) hi = mid;
      else lo = mid + 1;
    }
    if ((i - lo) % kDenseSplit) return;
  }
  const size_t ld = (size_t)DV * W;
  const long long end = i + kDenseSplit < nnz ? i + kDenseSplit : nnz;
  float* prow = part + (size_t)dense_slot(ks, i, k, nnz) * ld;
  for (int c0 = 0; c0 < DV; c0 += LPR) {
    const int c = c0 + cl;
    if (c >= DV) continue;
    float acc[W];
#pragma unroll
    for (int e = 0; e < W; ++e) acc[e] = 0.f;
    dense_list_sum<W>(ks, vs, i, end, k, c, ld, mode, psw, live, argmax, d_out, acc);
    dst<W>(prow + (size_t)c * W, acc);
  }
}

// columns c * W .. of the gradient of the row whose run starts at sorted position i
template <int W>
__device__ __forceinline__ void dense_row_grad(const int64_t* __restrict__ ks, const int64_t* __restrict__ vs, long long i,
                                               long long nnz, long long k, bool split, int c, size_t ld, int mode,
                                               const float* __restrict__ psw, const int* __restrict__ live,
                                               const int* __restrict__ argmax, const float* __restrict__ d_out,
                                               const float* __restrict__ part, float (&acc)[W]) {
#pragma unroll
  for (int e = 0; e < W; ++e) acc[e] = 0.f;
  if (!split) {
    dense_list_sum<W>(ks, vs, i, i + kDenseSplit < nnz ? i + kDenseSplit : nnz, k, c, ld, mode, psw, live, argmax, d_out, acc);
  } else {
    for (long long j = i; j < nnz; j += 4 * kDenseSplit) {  // the chunks' sums, in chunk order, four chunks in flight
      float v[4][W];
      bool more = true;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long long jj = j + (long long)u * kDenseSplit;
        const bool ok = more && jj < nnz && ks[jj] == k;
        more = ok;
#pragma unroll
        for (int e = 0; e < W; ++e) v[u][e] = 0.f;
        if (ok) dld<W>(part + (size_t)dense_slot(ks, jj, k, nnz) * ld + (size_t)c * W, v[u]);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int e = 0; e < W; ++e) acc[e] += v[u][e];
      if (!more) break;
    }
  }
}

// One lane group per sorted position; the group at a run's head owns the row: it sums the row's gradient and applies it once.
// opt 0: SGD, 1: element-wise Adagrad (state [R, D]), 2: row-wise Adagrad (state [R], += mean_e G_e^2), 3: dst = the gradient.
// Shuffles sit at wave-uniform points only (`own` gates the memory accesses, not the control flow around a shuffle).
template <int W>
__global__ __launch_bounds__(kDT) void dense_apply_kernel(long long nnz, int DV, int D, int lpr_log2,
                                                          const int64_t* __restrict__ ks, const int64_t* __restrict__ vs,
                                                          int mode, const float* __restrict__ psw,
                                                          const int* __restrict__ live, const int* __restrict__ argmax,
                                                          const float* __restrict__ d_out, const float* __restrict__ part,
                                                          int opt, float lr, float eps, float* __restrict__ state,
                                                          float* __restrict__ dstw) {
  const int LPR = 1 << lpr_log2;
  const int cl = threadIdx.x & (LPR - 1);
  const long long i = ((long long)blockIdx.x * kDT + threadIdx.x) >> lpr_log2;
  long long k = 0;
  bool own = false, split = false;
  if (i < nnz) {
    k = ks[i];
    own = k != 0 && (i == 0 || ks[i - 1] != k);
    split = own && i + kDenseSplit < nnz && ks[i + kDenseSplit] == k;
  }
  const size_t ld = (size_t)DV * W;
  const size_t row = own ? (size_t)(k - 1) : 0;
  float mult = lr;
  if (opt == 2) {  // the row's mean square first (rows wider than the lane group: the gradient is summed again below)
    float ss = 0.f;
    for (int c0 = 0; c0 < DV; c0 += LPR) {
      const int c = c0 + cl;
      float g[W];
#pragma unroll
      for (int e = 0; e < W; ++e) g[e] = 0.f;
      if (own && c < DV) dense_row_grad<W>(ks, vs, i, nnz, k, split, c, ld, mode, psw, live, argmax, d_out, part, g);
#pragma unroll
      for (int e = 0; e < W; ++e) ss = fmaf(g[e], g[e], ss);
    }
    for (int o = 1; o < LPR; o <<= 1) ss += __shfl_xor(ss, o, kWave);
    float s = 0.f;
    if (own) {
      s = state[row] + ss / (float)D;
      if (cl == 0) state[row] = s;
    }
    mult = lr / (sqrtf(s) + eps);
  }
  if (!own) return;
  for (int c0 = 0; c0 < DV; c0 += LPR) {
    const int c = c0 + cl;
    if (c >= DV) continue;
    float g[W], w[W];
    dense_row_grad<W>(ks, vs, i, nnz, k, split, c, ld, mode, psw, live, argmax, d_out, part, g);
    const size_t at = row * ld + (size_t)c * W;
    if (opt == 3) {
      dst<W>(dstw + at, g);
      continue;
    }
    dld<W>(dstw + at, w);
    if (opt == 1) {
      float s[W];
      dld<W>(state + at, s);
#pragma unroll
      for (int e = 0; e < W; ++e) {
        s[e] = s[e] + g[e] * g[e];
        w[e] = w[e] - lr * g[e] / (sqrtf(s[e]) + eps);
      }
      dst<W>(state + at, s);
    } else {
#pragma unroll
      for (int e = 0; e < W; ++e) w[e] = w[e] - mult * g[e];
    }
    dst<W>(dstw + at, w);
  }
}

// ---------------------------------------------------------------------------------------------------------------- host
static bool dense_vec4(int32_t D, std::initializer_list<const void*> ptrs) {
  if (D % 4 != 0) return false;
  for (const void* p : ptrs)
    if (((uintptr_t)p) & 15) return false;
  return true;
}

static int dense_lanes_log2(int DV) {
  int l = 0;
  while ((1 << l) < DV && (1 << l) < kWave) ++l;
  return l;
}

static int dense_sort_passes(int64_t R) {  // bytes of the largest key, R
  int bits = 0;
  while (bits < 64 && ((uint64_t)R >> bits)) ++bits;
  return bits < 8 ? 1 : (bits + 7) / 8;
}

// the arguments both calls share -> the tables by value
static int dense_check(const char* what, int32_t num_tables, int64_t B, int32_t D, int64_t nnz, const int64_t* indices,
                       const int64_t* offsets, const int64_t* row_base, const int64_t* padding, const float* psw, int32_t mode,
                       DenseTabs* tb) {
  if (num_tables < 1 || num_tables > TTX_MAX_TABLES_MIXED)
    TTX_FAIL(TTX_EINVAL, "%s: num_tables=%d outside [1, %d]", what, num_tables, TTX_MAX_TABLES_MIXED);
  if (B < 0 || nnz < 0) TTX_FAIL(TTX_EINVAL, "%s: negative size (B=%lld, nnz=%lld)", what, (long long)B, (long long)nnz);
  if (D <= 0) TTX_FAIL(TTX_EINVAL, "%s: D=%d must be positive", what, D);
  if (nnz >= (1ll << 31) || B >= (1ll << 31) || (int64_t)num_tables * B >= (1ll << 31))
    TTX_FAIL(TTX_EINVAL, "%s: nnz=%lld and num_tables*B=%lld must stay below 2^31", what, (long long)nnz,
             (long long)num_tables * (long long)B);
  if (mode < 0 || mode > 2) TTX_FAIL(TTX_EINVAL, "%s: mode=%d must be 0 (sum), 1 (mean) or 2 (max)", what, mode);
  if (psw && mode != 0) TTX_FAIL(TTX_EINVAL, "%s: per_sample_weights go with mode 0 (sum) only, got mode %d", what, mode);
  if (!row_base) TTX_FAIL(TTX_EINVAL, "%s: row_base is NULL", what);
  if (((uintptr_t)row_base) & 7) TTX_FAIL(TTX_EINVAL, "%s: row_base must be 8-byte aligned", what);
  if (row_base[0] != 0) TTX_FAIL(TTX_EINVAL, "%s: row_base[0]=%lld must be 0", what, (long long)row_base[0]);
  for (int k = 0; k < num_tables; ++k)
    if (row_base[k + 1] <= row_base[k])
      TTX_FAIL(TTX_EINVAL, "%s: row_base must be strictly increasing (entries %d, %d: %lld, %lld)", what, k, k + 1,
               (long long)row_base[k], (long long)row_base[k + 1]);
  if (row_base[num_tables] >= (1ll << 62)) TTX_FAIL(TTX_EINVAL, "%s: row_base[num_tables] must stay below 2^62", what);
  if (padding && (((uintptr_t)padding) & 7)) TTX_FAIL(TTX_EINVAL, "%s: padding must be 8-byte aligned", what);
  if (B > 0 && !offsets) TTX_FAIL(TTX_EINVAL, "%s: offsets is NULL", what);
  if (nnz > 0 && !indices) TTX_FAIL(TTX_EINVAL, "%s: indices is NULL", what);
  if ((((uintptr_t)offsets) & 7) || (((uintptr_t)indices) & 7))
    TTX_FAIL(TTX_EINVAL, "%s: indices and offsets must be 8-byte aligned", what);
  if (((uintptr_t)psw) & 3) TTX_FAIL(TTX_EINVAL, "%s: per_sample_weights must be 4-byte aligned", what);
  for (int k = 0; k < kDenseBases; ++k) tb->base[k] = row_base[k < num_tables ? k : num_tables];
  for (int k = 0; k < TTX_MAX_TABLES_MIXED; ++k) tb->pad[k] = (padding && k < num_tables && padding[k] >= 0) ? padding[k] : -1;
  return TTX_OK;
}

static size_t dense_part_rows(int64_t nnz) { return 2 * (size_t)((nnz + kDenseSplit - 1) / kDenseSplit); }

}  // namespace ttx

using namespace ttx;

extern "C" {

int ttx_dense_bags_info(int32_t D, int64_t nnz, int32_t* out) {
  if (!out) TTX_FAIL(TTX_EINVAL, "dense_bags_info: out is NULL");
  if (D <= 0 || nnz < 0) TTX_FAIL(TTX_EINVAL, "dense_bags_info: bad D / nnz");
  out[0] = kDenseSplit;  // a row with more lookups than this has its list split into chunks of this length
  out[1] = 0;            // no one-launch route: every batch size takes the sorted route
  return TTX_OK;
}

int ttx_dense_bags_forward(int32_t num_tables, int64_t B, int32_t D, int64_t nnz, const int64_t* indices, const int64_t* offsets,
                           const int64_t* row_base, const int64_t* padding, const float* per_sample_weights, int32_t mode,
                           const float* weight, float* output, int32_t* live, int32_t* argmax, ttx_stream_t stream) {
  const char* what = "dense_bags_forward";
  DenseTabs tb;
  const int rc = dense_check(what, num_tables, B, D, nnz, indices, offsets, row_base, padding, per_sample_weights, mode, &tb);
  if (rc) return rc;
  const long long nb = (long long)num_tables * B;
  if (nb == 0) return TTX_OK;
  if (!weight || !output) TTX_FAIL(TTX_EINVAL, "%s: weight / output is NULL", what);
  if ((((uintptr_t)weight) & 3) || (((uintptr_t)output) & 3)) TTX_FAIL(TTX_EINVAL, "%s: weight and output must be 4-byte aligned", what);
  if (mode == 1 && (!live || (((uintptr_t)live) & 3))) TTX_FAIL(TTX_EINVAL, "%s: mode 1 (mean) needs live (int32 per bag)", what);
  if (mode == 2 && (!argmax || (((uintptr_t)argmax) & 3))) TTX_FAIL(TTX_EINVAL, "%s: mode 2 (max) needs argmax (int32 [bags, D])", what);
  hipStream_t st = (hipStream_t)stream;
  const long long want = (nb + kDW - 1) / kDW;
  const unsigned blocks = (unsigned)(want < 4096 ? want : 4096);
  const bool v4 = dense_vec4(D, {weight, output, mode == 2 ? (const void*)argmax : nullptr});
  const int DV = v4 ? D / 4 : D, lg = dense_lanes_log2(DV);
#define TTX_DENSE_FWD(WW, MM)                                                                                                   \
  hipLaunchKernelGGL((dense_fwd_kernel<WW, MM>), dim3(blocks), dim3(kDT), 0, st, nb, (long long)B, DV, lg, (long long)nnz, indices, \
                     offsets, tb, per_sample_weights, weight, output, (int*)live, (int*)argmax)
  if (v4) {
    if (mode == 0) TTX_DENSE_FWD(4, 0);
    else if (mode == 1) TTX_DENSE_FWD(4, 1);
    else TTX_DENSE_FWD(4, 2);
  } else {
    if (mode == 0) TTX_DENSE_FWD(1, 0);
    else if (mode == 1) TTX_DENSE_FWD(1, 1);
    else TTX_DENSE_FWD(1, 2);
  }
#undef TTX_DENSE_FWD
  TTX_HIP(hipGetLastError());
  return TTX_OK;
}

size_t ttx_dense_bags_backward_workspace_bytes(int64_t num_bags, int64_t nnz, int32_t D) {
  (void)num_bags;
  if (nnz <= 0 || D <= 0) return 0;
  return 256 + 2 * align_up((size_t)nnz * 8) + align_up(sort_pairs_ws_bytes(nnz)) + align_up(dense_part_rows(nnz) * (size_t)D * 4);
}

int ttx_dense_bags_backward(int32_t optim, int32_t num_tables, int64_t B, int32_t D, int64_t nnz, const int64_t* indices,
                            const int64_t* offsets, const int64_t* row_base, const int64_t* padding,
                            const float* per_sample_weights, int32_t mode, const int32_t* live, const int32_t* argmax,
                            const float* grad_output, float lr, float eps, int32_t state_width, float* opt_state, float* weight,
                            float* d_weight, float* d_per_sample_weights, void* workspace, size_t workspace_bytes,
                            ttx_stream_t stream) {
  const char* what = "dense_bags_backward";
  DenseTabs tb;
  const int rc = dense_check(what, num_tables, B, D, nnz, indices, offsets, row_base, padding, per_sample_weights, mode, &tb);
  if (rc) return rc;
  if (optim != TTX_OPTIM_SGD && optim != TTX_OPTIM_ADAGRAD && optim != TTX_OPTIM_DENSE)
    TTX_FAIL(TTX_EINVAL, "%s: optim=%d must be TTX_OPTIM_SGD, _ADAGRAD or _DENSE", what, optim);
  if (optim == TTX_OPTIM_ADAGRAD ? (state_width != 1 && state_width != D) : state_width != 0)
    TTX_FAIL(TTX_EINVAL, "%s: state_width=%d does not match optim=%d (Adagrad: 1 or D=%d; otherwise 0)", what, state_width, optim, D);
  if (optim == TTX_OPTIM_ADAGRAD && (!opt_state || (((uintptr_t)opt_state) & 3)))
    TTX_FAIL(TTX_EINVAL, "%s: Adagrad needs opt_state (4-byte aligned)", what);
  float* target = optim == TTX_OPTIM_DENSE ? d_weight : weight;
  if (!target || (((uintptr_t)target) & 3))
    TTX_FAIL(TTX_EINVAL, "%s: %s is NULL or misaligned", what, optim == TTX_OPTIM_DENSE ? "d_weight" : "weight");
  if (d_per_sample_weights && mode != 0) TTX_FAIL(TTX_EINVAL, "%s: d_per_sample_weights goes with mode 0 (sum) only", what);
  if (d_per_sample_weights && (!weight || (((uintptr_t)weight) & 3) || (((uintptr_t)d_per_sample_weights) & 3)))
    TTX_FAIL(TTX_EINVAL, "%s: d_per_sample_weights needs weight, both 4-byte aligned", what);
  if (nnz > 0) {
    if (!grad_output || (((uintptr_t)grad_output) & 3)) TTX_FAIL(TTX_EINVAL, "%s: grad_output is NULL or misaligned", what);
    if (mode == 1 && (!live || (((uintptr_t)live) & 3))) TTX_FAIL(TTX_EINVAL, "%s: mode 1 (mean) needs live (int32 per bag)", what);
    if (mode == 2 && (!argmax || (((uintptr_t)argmax) & 3))) TTX_FAIL(TTX_EINVAL, "%s: mode 2 (max) needs argmax (int32 [bags, D])", what);
    if (workspace_bytes < ttx_dense_bags_backward_workspace_bytes((int64_t)num_tables * B, nnz, D) || !workspace)
      TTX_FAIL(TTX_EWORKSPACE, "%s: workspace of %zu bytes, need %zu", what, workspace ? workspace_bytes : (size_t)0,
               ttx_dense_bags_backward_workspace_bytes((int64_t)num_tables * B, nnz, D));
  }
  hipStream_t st = (hipStream_t)stream;
  const int64_t R = row_base[num_tables];
  if (optim == TTX_OPTIM_DENSE) TTX_HIP(hipMemsetAsync(d_weight, 0, (size_t)R * D * sizeof(float), st));
  if (nnz == 0) return TTX_OK;
  const long long nb = (long long)num_tables * B;
  char* ws = (char*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  int64_t* keys = (int64_t*)ws;
  int64_t* vals = (int64_t*)(ws + align_up((size_t)nnz * 8));
  char* sort_ws = ws + 2 * align_up((size_t)nnz * 8);
  float* part = (float*)(sort_ws + align_up(sort_pairs_ws_bytes(nnz)));
  {
    const long long want = (nnz + kDT - 1) / kDT;
    hipLaunchKernelGGL(dense_keys_kernel, dim3((unsigned)(want < 8192 ? want : 8192)), dim3(kDT), 0, st, (long long)nnz, nb,
                       (long long)B, indices, offsets, tb, keys, vals);
  }
  int64_t *ks = nullptr, *vs = nullptr;
  const int src = sort_pairs_desc(nnz, keys, vals, sort_ws, &ks, &vs, st, dense_sort_passes(R));
  if (src) return src;
  const int opt = optim == TTX_OPTIM_SGD ? 0 : optim == TTX_OPTIM_DENSE ? 3 : (state_width == D ? 1 : 2);  // (D == 1: the same)
  const bool v4 = dense_vec4(D, {grad_output, target, part, mode == 2 ? (const void*)argmax : nullptr,
                                 opt == 1 ? (const void*)opt_state : nullptr,
                                 d_per_sample_weights ? (const void*)weight : nullptr});
  const int DV = v4 ? D / 4 : D, lg = dense_lanes_log2(DV);
  const unsigned blocks = (unsigned)((((long long)nnz << lg) + kDT - 1) / kDT);
  const int* livep = (const int*)live;
  const int* argp = (const int*)argmax;
  if (v4) {
    if (d_per_sample_weights)
      hipLaunchKernelGGL(dense_psw_grad_kernel<4>, dim3(blocks), dim3(kDT), 0, st, (long long)nnz, DV, lg, keys, vals, grad_output,
                         weight, d_per_sample_weights);
    hipLaunchKernelGGL(dense_partial_kernel<4>, dim3(blocks), dim3(kDT), 0, st, (long long)nnz, DV, lg, ks, vs, mode,
                       per_sample_weights, livep, argp, grad_output, part);
    hipLaunchKernelGGL(dense_apply_kernel<4>, dim3(blocks), dim3(kDT), 0, st, (long long)nnz, DV, (int)D, lg, ks, vs, mode,
                       per_sample_weights, livep, argp, grad_output, part, opt, lr, eps, opt_state, target);
  } else {
    if (d_per_sample_weights)
      hipLaunchKernelGGL(dense_psw_grad_kernel<1>, dim3(blocks), dim3(kDT), 0, st, (long long)nnz, DV, lg, keys, vals, grad_output,
                         weight, d_per_sample_weights);
    hipLaunchKernelGGL(dense_partial_kernel<1>, dim3(blocks), dim3(kDT), 0, st, (long long)nnz, DV, lg, ks, vs, mode,
                       per_sample_weights, livep, argp, grad_output, part);
    hipLaunchKernelGGL(dense_apply_kernel<1>, dim3(blocks), dim3(kDT), 0, st, (long long)nnz, DV, (int)D, lg, ks, vs, mode,
                       per_sample_weights, livep, argp, grad_output, part, opt, lr, eps, opt_state, target);
  }
  TTX_HIP(hipGetLastError());
  return TTX_OK;
}

}  // extern "C"

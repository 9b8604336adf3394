// ttx_cache_carry.hip -- the row cache across a re-populate (include/ttx.h, "cache refresh"; not in the reference, whose
// populate decompresses every cache row anew).  gfx950, wave64.
//
// A populate hands the cache_size most frequent keys new row numbers and fills every row from the cores.  ttx_cache_carry then
// moves what the cache had learnt to where it now belongs: a key cached before AND after gets its old row and optimizer state
// in its new row; a key that is new to the cache keeps the decompressed row and starts from zero state.  The move is a
// permutation of rows, hence out of place: the caller hands in copies of cache_state / cache_weight / state taken before the
// populate.  Geometry-independent: it sees slots, states and rows only, so it serves all three populates.
#include "ttx_internal.h"

namespace ttx {

constexpr int kCC = 256;

template <bool VEC> struct CarryUnit { using T = float; };
template <> struct CarryUnit<true> { using T = float4; };

// Work-group = a tile of kCC consecutive slots, grid-stride over the tiles.  Scan: one slot per thread -- coalesced reads of the
// key and both states; a slot takes part iff it holds a key, its new state names a row and it is the copy of its key that
// hashtbl_find returns (the owner of the row: DESIGN.md 4.15).  The tile's participants are compacted IN SLOT ORDER into LDS
// (ballot + popcount per wave, the waves' counts added up), then moved by groups of G = 2^lg lanes, one row per group and
// step: a row of U units (VEC: 16-byte units, U = D / 4; else floats, U = D) is U / G accesses per lane, and a wave moves
// 64 / G rows at a time when D is small.  One writer per row: a row number is owned by one findable slot.
//   state_mode 0: no optimizer state; 1: one float per row; 2: a row of U units per row (moved like the weights).
//   list entry: {new row, old row or -1 (admitted)}.
template <bool VEC>
__global__ __launch_bounds__(kCC) void cache_carry_kernel(int32_t H, int32_t ntiles, const int64_t* __restrict__ hashtbl,
                                                         const int32_t* __restrict__ old_state,
                                                         const int32_t* __restrict__ new_state, int32_t cache_size, int32_t U,
                                                         int32_t lg, const float* __restrict__ old_w, float* __restrict__ w,
                                                         int32_t state_mode, const float* __restrict__ old_s,
                                                         float* __restrict__ s) {
  using T = typename CarryUnit<VEC>::T;
  __shared__ int2 list[kCC];
  __shared__ int wcnt[kCC / kWave];
  const int tid = threadIdx.x, lane = lane_id(), wv = tid / kWave;
  const int G = 1 << lg, grp = tid >> lg, l = tid & (G - 1), ngrp = kCC >> lg;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {  // (work-group uniform: the barriers below)
    const int64_t slot = (int64_t)tile * kCC + tid;
    int32_t n = -1, m = -1;
    bool part = false;
    if (slot < H) {
      const int64_t key = hashtbl[slot];
      n = new_state[slot];
      m = old_state[slot];
      part = key != -1 && n >= 0 && n < cache_size && hashtbl_find(key, H, hashtbl) == (int32_t)slot;
    }
    const unsigned long long b = __ballot(part);
    if (lane == 0) wcnt[wv] = __popcll(b);
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int k = 0; k < kCC / kWave; ++k) {
      const int c = wcnt[k];
      if (k < wv) base += c;
      total += c;
    }
    if (part) list[base + __popcll(b & lanemask_lt())] = make_int2(n, (m >= 0 && m < cache_size) ? m : -1);
    __syncthreads();
    for (int j = grp; j < total; j += ngrp) {
      const int2 e = list[j];
      const bool kept = e.y >= 0;
      if (kept) {
        const T* src = (const T*)old_w + (size_t)e.y * U;
        T* dst = (T*)w + (size_t)e.x * U;
        for (int u = l; u < U; u += G) dst[u] = src[u];
      }
      if (state_mode == 2) {
        T* dst = (T*)s + (size_t)e.x * U;
        if (kept) {
          const T* src = (const T*)old_s + (size_t)e.y * U;
          for (int u = l; u < U; u += G) dst[u] = src[u];
        } else {
          for (int u = l; u < U; u += G) dst[u] = T{};
        }
      } else if (state_mode == 1 && l == 0) {
        s[e.x] = kept ? old_s[e.y] : 0.f;
      }
    }
    __syncthreads();  // (the next tile writes list / wcnt)
  }
}

static bool ranges_overlap(const void* a, const void* b, size_t bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + bytes && y < x + bytes;
}

}  // namespace ttx

using namespace ttx;

extern "C" {

int ttx_cache_carry(int64_t H, const int64_t* hashtbl, const int32_t* old_state, const int32_t* cache_state, int64_t cache_size,
                    int32_t D, const float* old_weight, float* cache_weight, int32_t state_width, const float* old_opt_state,
                    float* opt_state, ttx_stream_t stream) {
  const char* what = "cache_carry";
  if (H <= 0 || H >= (1ll << 31)) TTX_FAIL(TTX_EINVAL, "%s: hashtbl_size=%lld must be in (0, 2^31)", what, (long long)H);
  if (cache_size < 0 || cache_size > H) TTX_FAIL(TTX_EINVAL, "%s: cache_size=%lld must be in [0, hashtbl_size]", what, (long long)cache_size);
  if (D <= 0) TTX_FAIL(TTX_EINVAL, "%s: D=%d must be > 0", what, D);
  if (state_width != 0 && state_width != 1 && state_width != D)
    TTX_FAIL(TTX_EINVAL, "%s: state_width=%d must be 0, 1 or D=%d", what, state_width, D);
  if (((uintptr_t)hashtbl) & 7) TTX_FAIL(TTX_EINVAL, "%s: hashtbl must be 8-byte aligned", what);
  if ((((uintptr_t)old_state) | ((uintptr_t)cache_state) | ((uintptr_t)old_weight) | ((uintptr_t)cache_weight) |
       ((uintptr_t)old_opt_state) | ((uintptr_t)opt_state)) & 3)
    TTX_FAIL(TTX_EINVAL, "%s: int32 / float pointers must be 4-byte aligned", what);
  if (cache_size == 0) return TTX_OK;
  if (!hashtbl || !old_state || !cache_state || !old_weight || !cache_weight) TTX_FAIL(TTX_EINVAL, "%s: NULL input / output", what);
  if (state_width != 0 && (!old_opt_state || !opt_state)) TTX_FAIL(TTX_EINVAL, "%s: state_width=%d needs both state arrays", what, state_width);
  const size_t wbytes = (size_t)cache_size * (size_t)D * 4, sbytes = (size_t)cache_size * (size_t)state_width * 4;
  if (ranges_overlap(old_weight, cache_weight, wbytes))
    TTX_FAIL(TTX_EINVAL, "%s: old_weight overlaps cache_weight (the move is a permutation: not in place)", what);
  if (state_width != 0 && ranges_overlap(old_opt_state, opt_state, sbytes))
    TTX_FAIL(TTX_EINVAL, "%s: old_opt_state overlaps opt_state (the move is a permutation: not in place)", what);
  const int mode = state_width == 0 ? 0 : (state_width == D ? 2 : 1);  // (D == 1: one float per row either way)
  uintptr_t al = (uintptr_t)old_weight | (uintptr_t)cache_weight;
  if (mode == 2) al |= (uintptr_t)old_opt_state | (uintptr_t)opt_state;
  const bool vec = D % 4 == 0 && (al & 15) == 0;
  const int U = vec ? D / 4 : D;
  int lg = 0;
  while (lg < 6 && (1 << lg) < U) ++lg;  // lanes per row: the power of two that covers U, at most a wave
  const int ntiles = (int)((H + kCC - 1) / kCC);
  const dim3 grid((unsigned)(ntiles < 2048 ? ntiles : 2048)), block(kCC);
  hipStream_t st = (hipStream_t)stream;
  if (vec)
    hipLaunchKernelGGL(cache_carry_kernel<true>, grid, block, 0, st, (int32_t)H, ntiles, hashtbl, old_state, cache_state,
                       (int32_t)cache_size, U, lg, old_weight, cache_weight, mode, old_opt_state, opt_state);
  else
    hipLaunchKernelGGL(cache_carry_kernel<false>, grid, block, 0, st, (int32_t)H, ntiles, hashtbl, old_state, cache_state,
                       (int32_t)cache_size, U, lg, old_weight, cache_weight, mode, old_opt_state, opt_state);
  TTX_HIP(hipGetLastError());
  return TTX_OK;
}

}  // extern "C"

// ttx_pad.hip -- padded bags -> ragged bags plus a live count (nn.EmbeddingBag's padding_idx; not in the reference).
//
// ttx_bags_compact is a stable stream compaction by flag (slot i is live iff indices[i] != padding_idx) that also carries the
// bag starts along: out_indices = the live slots in their original order with a zero tail, out_offsets[b] = live slots in
// front of bag b, *n_live = their number.  The scan is the one of the cache partition (ttx_cache.hip, partition_scatter_kernel):
// wave ballots and popcounts for the ranks inside a wave, a work-group's wave totals through LDS, tile totals through global
// memory across a LAUNCH boundary.  No atomics, no work-group waits on another one, every output element has exactly one
// writer (no memset in front): bit-identical from run to run, nothing read back, capturable.
//
// A tile is what one work-group of kPadThreads threads compacts: kPadWaves waves with `cpw` chunks of 64 V slots each (V = 2:
// 16-byte loads of two indices per lane when the pointer allows, else V = 1), wave w owning a contiguous run of the tile.  A
// wave walks its run twice -- once to count, once (now out of L2) to rank and scatter -- so nothing but counters lives in
// registers whatever cpw is.
//   nnz <= kPadOneLaunch:  ONE launch (pad_small_kernel).  One work-group's pass over the batch is cheap in bytes but a single
//                          compute unit moves them slowly (measured: 15 us for 20,480 slots, against 5 to 8 us for the
//                          launches of the tiled route), so the launch has a work-group per 1024 V slots and EVERY one of
//                          them builds the rank table of the WHOLE batch in LDS -- a ballot mask and a prefix per 64 slots,
//                          6 KiB at most -- from its own pass over the indices (out of L2: at most 256 KiB each).  With the
//                          table a work-group knows the destination of any slot: it scatters its own slots, writes its part
//                          of the zero tail and the offsets of its share of the bags, without a word from another one.
//   above:                 launch 1 counts every tile (tiles of >= 4096 slots, at most 1024 of them), launch 2 has every
//                          work-group add up the totals in front of its tile (<= 1024 ints), rank, scatter, write the
//                          destination of every slot and its part of the zero tail.  The 2-D form's bag starts are known
//                          per tile and are written by launch 2; offsets given as an array are gathered by a third launch.
#include "ttx_internal.h"

namespace ttx {

constexpr int kPadWaves = 16;
constexpr int kPadThreads = kPadWaves * kWave;         // 1024
constexpr long long kPadOneLaunch = 32768;             // slots one work-group takes in one launch (32 chunks of 64 per wave)
constexpr int kPadMaxTiles = 1024;                     // tile totals one work-group sums with one load per thread
constexpr int kPadMinCpw = 4;                          // chunks of 64 per wave in the tiled route: tiles of 4096 slots and up
constexpr int kPadBatch = 8;                           // chunks a wave of the one-launch route has in flight together

// flags and values of the V slots of this lane in the chunk at `i0` (the lane's first slot)
template <int V>
__device__ __forceinline__ void pad_load(const int64_t* __restrict__ indices, long long i0, long long end, int64_t pad,
                                         int64_t (&v)[V], bool (&f)[V]) {
  if constexpr (V == 2) {
    if (i0 + 1 < end) {
      const longlong2 t = *(const longlong2*)(indices + i0);
      v[0] = t.x; v[1] = t.y;
    } else {
      v[0] = i0 < end ? indices[i0] : pad;
      v[1] = pad;
    }
    f[0] = i0 < end && v[0] != pad;
    f[1] = i0 + 1 < end && v[1] != pad;
  } else {
    v[0] = i0 < end ? indices[i0] : pad;
    f[0] = i0 < end && v[0] != pad;
  }
}

// live slots of the wave's run [w0, w1)
template <int V>
__device__ __forceinline__ int pad_count_run(const int64_t* __restrict__ indices, long long w0, long long w1, int64_t pad) {
  int cnt = 0;
#pragma unroll 4
  for (long long c0 = w0; c0 < w1; c0 += kWave * V) {
    int64_t v[V];
    bool f[V];
    pad_load<V>(indices, c0 + (long long)lane_id() * V, w1, pad, v, f);
#pragma unroll
    for (int k = 0; k < V; ++k) cnt += __popcll(__ballot(f[k]));
  }
  return cnt;  // (wave-uniform)
}

// launch 1 of the tiled route: totals[tile] = live slots of the tile
template <int V>
__global__ __launch_bounds__(kPadThreads) void pad_count_kernel(long long nnz, int cpw, const int64_t* __restrict__ indices,
                                                                int64_t pad, int* __restrict__ totals) {
  __shared__ int wsum[kPadWaves];
  const int w = threadIdx.x / kWave;
  const long long run = (long long)cpw * kWave * V, t0 = (long long)blockIdx.x * run * kPadWaves;
  const long long w0 = min(nnz, t0 + w * run), w1 = min(nnz, w0 + run);
  const int cnt = pad_count_run<V>(indices, w0, w1, pad);
  if (lane_id() == 0) wsum[w] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int s = 0;
#pragma unroll
    for (int k = 0; k < kPadWaves; ++k) s += wsum[k];
    totals[blockIdx.x] = s;
  }
}

// The compaction of one tile of the tiled route.  totals == NULL: the only tile.  L > 0: bag b starts at slot b L and this
// work-group writes the out_offsets of the bags that start in its tile (else: pad_offsets_kernel, from dest).  dest [nnz + 1]
// int32: dest[i] = live slots in front of i.
template <int V>
__global__ __launch_bounds__(kPadThreads) void pad_compact_kernel(long long nnz, long long nb, int cpw,
                                                                  const int64_t* __restrict__ indices,
                                                                  long long L,
                                                                  int64_t pad, const int* __restrict__ totals,
                                                                  int64_t* __restrict__ out_indices, int64_t* out_offsets,
                                                                  int32_t* __restrict__ n_live, int* __restrict__ dest) {
  __shared__ int wsum[kPadWaves], red[2][kPadWaves];
  const int tid = threadIdx.x, lane = lane_id(), w = tid / kWave;
  const long long run = (long long)cpw * kWave * V, t0 = (long long)blockIdx.x * run * kPadWaves;
  const long long t1 = min(nnz, t0 + run * kPadWaves);
  const long long w0 = min(nnz, t0 + w * run), w1 = min(nnz, w0 + run);
  // the totals in front of this tile and of the whole batch (<= kPadMaxTiles of them: one load per thread)
  int before = 0, all = 0;
  if (totals) {
    const int nt = gridDim.x;
    const int v = tid < nt ? totals[tid] : 0;
    before = tid < (int)blockIdx.x ? v : 0;
    all = v;
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
      before += __shfl_xor(before, o, kWave);
      all += __shfl_xor(all, o, kWave);
    }
  }
  const int cnt = pad_count_run<V>(indices, w0, w1, pad);
  if (lane == 0) { wsum[w] = cnt; red[0][w] = before; red[1][w] = all; }
  __syncthreads();
  int base = 0, n = 0, own = 0;  // live slots in front of this wave's run, of the batch, of this tile
#pragma unroll
  for (int k = 0; k < kPadWaves; ++k) {
    base += red[0][k] + (k < w ? wsum[k] : 0);
    n += red[1][k];
    own += wsum[k];
  }
  if (!totals) n = own;
  // rank and scatter (the second walk: the run comes out of L2)
  for (long long c0 = w0; c0 < w1; c0 += kWave * V) {
    const long long i0 = c0 + (long long)lane * V;
    int64_t v[V];
    bool f[V];
    pad_load<V>(indices, i0, w1, pad, v, f);
    unsigned long long m[V];
    int r = base;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      m[k] = __ballot(f[k]);
      r += __popcll(m[k] & lanemask_lt());
    }
    int d[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      d[k] = r;
      if (f[k]) out_indices[r] = v[k];
      r += f[k] ? 1 : 0;
      base += __popcll(m[k]);
    }
    if constexpr (V == 2) {
      if (i0 + 1 < w1) *(int2*)(dest + i0) = make_int2(d[0], d[1]);  // (i0 is even: the tile and run starts are)
      else if (i0 < w1) dest[i0] = d[0];
    } else {
      if (i0 < w1) dest[i0] = d[0];
    }
  }
  // this tile's part of the zero tail [n, nnz)
  for (long long i = max((long long)n, t0) + tid; i < t1; i += kPadThreads) out_indices[i] = 0;
  if (t1 == nnz && tid == 0) {  // (the last tile: the closing entries)
    dest[nnz] = n;
    out_offsets[nb] = n;
    *n_live = n;
  }
  if (L > 0) {
    __syncthreads();  // the destinations above are read by other waves of this work-group
    const long long b0 = (t0 + L - 1) / L, b1 = min(nb, (t1 + L - 1) / L);
    for (long long b = b0 + tid; b < b1; b += kPadThreads) out_offsets[b] = dest[b * L];
  }
}

// The one-launch route: see the head of the file.  Chunk g = slots [g 64 V, (g + 1) 64 V); mask[g V + k] bit l = slot
// g 64 V + l V + k is live; pre[g] = live slots in front of chunk g.  L > 0: bag b starts at slot b L; else offsets [nb + 1].
template <int V>
__global__ __launch_bounds__(kPadThreads) void pad_small_kernel(int nnz, int nb, const int64_t* __restrict__ indices,
                                                                const int64_t* __restrict__ offsets, int L, int64_t pad,
                                                                int64_t* __restrict__ out_indices,
                                                                int64_t* __restrict__ out_offsets, int32_t* __restrict__ n_live) {
  constexpr int kMaxG = (int)(kPadOneLaunch / kWave);  // chunks of 64 slots in the largest batch of this route
  constexpr int CS = kWave * V;
  __shared__ unsigned long long mask[kMaxG];
  __shared__ int pre[kMaxG];
  __shared__ int wt[kPadWaves];
  const int tid = threadIdx.x, lane = lane_id(), w = tid / kWave;
  const int G = (nnz + CS - 1) / CS;
  // the table of the whole batch: wave w takes chunks w, w + 16, ..., kPadBatch of them in flight
  for (int g0 = w; g0 < G; g0 += kPadWaves * kPadBatch) {
    bool f[kPadBatch][V];
#pragma unroll
    for (int u = 0; u < kPadBatch; ++u) {
      int64_t v[V];
      const int g = g0 + u * kPadWaves;
      pad_load<V>(indices, g < G ? (long long)g * CS + lane * V : (long long)nnz, nnz, pad, v, f[u]);
    }
#pragma unroll
    for (int u = 0; u < kPadBatch; ++u) {
      const int g = g0 + u * kPadWaves;
      int c = 0;
#pragma unroll
      for (int k = 0; k < V; ++k) {
        const unsigned long long m = __ballot(f[u][k]);
        c += __popcll(m);
        if (lane == 0 && g < G) mask[g * V + k] = m;
      }
      if (lane == 0 && g < G) pre[g] = c;
    }
  }
  __syncthreads();
  {  // exclusive scan of the chunk counts (G <= 512: one per thread)
    const int c = tid < G ? pre[tid] : 0;
    const int inc = wave_incl_scan(c);
    if (lane == kWave - 1) wt[w] = inc;
    __syncthreads();
    int run = 0;
    for (int k = 0; k < w; ++k) run += wt[k];
    if (tid < G) pre[tid] = run + inc - c;
  }
  __syncthreads();
  int n = 0;
#pragma unroll
  for (int k = 0; k < kPadWaves; ++k) n += wt[k];
  auto rank = [&](int s) -> int {  // live slots in front of slot s
    if (s >= nnz) return n;
    const int g = s / CS, j = s - g * CS, ln = j / V;
    const unsigned long long lt = (1ull << ln) - 1ull;
    int r = pre[g];
#pragma unroll
    for (int k = 0; k < V; ++k) r += __popcll(mask[g * V + k] & lt);
    if (V == 2 && (j & 1)) r += (int)((mask[g * V] >> ln) & 1ull);
    return r;
  };
  // this work-group's slots: chunk blockIdx.x 16 + w (out of L1 / L2 now)
  const int t0 = min(nnz, (int)blockIdx.x * kPadWaves * CS), t1 = min(nnz, t0 + kPadWaves * CS);
  {
    const int i0 = t0 + w * CS + lane * V;
    int64_t v[V];
    bool f[V];
    pad_load<V>(indices, i0, nnz, pad, v, f);
    int r = rank(i0);
#pragma unroll
    for (int k = 0; k < V; ++k) {
      if (f[k]) out_indices[r] = v[k];
      r += f[k] ? 1 : 0;
    }
  }
  for (int i = max(n, t0) + tid; i < t1; i += kPadThreads) out_indices[i] = 0;  // its part of the zero tail [n, nnz)
  if (L > 0) {  // the bags that start in its slots
    const int b0 = (t0 + L - 1) / L, b1 = min(nb, (t1 + L - 1) / L);
    for (int b = b0 + tid; b < b1; b += kPadThreads) out_offsets[b] = rank(b * L);
  } else {      // its share of the bags
    const int per = (nb + (int)gridDim.x - 1) / (int)gridDim.x;
    const int b1 = min(nb, ((int)blockIdx.x + 1) * per);
    for (int b = (int)blockIdx.x * per + tid; b < b1; b += kPadThreads) {
      const long long s = offsets[b];
      out_offsets[b] = rank(s < 0 ? 0 : (s > nnz ? nnz : (int)s));
    }
  }
  if (blockIdx.x == gridDim.x - 1 && tid == 0) {
    out_offsets[nb] = n;
    *n_live = n;
  }
}

// launch 3 of the tiled route with offsets given as an array: out_offsets[b] = destination of bag b's first slot
__global__ __launch_bounds__(256) void pad_offsets_kernel(long long nb, long long nnz, const int64_t* __restrict__ offsets,
                                                          const int* __restrict__ dest, int64_t* __restrict__ out_offsets) {
  for (long long b = (long long)blockIdx.x * 256 + threadIdx.x; b < nb; b += (long long)gridDim.x * 256) {
    long long s = offsets[b];
    s = s < 0 ? 0 : (s > nnz ? nnz : s);
    out_offsets[b] = dest[s];
  }
}

// chunks of 64 V slots per wave and the number of tiles of a batch
static void pad_tiling(long long nnz, int V, int* cpw, long long* tiles) {
  const long long per = (long long)kPadThreads * V;  // slots of a tile per chunk
  long long c;
  if (nnz <= kPadOneLaunch) {
    c = (nnz + per - 1) / per;
  } else {
    c = (nnz + per * kPadMaxTiles - 1) / (per * kPadMaxTiles);
    if (c < kPadMinCpw / V) c = kPadMinCpw / V;
  }
  if (c < 1) c = 1;
  *cpw = (int)c;
  *tiles = (nnz + per * c - 1) / (per * c);
}

static size_t pad_dest_bytes(long long nnz) { return align_up((size_t)(nnz + 1) * sizeof(int)); }

}  // namespace ttx

using namespace ttx;

extern "C" {

size_t ttx_bags_compact_workspace_bytes(int64_t nb, int64_t nnz) {
  (void)nb;
  if (nnz < 0 || nnz >= (1ll << 31)) return 0;
  return pad_dest_bytes(nnz) + align_up((size_t)kPadMaxTiles * sizeof(int));
}

int ttx_bags_compact(int64_t nb, int64_t nnz, const int64_t* indices, const int64_t* offsets, int64_t L, int64_t padding_idx,
                     int64_t* out_indices, int64_t* out_offsets, int32_t* n_live, void* workspace, size_t workspace_bytes,
                     ttx_stream_t stream) {
  if (nb < 0 || nnz < 0 || nnz >= (1ll << 31)) TTX_FAIL(TTX_EINVAL, "bags_compact: bad nb / nnz");
  if (!offsets && (L < 0 || (L > 0 && nb > nnz / L) || nb * L != nnz))
    TTX_FAIL(TTX_EINVAL, "bags_compact: without offsets the batch is nb bags of L slots (nnz == nb * L)");
  hipStream_t st = (hipStream_t)stream;
  if (nnz == 0 || nb == 0) {  // nothing to compact: zero offsets and a zero count, where the caller has buffers for them
    if (out_offsets) TTX_HIP(hipMemsetAsync(out_offsets, 0, (size_t)(nb + 1) * sizeof(int64_t), st));
    if (n_live) TTX_HIP(hipMemsetAsync(n_live, 0, sizeof(int32_t), st));
    return TTX_OK;
  }
  if (!indices || !out_indices || !out_offsets || !n_live) TTX_FAIL(TTX_EINVAL, "bags_compact: NULL input / output");
  if (!workspace || workspace_bytes < ttx_bags_compact_workspace_bytes(nb, nnz))
    TTX_FAIL(TTX_EINVAL, "bags_compact: workspace too small (ttx_bags_compact_workspace_bytes)");
  if (((uintptr_t)workspace) & 7) TTX_FAIL(TTX_EINVAL, "bags_compact: workspace must be 8-byte aligned");
  int* dest = (int*)workspace;
  int* totals = (int*)((char*)workspace + pad_dest_bytes(nnz));
  const bool v2 = (((uintptr_t)indices) & 15) == 0;
  int cpw;
  long long tiles;
  pad_tiling(nnz, v2 ? 2 : 1, &cpw, &tiles);
  const long long Lk = offsets ? 0 : L;
  if (nnz <= kPadOneLaunch && nb <= kPadOneLaunch) {  // (far more bags than slots: the tiled route's offsets gather)
    const int per = kPadThreads * (v2 ? 2 : 1);
    const unsigned grid = (unsigned)((nnz + per - 1) / per);
    if (v2)
      hipLaunchKernelGGL(pad_small_kernel<2>, dim3(grid), dim3(kPadThreads), 0, st, (int)nnz, (int)nb, indices, offsets, (int)Lk,
                         padding_idx, out_indices, out_offsets, n_live);
    else
      hipLaunchKernelGGL(pad_small_kernel<1>, dim3(grid), dim3(kPadThreads), 0, st, (int)nnz, (int)nb, indices, offsets, (int)Lk,
                         padding_idx, out_indices, out_offsets, n_live);
    TTX_HIP(hipGetLastError());
    return TTX_OK;
  }
  const bool one = tiles == 1;
  if (!one) {
    if (v2) hipLaunchKernelGGL(pad_count_kernel<2>, dim3((unsigned)tiles), dim3(kPadThreads), 0, st, (long long)nnz, cpw, indices,
                               padding_idx, totals);
    else hipLaunchKernelGGL(pad_count_kernel<1>, dim3((unsigned)tiles), dim3(kPadThreads), 0, st, (long long)nnz, cpw, indices,
                            padding_idx, totals);
    TTX_HIP(hipGetLastError());
  }
  if (v2)
    hipLaunchKernelGGL(pad_compact_kernel<2>, dim3((unsigned)tiles), dim3(kPadThreads), 0, st, (long long)nnz, (long long)nb, cpw,
                       indices, Lk, padding_idx, one ? nullptr : totals, out_indices, out_offsets, n_live, dest);
  else
    hipLaunchKernelGGL(pad_compact_kernel<1>, dim3((unsigned)tiles), dim3(kPadThreads), 0, st, (long long)nnz, (long long)nb, cpw,
                       indices, Lk, padding_idx, one ? nullptr : totals, out_indices, out_offsets, n_live, dest);
  TTX_HIP(hipGetLastError());
  if (offsets) {
    const long long blocks = (nb + 255) / 256;
    hipLaunchKernelGGL(pad_offsets_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, st, (long long)nb,
                       (long long)nnz, offsets, dest, out_offsets);
    TTX_HIP(hipGetLastError());
  }
  return TTX_OK;
}

}  // extern "C"

// ttx_merge.hip -- per-table bags -> the table-major batch of a table-batched lookup (not in the reference).
//
// ttx_bags_merge concatenates the (indices, bags[, weights]) of the tables of one group into the batch that
// TableBatchedTTEmbeddingBag.forward takes: table k's slots at base_k = sum_{j<k} nnz_j, its bag starts shifted by base_k, int32
// inputs widened, absent weights filled with 1.0f and every slot that holds table k's padding value rewritten to one sentinel.
// Everything a table contributes -- four pointers-or-values, a prefix sum, a bag length, a flag byte -- travels BY VALUE in the
// kernel's argument block (MergeArgs, below 4 KiB for TTX_MAX_TABLES_MIXED tables): no pointer table is copied to the device,
// so the call never synchronises and is capturable.  More tables than that: one launch per TTX_MAX_TABLES_MIXED of them, each
// told where its slots and its bag rows start; the last one writes the closing offset.
//
// One grid, three block ranges:
//   [0, slot_blocks)      1024 output slots each.  Output slots are taken in PAIRS that are 16-byte aligned in out_indices, so a
//                         pair inside one table goes out as one 16-byte store; it comes in as one 16-byte load when the table is
//                         int64 and its source pair is 16-byte aligned too (an odd base_k shifts the source by one slot: two 8-byte
//                         loads then), as two 4-byte loads when the table is int32.  A work-group finds the table of its first slot
//                         by a search over the prefix sums in the arguments and walks on from there -- block-uniform, scalar loads.
//   [.., + ntab * bpt)    the bag starts: bpt = ceil(B / 256) blocks per table, one entry per thread.
//   the last one          the closing offset (only in the launch that owes it).
// Every output element has exactly one writer; no atomics, no memset in front, no workspace, no work-group waits on another.
#include "ttx_internal.h"

namespace ttx {

constexpr int kMergeThreads = 256;
constexpr int kMergePairs = 2;                                    // 16-byte pairs per thread
constexpr int kMergeTile = kMergeThreads * kMergePairs * 2;       // output slots per work-group
constexpr int kMergeI32 = 1, kMergeO32 = 2, kMergePad = 4;        // MergeArgs::flags

struct MergeArgs {
  const void* idx[TTX_MAX_TABLES_MIXED];    // int64 or int32 (kMergeI32), pre[k + 1] - pre[k] of them
  const void* bags[TTX_MAX_TABLES_MIXED];   // bag starts, int64 or int32 (kMergeO32); NULL: bag b starts at b * L[k]
  const float* w[TTX_MAX_TABLES_MIXED];     // NULL: 1.0f
  int64_t pad[TTX_MAX_TABLES_MIXED];        // the padding value (kMergePad)
  int pre[TTX_MAX_TABLES_MIXED + 1];        // slots of this launch in front of table k
  int L[TTX_MAX_TABLES_MIXED];
  unsigned char flags[TTX_MAX_TABLES_MIXED];
};
// the kernel-argument segment: 4 KiB is what every HIP runtime takes; MergeArgs plus the scalars below stay under it
static_assert(sizeof(MergeArgs) + 96 <= 4096, "TTX_MAX_TABLES_MIXED tables must fit one kernel-argument segment: lower the per-launch bound");

// ntab tables of this launch; base / row0: output slot / bag row of its first table; shift = 1 iff out_indices + base is 8 bytes
// past a 16-byte boundary (pairs then start one slot early); close_at >= 0: out_offsets[close_at] = total is this launch's too
__global__ __launch_bounds__(kMergeThreads) void merge_bags_kernel(const MergeArgs A, int ntab, long long B, int bpt, int slot_blocks,
                                                                   long long base, long long row0, int shift, int64_t sentinel,
                                                                   long long close_at, long long total,
                                                                   int64_t* __restrict__ out_indices,
                                                                   int64_t* __restrict__ out_offsets,
                                                                   float* __restrict__ out_weights) {
  const int tid = threadIdx.x;
  const int blk = blockIdx.x;
  if (blk < slot_blocks) {
    const int n = A.pre[ntab];
    // slots [lo, hi) of this launch; slot i sits at virtual position i + shift, pairs start at even positions
    const long long v0 = (long long)blk * kMergeTile;
    const int lo = (int)max(0ll, v0 - shift), hi = (int)min((long long)n, v0 + kMergeTile - shift);
    int k = 0;
    for (int step = TTX_MAX_TABLES_MIXED / 2; step > 0; step >>= 1)  // the last table that starts at or in front of lo
      if (k + step < ntab && A.pre[k + step] <= lo) k += step;
    for (; k < ntab && A.pre[k] < hi; ++k) {
      const int t0 = A.pre[k], t1 = A.pre[k + 1];
      if (t1 <= lo || t1 == t0) continue;
      const int flags = A.flags[k];
      const bool i32 = flags & kMergeI32, padded = flags & kMergePad;
      const int64_t pad = A.pad[k];
      const int64_t* s64 = (const int64_t*)A.idx[k];
      const int32_t* s32 = (const int32_t*)A.idx[k];
      const float* w = A.w[k];
      const int a = max(lo, t0), b = min(hi, t1);
#pragma unroll
      for (int u = 0; u < kMergePairs; ++u) {
        const long long i0 = v0 + 2 * (u * kMergeThreads + tid) - shift;  // this thread's pair: slots i0, i0 + 1
        const bool in0 = i0 >= a && i0 < b, in1 = i0 + 1 >= a && i0 + 1 < b;
        if (!in0 && !in1) continue;
        const long long s = i0 - t0;  // source slot of i0
        int64_t x0 = 0, x1 = 0;
        if (i32) {
          if (in0) x0 = s32[s];
          if (in1) x1 = s32[s + 1];
        } else if (in0 && in1 && (((uintptr_t)(s64 + s)) & 15) == 0) {
          const longlong2 t = *(const longlong2*)(s64 + s);
          x0 = t.x; x1 = t.y;
        } else {
          if (in0) x0 = s64[s];
          if (in1) x1 = s64[s + 1];
        }
        if (padded) {
          x0 = x0 == pad ? sentinel : x0;
          x1 = x1 == pad ? sentinel : x1;
        }
        int64_t* dst = out_indices + base + i0;
        if (in0 && in1) *(longlong2*)dst = make_longlong2(x0, x1);
        else if (in0) dst[0] = x0;
        else dst[1] = x1;
        if (out_weights) {
          if (in0) out_weights[base + i0] = w ? w[s] : 1.0f;
          if (in1) out_weights[base + i0 + 1] = w ? w[s + 1] : 1.0f;
        }
      }
    }
    return;
  }
  const int ob = blk - slot_blocks;
  if (bpt > 0 && ob < ntab * bpt) {
    const int k = ob / bpt;
    const long long b = (long long)(ob - k * bpt) * kMergeThreads + tid;
    if (b >= B) return;
    const long long nnz = A.pre[k + 1] - A.pre[k];
    const void* bags = A.bags[k];
    long long s;
    if (!bags) s = b * A.L[k];
    else if (A.flags[k] & kMergeO32) s = ((const int32_t*)bags)[b];
    else s = ((const int64_t*)bags)[b];
    s = s < 0 ? 0 : (s > nnz ? nnz : s);
    out_offsets[row0 + (long long)k * B + b] = base + A.pre[k] + s;
    return;
  }
  if (tid == 0 && close_at >= 0) out_offsets[close_at] = total;
}

}  // namespace ttx

using namespace ttx;

extern "C" {

int ttx_bags_merge(int32_t ntab, int64_t B, int32_t include_last_offset, const void* const* indices, const int64_t* nnz,
                   const int32_t* index_bytes, const void* const* offsets, const int32_t* offset_bytes, const int64_t* L,
                   const float* const* weights, const int64_t* padding, const uint8_t* has_padding, int64_t sentinel,
                   int64_t* out_indices, int64_t* out_offsets, float* out_weights, ttx_stream_t stream) {
  (void)include_last_offset;  // (B bag starts are read per table either way: a closing entry behind them is not looked at)
  if (ntab < 1) TTX_FAIL(TTX_EINVAL, "bags_merge: ntab must be >= 1, got %d", ntab);
  if (B < 0) TTX_FAIL(TTX_EINVAL, "bags_merge: negative B");
  if (!indices || !nnz || !offsets || !L) TTX_FAIL(TTX_EINVAL, "bags_merge: NULL per-table array (indices / nnz / offsets / L)");
  if (padding && !has_padding) TTX_FAIL(TTX_EINVAL, "bags_merge: padding values without has_padding");
  long long N = 0;
  for (int k = 0; k < ntab; ++k) {
    if (nnz[k] < 0) TTX_FAIL(TTX_EINVAL, "bags_merge: table %d: negative nnz", k);
    N += nnz[k];
    if (N >= (1ll << 31)) TTX_FAIL(TTX_EINVAL, "bags_merge: the merged batch must hold fewer than 2^31 slots");
    const int ib = index_bytes ? index_bytes[k] : 8, ob = offset_bytes ? offset_bytes[k] : 8;
    if ((ib != 4 && ib != 8) || (ob != 4 && ob != 8)) TTX_FAIL(TTX_EINVAL, "bags_merge: table %d: element widths are 4 or 8 bytes", k);
    if (nnz[k] > 0 && !indices[k]) TTX_FAIL(TTX_EINVAL, "bags_merge: table %d: NULL indices", k);
    if (((uintptr_t)indices[k]) & (ib - 1)) TTX_FAIL(TTX_EINVAL, "bags_merge: table %d: indices not aligned to their element", k);
    if (offsets[k]) {
      if (((uintptr_t)offsets[k]) & (ob - 1)) TTX_FAIL(TTX_EINVAL, "bags_merge: table %d: offsets not aligned to their element", k);
    } else if (L[k] < 0 || (L[k] > 0 && B > nnz[k] / L[k]) || B * L[k] != nnz[k]) {
      TTX_FAIL(TTX_EINVAL, "bags_merge: table %d: without offsets the table is B bags of L slots (nnz == B * L)", k);
    }
    if (weights && weights[k] && (((uintptr_t)weights[k]) & 3)) TTX_FAIL(TTX_EINVAL, "bags_merge: table %d: weights not 4-byte aligned", k);
  }
  if (B > 0 && (long long)ntab > ((1ll << 62) / B)) TTX_FAIL(TTX_EINVAL, "bags_merge: ntab * B overflows");
  if (!out_offsets) TTX_FAIL(TTX_EINVAL, "bags_merge: NULL out_offsets");
  if (N > 0 && !out_indices) TTX_FAIL(TTX_EINVAL, "bags_merge: NULL out_indices");
  if (N > 0 && weights && !out_weights) TTX_FAIL(TTX_EINVAL, "bags_merge: NULL out_weights");
  if ((((uintptr_t)out_indices) & 7) || (((uintptr_t)out_offsets) & 7) || (((uintptr_t)out_weights) & 3))
    TTX_FAIL(TTX_EINVAL, "bags_merge: outputs not aligned to their element");
  const long long bpt = (B + kMergeThreads - 1) / kMergeThreads;
  if (bpt * TTX_MAX_TABLES_MIXED + (1ll << 21) + 1 >= (1ll << 31)) TTX_FAIL(TTX_EINVAL, "bags_merge: too many bags per table");
  hipStream_t st = (hipStream_t)stream;
  long long base = 0;
  for (int k0 = 0; k0 < ntab; k0 += TTX_MAX_TABLES_MIXED) {
    const int nt = ntab - k0 < TTX_MAX_TABLES_MIXED ? ntab - k0 : TTX_MAX_TABLES_MIXED;
    MergeArgs A;
    memset(&A, 0, sizeof(A));
    int n = 0;
    for (int j = 0; j < nt; ++j) {
      const int k = k0 + j;
      A.idx[j] = indices[k];
      A.bags[j] = offsets[k];
      A.w[j] = weights ? weights[k] : nullptr;
      A.pre[j] = n;
      A.L[j] = offsets[k] ? 0 : (int)L[k];
      const bool padded = padding && has_padding[k];
      A.pad[j] = padded ? padding[k] : 0;
      A.flags[j] = (unsigned char)(((index_bytes && index_bytes[k] == 4) ? kMergeI32 : 0) |
                                   ((offset_bytes && offset_bytes[k] == 4) ? kMergeO32 : 0) | (padded ? kMergePad : 0));
      n += (int)nnz[k];
    }
    for (int j = nt; j <= TTX_MAX_TABLES_MIXED; ++j) A.pre[j] = n;
    const int shift = n > 0 ? (int)((((uintptr_t)(out_indices + base)) >> 3) & 1) : 0;
    const int slot_blocks = (int)(((long long)n + shift + kMergeTile - 1) / kMergeTile);
    const bool last = k0 + nt == ntab;
    const long long blocks = slot_blocks + (long long)nt * bpt + (last ? 1 : 0);
    if (blocks > 0) {
      hipLaunchKernelGGL(merge_bags_kernel, dim3((unsigned)blocks), dim3(kMergeThreads), 0, st, A, nt, (long long)B, (int)bpt, slot_blocks,
                         base, (long long)k0 * B, shift, sentinel, last ? (long long)ntab * B : -1ll, N, out_indices, out_offsets,
                         weights ? out_weights : nullptr);
      TTX_HIP(hipGetLastError());
    }
    base += n;
  }
  return TTX_OK;
}

}  // extern "C"

// ttx_tt_expand.hip -- a RANGE of a three-core TT table's rows, [row_begin, row_end) of one table, expanded to dense fp32 rows
// by one kernel that takes no indices: no plan, no sort, nothing read back.  include/ttx.h "dense rows"; DESIGN.md section 4.22.
//
// Row n = (i0 p1 + i1) p2 + i2: the p2 rows of one (i0, i1) PREFIX share x_0 = core_0[i0] core_1[i1] and are one small GEMM
//   rows[(i2), (a, b), c] = x_0[(a, b), k2] core_2[i2][k2, c]
// A work-group takes one prefix that meets the range, times one block of its i2 (the first and the last prefix of a range are
// partial; with few prefixes a prefix's i2 are spread over several work-groups, each of which recomputes the cheap x_0).  The
// grid is arithmetic on row_begin, row_end and p alone.  Both products run on v_mfma_f32_16x16x4f32, TRANSPOSED, so that a
// lane's four accumulators are contiguous outputs:
//   product 1   x_0^T: M = the core-1 columns (b, k2) with k2 padded to K2p = 16 ceil(r2 / 16), N = a (q0 <= 16 padded to 16),
//               K = k1 in blocks of 4.  A = core_1[i1][k1 = 4 kb + (l >> 4)][(b, k2) = 16 mt + (l & 15)], B = core_0[i0][a = l & 15]
//               [k1], both straight from memory, zero outside the slices.  The waves split the M tiles.  A lane's accumulators
//               are k2 .. k2 + 3 of row (a, b): ONE 16-byte LDS store into X[(a, b)][k2]; the columns [r2, K2p) get the zeros
//               the padded A rows produce.
//   product 2   M = the columns e = (i2 - lo) Q2P + c of the work-group's i2 block (Q2P = 4 ceil(q2 / 4): a 16-row tile packs
//               16 / Q2P rows of the table where q2 is small), N = 16 rows (a, b), K = k2.  B = X: a wave holds the fragments of
//               its NTW N tiles (NTW KB registers) for its whole walk; A = core_2[i2][k2 = 4 kb + (l >> 4)][c] straight from the
//               contiguous core-2 slices, the NEXT tile's fragments requested before this tile's MFMAs.  The waves split the M
//               tiles; where q0 q1 > 16 NTW the walk is repeated per group of NTW N tiles.  A lane holds c .. c + 3 of row
//               (i2, (a, b)): one 16-byte store where q2 % 4 == 0 and `out` is 16-byte aligned, scalar stores otherwise.
// X (fp32): row (a, b) at (a q1 + b) XS floats, XS = K2p + 4, so XS / 4 is odd: the 64 lanes of a
// product-2 fragment read, word (l & 15) XS + (l >> 4) + 4 kb, fall on 64 different banks.
// One writer per element, no atomics: bit-identical from run to run; the launch is capturable.
#include "ttx_internal.h"
#include "ttx_magic.h"

namespace ttx {
namespace {

constexpr int kExThreads = 256;
constexpr int kExWaves = kExThreads / kWave;
constexpr int kExMaxRank = 128;          // r1, r2
constexpr int kExMaxQ2 = 32;
constexpr int kExLdsMax = 64 * 1024;     // x_0 of one prefix
constexpr int kExBlockMax = 1 << 16;     // rows (i2) of a work-group, at most: 32-bit offsets into its core-2 slices, e < 2^21
constexpr int kExTargetWgs = 1024;       // a short range is split until it has about this many work-groups
constexpr int kExMinTiles = 16;          // M tiles of product 2 a split leaves a work-group, at least (4 per wave)
constexpr long long kExLaunchWgs = 1ll << 30;

typedef float f32x4 __attribute__((ext_vector_type(4)));

// everything the kernel needs of a geometry (host-derived; travels by value)
struct ExShape {
  int q0, q1, q2, r1, r2;
  int K2p;   // r2 padded to 16
  int M1;    // q1 K2p: rows of x_0^T
  int N1;    // q1 r2: columns of a core-1 slice
  int Q2P;   // q2 padded to 4
  int R;     // q0 q1: rows (a, b)
  int XS;    // floats between rows of X
  int KB;    // K blocks (of 4) product 2 keeps in registers: 8, 16 or 32
  int NTW;   // N tiles of a wave's walk: 1, 2 or 4
  int NG;    // walks: ceil(ceil(R / 16) / NTW)
  int D;
  int sl[3]; // floats of a slice of core t
  int lds_bytes;
};

// host-only, touches no device.  false: not a shape of this kernel.
bool ex_shape(const ttx_geom* g, ExShape* o) {
  if (!g || g->T != 3 || g->num_tables <= 0 || g->r[0] != 1 || g->r[3] != 1) return false;
  for (int t = 0; t < 3; ++t)
    if (g->q[t] <= 0) return false;
  const int r1 = g->r[1], r2 = g->r[2];
  if (r1 <= 0 || r2 <= 0 || r1 > kExMaxRank || r2 > kExMaxRank) return false;
  if (g->q[0] > 16 || g->q[1] > 64 || g->q[2] > kExMaxQ2) return false;
  ExShape s;
  memset(&s, 0, sizeof(s));
  s.q0 = g->q[0]; s.q1 = g->q[1]; s.q2 = g->q[2]; s.r1 = r1; s.r2 = r2;
  s.K2p = (r2 + 15) / 16 * 16;
  s.M1 = s.q1 * s.K2p;
  s.N1 = s.q1 * r2;
  s.Q2P = (s.q2 + 3) / 4 * 4;
  s.R = s.q0 * s.q1;
  s.XS = s.K2p + 4;
  s.KB = r2 <= 32 ? 8 : (r2 <= 64 ? 16 : 32);
  const int NT = (s.R + 15) / 16;
  s.NTW = NT == 1 ? 1 : (NT == 2 ? 2 : 4);
  s.NG = (NT + s.NTW - 1) / s.NTW;
  s.D = s.R * s.q2;
  s.sl[0] = s.q0 * r1;
  s.sl[1] = r1 * s.N1;
  s.sl[2] = r2 * s.q2;
  s.lds_bytes = s.R * s.XS * 4;
  if (s.lds_bytes > kExLdsMax) return false;
  if (o) *o = s;
  return true;
}

// one launch: the prefixes [first, first + npf) of a range, nsplit work-groups each
struct ExArgs {
  ExShape sh;
  int p1, p2;
  int i0b, i1b;        // (i0, i1) of the launch's first prefix
  int npf;             // prefixes of the launch
  int nsplit, BL;      // work-groups of a prefix; rows (i2) of a work-group
  int i2_first;        // the first prefix starts here ...
  int i2_last_end;     // ... and the last one ends here
  long long row_off;   // row of `out` that (prefix 0 of the launch, i2 = 0) would be
  TableDiv dp1;        // (i1b + prefix) / p1
  TableDiv dq2;        // (e / 4) / (Q2P / 4)
};

// the A fragments of product 2's M tile `tile`: column e = 16 tile + (l & 15) = (i2 - lo) Q2P + c, k2 = 4 kb + (l >> 4); zero
// where the tile, the row i2, the column c or k2 does not exist (nothing is read there)
template <int KB>
__device__ __forceinline__ void load_a2(float (&af)[KB], const float* __restrict__ c2lo, int tile, int ntiles, int nrow,
                                        const ExArgs& A, int li, int lg) {
  const ExShape& sh = A.sh;
  const unsigned e = 16u * (unsigned)tile + li;
  const unsigned dj = table_quot(e >> 2, A.dq2.mul, A.dq2.sh);
  const int c = (int)(e - dj * sh.Q2P);
  const bool ok = tile < ntiles && (int)dj < nrow && c < sh.q2;
  int lim = ok ? sh.r2 - lg : 0;
  asm volatile("" : "+v"(lim));  // (opaque: else the compiler keeps a lane mask per K block, (4 kb < r2 - lg), across the whole walk)
  unsigned off = (ok ? dj * (unsigned)sh.sl[2] + c : 0u) + lg * sh.q2;  // (floats from slice lo: < 2^16 * 2^12 + 2^12)
  const unsigned step = 4u * sh.q2;
#pragma unroll
  for (int kb = 0; kb < KB; ++kb)
    if (16 * (kb / 4) < sh.r2) {  // (uniform, per 4 K blocks: few conditions for the compiler to keep)
      af[kb] = 4 * kb < lim ? c2lo[off] : 0.f;
      off += step;
    }
}

template <int KB, int NTW>
__global__ __launch_bounds__(kExThreads) void tt_expand_kernel(ExArgs A, const float* __restrict__ c0, const float* __restrict__ c1,
                                                               const float* __restrict__ c2, float* __restrict__ out, int vec) {
  extern __shared__ __attribute__((aligned(16))) float X[];  // [R][XS]: x_0 of the prefix
  const ExShape& sh = A.sh;
  const unsigned wg = blockIdx.x;
  const unsigned g = A.nsplit == 1 ? wg : wg / (unsigned)A.nsplit;  // prefix of the launch
  const int s = (int)(wg - g * (unsigned)A.nsplit);
  int lo = s * A.BL;                                                 // (s BL < p2 <= 2^30)
  int hi = A.p2 - lo < A.BL ? A.p2 : lo + A.BL;
  if (g == 0) lo = max(lo, A.i2_first);
  if (g == (unsigned)A.npf - 1) hi = min(hi, A.i2_last_end);
  if (lo >= hi) return;  // (the whole work-group, before any barrier)
  const unsigned j1 = (unsigned)A.i1b + g;                           // (< 2^31: the launch's prefixes)
  const unsigned di0 = table_quot(j1, A.dp1.mul, A.dp1.sh);
  const int i1 = (int)(j1 - di0 * (unsigned)A.p1), i0 = A.i0b + (int)di0;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int li = lane & 15, lg = lane >> 4;

  // ---- product 1: x_0^T tile by tile into X
  {
    const float* c0s = c0 + (size_t)i0 * sh.sl[0];
    const float* c1s = c1 + (size_t)i1 * sh.sl[1];
    const int nm = (sh.M1 + 15) / 16;
    const bool okB = li < sh.q0;
    const float* bp = c0s + (okB ? li : 0) * sh.r1 + lg;
    for (int mt = wave; mt < nm; mt += kExWaves) {
      const int m = 16 * mt + li;
      const int b = m / sh.K2p, k2 = m - b * sh.K2p;
      const bool okA = m < sh.M1 && k2 < sh.r2;
      const float* ap = c1s + (okA ? b * sh.r2 + k2 : 0) + (size_t)lg * sh.N1;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      for (int k0 = 0; k0 < sh.r1; k0 += 16) {
        float av[4], bv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bool in = k0 + 4 * j + lg < sh.r1;
          av[j] = (okA && in) ? ap[(size_t)(k0 + 4 * j) * sh.N1] : 0.f;
          bv[j] = (okB && in) ? bp[k0 + 4 * j] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], bv[j], acc, 0, 0, 0);
      }
      const int ms = 16 * mt + 4 * lg;  // (a multiple of 4, as M1 and K2p are: the four share b, and all exist or none)
      if (okB && ms < sh.M1) {
        const int bs = ms / sh.K2p;
        *(f32x4*)(X + (size_t)(li * sh.q1 + bs) * sh.XS + (ms - bs * sh.K2p)) = acc;
      }
    }
  }
  __syncthreads();  // X is whole

  // ---- product 2: the walk over the M tiles of [lo, hi), once per group of NTW N tiles
  const int ntiles = ((hi - lo) * sh.Q2P + 15) >> 4;  // ((hi - lo) <= 2^16, Q2P <= 32)
  const float* c2lo = c2 + (size_t)lo * sh.sl[2];  // slice lo of core 2
  const long long row0 = A.row_off + (long long)g * A.p2 + lo;
  for (int ng = 0; ng < sh.NG; ++ng) {
    float xf[NTW][KB];
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) {
      const int rho = 16 * (ng * NTW + nt) + li;
      const float* xp = X + (size_t)(rho < sh.R ? rho : 0) * sh.XS + lg;
#pragma unroll
      for (int kb = 0; kb < KB; ++kb)
        if (16 * (kb / 4) < sh.r2)  // (uniform)
          xf[nt][kb] = rho < sh.R ? xp[4 * kb] : 0.f;  // (4 kb + lg < K2p: inside the row)
    }
    float an[KB];
    load_a2<KB>(an, c2lo, wave, ntiles, hi - lo, A, li, lg);
    for (int tile = wave; tile < ntiles; tile += kExWaves) {
      float af[KB];
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) af[kb] = an[kb];
      load_a2<KB>(an, c2lo, tile + kExWaves, ntiles, hi - lo, A, li, lg);  // (travels beside this tile's MFMAs)
      f32x4 acc[NTW];
#pragma unroll
      for (int nt = 0; nt < NTW; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kb = 0; kb < KB; ++kb)
        if (16 * (kb / 4) < sh.r2) {
#pragma unroll
          for (int nt = 0; nt < NTW; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[kb], xf[nt][kb], acc[nt], 0, 0, 0);
        }
      // this lane's four: columns e .. e + 3 = c .. c + 3 of row i2 = lo + dj (e and Q2P multiples of 4: one i2)
      const unsigned e = 16u * (unsigned)tile + 4u * lg;
      const unsigned dj = table_quot(e >> 2, A.dq2.mul, A.dq2.sh);
      const int c = (int)(e - dj * sh.Q2P);
      if (lo + (int)dj < hi && c < sh.q2) {
        float* op = out + (size_t)(row0 + dj) * sh.D + c;
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) {
          const int rho = 16 * (ng * NTW + nt) + li;
          if (rho < sh.R) {
            float* o = op + (size_t)rho * sh.q2;
            if (vec) {  // (q2 % 4 == 0 and `out` 16-byte aligned: D % 4 == 0, the piece is aligned, c + 3 < q2)
              *(f32x4*)o = acc[nt];
            } else {
#pragma unroll
              for (int i = 0; i < 4; ++i)
                if (c + i < sh.q2) o[i] = acc[nt][i];
            }
          }
        }
      }
    }
  }
}

template <int KB, int NTW>
int launch_expand(const ExArgs& A, const float* const* c, float* out, int vec, hipStream_t st) {
  const void* fn = (const void*)tt_expand_kernel<KB, NTW>;
  if (A.sh.lds_bytes > 48 * 1024) {
    const int rc = allow_dynamic_lds(fn, A.sh.lds_bytes);
    if (rc) return rc;
  }
  hipLaunchKernelGGL((tt_expand_kernel<KB, NTW>), dim3((unsigned)((long long)A.npf * A.nsplit)), dim3(kExThreads), A.sh.lds_bytes, st,
                     A, c[0], c[1], c[2], out, vec);
  TTX_HIP(hipGetLastError());
  return TTX_OK;
}

template <int KB>
int launch_expand_nt(const ExArgs& A, const float* const* c, float* out, int vec, hipStream_t st) {
  switch (A.sh.NTW) {
    case 1: return launch_expand<KB, 1>(A, c, out, vec, st);
    case 2: return launch_expand<KB, 2>(A, c, out, vec, st);
    default: return launch_expand<KB, 4>(A, c, out, vec, st);
  }
}

}  // namespace
}  // namespace ttx

using namespace ttx;

extern "C" {

int ttx_tt_expand_supported(const ttx_geom* g) { return ex_shape(g, nullptr) ? 1 : 0; }

int ttx_tt_expand(const ttx_geom* g, int32_t table, int64_t row_begin, int64_t row_end, const float* const* cores, float* out,
                  ttx_stream_t stream) {
  if (!g) TTX_FAIL(TTX_EINVAL, "tt_expand: geometry is NULL");
  if (g->T < 2 || g->T > TTX_MAX_CORES) TTX_FAIL(TTX_EINVAL, "tt_expand: T=%d: number of TT cores must be 2..4", g->T);
  if (g->num_tables <= 0) TTX_FAIL(TTX_EINVAL, "tt_expand: num_tables=%d must be > 0", g->num_tables);
  ExArgs A;
  memset(&A, 0, sizeof(A));
  if (!ex_shape(g, &A.sh))
    TTX_FAIL(TTX_EUNSUPPORTED,
             "tt_expand: not a shape of the expand kernel (T = 3, ranks <= %d, q0 <= 16, q1 <= 64, q2 <= %d, x_0 of a prefix within "
             "%d KiB of LDS)", kExMaxRank, kExMaxQ2, kExLdsMax / 1024);
  const ExShape& sh = A.sh;
  if (table < 0 || table >= g->num_tables) TTX_FAIL(TTX_EINVAL, "tt_expand: table %d out of range [0, %d)", table, g->num_tables);
  // the table's own row factors and its first slice in every core (p_tables: table after table)
  const bool mixed = g->p_tables && g->num_tables > 1;
  if (mixed && g->num_tables > TTX_MAX_TABLES_MIXED)
    TTX_FAIL(TTX_EINVAL, "tt_expand: num_tables=%d: at most %d tables with per-table row factors", g->num_tables, TTX_MAX_TABLES_MIXED);
  long long p[3], base[3];
  for (int t = 0; t < 3; ++t) {
    base[t] = 0;
    if (mixed) {
      for (int k = 0; k <= table; ++k) {
        const int pk = g->p_tables[(size_t)k * 3 + t];
        if (pk <= 0) TTX_FAIL(TTX_EINVAL, "tt_expand: table %d core %d: p must be > 0", k, t);
        if (k < table) base[t] += pk;
        p[t] = pk;
      }
    } else {
      p[t] = g->p[t];
      base[t] = (long long)table * p[t];
    }
    if (p[t] <= 0 || p[t] > (1ll << 30) || base[t] + p[t] > (1ll << 30))
      TTX_FAIL(TTX_EINVAL, "tt_expand: core %d: p=%lld must be in [1, 2^30], and the core's slices at most 2^30", t, p[t]);
  }
  if (p[0] * p[1] > (1ll << 62) / p[2]) TTX_FAIL(TTX_EINVAL, "tt_expand: prod(p) too large");
  const long long rows = p[0] * p[1] * p[2];
  if (row_begin < 0 || row_end < row_begin || row_end > rows)
    TTX_FAIL(TTX_EINVAL, "tt_expand: rows [%lld, %lld) are not a range of the table's %lld", (long long)row_begin, (long long)row_end, rows);
  if (row_begin == row_end) return TTX_OK;
  if (!cores || !cores[0] || !cores[1] || !cores[2] || !out) TTX_FAIL(TTX_EINVAL, "tt_expand: NULL cores / out");
  if ((((uintptr_t)cores[0]) | ((uintptr_t)cores[1]) | ((uintptr_t)cores[2]) | ((uintptr_t)out)) & 3)
    TTX_FAIL(TTX_EINVAL, "tt_expand: cores and out must be 4-byte aligned");
  (void)hipGetLastError();  // (an earlier, unrelated call's error is not this launch's)

  const int p1 = (int)p[1], p2 = (int)p[2];
  const long long pf_begin = row_begin / p2, pf_last = (row_end - 1) / p2;
  const long long npf = pf_last - pf_begin + 1;
  const int i2b = (int)(row_begin - pf_begin * p2), i2e = (int)(row_end - pf_last * p2);
  // the i2 block of a work-group: all of p2 with many prefixes; with few, blocks that still leave every wave several M tiles
  long long want = npf >= kExTargetWgs ? 1 : (kExTargetWgs + npf - 1) / npf;
  long long BL = (p2 + want - 1) / want;
  const long long minBL = ((long long)kExMinTiles * 16 + sh.Q2P - 1) / sh.Q2P;
  if (BL < minBL) BL = minBL;
  if (BL > kExBlockMax) BL = kExBlockMax;
  A.BL = (int)BL;
  A.nsplit = (int)((p2 + BL - 1) / BL);
  A.p1 = p1;
  A.p2 = p2;
  A.dq2 = table_div((unsigned)(sh.Q2P / 4), (1ull << 19) + 16);  // (e / 4 < 2^19 + 16: e < 2^21 + 64)
  const float* c[3] = {cores[0] + (size_t)base[0] * sh.sl[0], cores[1] + (size_t)base[1] * sh.sl[1],
                       cores[2] + (size_t)base[2] * sh.sl[2]};
  const int vec = (sh.q2 % 4 == 0 && (((uintptr_t)out) & 15) == 0) ? 1 : 0;
  const long long per_launch = kExLaunchWgs / A.nsplit;  // (nsplit <= 2^14: at least 2^16 prefixes, at most 2^30 work-groups)
  for (long long g0 = 0; g0 < npf; g0 += per_launch) {
    const long long n = npf - g0 < per_launch ? npf - g0 : per_launch;
    const long long pf = pf_begin + g0;
    A.i0b = (int)(pf / p1);
    A.i1b = (int)(pf - (long long)A.i0b * p1);
    A.npf = (int)n;
    A.i2_first = g0 == 0 ? i2b : 0;
    A.i2_last_end = g0 + n == npf ? i2e : p2;
    A.row_off = g0 * p2 - i2b;
    A.dp1 = table_div((unsigned)p1, (unsigned long long)A.i1b + (unsigned long long)n);
    int rc;
    switch (sh.KB) {
      case 8: rc = launch_expand_nt<8>(A, c, out, vec, (hipStream_t)stream); break;
      case 16: rc = launch_expand_nt<16>(A, c, out, vec, (hipStream_t)stream); break;
      default: rc = launch_expand_nt<32>(A, c, out, vec, (hipStream_t)stream); break;
    }
    if (rc) return rc;
  }
  return TTX_OK;
}

}  // extern "C"

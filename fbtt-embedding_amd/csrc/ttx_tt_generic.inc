// ttx_tt_generic.inc -- the generic contraction kernels: any T in {2,3,4}, any q / ranks.
// Included by ttx_tt.hip (shares CorePtrs / Partials / FastDiv / mfma4 / Plan).
//
// A CHUNK is <= MC lookups of one pivot slice (core 1, r1 x q1 r2 floats).  What round 3 changed: the slice is
// no longer staged whole.  The kernels walk it in BLOCKS of KB rows (a K block of r1, a multiple of 32) by PW
// columns (a column pass: bpp of x_0's q1 column blocks, which the tail never mixes -- the same observation the
// r = 64 specialisations use, Shape3::NP), so the LDS carve depends on the tile sizes (KB, bpp * r2, MC), not on
// the size of the slice:
//   forward   for every column pass:  X0 = sum over K blocks of A[:, kb] * B1[kb, pass]   (MFMA, accumulating in LDS)
//                                     tail stages on the pass's rows (a, b) of x_0 -> output rows
//   backward  for every column pass:  X0 as above; fused tail: thin-core partials (added across passes) and d x_0 in
//                                     place; then per K block  d core_1[kb, pass] = A[:, kb]^T * d x_0   (chunk partial)
//                                     and  d core_0[:, kb] += d x_0 * B1[kb, pass]^T                   (lookup partial)
// One block (nkb == ncp == 1) is the round-1 kernel: same staging, same order of additions.  More blocks change
// the order in which a lookup's d core_0 / d core_2 terms are added (pass by pass), nothing else.
// The reference contracts any (m, k, n) through cublasGemmBatchedEx (tt_embeddings_cuda.cu:993-1054, :529-591);
// what bounds this kernel is one q1 block of x_0 (MC q0 rows x r2 columns) plus a KB x r2 block of core_1:
// ranks up to ~600 at T = 3.

// LDS carve (float offsets) + tile extents.  A PASS (of lookups) is <= SC of the chunk's lookups: one X0 tile of
// rS rows (SC*q0 padded to 32); several lookup passes only when the slice is staged as ONE block.
struct Lds {
  int MC, SC;
  int rS;    // rows of one lookup pass
  int nsub;  // lookup passes of a full chunk
  int KB;    // rows of a K block (multiple of 32)
  int KBt;   // 16-wide tiles of a K block
  int nkb;   // K blocks covering r1
  int bpp;   // q1 blocks per column pass (T >= 3)
  int ncp;   // column passes
  int PW;    // columns of a full column pass
  int N1t;   // 16-wide tiles covering PW
  int ld;    // row stride of Bs and X0 (>= 16*N1t, == 2 mod 32)
  int ldA;   // row stride of As (>= KB, == 2 mod 32)
  int tiled;    // more than one block
  int persist;  // d core_1 accumulates in registers across lookup passes (one block only)
  int oB, oA, oX0, oX1, oG, oC, oI;
  int szX1;  // per-lookup floats of X1 for one column pass (T == 4)
  int cLds;  // forward: last-core slices of a pass are staged in LDS
  int bytes;
  int dbg;   // ablation mask (bench/ablate only): phases to skip, results invalid when != 0
  FastDiv fdD, fdD4, fdN1, fdQ0, fdSl2, fdSC;
};

static TTX_KNOB(int, g_chunk_override, 0);
#ifdef TTX_TEST_HOOKS
int g_debug_skip = 0;     // (declared in ttx_tt_common.h: the specialised kernels' translation units read them)
int g_disable_spec = 0;
long long* g_stamps = nullptr;
int g_old_stores = 0;
int g_partial_flavour = 0;
#endif
static TTX_KNOB(int, g_lds_budget, 160 * 1024);  // (tests shrink it to drive small shapes through the block walk)
static bool spec_shape(const Dims& d);  // ttx_tt_spec.inc covers this geometry
static int spec_mc(const Dims& d, long long nnz);  // ... with this many lookups per chunk
long long* debug_stamps() { return g_stamps; }

static int stride2(int n) {  // smallest s >= n with s % 32 == 2
  int s = (n + 29) / 32 * 32 + 2;
  return s;
}

// bpp <= 0 / KB <= 0: the whole slice in one block
static Lds make_lds(const Dims& d, int MC, bool bwd, int bpp, int KB) {
  Lds L;
  memset(&L, 0, sizeof(L));
  const int K0 = d.k[0], N1 = d.n[0], q0 = d.q[0];
  const int K0p = (K0 + 31) / 32 * 32;
  if (KB <= 0 || KB > K0p) KB = K0p;
  KB = (KB + 31) / 32 * 32;
  if (d.T < 3) bpp = 1;
  else if (bpp <= 0 || bpp > d.q[1]) bpp = d.q[1];
  L.MC = MC;
  L.KB = KB;
  L.nkb = (K0 + KB - 1) / KB;
  L.KBt = L.nkb == 1 ? (K0 + 15) / 16 : KB / 16;
  L.bpp = bpp;
  L.ncp = d.T >= 3 ? (d.q[1] + bpp - 1) / bpp : 1;
  L.PW = d.T >= 3 ? bpp * d.k[1] : N1;
  L.N1t = (L.PW + 15) / 16;
  L.ld = stride2(L.N1t * 16);
  L.ldA = stride2(KB);
  L.tiled = (L.nkb > 1 || L.ncp > 1) ? 1 : 0;
  // register-resident d core_1 needs <= 2 (N-pair) jobs per wave and one group of <= 4 r1 tiles
  const int npairs = (L.N1t + 1) / 2;
  L.persist = (!L.tiled && L.KBt <= 4 && npairs <= 2 * kWaves) ? 1 : 0;
  int sc = 32 / q0;
  if (sc < 1) sc = 1;
  if (sc > MC || (bwd && !L.persist) || L.tiled) sc = MC;
  L.SC = sc;
  L.rS = (sc * q0 + 31) / 32 * 32;
  L.nsub = (MC + sc - 1) / sc;
  L.szX1 = (d.T == 4) ? q0 * bpp * d.n[1] : 0;
  const int sl2 = d.T > 2 ? d.slice[2] : 0;
  L.cLds = (!bwd && d.T > 2 && d.n[1] <= 8 && sc * sl2 <= 4096) ? 1 : 0;
  long long o = 0;
  auto take = [&](long long n) { long long r = o; o += (n + 3) / 4 * 4; return (int)r; };
  L.oB = take((long long)KB * L.ld);
  L.oA = take((long long)L.nsub * L.rS * L.ldA);
  L.oX0 = take((long long)L.rS * L.ld);
  L.oX1 = take((long long)sc * L.szX1);
  L.oG = take(bwd && d.T >= 3 ? (long long)MC * d.D : 0);
  L.oC = take(L.cLds ? sc * sl2 : 0);
  L.oI = take(MC * (bwd ? 8 : 4));  // int4 lookup records (+ backward: the rows of their thin-core partials)
  L.bytes = o * 4 > (1ll << 30) ? (1 << 30) : (int)(o * 4);
  L.fdD = make_fd(d.D);
  L.fdN1 = make_fd(N1);
  L.fdQ0 = make_fd(q0);
  L.fdD4 = make_fd(d.D / 4 > 0 ? d.D / 4 : 1);
  L.fdSl2 = make_fd(sl2 > 0 ? sl2 : 1);
  L.fdSC = make_fd(sc);
  L.dbg = g_debug_skip;
  return L;
}

// lookups per chunk and the block walk of the generic kernels for this geometry (MC == 0: nothing fits)
struct TileCfg {
  int MC, bpp, KB;
};
static TileCfg choose_tiles(const Dims& d) {
  const int budget = g_lds_budget;
  const int mc_hi = g_chunk_override > 0 ? g_chunk_override : 0;
  auto fits = [&](int mc, int cap) {
    return make_lds(d, mc, true, 0, 0).bytes <= (cap < budget ? cap : budget);
  };
  if (mc_hi) {
    if (fits(mc_hi, budget)) return TileCfg{mc_hi, 0, 0};
  } else {
    // the slice as one block: three, then two work-groups per CU (160 KiB of LDS), else whatever fits
    for (int mc = 16; mc >= 8; mc >>= 1)
      if (fits(mc, 53 * 1024)) return TileCfg{mc, 0, 0};
    for (int mc = 32; mc >= 8; mc >>= 1)
      if (fits(mc, 80 * 1024)) return TileCfg{mc, 0, 0};
    for (int mc = 16; mc >= 1; mc >>= 1)
      if (fits(mc, budget)) return TileCfg{mc, 0, 0};
  }
  // walk the slice in blocks: as many lookups per chunk as possible (a block of core_1 is staged once per chunk), then
  // as few blocks as possible (every block costs a staging round and its barriers); a carve that leaves room for two
  // work-groups per CU is taken when it costs at most twice the blocks
  const int K0p = (d.k[0] + 31) / 32 * 32;
  const int q1 = d.T >= 3 ? d.q[1] : 1;
  auto search = [&](int cap, long long* cost_out) {
    for (int mc = mc_hi ? mc_hi : 16; mc >= 1; mc >>= 1) {
      TileCfg best{0, 0, 0};
      long long best_cost = -1;
      for (int bpp = q1; bpp >= 1; --bpp) {
        for (int kb = K0p; kb >= 32; kb = (kb / 2 + 31) / 32 * 32) {
          const Lds L = make_lds(d, mc, true, bpp, kb);
          if (L.bytes <= cap) {
            const long long cost = (long long)L.ncp * L.nkb;
            if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = TileCfg{mc, bpp, kb}; }
            break;  // (smaller K blocks of this bpp only cost more)
          }
          if (kb == 32) break;
        }
      }
      if (best_cost >= 0) { *cost_out = best_cost; return best; }
      if (mc_hi) break;
    }
    *cost_out = -1;
    return TileCfg{0, 0, 0};
  };
  long long cost1 = -1, cost0 = -1;
  const TileCfg one = search(budget, &cost1);
  if (one.MC > 0 && budget > 80 * 1024) {
    const TileCfg two = search(80 * 1024, &cost0);
    if (two.MC >= one.MC && cost0 <= 2 * cost1) return two;
  }
  return one;
}

static bool t4_merge_dims(const Dims& d, Dims* d3);
int choose_chunk(const Dims& d, long long nnz) {
  if (spec_shape(d)) return spec_mc(d, nnz);  // wave-independent kernels: Shape3::MC of the variant picked for nnz
  Dims d3;
  if (t4_merge_dims(d, &d3)) return spec_mc(d3, nnz);  // four cores on the three-core kernels
  return choose_tiles(d).MC;
}

// ------------------------------------------------------------- kernels -----

// the block of core_1's slice a staging round holds
struct Blk {
  int kbase, krows;  // rows [kbase, kbase + krows) of the slice (the K index r1)
  int cbase, pcols;  // columns [cbase, cbase + pcols)
  int b0, nbp;       // T >= 3: x_0's q1 blocks [b0, b0 + nbp)   (pcols = nbp * r2)
  int n1t;           // 16-column tiles covering pcols
};
__device__ __forceinline__ Blk make_blk(const Dims& d, const Lds& L, int cp, int kb) {
  Blk b;
  b.kbase = kb * L.KB;
  b.krows = min(L.KB, d.k[0] - b.kbase);
  if (d.T >= 3) {
    b.b0 = cp * L.bpp;
    b.nbp = min(L.bpp, d.q[1] - b.b0);
    b.cbase = b.b0 * d.k[1];
    b.pcols = b.nbp * d.k[1];
  } else {
    b.b0 = 0;
    b.nbp = 1;
    b.cbase = 0;
    b.pcols = d.n[0];
  }
  b.n1t = (b.pcols + 15) / 16;
  return b;
}

// As row of (lookup j of the chunk, core-0 row a)
__device__ __forceinline__ int a_row(const Lds& L, int q0, unsigned j, unsigned a) {
  unsigned jl;
  const unsigned h = fdivmod(j, L.fdSC, jl);
  return h * L.rS + jl * q0 + a;
}

// one staging round: block `b` of B1 and the matching columns of the chunk's stacked core-0 slices -> LDS
// (lookup-pass-major, zero padded to the MFMA tile extents).  Dependent global loads: lrec -> core-0 rows.
// sync_before: some wave may still be reading the previous block (or X0 / X1 / Cs of the previous pass).
__device__ __forceinline__ void stage_block(const Dims& d, const CorePtrs& C, const Lds& L, float* smem, int s,
                                            int len, const Blk& b, bool sync_before) {
  const int tid = threadIdx.x;
  const int K0 = d.k[0], N1 = d.n[0], q0 = d.q[0];
  const int4* I = (const int4*)(smem + L.oI);
  float* Bs = smem + L.oB;
  float* As = smem + L.oA;
  const float* __restrict__ B1 = C.c[1] + (size_t)s * d.slice[1];
  if (sync_before) __syncthreads();
  // zero A where the MFMA reads rows past the chunk / columns past the block, and B when the block does not fill its
  // tiles (full chunks of full blocks -- the common case of the walk -- need neither the stores nor the barrier)
  const bool padB = (b.krows != L.KB) || (b.pcols & 15);
  const int npass = (len + L.SC - 1) / L.SC;
  const bool padA = (b.krows != L.KB) || (len * q0 != npass * L.rS);
  if (padA)
    for (int e = tid; e < npass * L.rS * L.ldA; e += kThreads) As[e] = 0.f;
  if (padB)
    for (int e = tid; e < L.KB * L.ld; e += kThreads) Bs[e] = 0.f;
  if (padA || padB) __syncthreads();
  constexpr int kStageNF = 8;  // loads in flight per thread: a block is tens of KB from L2, one load at a time is its latency x 16
  if (((N1 | b.cbase | b.pcols) & 3) == 0) {
    const int pc4 = b.pcols / 4;
    const FastDiv f4 = make_fd(pc4);
    const int total = b.krows * pc4;
    for (int e0 = tid; e0 < total; e0 += kThreads * kStageNF) {
      float4 v[kStageNF];
      unsigned row[kStageNF], c4[kStageNF];
#pragma unroll
      for (int u = 0; u < kStageNF; ++u) {
        const int e = e0 + u * kThreads;
        row[u] = 0; c4[u] = 0;
        if (e < total) {
          row[u] = fdivmod((unsigned)e, f4, c4[u]);
          v[u] = *(const float4*)(B1 + (size_t)(b.kbase + row[u]) * N1 + b.cbase + c4[u] * 4);
        }
      }
#pragma unroll
      for (int u = 0; u < kStageNF; ++u)
        if (e0 + u * kThreads < total) {
          float2* dst = (float2*)(Bs + row[u] * L.ld + c4[u] * 4);  // ld is even: 8-byte aligned
          dst[0] = make_float2(v[u].x, v[u].y);
          dst[1] = make_float2(v[u].z, v[u].w);
        }
    }
  } else {
    const FastDiv f1 = make_fd(b.pcols);
    for (int e = tid; e < b.krows * b.pcols; e += kThreads) {
      unsigned col;
      const unsigned row = fdivmod((unsigned)e, f1, col);
      Bs[row * L.ld + col] = B1[(size_t)(b.kbase + row) * N1 + b.cbase + col];
    }
  }
  const int sl0 = d.slice[0];  // q0 * r1
  if (((K0 | b.krows) & 3) == 0) {  // (kbase is a multiple of 32)
    const int kr4 = b.krows / 4, per = q0 * kr4;
    const FastDiv fper = make_fd(per), fk4 = make_fd(kr4);
    const int total = len * per;
    for (int e0 = tid; e0 < total; e0 += kThreads * 4) {
      float4 v[4];
      int at[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = e0 + u * kThreads;
        at[u] = 0;
        if (e < total) {
          unsigned rem, c4;
          const unsigned j = fdivmod((unsigned)e, fper, rem);
          const unsigned a = fdivmod(rem, fk4, c4);
          v[u] = *(const float4*)(C.c[0] + (size_t)I[j].y * sl0 + a * K0 + b.kbase + c4 * 4);
          at[u] = a_row(L, q0, j, a) * L.ldA + c4 * 4;
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (e0 + u * kThreads < total) {
          float2* dst = (float2*)(As + at[u]);
          dst[0] = make_float2(v[u].x, v[u].y);
          dst[1] = make_float2(v[u].z, v[u].w);
        }
    }
  } else {
    const int per = q0 * b.krows;
    const FastDiv fper = make_fd(per), fk = make_fd(b.krows);
    for (int e = tid; e < len * per; e += kThreads) {
      unsigned rem, k;
      const unsigned j = fdivmod((unsigned)e, fper, rem);
      const unsigned a = fdivmod(rem, fk, k);
      As[a_row(L, q0, j, a) * L.ldA + k] = (C.c[0] + (size_t)I[j].y * sl0)[a * K0 + b.kbase + k];
    }
  }
  __syncthreads();
}

// ---- GEMM 1:  one 16-row tile of X0 x NB column tiles (+)= As * Bs, k-step {k, k+8, k+16, k+24} ----
// arow0: As row of the tile; xrow0: X0 row of the tile (within the lookup pass); accum: add to what the
// previous K blocks left there
template <int NB>
__device__ __forceinline__ void x0_group(const Dims& d, const Lds& L, float* smem, int arow0, int xrow0,
                                         int n0, float* rows_out, int j0, int lenS, bool accum) {
  const int lane = lane_id();
  const int i16 = lane & 15, kq = lane >> 4;
  const float* arow = smem + L.oA + (arow0 + i16) * L.ldA + 8 * kq;
  const float* bbase = smem + L.oB + 8 * kq * L.ld + n0 * 16 + i16;
  float* xo = smem + L.oX0 + (xrow0 + kq * 4) * L.ld + n0 * 16 + i16;
  f32x4 acc[NB];
#pragma unroll
  for (int x = 0; x < NB; ++x) acc[x] = (f32x4){0.f, 0.f, 0.f, 0.f};
  if (accum && !rows_out) {
#pragma unroll
    for (int x = 0; x < NB; ++x)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[x][r] = xo[r * L.ld + x * 16];
  }
  // software pipeline: the B fragments of k-step t+1 are read from LDS while the
  // MFMAs of k-step t issue
  float bcur[NB];
#pragma unroll
  for (int x = 0; x < NB; ++x) bcur[x] = bbase[x * 16];
  for (int kb = 0; kb < L.KB; kb += 32) {
    float a[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) a[t] = arow[kb + t];
    __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);  // the 8 A fragments (4 x ds_read2)
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int kn = (t < 7) ? kb + t + 1 : kb + 32;  // k-steps of a block are kb+0..7 (+8*kq)
      const float* bn = bbase + (kn < L.KB ? kn : 0) * L.ld;  // last prefetch wraps (unused)
      float bnxt[NB];
#pragma unroll
      for (int x = 0; x < NB; ++x) bnxt[x] = bn[x * 16];
#pragma unroll
      for (int x = 0; x < NB; ++x) acc[x] = mfma4(a[t], bcur[x], acc[x]);
#pragma unroll
      for (int x = 0; x < NB; ++x) bcur[x] = bnxt[x];
      __builtin_amdgcn_sched_group_barrier(0x100, (NB + 1) / 2, 0);  // DS reads of step t+1
      __builtin_amdgcn_sched_group_barrier(0x008, NB, 0);            // MFMAs of step t
    }
  }
  // C/D layout: col = lane & 15, row = (lane >> 4) * 4 + r
  if (rows_out) {  // T == 2 forward: rows straight to HBM (the same lane adds the next K block to them)
    const int4* I = (const int4*)(smem + L.oI);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = xrow0 + kq * 4 + r;
      unsigned a_;
      const unsigned jl = fdivmod((unsigned)row, L.fdQ0, a_);
      if ((int)jl < lenS) {
        float* o = rows_out + (size_t)I[j0 + jl].x * d.D + a_ * d.n[0];
#pragma unroll
        for (int x = 0; x < NB; ++x) {
          const int col = (n0 + x) * 16 + i16;
          if (col < d.n[0]) o[col] = accum ? o[col] + acc[x][r] : acc[x][r];
        }
      }
    }
  } else {
#pragma unroll
    for (int x = 0; x < NB; ++x)
#pragma unroll
      for (int r = 0; r < 4; ++r) xo[r * L.ld + x * 16] = acc[x][r];
  }
}

// X0 of lookup pass h (all rS rows: rows past the pass come out as zeros), the block's n1t column tiles
__device__ __forceinline__ void gemm_x0(const Dims& d, const Lds& L, float* smem, int h, int n1t,
                                        float* rows_out, int j0, int lenS, bool accum) {
  const int w = threadIdx.x / kWave;
  const int mtiles = L.rS / 16;
  // column-group width: the widest of 8/4/2/1 tiles that still gives every wave a job
  int NB = 8;
  while (NB > 1 && mtiles * ((n1t + NB - 1) / NB) < kWaves) NB >>= 1;
  const int ngroups = (n1t + NB - 1) / NB;
  for (int job = w; job < mtiles * ngroups; job += kWaves) {
    const int mt = job / ngroups, g = job - mt * ngroups;
    int n0 = g * NB;
    int cnt = min(NB, n1t - n0);
    const int ar = h * L.rS + mt * 16, xr = mt * 16;
    while (cnt > 0) {
      if (cnt >= 8) { x0_group<8>(d, L, smem, ar, xr, n0, rows_out, j0, lenS, accum); n0 += 8; cnt -= 8; }
      else if (cnt >= 4) { x0_group<4>(d, L, smem, ar, xr, n0, rows_out, j0, lenS, accum); n0 += 4; cnt -= 4; }
      else if (cnt >= 2) { x0_group<2>(d, L, smem, ar, xr, n0, rows_out, j0, lenS, accum); n0 += 2; cnt -= 2; }
      else { x0_group<1>(d, L, smem, ar, xr, n0, rows_out, j0, lenS, accum); n0 += 1; cnt -= 1; }
    }
  }
}

// rows of a tail stage inside a column pass: local row = a*nb + b  <->  row a*oA + oB0 + b of the whole lookup
struct RowMap {
  int nb, oA, oB0;
};

// ---- forward tail stage: out[m x NT] = x[m x k] * C[k x NT] per lookup, C from LDS or HBM ----
// item = (lookup jl of the pass, local row); x addressing: row = a*nb + b -> X + jl*sJ + a*sA + b*sB
template <int NT>
__device__ __forceinline__ void fwd_stage(int lenS, int j0, int m, int k, RowMap rm, int sJ, int sA, int sB,
                                          const float* X, const float* Cs, int cJ, bool c_lds,
                                          const float* Cg, int slice, const int4* I, int which,
                                          float* out_lds, int oJ, float* __restrict__ rows, int D) {
  const FastDiv fm = make_fd(m), fnb = make_fd(rm.nb);
  for (int e = threadIdx.x; e < lenS * m; e += kThreads) {
    unsigned row, b;
    const unsigned jl = fdivmod((unsigned)e, fm, row);
    const unsigned a = fdivmod(row, fnb, b);
    const float* xi = X + jl * sJ + a * sA + b * sB;
    const int4 rec = I[j0 + jl];
    const int sid = which == 2 ? rec.z : rec.w;
    const float* c = c_lds ? Cs + jl * cJ : Cg + (size_t)sid * slice;
    float acc[NT];
#pragma unroll
    for (int x = 0; x < NT; ++x) acc[x] = 0.f;
#pragma unroll 4
    for (int kk = 0; kk < k; ++kk) {
      const float xv = xi[kk];
#pragma unroll
      for (int x = 0; x < NT; ++x) acc[x] = fmaf(xv, c[kk * NT + x], acc[x]);
    }
    float* o = rows ? rows + (size_t)rec.x * D + (size_t)(a * rm.oA + rm.oB0 + b) * NT : out_lds + jl * oJ + row * NT;
#pragma unroll
    for (int x = 0; x < NT; ++x) o[x] = acc[x];
  }
}

// generic (any n) version: item = (jl, local row, col), C from HBM
__device__ __forceinline__ void fwd_stage_any(int lenS, int j0, int m, int k, int n, RowMap rm, int sJ, int sA,
                                              int sB, const float* X, const float* Cg, int slice,
                                              const int4* I, int which, float* out_lds, int oJ,
                                              float* __restrict__ rows, int D) {
  const FastDiv fper = make_fd(m * n), fn = make_fd(n), fnb = make_fd(rm.nb);
  for (int e = threadIdx.x; e < lenS * m * n; e += kThreads) {
    unsigned rem, col, b;
    const unsigned jl = fdivmod((unsigned)e, fper, rem);
    const unsigned row = fdivmod(rem, fn, col);
    const unsigned a = fdivmod(row, fnb, b);
    const float* xi = X + jl * sJ + a * sA + b * sB;
    const int4 rec = I[j0 + jl];
    const int sid = which == 2 ? rec.z : rec.w;
    const float* c = Cg + (size_t)sid * slice + col;
    float acc = 0.f;
    for (int kk = 0; kk < k; ++kk) acc = fmaf(xi[kk], c[kk * n], acc);
    if (rows) rows[(size_t)rec.x * D + (size_t)(a * rm.oA + rm.oB0 + b) * n + col] = acc;
    else out_lds[jl * oJ + rem] = acc;
  }
}

#define TTX_NT_SWITCH(nt, CALL)          \
  switch (nt) {                          \
    case 1: { CALL(1); } break;          \
    case 2: { CALL(2); } break;          \
    case 3: { CALL(3); } break;          \
    case 4: { CALL(4); } break;          \
    case 5: { CALL(5); } break;          \
    case 6: { CALL(6); } break;          \
    case 7: { CALL(7); } break;          \
    case 8: { CALL(8); } break;          \
    default: break;                      \
  }

// tail of one (column pass, lookup pass): x_0's rows (a, b), b in the pass -> output rows (T == 3), through x_1 (T == 4)
__device__ __forceinline__ void fwd_tail(const Dims& d, const CorePtrs& C, const Lds& L, float* smem, const Blk& b,
                                         int j0, int lenS, float* __restrict__ rows) {
  const int4* I = (const int4*)(smem + L.oI);
  const float* X0 = smem + L.oX0;
  float* X1 = smem + L.oX1;
  const float* Cs = smem + L.oC;
  const int q0 = d.q[0];
  {  // stage t = 1: x_1[(a,b)][n1] = x_0[(a,b)][k1] * core_2[i_2][k1 x n1]
    const int k1 = d.k[1], n1 = d.n[1], q1 = d.q[1];
    const bool last = (d.T == 3);
    const int sl2 = d.slice[2];
    const RowMap rm{b.nbp, q1, b.b0};
    const int m = q0 * b.nbp;
    if (n1 <= 8) {
#define CALL(NT) fwd_stage<NT>(lenS, j0, m, k1, rm, q0 * L.ld, L.ld, k1, X0, Cs, sl2, L.cLds != 0, C.c[2], sl2, I, 2, \
                               X1, L.szX1, last ? rows : nullptr, d.D)
      TTX_NT_SWITCH(n1, CALL)
#undef CALL
    } else {
      fwd_stage_any(lenS, j0, m, k1, n1, rm, q0 * L.ld, L.ld, k1, X0, C.c[2], sl2, I, 2, X1, L.szX1,
                    last ? rows : nullptr, d.D);
    }
  }
  if (d.T == 4) {
    __syncthreads();
    // stage t = 2: row[(a,b,c)][n2] = x_1[(a,b,c)][k2] * core_3[i_3][k2 x n2]
    const int k2 = d.k[2], n2 = d.n[2], q2 = d.q[2];
    const int nb = b.nbp * q2, m = q0 * nb;
    const RowMap rm{nb, d.q[1] * q2, b.b0 * q2};
    if (n2 <= 8) {
    // (Cs / X1 stand in for the unused LDS-operand and LDS-output arguments: with literal nullptrs there the ROCm 7.2
    //  inliner crashes on this instantiation set -- updateCGAndAnalysisManagerForPass, segmentation fault)
#define CALL(NT) fwd_stage<NT>(lenS, j0, m, k2, rm, L.szX1, nb * k2, k2, X1, Cs, 0, false, C.c[3], d.slice[3], I, 3, \
                               X1, 0, rows, d.D)
      TTX_NT_SWITCH(n2, CALL)
#undef CALL
    } else {
      fwd_stage_any(lenS, j0, m, k2, n2, rm, L.szX1, nb * k2, k2, X1, C.c[3], d.slice[3], I, 3, nullptr, 0, rows, d.D);
    }
  }
}

__global__ __launch_bounds__(kThreads, 3) void fwd_kernel(Dims d, Plan P, CorePtrs C,
                                                         float* __restrict__ rows, Lds L,
                                                         float* __restrict__ zout, long long nzero) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  zero_output(zout, nzero);
  const int chunk = blockIdx.x;
  const int4 cr = P.chunk_rec[chunk];
  const int s = cr.x, start = cr.y, len = cr.z;
  if (len == 0) return;
  const int tid = threadIdx.x;
  int4* I = (int4*)(smem + L.oI);
  float* Cs = smem + L.oC;
  if (tid < len) I[tid] = P.lrec[start + tid];
  __syncthreads();  // (the staging round reads every lookup's record; it has no barrier of its own in front of that when nothing is padded)
  const int npass = (len + L.SC - 1) / L.SC;   // (more than one only when the slice is a single block)
  bool first = true;
  for (int cp = 0; cp < L.ncp; ++cp) {
    for (int h = 0; h < npass; ++h) {
      const int j0 = h * L.SC;
      const int lenS = min(L.SC, len - j0);
      Blk b = make_blk(d, L, cp, 0);
      for (int kb = 0; kb < L.nkb; ++kb) {
        b = make_blk(d, L, cp, kb);
        if (L.tiled || first) stage_block(d, C, L, smem, s, len, b, !first);
        else if (kb == 0) __syncthreads();  // the previous lookup pass is done with X0 / X1 / Cs
        first = false;
        if (kb == L.nkb - 1 && L.cLds) {  // last-core slices of this pass -> LDS (overlaps the GEMM)
          const int sl2 = d.slice[2];
          for (int e = tid; e < lenS * sl2; e += kThreads) {
            unsigned rem;
            const unsigned jl = fdivmod((unsigned)e, L.fdSl2, rem);
            Cs[e] = (C.c[2] + (size_t)I[j0 + jl].z * sl2)[rem];
          }
        }
        if (!(L.dbg & 1)) gemm_x0(d, L, smem, h, b.n1t, d.T == 2 ? rows : nullptr, j0, lenS, kb > 0);
      }
      if (d.T == 2) continue;
      __syncthreads();
      if (L.dbg & 2) continue;
      fwd_tail(d, C, L, smem, b, j0, lenS, rows);
    }
  }
}

// ---- backward tail stage, fused: for one (lookup, column kk) pair walk the pass's rows once,
//   d core partial[kk][0..NT) (+)= sum_row x[row][kk] * G[row][0..NT)     -> HBM
//   d x[row][kk]               = sum_c   G[row][c]  * C[kk][c]          -> over x in place
// (only this thread ever reads x[.][kk] of that lookup, so in place is safe without a barrier; the same thread
//  owns the partial's elements in every column pass, so adding to them needs none either)
// x row (a, b) at X + jl*sJ + a*sA + b*sB; its gradient row is row a*gA + gB0 + b of G + (gBase + jl)*gJ
template <int NT>
__device__ __forceinline__ void bwd_stage_fused(int lenS, int j0, int k, int na, int nb, int sJ, int sA,
                                                int sB, float* X, const float* G, int gJ, int gBase, int gA, int gB0,
                                                const float* Cg, int slice, const int4* I, const int4* IP, int which,
                                                float* __restrict__ pc, bool accum) {
  const FastDiv fk = make_fd(k);
  for (int e = threadIdx.x; e < lenS * k; e += kThreads) {
    unsigned kk;
    const unsigned jl = fdivmod((unsigned)e, fk, kk);
    const int4 rec = I[j0 + jl];
    const int sid = which == 2 ? rec.z : rec.w;
    const float* cg = Cg + (size_t)sid * slice + kk * NT;
    float c[NT], acc[NT];
#pragma unroll
    for (int x = 0; x < NT; ++x) { c[x] = cg[x]; acc[x] = 0.f; }
    float* xb = X + jl * sJ + kk;
    const float* gj = G + (gBase + jl) * gJ;
    for (int a = 0; a < na; ++a) {
      float* xa = xb + a * sA;
      const float* g = gj + (a * gA + gB0) * NT;
#pragma unroll 4
      for (int b = 0; b < nb; ++b) {
        const float xv = xa[b * sB];
        float dx = 0.f;
#pragma unroll
        for (int x = 0; x < NT; ++x) {
          const float gv = g[x];
          acc[x] = fmaf(xv, gv, acc[x]);
          dx = fmaf(gv, c[x], dx);
        }
        xa[b * sB] = dx;
        g += NT;
      }
    }
    float* o = pc + (size_t)(which == 2 ? IP[j0 + jl].z : IP[j0 + jl].w) * slice + kk * NT;
#pragma unroll
    for (int x = 0; x < NT; ++x) o[x] = accum ? o[x] + acc[x] : acc[x];
  }
}

// generic two-phase version (any n): (a) partial, barrier, (b) d x in place
__device__ __forceinline__ void bwd_stage_any(int lenS, int j0, int k, int n, int na, int nb, int sJ, int sA,
                                              int sB, float* X, const float* G, int gJ, int gBase, int gA, int gB0,
                                              const float* Cg, int slice, const int4* I, const int4* IP, int which,
                                              float* __restrict__ pc, bool accum) {
  const FastDiv fn = make_fd(n), fnb = make_fd(nb);
  const int m = na * nb;
  {
    const FastDiv fp = make_fd(k * n);
    for (int e = threadIdx.x; e < lenS * k * n; e += kThreads) {
      unsigned rem, col;
      const unsigned jl = fdivmod((unsigned)e, fp, rem);
      const unsigned kk = fdivmod(rem, fn, col);
      const float* gi = G + (gBase + jl) * gJ + col;
      const float* xj = X + jl * sJ + kk;
      float acc = 0.f;
      for (int a = 0; a < na; ++a)
        for (int b = 0; b < nb; ++b) acc = fmaf(xj[a * sA + b * sB], gi[(size_t)(a * gA + gB0 + b) * n], acc);
      float* o = pc + (size_t)(which == 2 ? IP[j0 + jl].z : IP[j0 + jl].w) * slice + rem;
      *o = accum ? *o + acc : acc;
    }
  }
  __syncthreads();
  {
    const FastDiv fp = make_fd(m * k), fk = make_fd(k);
    for (int e = threadIdx.x; e < lenS * m * k; e += kThreads) {
      unsigned rem, kk, b;
      const unsigned jl = fdivmod((unsigned)e, fp, rem);
      const unsigned row = fdivmod(rem, fk, kk);
      const unsigned a = fdivmod(row, fnb, b);
      const int4 rec = I[j0 + jl];
      const int sid = which == 2 ? rec.z : rec.w;
      const float* ct = Cg + (size_t)sid * slice + kk * n;
      const float* gi = G + (gBase + jl) * gJ + (size_t)(a * gA + gB0 + b) * n;
      float acc = 0.f;
      for (int c = 0; c < n; ++c) acc = fmaf(gi[c], ct[c], acc);
      X[jl * sJ + a * sA + b * sB + kk] = acc;
    }
  }
}

// ---- GEMM 2: d core_1 tiles += As^T * dX0 over one lookup pass, k-step rows {m, m+8, m+16, m+24} ----
// acc[x][y]: x = column tile of the pair (np*2 + x), y = r1 tile k0t + y (of the staged K block)
template <int KB, bool TWO>
__device__ __forceinline__ void db1_accum(const Lds& L, const float* smem, int h, int np, int k0t,
                                          f32x4 (&acc)[2][KB]) {
  const int lane = lane_id();
  const int i16 = lane & 15, kq = lane >> 4;
  const float* xr = smem + L.oX0 + 8 * kq * L.ld + np * 32 + i16;
  const float* ar = smem + L.oA + (h * L.rS + 8 * kq) * L.ldA + k0t * 16 + i16;
  // software pipeline: operands of k-step t+1 are read while the MFMAs of step t issue
  float bc0 = xr[0], bc1 = TWO ? xr[16] : 0.f, ac[KB];
#pragma unroll
  for (int y = 0; y < KB; ++y) ac[y] = ar[y * 16];
  for (int mb = 0; mb < L.rS; mb += 32) {
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int mx = (t < 7) ? mb + t + 1 : mb + 32;  // row steps of a block are mb+0..7 (+8*kq)
      const int mn = (mx < L.rS) ? mx : 0;            // last prefetch wraps (unused)
      const float bn0 = xr[mn * L.ld];
      const float bn1 = TWO ? xr[mn * L.ld + 16] : 0.f;
      float an[KB];
#pragma unroll
      for (int y = 0; y < KB; ++y) an[y] = ar[mn * L.ldA + y * 16];
#pragma unroll
      for (int y = 0; y < KB; ++y) {
        acc[0][y] = mfma4(ac[y], bc0, acc[0][y]);
        if (TWO) acc[1][y] = mfma4(ac[y], bc1, acc[1][y]);
      }
      bc0 = bn0;
      bc1 = bn1;
#pragma unroll
      for (int y = 0; y < KB; ++y) ac[y] = an[y];
      __builtin_amdgcn_sched_group_barrier(0x100, 1 + (KB + 1) / 2, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, (TWO ? 2 : 1) * KB, 0);
    }
  }
}

// the block's tiles -> the chunk's partial of d core_1 (row kbase + .., column cbase + ..)
template <int KB>
__device__ __forceinline__ void db1_store(const Dims& d, const Blk& b, int np, int k0t,
                                          const f32x4 (&acc)[2][KB], float* __restrict__ pc) {
  const int lane = lane_id();
  const int i16 = lane & 15, kq = lane >> 4;
  const int N1 = d.n[0];
#pragma unroll
  for (int x = 0; x < 2; ++x) {
    const int col = (np * 2 + x) * 16 + i16;
#pragma unroll
    for (int y = 0; y < KB; ++y)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int kk = (k0t + y) * 16 + kq * 4 + r;
        if (kk < b.krows && col < b.pcols) pc[(size_t)(b.kbase + kk) * N1 + b.cbase + col] = acc[x][y][r];
      }
  }
}

template <int KB>
__device__ __forceinline__ void db1_zero(f32x4 (&acc)[2][KB]) {
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < KB; ++y) acc[x][y] = (f32x4){0.f, 0.f, 0.f, 0.f};
}

// ---- GEMM 3: d core_0 partial rows (+)= dX0 * Bs^T over the block's columns, k-step columns {c, c+1, c+2, c+3} ----
template <int KB>
__device__ __forceinline__ void da_group(const Dims& d, const Lds& L, const float* smem, const Blk& b, int mt,
                                         int k0t, int j0, int lenS, float* __restrict__ pc, bool accum) {
  const int lane = lane_id();
  const int i16 = lane & 15, kq = lane >> 4;
  const float* xr = smem + L.oX0 + (mt * 16 + i16) * L.ld + kq;
  const float* br = smem + L.oB + (k0t * 16 + i16) * L.ld + kq;
  const int ncols = b.n1t * 16;
  f32x4 acc[KB];
#pragma unroll
  for (int y = 0; y < KB; ++y) acc[y] = (f32x4){0.f, 0.f, 0.f, 0.f};
  // software pipeline over 16-column blocks: the 4 k-steps of block c+16 are read while
  // the MFMAs of block c issue
  float ac[4], bc[4][KB];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    ac[u] = xr[u * 4];
#pragma unroll
    for (int y = 0; y < KB; ++y) bc[u][y] = br[y * 16 * L.ld + u * 4];
  }
  for (int c = 0; c < ncols; c += 16) {
    const int cn = (c + 16 < ncols) ? c + 16 : 0;  // last prefetch wraps (unused)
    float an[4], bn[4][KB];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      an[u] = xr[cn + u * 4];
#pragma unroll
      for (int y = 0; y < KB; ++y) bn[u][y] = br[y * 16 * L.ld + cn + u * 4];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int y = 0; y < KB; ++y) acc[y] = mfma4(ac[u], bc[u][y], acc[y]);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      ac[u] = an[u];
#pragma unroll
      for (int y = 0; y < KB; ++y) bc[u][y] = bn[u][y];
    }
    __builtin_amdgcn_sched_group_barrier(0x100, 2 + 2 * KB, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 4 * KB, 0);
  }
  const int4* I = (const int4*)(smem + L.oI);
  const int K0 = d.k[0], sl0 = d.slice[0];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = mt * 16 + kq * 4 + r;
    unsigned a_;
    const unsigned jl = fdivmod((unsigned)row, L.fdQ0, a_);
    if ((int)jl < lenS) {
      // (row of the partial: position in core 0's sorted order; the same lane owns these elements in every column pass)
      float* o = pc + (size_t)I[L.MC + j0 + jl].x * sl0 + a_ * K0 + b.kbase;
#pragma unroll
      for (int y = 0; y < KB; ++y) {
        const int kk = (k0t + y) * 16 + i16;
        if (kk < b.krows) o[kk] = accum ? o[kk] + acc[y][r] : acc[y][r];
      }
    }
  }
}

// all d core_0 tiles of one lookup pass and block, spread over the waves
__device__ __forceinline__ void gemm_da(const Dims& d, const Lds& L, const float* smem, const Blk& b, int j0, int lenS,
                                        float* __restrict__ pc, bool accum) {
  const int w = threadIdx.x / kWave;
  const int mtiles = (lenS * d.q[0] + 15) / 16;
  int KB = 4;
  while (KB > 1 && mtiles * ((L.KBt + KB - 1) / KB) < kWaves) KB >>= 1;
  const int ngroups = (L.KBt + KB - 1) / KB;
  for (int job = w; job < mtiles * ngroups; job += kWaves) {
    const int mt = job / ngroups, g = job - mt * ngroups;
    int k0t = g * KB;
    int cnt = min(KB, L.KBt - k0t);
    while (cnt > 0) {
      if (cnt >= 4) { da_group<4>(d, L, smem, b, mt, k0t, j0, lenS, pc, accum); k0t += 4; cnt -= 4; }
      else if (cnt >= 2) { da_group<2>(d, L, smem, b, mt, k0t, j0, lenS, pc, accum); k0t += 2; cnt -= 2; }
      else { da_group<1>(d, L, smem, b, mt, k0t, j0, lenS, pc, accum); k0t += 1; cnt -= 1; }
    }
  }
}

// T == 2: d x_0 of a lookup pass is the bag gradient itself, [q0 x q1], zero-padded to the MFMA tile
__device__ __forceinline__ void bwd_load_dx0(const Dims& d, const Lds& L, float* smem, int B, int table,
                                             const int64_t* __restrict__ rowidx, const float* __restrict__ d_output,
                                             const Partials& PC, int j0, int lenS) {
  const int tid = threadIdx.x;
  const int q0 = d.q[0], D = d.D;
  const int4* I = (const int4*)(smem + L.oI);
  float* X0 = smem + L.oX0;
  for (int e = tid; e < L.rS * L.ld; e += kThreads) X0[e] = 0.f;
  __syncthreads();
  for (int e = tid; e < lenS * D; e += kThreads) {
    unsigned rem, col;
    const unsigned jl = fdivmod((unsigned)e, L.fdD, rem);
    const unsigned a = fdivmod(rem, L.fdN1, col);
    X0[(jl * q0 + a) * L.ld + col] = d_output[((size_t)table * B + rowidx[I[j0 + jl].x]) * D + rem] *
                                     (PC.psw ? PC.psw[I[j0 + jl].x] : 1.f);
  }
  __syncthreads();
}

// the per-lookup tail of one (column pass, lookup pass), T >= 3: X0 holds x_0's block; leaves d x_0 there and adds
// the pass's share to the thin cores' partials (accum: a later column pass)
__device__ __forceinline__ void bwd_tail(const Dims& d, const CorePtrs& C, const Lds& L, float* smem, const Partials& PC,
                                         const Blk& b, int j0, int lenS, bool accum) {
  const int T = d.T, q0 = d.q[0], D = d.D;
  const int4* I = (const int4*)(smem + L.oI);
  const int4* IP = I + L.MC;  // rows of the lookups' thin-core partials (bwd_kernel)
  float* X0 = smem + L.oX0;
  float* X1 = smem + L.oX1;
  float* Gb = smem + L.oG;
  const int q1 = d.q[1];
  if (T == 4) {
    // x_1 = x_0 * core_2[i_2]  (needed by the gradient of core 3)
    const int k1 = d.k[1], n1 = d.n[1];
    const RowMap rm{b.nbp, q1, b.b0};
    const int m1p = q0 * b.nbp;
    if (n1 <= 8) {
#define CALL(NT) fwd_stage<NT>(lenS, j0, m1p, k1, rm, q0 * L.ld, L.ld, k1, X0, nullptr, 0, false, C.c[2], d.slice[2], I, 2, \
                               X1, L.szX1, nullptr, D)
      TTX_NT_SWITCH(n1, CALL)
#undef CALL
    } else {
      fwd_stage_any(lenS, j0, m1p, k1, n1, rm, q0 * L.ld, L.ld, k1, X0, C.c[2], d.slice[2], I, 2, X1, L.szX1, nullptr, D);
    }
    __syncthreads();
    // stage t = 2 on x_1 (rows (a, b, c) x k2) with G = bag gradient rows a*q1*q2 + b0*q2 + (bl*q2 + c)
    const int k2 = d.k[2], n2 = d.n[2], q2 = d.q[2];
    const int nb = b.nbp * q2;
    if (n2 <= 8) {
#define CALL(NT) bwd_stage_fused<NT>(lenS, j0, k2, q0, nb, L.szX1, nb * k2, k2, X1, Gb, D, j0, q1 * q2, b.b0 * q2, \
                                     C.c[3], d.slice[3], I, IP, 3, PC.pc[3], accum)
      TTX_NT_SWITCH(n2, CALL)
#undef CALL
    } else {
      bwd_stage_any(lenS, j0, k2, n2, q0, nb, L.szX1, nb * k2, k2, X1, Gb, D, j0, q1 * q2, b.b0 * q2, C.c[3], d.slice[3],
                    I, IP, 3, PC.pc[3], accum);
    }
    __syncthreads();
  }
  // stage t = 1 on x_0 (row (a, bl) at a*ld + bl*k1) with G1 = bag gradient (T == 3) or d x_1 (the pass's own rows)
  {
    const int k1 = d.k[1], n1 = d.n[1];
    const float* Gin = (T == 3) ? Gb : X1;
    const int gJ = (T == 3) ? D : L.szX1;
    const int gBase = (T == 3) ? j0 : 0;
    const int gA = (T == 3) ? q1 : b.nbp, gB0 = (T == 3) ? b.b0 : 0;
    if (n1 <= 8) {
#define CALL(NT) bwd_stage_fused<NT>(lenS, j0, k1, q0, b.nbp, q0 * L.ld, L.ld, k1, X0, Gin, gJ, gBase, gA, gB0, \
                                     C.c[2], d.slice[2], I, IP, 2, PC.pc[2], accum)
      TTX_NT_SWITCH(n1, CALL)
#undef CALL
    } else {
      bwd_stage_any(lenS, j0, k1, n1, q0, b.nbp, q0 * L.ld, L.ld, k1, X0, Gin, gJ, gBase, gA, gB0, C.c[2], d.slice[2], I, IP,
                    2, PC.pc[2], accum);
    }
    __syncthreads();
  }
}

// the slice as ONE block, several lookup passes: d core_1 held in registers across the passes
// (KB = r1 tiles, <= 2 jobs/wave)
template <int KB>
__device__ __forceinline__ void bwd_passes(const Dims& d, const CorePtrs& C, const Lds& L, float* smem, int B,
                                           int table, const int64_t* __restrict__ rowidx,
                                           const float* __restrict__ d_output, const Partials& PC, const Blk& b,
                                           int chunk, int len) {
  const int w = threadIdx.x / kWave;
  const int npairs = (L.N1t + 1) / 2;
  f32x4 acc0[2][KB], acc1[2][KB];
  db1_zero<KB>(acc0);
  db1_zero<KB>(acc1);
  const int np0 = w, np1 = w + kWaves;
  const int npass = (len + L.SC - 1) / L.SC;
  for (int h = 0; h < npass; ++h) {
    const int j0 = h * L.SC;
    const int lenS = min(L.SC, len - j0);
    if (h > 0) __syncthreads();  // the previous pass is done with X0 / X1
    if (d.T == 2) {
      bwd_load_dx0(d, L, smem, B, table, rowidx, d_output, PC, j0, lenS);
    } else {
      if (!(L.dbg & 1)) gemm_x0(d, L, smem, h, b.n1t, nullptr, j0, lenS, false);  // recompute x_0 of this pass
      __syncthreads();
      if (!(L.dbg & 2)) bwd_tail(d, C, L, smem, PC, b, j0, lenS, false);
    }
    if (!(L.dbg & 4)) {
      if (np0 < npairs) {
        if (np0 * 2 + 1 < L.N1t) db1_accum<KB, true>(L, smem, h, np0, 0, acc0);
        else db1_accum<KB, false>(L, smem, h, np0, 0, acc0);
      }
      if (np1 < npairs) {
        if (np1 * 2 + 1 < L.N1t) db1_accum<KB, true>(L, smem, h, np1, 0, acc1);
        else db1_accum<KB, false>(L, smem, h, np1, 0, acc1);
      }
    }
    if (!(L.dbg & 8)) gemm_da(d, L, smem, b, j0, lenS, PC.pc[0], false);
  }
  float* pc = PC.pc[1] + (size_t)chunk * d.slice[1];
  if (np0 < npairs) db1_store<KB>(d, b, np0, 0, acc0, pc);
  if (np1 < npairs) db1_store<KB>(d, b, np1, 0, acc1, pc);
}

__global__ __launch_bounds__(kThreads, 3) void bwd_kernel(Dims d, Plan P, CorePtrs C, int B,
                                                         const int64_t* __restrict__ rowidx,
                                                         const float* __restrict__ d_output,
                                                         Partials PC, Lds L) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  zero_hot_counters(PC);
  const int chunk = blockIdx.x;
  const int4 cr = P.chunk_rec[chunk];
  const int s = cr.x, start = cr.y, len = cr.z;
  if (len == 0) return;
  const int tid = threadIdx.x;
  const int D = d.D;
  if (L.dbg & 16) return;
  int4* I = (int4*)(smem + L.oI);
  if (tid < len) {  // partial gradients of the thin cores are stored in the cores' SORTED order (Plan::ipos)
    const int4 rec = P.lrec[start + tid];
    const int n = rec.x;
    I[tid] = rec;
    I[L.MC + tid] = make_int4(P.ipos[0][n], 0, d.T > 2 ? P.ipos[2][n] : 0, d.T > 3 ? P.ipos[3][n] : 0);
  }
  __syncthreads();
  const int table = PC.tableidx ? (int)PC.tableidx[I[0].x] : s / d.p[1];
  if (d.T >= 3) {
    // bag gradients of the chunk's lookups
    float* Gb = smem + L.oG;
    if ((D & 3) == 0) {
      const int d4 = D / 4;
      for (int e = tid; e < len * d4; e += kThreads) {
        unsigned rem;
        const unsigned j = fdivmod((unsigned)e, L.fdD4, rem);
        float4 gq = ((const float4*)(d_output + ((size_t)table * B + rowidx[I[j].x]) * D))[rem];
        if (PC.psw) { const float sw = PC.psw[I[j].x]; gq.x *= sw; gq.y *= sw; gq.z *= sw; gq.w *= sw; }
        ((float4*)Gb)[e] = gq;
      }
    } else {
      for (int e = tid; e < len * D; e += kThreads) {
        unsigned rem;
        const unsigned j = fdivmod((unsigned)e, L.fdD, rem);
        Gb[e] = d_output[((size_t)table * B + rowidx[I[j].x]) * D + rem] * (PC.psw ? PC.psw[I[j].x] : 1.f);
      }
    }
    // (visible to the tail after the barriers of the staging round)
  }
  if (L.persist) {
    const Blk b = make_blk(d, L, 0, 0);
    stage_block(d, C, L, smem, s, len, b, false);
    const int kb = L.KBt <= 1 ? 1 : (L.KBt <= 2 ? 2 : 4);
    if (kb == 1) bwd_passes<1>(d, C, L, smem, B, table, rowidx, d_output, PC, b, cr.w, len);
    else if (kb == 2) bwd_passes<2>(d, C, L, smem, B, table, rowidx, d_output, PC, b, cr.w, len);
    else bwd_passes<4>(d, C, L, smem, B, table, rowidx, d_output, PC, b, cr.w, len);
    return;
  }
  // one lookup pass (SC == MC), the slice block by block; d core_1 tiles computed and stored group by group
  const int w = tid / kWave;
  float* pc1 = PC.pc[1] + (size_t)cr.w * d.slice[1];  // .w = the chunk's partial slot
  bool first = true;
  for (int cp = 0; cp < L.ncp; ++cp) {
    int resident = -1;  // K block in LDS
    if (d.T == 2) {
      bwd_load_dx0(d, L, smem, B, table, rowidx, d_output, PC, 0, len);
    } else {
      for (int kb = 0; kb < L.nkb; ++kb) {
        const Blk b = make_blk(d, L, cp, kb);
        stage_block(d, C, L, smem, s, len, b, !first);
        first = false;
        resident = kb;
        if (!(L.dbg & 1)) gemm_x0(d, L, smem, 0, b.n1t, nullptr, 0, len, kb > 0);
      }
      __syncthreads();
      if (!(L.dbg & 2)) bwd_tail(d, C, L, smem, PC, make_blk(d, L, cp, 0), 0, len, cp > 0);
    }
    for (int i = 0; i < L.nkb; ++i) {
      const int kb = (d.T == 2) ? i : L.nkb - 1 - i;  // (the last K block of the recompute is still staged)
      const Blk b = make_blk(d, L, cp, kb);
      if (kb != resident) {
        stage_block(d, C, L, smem, s, len, b, !first);
        first = false;
        resident = kb;
      }
      const int npairs = (b.n1t + 1) / 2;
      if (!(L.dbg & 4)) {
        for (int np = w; np < npairs; np += kWaves) {
          const bool two = (np * 2 + 1) < b.n1t;
          for (int k0t = 0; k0t < L.KBt; k0t += 4) {
            f32x4 acc[2][4];
            db1_zero<4>(acc);
            if (two) db1_accum<4, true>(L, smem, 0, np, k0t, acc);
            else db1_accum<4, false>(L, smem, 0, np, k0t, acc);
            db1_store<4>(d, b, np, k0t, acc, pc1);
          }
        }
      }
      if (!(L.dbg & 8)) gemm_da(d, L, smem, b, 0, len, PC.pc[0], cp > 0);
    }
  }
}

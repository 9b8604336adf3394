// ttx_tt_spec.inc -- shape-specialised, wave-independent contraction kernels (3 cores, q0 == 4).
// Included by ttx_tt.hip (shares CorePtrs / Partials / mfma4 / Plan).
//
// Why: hardware counters of the generic kernels (profiles/r01_generic_pmc.md) show ~19 non-MFMA
// instructions per MFMA and 39 % of wave time parked on barriers/waitcnt -- instruction-issue
// bound, MFMA pipe 19 % busy.  For the benchmark's shape family everything that costs
// instructions can be removed:
//   * all extents are template constants: index arithmetic folds away, loops unroll;
//   * a wave owns one 16-row M tile = 4 lookups (q0 = 4) end to end, so there is NO block barrier
//     in the main loop -- waves drift apart and one wave's MFMA phase hides another's VALU phase;
//   * with q0 = 4 and r2 % 16 == 0 the MFMA C/D layout puts, for lookup j = lane>>4 and column
//     kk = h*16 + (lane&15), all 16 rows (a, b) of x_0 into ONE lane: acc[b*HH + h][a].  The fused
//     backward tail (d core_2 partial and d x_0) therefore runs on the accumulator registers
//     directly, no LDS round trip for x_0;
//   * d core_1: whenever a pass has a multiple of four column tiles (every instantiated shape), wave w owns
//     column tiles over ALL waves' rows -- A and d x_0 of every tile sit in LDS -- so after one barrier it
//     multiplies them for its columns and stores the result: 2*K0T accumulator tiles, no reduction
//     (Shape3::COOP).  Otherwise it is accumulated per wave over the wave's groups and reduced across the
//     four waves through LDS;
//   * x_0's q1 column blocks are never mixed by the tail, so a shape can walk them in NP passes
//     (Shape3::NP): only that block of core_1 is staged, which is what makes r = 64 fit and what runs
//     fastest at r = 32 (one M-tile per wave, next block of core_1 in flight).
// Same plan, same partial-buffer contract and the same reduce_apply kernel as the generic path;
// same summation orders inside a lookup, so results agree with the generic kernels to rounding.

#ifndef TTX_SETPRIO
#define TTX_SETPRIO 0
#endif
#if TTX_SETPRIO
#define TTX_PRIO(x) __builtin_amdgcn_s_setprio(x)
#else
#define TTX_PRIO(x) do {} while (0)
#endif

#ifndef TTX_WGS32
#define TTX_WGS32 2
#endif
#ifndef TTX_MFMA_TAIL
#define TTX_MFMA_TAIL 1
#endif
#ifndef TTX_BFS
#define TTX_BFS 1
#endif
#ifndef TTX_GPP
#define TTX_GPP 1
#endif
#ifndef TTX_LATEB
#define TTX_LATEB 1
#endif
template <int R1_, int Q1_, int R2_, int Q2_, int NP_ = 1, int MC_ = 32, int Q0_ = 4>
struct Shape3 {
  static constexpr int Q0 = Q0_, R1 = R1_, Q1 = Q1_, R2 = R2_, Q2 = Q2_;
  static constexpr int LPG = 16 / Q0;                  // lookups per 16-row group (q0 = 4: 4, q0 = 2: 8)
  // A lane's four accumulator rows kq*4 + r belong to LPR lookups of the group: row r is core-0 row r % Q0 of lookup
  // kq*LPR + r / Q0 (q0 = 4: the one lookup kq; q0 = 2: two lookups, two rows each)
  static constexpr int LPR = 4 / Q0;
  static_assert(Q0 == 4 || Q0 == 2, "q0 = 4 or 2");
  // Column passes: x_0 has N1 = q1*r2 columns, made of q1 blocks of r2 that the tail never mixes.
  // NP == 1 keeps all of them in accumulator registers at once (r <= 32).  For r = 64 that would
  // be 64 + 256 accumulator registers and 66 KB of core_1 in LDS, so the kernels walk the q1
  // blocks in NP passes of PW columns: only that block of core_1 is staged, d core_1 of the block
  // is reduced and stored per pass, d core_0 / d core_2 accumulate across passes in registers.
  static constexpr int NP = NP_, MC = MC_;             // passes, lookups per chunk
  // r = 64, q0 = 4 (round 4): the backward stages its lookups' gradient rows PER COLUMN PASS -- the 4*BPP*Q2 values the pass's
  // tail reads, re-read from L2 every pass -- instead of whole rows of D: 57.8 -> 51.8 KB of LDS at q = [4,4,8], which is what
  // lets a THIRD work-group onto the CU (160 KB; the registers were at 168 already)
  // (round 5: also wherever whole rows would be 1024+ floats per lookup -- q1 = 16, q2 = 32: 66 .. 131 KB of LDS, one work-group per CU or
  //  none -- with up to four float4 per lane and pass: Shape3::NPL)
  static constexpr bool GPP = TTX_GPP && (R1_ == 64 || Q0_ * Q1_ * Q2_ >= 1024) && Q0_ == 4 && NP_ > 1;
  // partial gradients leave the backward kernel with non-temporal stores: they are read once, by the next
  // kernel, and a plain store parks 17 MB of dirty lines in L2 that the end of the kernel has to write back
  // (measured: step -3.8 % at r = 32, -2.8 % at 327k lookups, +1.4 % at r = 64 -> off there)
  static constexpr bool NT = R1_ <= 32;
  // ... and (exact shapes) as whole float4s: d core_0 and the cooperative d core_1 are computed TRANSPOSED (MFMA operands swapped:
  // the same products summed in the same order), so that an accumulator's four registers are four consecutive floats of one partial
  // row.  A 16-byte store can go write-through (sc1) at the price of a plain one -- a 4-byte one cannot -- which is what lets the
  // launch choose the flavour by its partial bytes (PStore, partial_store_flavour below).  OldStores<S> switches it off; the
  // padded variants and the sub-chunk walk (MULTI) do not have it (spec_bwd_kernel).
  static constexpr bool W16 = NT;
  // large batches may put several sub-chunks of MC lookups into one chunk of the plan (kernel variant MULTI)
  static constexpr bool SUB_ = R1_ <= 32 && Q2_ <= 8;  // (q2 = 16: the walk's operands in flight do not fit the registers)
  // d core_1 of a pass: with as many column tiles as waves (or a multiple), wave w
  // computes column tiles [w*TPW, (w+1)*TPW) over ALL four waves' rows, straight from the A / d x_0 regions the
  // waves already keep in LDS -- TPW*K0T accumulator tiles instead of PNT*K0T, one barrier instead of a
  // cross-wave reduction through LDS (measured 2.7 us of the 19.6 us kernel at the benchmark shape)
  static constexpr bool COOP = (Q1_ * R2_ / NP_ / 16) % kWaves == 0;
  static constexpr int TPW = COOP ? (Q1_ * R2_ / NP_ / 16) / kWaves : (Q1_ * R2_ / NP_ / 16);
  static constexpr int GPW = MC / (LPG * kWaves);      // 16-row groups (LPG lookups) per wave
  static constexpr bool SUB = SUB_ && COOP;            // (sub-chunks need the cooperative d core_1)
  static constexpr int K0 = R1, K0P = R1 < 32 ? 32 : R1, K0T = R1 / 16;
  static constexpr int N1 = Q1 * R2, HH = R2 / 16;
  static constexpr int PW = N1 / NP, PNT = PW / 16, BPP = Q1 / NP;  // pass width, its tiles, its q1 blocks
  static constexpr int D = Q0 * Q1 * Q2;
  static constexpr int SL0 = Q0 * R1, SL1 = R1 * N1, SL2 = R2 * Q2;
  static constexpr int LD = (PW + 29) / 32 * 32 + 2;   // == 2 (mod 32): row stride of a wave's x_0 / d x_0 tile
  // The WHOLE core_1 slice stays staged while the accumulators walk it in NP column passes, wherever it is at most 17 KB
  // (r = 32 with q1 = 4: 16.6 KB; round 4).  Column passes used to re-stage their block every pass of every sub-chunk -- two
  // work-group barriers and 8 KB from L2 into LDS each time, for a slice that is the same for all lookups of the chunk.  Staged
  // once per chunk, the forward has no barrier at all after it and the backward only those of the cooperative d core_1.
  static constexpr int LDBF = (N1 + 29) / 32 * 32 + 2;
  static constexpr bool BFS = TTX_BFS && NP_ > 1 && K0P * LDBF <= 4352;
  static constexpr int LDB = BFS ? LDBF : LD;          // row stride of the staged core_1 block (== 2 mod 32 as well)
  static constexpr int BW = BFS ? N1 : PW;             // its width
  static constexpr int LDA = (K0P + 29) / 32 * 32 + 2;
  static constexpr int szB = (K0P * LDB + 3) / 4 * 4;
  static constexpr int szA = 16 * LDA, szX = (16 * LD + 3) / 4 * 4;
  // LDS: [B block][A of wave 0..3][X of wave 0..3][per-wave gradient rows (bwd) / last-core slices (fwd)]
  // RG: groups per wave whose A / X / gradient regions stay resident (column passes re-read A every pass,
  // the cooperative d core_1 reads every group's A and d x_0); otherwise one region per wave is reused
  static constexpr int RG = (NP_ > 1 || COOP) ? GPW : 1;
  static constexpr int oB = 0, oA = szB, oX = oA + kWaves * RG * szA, oG = oX + kWaves * RG * szX;
  // gradient rows of the group's 4 lookups: row stride D + 4 floats, so that the four lookups' broadcast float4
  // reads of the backward tail fall on different banks
  static constexpr int GD = GPP ? 4 * BPP * Q2 + 4 : D + 4;  // (GPP: [a][block of the pass][x] of one lookup)
  static constexpr int NPL = GPP ? (BPP * Q2 + 15) / 16 : 1;  // (GPP) float4s of a lookup's pass values per lane of its quarter
  static constexpr int szGb = LPG * GD, szGf = LPG * SL2;
  // forward, TRANSPOSED accumulators (round 4): with the MFMA operands swapped the x_0 tile comes out with the lookup ROW in
  // the lane (i16 = row (lookup, a)) and the r2 index spread over (register r, lane quarter kq): kk = h*16 + kq*4 + r.  The last
  // core then contracts inside the lane quarter over its 4*HH values of kk and only the four quarters are left to be summed --
  // two v_permlane{32,16}_swap reduce-scatter steps (NVT/2 + NVT/4 swaps) instead of a 16-lane butterfly of NV - NV/16
  // ds_bpermute + 2 v_cndmask steps (rounds 1-3).  q0 = 4 (FMT): the in-quarter contraction runs on v_mfma_f32_4x4x1 (a block of
  // four lanes = the four rows of one lookup); q0 = 2: on v_fma with C2T last-core values per lane.
  static constexpr int C2T = HH * 4 * Q2;           // last-core values a lane holds per group (VALU tail)
  static constexpr bool FMT = TTX_MFMA_TAIL && Q0 == 4;
  static constexpr int NVT = BPP * Q2;              // values of one output row (lookup, a) per pass
  static constexpr int PERT = NVT / 4;              // ... of which a lane ends up with PERT
  static_assert(NVT % 4 == 0 && (PERT == 1 || PERT == 2 || PERT % 4 == 0), "reduce-scatter over the four lane quarters");
  static_assert(FMT || GPW * C2T <= 128, "the VALU forward tail keeps C2T last-core values per group in registers");
  // one column pass: the staged block is the whole core_1 slice -- the sub-chunks of a chunk share it (staged once)
  static constexpr bool B1ONCE = NP_ == 1 || BFS;
  // backward tail on the matrix pipe (v_mfma_f32_4x4x1, see spec_bwd_kernel): one lookup per lane quarter
  static constexpr bool MT = TTX_MFMA_TAIL && LPR == 1;
  static_assert(!GPP || MT, "per-pass gradient rows are read by the MFMA tail");
  static constexpr int lds_floats_bwd = oG + kWaves * RG * szGb, lds_floats_fwd = oX;
  // work-groups per CU the kernels are compiled for: r = 128 stages 137 KB of LDS -- one work-group, the whole register file;
  // r = 64 with per-pass gradient rows: three where the backward's LDS allows (160 KB per CU), 168 registers
  // (round 5: q1 = 16 and q2 = 32 stage 66 KB of whole gradient rows -- one work-group per CU whatever the rank, and the register file with it)
  static constexpr int WGS = (R1_ > 64 || lds_floats_bwd * 4 * 2 > 160 * 1024) ? 1
                             : (R1_ <= 32 ? TTX_WGS32 : ((GPP && lds_floats_bwd * 4 * 3 <= 160 * 1024) ? 3 : 2));
  static_assert(R1 % 16 == 0 && R2 % 16 == 0 && N1 % 16 == 0 && Q1 % NP == 0, "tile-aligned ranks only");
  static_assert(K0T * TPW <= 16, "d core_1 accumulators of one pass (per wave) must fit the register file");
  static_assert(MC % (LPG * kWaves) == 0 && GPW >= 1, "");
  static_assert(Q2 <= 32 && Q2 % 4 == 0 && D % 4 == 0, "");
  static constexpr int BV4 = (K0 * BW / 4 + kThreads - 1) / kThreads;  // float4 rounds of the work-group over a core_1 block
  static constexpr bool BFULL = (K0 * BW / 4) % kThreads == 0;         // (whole rounds: no predicate in the staging loops)
  static_assert((K0 * BW / 4) % kThreads == 0 || K0 * BW / 4 < kThreads, "core_1 block staging: whole float4 rounds, or part of one");
  // the cross-wave d core_1 reduction reuses the X regions: one r1 tile row (PNT tiles) per round
  static_assert(kWaves * PNT * 256 <= kWaves * szX, "reduction scratch");
};
#ifdef TTX_TEST_HOOKS
// A/B (test library, ttx_debug_skip bit 18): the same shape with the partial gradients stored as before -- products in the
// C/D layout, 4-byte non-temporal stores.  A type of its own, so the product library instantiates nothing for it.
template <class S_>
struct OldStores : S_ {
  static constexpr bool W16 = false;
};
#endif

// lookup records (+ bag rows) of a wave's groups, one per lane: lane l < LPG*GPW holds record l%LPG of the wave's group
// l/LPG.  Only the fused-pooling forward still uses this form (one lane per lookup counts its bag's arrival); the operands
// are fetched through lane_rec below.  (Cold scalar loads serialise through the scalar cache, and a select-chain over
// broadcast copies gets lowered to a dynamically indexed scratch array: both were measured to cost microseconds.)
struct WaveRecs {
  int4 rec;  // {n, sid_0, sid_2, sid_3}, x = -1 for a missing lookup
  int row;   // bag row, -1 if the plan carries none
};
template <int GPW, int LPG>
__device__ __forceinline__ WaveRecs load_recs(const Plan& P, int start, int len, int w, bool has_row) {
  const int lane = lane_id();
  const int gi = lane / LPG, c = lane % LPG;
  const int pos = (w + gi * kWaves) * LPG + c;  // lookup position inside the chunk
  WaveRecs r;
  r.rec = make_int4(-1, 0, 0, 0);
  r.row = -1;
  if (lane < LPG * GPW && pos < len) {
    r.rec = P.lrec[start + pos];
    if (has_row) r.row = P.lrow[start + pos];
  }
  return r;
}
// ---- padded shapes (round 3, PAD variants of the kernels): a geometry with q0 <= Q0, q1 <= Q1, q2 <= Q2, r1 <= R1,
// r2 <= R2 runs on the template's tiles -- ranks that are not multiples of 16 (the reference tests' 13 / 12), factors like
// q = [3, 4, 5].  Only the global loads and stores know: they translate between the REAL layouts in HBM (cores, gradient
// rows, output rows, partial gradients: exactly what the reference / reduce_apply see) and the template's padded tiles,
// reading zeros for what lies outside and storing nothing there.  Everything between -- LDS layouts, MFMA loops, register
// tails -- is the exact-shape kernel.  (Vector loads become four guarded scalar loads: real rows are not 16-byte aligned.)
struct RealDims {
  int q0, q1, q2, r1, r2;
  int sl0, sl1, sl2, n1, D;  // q0 r1 | r1 q1 r2 | r2 q2 | q1 r2 | q0 q1 q2
  // (read by every variant, PAD or not) the last core is PER LOOKUP, in pivot order: slice index = the lookup's position in the
  // plan, and so is the row of its partial gradient -- four cores on these kernels, the last two contracted beforehand (ttx_tt.hip)
  int c2n;
  // bit 0 / 1 / 2: r1 / r2 / q2 is a multiple of 4 (and the arrays are 16-byte aligned) -- the rows of core 0 / of core 1's blocks /
  // of the last core, the gradient and output rows and the d core_2 partials then start on a float4 and hold whole float4s, and the
  // padded variants' guarded loads / stores of them go by float4 (a guard per vector), like the exact kernels'.  (Round 4: sixteen
  // guarded 4-byte non-temporal stores per lane and kk row of d core_2, lane stride q2 floats, were 263 of the padded backward's
  // 357 us at q = [4,8,16], ranks [24,32].)
  int v4;
  // (read by the single-sub-chunk kernels) table of pivot slice s = table_quot(s, tmul, tsh) (ttx_magic.h): s / p_1 as the host's
  // magic pair -- 0 whatever s with one table -- in place of the ~30 instructions of a division between the chunk record and
  // the lookup records' requests
  unsigned tmul;
  int tsh;
};
// one guarded element of a padded variant.  (A branch-free form -- load from `p` or from a valid dummy address, select afterwards --
// was measured slower: ranks [13,12] 0.0456 against 0.0438 ms/step.)
__device__ __forceinline__ float ld_guard(const float* __restrict__ p, bool ok, const float* __restrict__ /*safe*/) {
  return ok ? *p : 0.f;
}
// four consecutive elements src[0..4) of which the first `nvalid` exist (nvalid <= 0: none)
__device__ __forceinline__ float4 ld4_guard(const float* __restrict__ src, int nvalid, const float* __restrict__ safe, bool v4) {
  if (v4) {  // (kernel-uniform, RealDims::v4: then nvalid is a multiple of 4 and src a float4)
    const float4 t = *(const float4*)(nvalid > 0 ? src : safe);
    return nvalid > 0 ? t : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  return make_float4(ld_guard(src, nvalid > 0, safe), ld_guard(src + 1, nvalid > 1, safe), ld_guard(src + 2, nvalid > 2, safe),
                     ld_guard(src + 3, nvalid > 3, safe));
}

// columns [pass*PW, (pass+1)*PW) of B1 -> registers -> LDS (zero rows K0..K0P when r1 = 16)
template <class S>
struct BBlock { float4 v[S::BV4]; };
template <class S, bool PAD = false>
__device__ __forceinline__ void spec_fetch_b(const float* __restrict__ B1, int pass, BBlock<S>& b, const RealDims& R) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < S::BV4; ++i) {
    const int e = tid + i * kThreads;
    const int row = e / (S::BW / 4), c4 = e % (S::BW / 4);
    const int col0 = S::BFS ? 0 : pass * S::PW;           // (BFS: the whole slice, whatever the pass)
    if (S::BFULL || e < S::K0 * S::BW / 4) {
      if constexpr (!PAD) {
        b.v[i] = *(const float4*)(B1 + (size_t)row * S::N1 + col0 + c4 * 4);
      } else {
        const int col = col0 + c4 * 4;                    // padded column: q1 block col / R2, r2 index col % R2
        const int bq = col / S::R2, kk = col % S::R2;
        b.v[i] = ld4_guard(B1 + (size_t)row * R.n1 + bq * R.r2 + kk, (row < R.r1 && bq < R.q1) ? R.r2 - kk : 0, B1, (R.v4 & 2) != 0);
      }
    }
  }
}
template <class S>
__device__ __forceinline__ void spec_put_b(const BBlock<S>& b, float* Bs) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < S::BV4; ++i) {
    const int e = tid + i * kThreads;
    const int row = e / (S::BW / 4), c4 = e % (S::BW / 4);
    if (S::BFULL || e < S::K0 * S::BW / 4) {
      float2* dst = (float2*)(Bs + row * S::LDB + c4 * 4);
      dst[0] = make_float2(b.v[i].x, b.v[i].y);
      dst[1] = make_float2(b.v[i].z, b.v[i].w);
    }
  }
}
// once per work-group: zero rows K0..K0P of Bs (r1 = 16) and this wave's A region (columns K0..K0P stay zero)
// (ALLA: the whole A region -- the backward's cooperative d core_1 multiplies EVERY group's A rows, also those of a group
//  without lookups that nobody wrote: they must be finite.  The forward reads only what it wrote, and columns K0..K0P.)
template <class S, bool ALLA>
__device__ __forceinline__ void spec_zero_pads(float* Bs, float* Aw) {
  const int tid = threadIdx.x, lane = lane_id();
  if (S::K0P != S::K0)
    for (int e = tid; e < (S::K0P - S::K0) * S::LDB; e += kThreads) Bs[S::K0 * S::LDB + e] = 0.f;
  if (ALLA || S::K0P != S::K0)
    for (int e = lane; e < S::RG * S::szA; e += kWave) Aw[e] = 0.f;  // (the wave's RG regions are contiguous)
}

// X0[16 x PW] = Aw * Bs into accumulator registers (k-step {k, k+8, k+16, k+24}).  TRANS: the two MFMA operands swapped --
// the same products summed in the same order, the tile comes out transposed: lane (kq, i16) holds
// x_0[row i16][column x*16 + kq*4 + r] in acc[x][r] instead of x_0[row kq*4 + r][column x*16 + i16].
template <class S, bool TRANS = false>
__device__ __forceinline__ void spec_gemm_x0(const float* Aw, const float* Bs, f32x4 (&acc)[S::PNT]) {
  const int lane = lane_id();
  const int i16 = lane & 15, kq = lane >> 4;
  const float* arow = Aw + i16 * S::LDA + 8 * kq;
  const float* bbase = Bs + 8 * kq * S::LDB + i16;
#pragma unroll
  for (int x = 0; x < S::PNT; ++x) acc[x] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float bcur[S::PNT];
#pragma unroll
  for (int x = 0; x < S::PNT; ++x) bcur[x] = bbase[x * 16];
  TTX_PRIO(1);
#pragma unroll
  for (int kb = 0; kb < S::K0P; kb += 32) {
    float a[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) a[t] = arow[kb + t];
    __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int kn = (t < 7) ? kb + t + 1 : kb + 32;
      const float* bn = bbase + (kn < S::K0P ? kn : 0) * S::LDB;
      float bnxt[S::PNT];
#pragma unroll
      for (int x = 0; x < S::PNT; ++x) bnxt[x] = bn[x * 16];
#pragma unroll
      for (int x = 0; x < S::PNT; ++x) acc[x] = TRANS ? mfma4(bcur[x], a[t], acc[x]) : mfma4(a[t], bcur[x], acc[x]);
#pragma unroll
      for (int x = 0; x < S::PNT; ++x) bcur[x] = bnxt[x];
      __builtin_amdgcn_sched_group_barrier(0x100, (S::PNT + 1) / 2, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, S::PNT, 0);
    }
  }
  TTX_PRIO(0);
}

// accumulator tile set -> Xw[16 x LD] (C/D layout: row = kq*4 + r, col = x*16 + i16)
template <class S>
__device__ __forceinline__ void spec_store_x(const f32x4 (&acc)[S::PNT], float* Xw) {
  const int lane = lane_id();
  float* xo = Xw + ((lane >> 4) * 4) * S::LD + (lane & 15);
#pragma unroll
  for (int x = 0; x < S::PNT; ++x)
#pragma unroll
    for (int r = 0; r < 4; ++r) xo[r * S::LD + x * 16] = acc[x][r];
}

// reduce-scatter steps over the lane QUARTERS (lane bits 32 and 16) on gfx950's half-exchange instructions:
// v_permlane32_swap(x, y) leaves [x.lo | y.lo] and [x.hi | y.hi] (lo / hi = lanes 0..31 / 32..63), v_permlane16_swap the same
// over odd / even 16-lane rows -- their sum is, in the lanes with the bit clear, x of both halves, in the others y of both:
// one swap + one add per value kept.  VALU, no LDS pipe, no select.
template <int N, int CAP>
__device__ __forceinline__ void swap32_step(float (&v)[CAP]) {
#pragma unroll
  for (int i = 0; i < N / 2; ++i) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[i]), __float_as_uint(v[i + N / 2]), false, false);
    v[i] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
  }
}
template <int N, int CAP>
__device__ __forceinline__ void swap16_step(float (&v)[CAP]) {
#pragma unroll
  for (int i = 0; i < N / 2; ++i) {
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v[i]), __float_as_uint(v[i + N / 2]), false, false);
    v[i] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
  }
}

// ---- bag pooling inside the forward kernel (small batches) -----------------------------------------------------------
// The separate pooling launch re-reads rows the contraction has just written and costs ~5 us of a 43 us step for a
// 2.6 MB sum.  Fused: a wave publishes its lookups' rows WRITE-THROUGH (sc1 stores), drains them, and counts every
// lookup into its bag's arrival counter; the lookup that completes a bag sums the bag's rows IN INDEX ORDER -- the
// order of the reference's reduce_output_kernel (tt_embeddings_cuda.cu:920-962) and of pool4_small_kernel, so the
// output is bit-identical to the unfused path's -- with sc1 loads (the rows may come from any CU on any XCD:
// MI355X_MICROARCH.md "inter-workgroup visibility", cdna_hip_programming.md Guideline 16 R1) and writes the bag's output row.
// Counters: `arrive[first lookup of the bag]`, zero on entry; the completing lookup resets its counter, so the array
// is zero again when the kernel ends (the caller keeps ONE zero-initialised array per stream; no memset per call).
struct PoolFuse {
  int* arrive;              // [nnz]; NULL = pooling stays a launch of its own
  const int64_t* offsets;   // [bags + 1], include_last_offset form, table-major bags
  const int64_t* rowidx;    // bag row of lookup n (used when the plan carries none)
  const int64_t* tableidx;  // table of lookup n (tables of different row factors), or NULL: table = pivot slice / p1
  const float* psw;         // per_sample_weights by lookup, or NULL
  float* out;               // [bags][D]
  int B, bags, p1;
  unsigned rows_bytes;      // extent of `rows` (buffer descriptor)
  int dbg;                  // ablation (timing only): 1 = no arrival at all, 2 = arrivals but no pooling of completed bags
};

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
#ifndef TTX_POOL_NF
#define TTX_POOL_NF 24
#endif
constexpr int kPoolNF = TTX_POOL_NF;  // rows in flight per 16-lane group of a completing lookup
constexpr int kAuxSc1 = 16;  // raw buffer op cache policy: sc1 = write-through store / L1-bypassing load
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);
}
// N = 4 / 2 / 1 consecutive floats at byte offset `off` of the buffer, write-through
template <int N>
__device__ __forceinline__ void st_sc1(__amdgpu_buffer_rsrc_t rs, unsigned off, const float* v) {
  if constexpr (N == 4) {
    const u32x4 w = {__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])};
    __builtin_amdgcn_raw_buffer_store_b128(w, rs, (int)off, 0, kAuxSc1);
  } else if constexpr (N == 2) {
    const u32x2 w = {__float_as_uint(v[0]), __float_as_uint(v[1])};
    __builtin_amdgcn_raw_buffer_store_b64(w, rs, (int)off, 0, kAuxSc1);
  } else {
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[0]), rs, (int)off, 0, kAuxSc1);
  }
}
__device__ __forceinline__ float4 ld4_sc1(__amdgpu_buffer_rsrc_t rs, unsigned off) {
  const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)off, 0, kAuxSc1);
  return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}

// empty bags get their zeros here (every other bag is written, whole, by the lookup that completes it)
__device__ __forceinline__ void zero_empty_bags(const PoolFuse& F, int D) {
  const int d4 = D / 4;
  for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < (long long)F.bags * d4; e += (long long)gridDim.x * kThreads) {
    const int bag = (int)(e / d4);
    if (F.offsets[bag + 1] == F.offsets[bag]) ((float4*)F.out)[e] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// arrival of the wave's lookups + pooling of the bags they complete.  bstart / blen: first lookup and length of the bag
// of the lookup this lane holds the record of (lanes < nrec; blen == 0: no lookup).  Wave-uniform call, after the
// wave's row stores.
template <int D>
__device__ __forceinline__ void pool_arrive(const PoolFuse& F, __amdgpu_buffer_rsrc_t rrows, int bstart, int blen, int bag) {
  const int lane = lane_id(), q = lane >> 4, l16 = lane & 15;
  if (F.dbg & 1) return;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's rows have left for memory (write-through)
  // (round 3 advisor: the sc1 policy bits and the waitcnt order the HARDWARE; the fences order the COMPILER as well -- a release in
  //  front of the count, an acquire behind the count that completes a bag -- so that neither the row stores nor the pooled loads
  //  can be moved across the relaxed atomic)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  bool done = false;
  if (blen > 0) {
    const int old = __hip_atomic_fetch_add(F.arrive + bstart, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    done = old + 1 == blen;
    if (done) __hip_atomic_store(F.arrive + bstart, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (nobody else counts into it any more)
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  unsigned long long m = __ballot(done);
  if (F.dbg & 2) m = 0;
  while (m) {  // (wave-uniform) up to four completed bags per round, one per 16-lane quarter
    unsigned long long mm = m;
    for (int i = 0; i < q; ++i) mm &= mm - 1;
    const int src = mm ? __ffsll((long long)mm) - 1 : 0;
    const bool act = mm != 0;
    const int n0 = __shfl(bstart, src, kWave), len = act ? __shfl(blen, src, kWave) : 0, bg = __shfl(bag, src, kWave);
    constexpr int D4 = D / 4;
#pragma unroll
    for (int e0 = 0; e0 < D4; e0 += 16) {
      const int e = e0 + l16;
      const bool ev = (D4 % 16 == 0) || e < D4;
      float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
      // kPoolNF rows in flight (the registers of the contraction are free by now), added in index order: the benchmark's
      // 20-lookup bags take ONE round of loads -- every round is a trip to memory at the very end of the kernel
      for (int j = 0; j < len; j += kPoolNF) {
        float4 v[kPoolNF];
#pragma unroll
        for (int u = 0; u < kPoolNF; ++u)
          if (j + u < len && ev) v[u] = ld4_sc1(rrows, (unsigned)(((size_t)(n0 + j + u) * D4 + e) * 16));
#pragma unroll
        for (int u = 0; u < kPoolNF; ++u)
          if (j + u < len && ev) {
            if (F.psw) {
              const float wj = F.psw[n0 + j + u];
              acc.x = fmaf(wj, v[u].x, acc.x); acc.y = fmaf(wj, v[u].y, acc.y); acc.z = fmaf(wj, v[u].z, acc.z); acc.w = fmaf(wj, v[u].w, acc.w);
            } else {
              acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; acc.w += v[u].w;
            }
          }
      }
      if (act && ev) ((float4*)F.out)[(size_t)bg * D4 + e] = acc;
    }
    m &= m - 1; m &= m - 1; m &= m - 1; m &= m - 1;  // the four lowest are done
  }
}

// record of lookup `jl` (0..LPG-1) of the wave's group `gi`, read by the lane that needs it: the 16 (or more) lanes that share a
// lookup read the same 16 bytes -- one request -- and nothing has to cross lanes afterwards (rounds 1-3 loaded one record per lane
// and handed them round with ds_bpermute: 12-17 LDS-pipe instructions per group).  x = -1 for a lookup beyond the chunk.
template <class S>
__device__ __forceinline__ int4 lane_rec(const Plan& P, int start, int len, int w, int gi, int jl, int c2n) {
  const int pos = (w + gi * kWaves) * S::LPG + jl;
  int4 r = make_int4(-1, 0, 0, 0);
  if (pos < len) {
    r = P.lrec[start + pos];
    if (c2n) r.z = r.x;  // (RealDims::c2n: the last core's slices are per LOOKUP -- M_n, ttx_tt.hip)
  }
  return r;
}

// PER consecutive finished values of an output row at float offset `at` of `rows` (aligned to PER floats, at most a float4 at a time)
template <int PER, bool FUSE>
__device__ __forceinline__ void spec_store_out(float* __restrict__ rows, __amdgpu_buffer_rsrc_t rrows, size_t at, const float* v) {
  if constexpr (PER >= 4) {
#pragma unroll
    for (int j = 0; j < PER; j += 4) {
      if constexpr (FUSE) st_sc1<4>(rrows, (unsigned)((at + j) * 4), v + j);
      else *(float4*)(rows + at + j) = make_float4(v[j], v[j + 1], v[j + 2], v[j + 3]);
    }
  } else if constexpr (FUSE) {
    st_sc1<PER>(rrows, (unsigned)(at * 4), v);
  } else if constexpr (PER == 2) {
    *(float2*)(rows + at) = make_float2(v[0], v[1]);
  } else {
    rows[at] = v[0];
  }
}

// what the forward of one (sub-)chunk fetches per wave.  Transposed accumulators: lane (quarter kq, i16) works for ROW i16 of
// the group's 16-row tile = core-0 row a = i16 % Q0 of lookup jl = i16 / Q0.
template <class S>
struct FwdLoads {
  static constexpr int NC2 = S::FMT ? S::HH * 4 * (S::Q2 / 4) : S::C2T;  // last-core values a lane holds per group
  int4 rec[S::GPW];
  float4 av[S::GPW][S::K0T];  // row i16 of the group's stacked core-0 slices, columns 4*(kq + 4i) ..
  // FMT: [(h*4 + r)*(Q2/4) + xb] = core_2[kk = h*16 + kq*4 + r][4*xb + (lane & 3)];  else [(h*4 + r)*Q2 + x] = core_2[kk][x]
  float c2[S::GPW][NC2];
};
// stage 1 of the chain: the records as they lie in the plan.  (Round 6, as in the backward: nothing here READS what it requests -- a
// default merged with the loaded record, the RealDims::c2n fix-up behind the load, were register copies of a value just requested,
// i.e. a wait for every load the wave had issued for the next sub-chunk in front of it.  A lane behind the sub-chunk's end
// fetches the sub-chunk's first record and stage 2 discards it by position.)
template <class S>
struct FwdRecs {
  int4 rec[S::GPW];
  int len;
};
template <class S>
__device__ __forceinline__ void fwd_load_recs(FwdRecs<S>& Q, const Plan& P, int start, int len, int w) {
  const int jl = (lane_id() & 15) / S::Q0;
  Q.len = len;
#pragma unroll
  for (int gi = 0; gi < S::GPW; ++gi) {
    const int pos = (w + gi * kWaves) * S::LPG + jl;
    Q.rec[gi] = P.lrec[start + (pos < len ? pos : 0)];
  }
}
template <class S, bool PAD>
__device__ __forceinline__ void fwd_load(FwdLoads<S>& L, const FwdRecs<S>& Q, const CorePtrs& C, const RealDims& R) {
  const int lane = lane_id(), i16 = lane & 15, kq = lane >> 4, t4 = lane & 3;
  const int a = i16 % S::Q0;
  int4 rec[S::GPW];
#pragma unroll
  for (int gi = 0; gi < S::GPW; ++gi) {
    const bool there = ((int)threadIdx.x / kWave + gi * kWaves) * S::LPG + i16 / S::Q0 < Q.len;
    rec[gi] = there ? Q.rec[gi] : make_int4(-1, 0, 0, 0);
    if (R.c2n) rec[gi].z = rec[gi].x;  // (RealDims::c2n: the last core's slices are per LOOKUP -- M_n, ttx_tt.hip)
  }
#pragma unroll
  for (int gi = 0; gi < S::GPW; ++gi) {
    L.rec[gi] = rec[gi];
    const bool live = rec[gi].x >= 0;
    const size_t sid0 = (size_t)(live ? rec[gi].y : 0), sid2 = (size_t)(live ? rec[gi].z : 0);
#pragma unroll
    for (int i = 0; i < S::K0T; ++i) {
      const int k = 4 * (kq + 4 * i);
      L.av[gi][i] = make_float4(0.f, 0.f, 0.f, 0.f);
      if constexpr (!PAD) {
        if (live) L.av[gi][i] = *(const float4*)(C.c[0] + sid0 * S::SL0 + a * S::K0 + k);
      } else {
        L.av[gi][i] = ld4_guard(C.c[0] + sid0 * R.sl0 + a * R.r1 + k, (live && a < R.q0) ? R.r1 - k : 0, C.c[0], (R.v4 & 1) != 0);
      }
    }
#pragma unroll
    for (int hr = 0; hr < S::HH * 4; ++hr) {
      const int kk = (hr / 4) * 16 + kq * 4 + hr % 4;
      if constexpr (S::FMT) {
#pragma unroll
        for (int xb = 0; xb < S::Q2 / 4; ++xb) {
          const int x = 4 * xb + t4;
          if constexpr (!PAD) L.c2[gi][hr * (S::Q2 / 4) + xb] = C.c[2][sid2 * S::SL2 + kk * S::Q2 + x];
          else L.c2[gi][hr * (S::Q2 / 4) + xb] = ld_guard(C.c[2] + sid2 * R.sl2 + kk * R.q2 + x, kk < R.r2 && x < R.q2, C.c[2]);
        }
      } else if constexpr (!PAD) {
        const float4* cg = (const float4*)(C.c[2] + sid2 * S::SL2 + kk * S::Q2);
#pragma unroll
        for (int x4 = 0; x4 < S::Q2 / 4; ++x4) {
          const float4 t = cg[x4];
          L.c2[gi][hr * S::Q2 + 4 * x4] = t.x; L.c2[gi][hr * S::Q2 + 4 * x4 + 1] = t.y;
          L.c2[gi][hr * S::Q2 + 4 * x4 + 2] = t.z; L.c2[gi][hr * S::Q2 + 4 * x4 + 3] = t.w;
        }
      } else {
        const float* cg = C.c[2] + sid2 * R.sl2 + kk * R.q2;
#pragma unroll
        for (int x4 = 0; x4 < S::Q2 / 4; ++x4) {
          const float4 t = ld4_guard(cg + 4 * x4, kk < R.r2 ? R.q2 - 4 * x4 : 0, C.c[2], (R.v4 & 4) != 0);
          L.c2[gi][hr * S::Q2 + 4 * x4] = t.x; L.c2[gi][hr * S::Q2 + 4 * x4 + 1] = t.y;
          L.c2[gi][hr * S::Q2 + 4 * x4 + 2] = t.z; L.c2[gi][hr * S::Q2 + 4 * x4 + 3] = t.w;
        }
      }
    }
  }
}

// ---- kernarg preload (round 6).  gfx950's command processor can put the first 14 dwords of the kernel arguments into SGPRs
// before the first wave starts (-mllvm -amdgpu-kernarg-preload-count, .amdhsa_user_sgpr_kernarg_preload_length) -- plain
// pointers / integers only, a struct passed by value is not eligible.  The contraction kernels are a chain of dependent trips to
// memory (kernel arguments -> chunk record -> lookup records -> operands): the seven pointers the first three trips need lead
// the argument list as plain pointers and replace the struct members, so the chunk record is requested by the wave's first
// instruction instead of behind an s_load of the argument segment.  (TTX_NO_KHEAD: the old argument list, for A/B builds.)
#ifndef TTX_NO_KHEAD
#define TTX_KHEAD_PARAMS const int4* k_chunk_rec, const int4* k_lrec, const int* k_lrow, const int* k_hdr, const float* k_c0, \
                         const float* k_c1, const float* k_c2,
#define TTX_KHEAD_ARGS(P, C) (P).chunk_rec, (P).lrec, (P).lrow, (P).hdr, (C).c[0], (C).c[1], (C).c[2],
#define TTX_KHEAD_ADOPT(P, C)                                                                                         \
  do {                                                                                                                \
    (P).chunk_rec = const_cast<int4*>(k_chunk_rec); (P).lrec = const_cast<int4*>(k_lrec); (P).lrow = const_cast<int*>(k_lrow); \
    (P).hdr = const_cast<int*>(k_hdr); (C).c[0] = const_cast<float*>(k_c0); (C).c[1] = const_cast<float*>(k_c1);       \
    (C).c[2] = const_cast<float*>(k_c2);                                                                              \
  } while (0)
#else
#define TTX_KHEAD_PARAMS
#define TTX_KHEAD_ARGS(P, C)
#define TTX_KHEAD_ADOPT(P, C) do { } while (0)
#endif
// chunk record of work-group b, addressed as pointer + 32-bit byte offset: the scalar load then takes the offset in a register of
// its own and reads THROUGH the pointer's registers -- the ones it arrived in with the wave -- instead of through a 64-bit sum
// that has to be formed first (16 b < 2^32: a plan has fewer than 2^28 chunk slots)
__device__ __forceinline__ int4 chunk_record(const int4* __restrict__ recs, unsigned b) {
  return *(const int4*)((const char*)recs + b * 16u);
}
template <class S, bool MULTI, bool FUSE = false, bool PAD = false>
__global__ __launch_bounds__(kThreads, S::WGS) void spec_fwd_kernel(TTX_KHEAD_PARAMS Plan P, CorePtrs C, float* __restrict__ rows,
                                                             float* __restrict__ zout, long long nzero, PoolFuse F, RealDims R) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  static_assert(!FUSE || (!MULTI && !PAD), "fused pooling: single sub-chunk, exact shape");
  TTX_KHEAD_ADOPT(P, C);
  // (the sub-chunk walk zeroes first, as it always did: its entry is paid once per several sub-chunks)
  constexpr bool EARLY = !MULTI;
  if constexpr (!EARLY) {
    if constexpr (FUSE) zero_empty_bags(F, S::D);
    else zero_output(zout, nzero);
  }
  const int4 cr = EARLY ? chunk_record(P.chunk_rec, blockIdx.x) : P.chunk_rec[blockIdx.x];
  // (round 6) the whole record HERE: the compiler fetched its three words one after the other, each in front of the branch that
  // reads it first (length -> slice -> start: three trips of the scalar cache in a row)
  // (single sub-chunk: ... and with it every argument that does not arrive with the wave and that the path to the first MFMA
  //  reads.  Left to the compiler, each was fetched in front of its first use and waited for there: the output to zero and its
  //  length, two dependent trips to the argument segment in FRONT of the chunk record's request, and RealDims::c2n in the
  //  middle of the operand requests.  All of them are one round of the scalar cache now, the chunk record's.)
  if constexpr (!EARLY) {
    asm volatile("" ::"s"(cr.x), "s"(cr.y), "s"(cr.z));
  } else if constexpr (FUSE) {
    asm volatile("" ::"s"(cr.x), "s"(cr.y), "s"(cr.z), "s"(rows), "s"(R.c2n), "s"(R.tmul), "s"(R.tsh), "s"(F.arrive), "s"(F.offsets),
                 "s"(F.rowidx), "s"(F.tableidx), "s"(F.psw), "s"(F.out), "s"(F.B), "s"(F.bags), "s"(F.rows_bytes), "s"(F.dbg));
    zero_empty_bags(F, S::D);
  } else {
    const int grid = P.max_chunks;  // (zero_output's stride: the launch's grid is the plan's chunk slots, an argument like the others)
    asm volatile("" ::"s"(cr.x), "s"(cr.y), "s"(cr.z), "s"(rows), "s"(zout), "s"(nzero), "s"(R.c2n), "s"(grid));
    zero_output(zout, nzero, (unsigned)grid);
  }
  const int s = cr.x, start0 = cr.y, len0 = cr.z;
  if (len0 == 0) return;
  const int lane = lane_id(), w = threadIdx.x / kWave;
  const int i16 = lane & 15, kq = lane >> 4, t4 = lane & 3;
  const __amdgpu_buffer_rsrc_t rrows = make_rsrc(rows, FUSE ? F.rows_bytes : 0u);
  float* Bs = smem + S::oB;
  float* Aw0 = smem + S::oA + w * S::RG * S::szA;  // this wave's A region(s)
  const float* B1 = C.c[1] + (size_t)s * (PAD ? R.sl1 : S::SL1);
  const int nsub = MULTI ? (len0 + S::MC - 1) / S::MC : 1;
  const int a = i16 % S::Q0;
  FwdRecs<S> rq;          // records in flight (MULTI: of the sub-chunk after the next)
  FwdLoads<S> cur, nxt;   // operands of this sub-chunk / (MULTI) in flight for the next: the chain records -> operands runs
                          // ahead of the arithmetic, as in spec_bwd_kernel
  BBlock<S> bb;
  if constexpr (MULTI) {
    fwd_load_recs<S>(rq, P, start0, min(S::MC, len0), w);
    fwd_load<S, PAD>(cur, rq, C, R);
    if (nsub > 1) fwd_load_recs<S>(rq, P, start0 + S::MC, min(S::MC, len0 - S::MC), w);
    spec_fetch_b<S, PAD>(B1, 0, bb, R);
    if constexpr (S::B1ONCE) {  // the slice is staged here, once, outside the walk (its registers are free inside)
      spec_zero_pads<S, false>(Bs, Aw0);
      spec_put_b<S>(bb, Bs);
      __syncthreads();
    }
  }
  int sc = 0;
  do {  // sub-chunks of S::MC lookups (see spec_bwd_kernel)
  const int start = MULTI ? start0 + sc * S::MC : start0, len = MULTI ? min(S::MC, len0 - sc * S::MC) : len0;
  const int ngroups = (len + S::LPG - 1) / S::LPG;
  if (MULTI && sc > 0 && !S::B1ONCE) __syncthreads();  // everyone is done with the previous sub-chunk's core_1 block
  // ---- every global load of this wave is issued here, before any compute ----
  int bstart = 0, blen = 0, bag = 0;  // fused pooling: the bag of the lookup this lane holds the record of
  if constexpr (FUSE) {
    const bool has_row = P.hdr[3] != 0;
    const WaveRecs wr = load_recs<S::GPW, S::LPG>(P, start, len, w, has_row);
    if (wr.rec.x >= 0) {
      const long long tb = F.tableidx ? F.tableidx[wr.rec.x] : (long long)table_quot((unsigned)s, R.tmul, R.tsh);  // (= s / F.p1)
      const long long row = has_row ? (long long)wr.row : F.rowidx[wr.rec.x];
      bag = (int)(tb * F.B + row);
      const long long o0 = F.offsets[bag], o1 = F.offsets[bag + 1];
      bstart = (int)o0;
      blen = (int)(o1 - o0);
      // (offsets that do not describe this lookup -- not the ones its bag row came from -- must not leave a counter
      //  behind: such a lookup is written as a row and counted nowhere)
      if (wr.rec.x < o0 || wr.rec.x >= o1) blen = 0;
    }
  }
  if constexpr (!MULTI) {
    fwd_load_recs<S>(rq, P, start, len, w);
#ifndef TTX_B1_LATE
    spec_fetch_b<S, PAD>(B1, 0, bb, R);  // (behind the records' requests, in front of the wait for them: the slice travels under it)
    fwd_load<S, PAD>(cur, rq, C, R);
#else
    fwd_load<S, PAD>(cur, rq, C, R);
    spec_fetch_b<S, PAD>(B1, 0, bb, R);
#endif
  } else if (sc + 1 < nsub) {
    fwd_load<S, PAD>(nxt, rq, C, R);
    if (sc + 2 < nsub) fwd_load_recs<S>(rq, P, start0 + (sc + 2) * S::MC, min(S::MC, len0 - (sc + 2) * S::MC), w);
  }
  int4 (&rec)[S::GPW] = cur.rec;
  float4 (&av)[S::GPW][S::K0T] = cur.av;
  float (&c2)[S::GPW][FwdLoads<S>::NC2] = cur.c2;
  if (!MULTI || (sc == 0 && !S::B1ONCE)) spec_zero_pads<S, false>(Bs, Aw0);
#pragma unroll
  for (int pass = 0; pass < S::NP; ++pass) {
    // the staged core_1: a block per column pass -- or (Shape3::B1ONCE) the whole slice once per chunk, after which the waves
    // of a forward work-group never meet again
    if (pass > 0 && !S::B1ONCE) __syncthreads();  // every wave is done with the previous block
    if (S::B1ONCE ? (pass == 0 && !MULTI) : true) {
      spec_put_b<S>(bb, Bs);
      if (!S::B1ONCE) {
        if (pass + 1 < S::NP) spec_fetch_b<S, PAD>(B1, pass + 1, bb, R);  // next block in flight
        else if (MULTI && sc + 1 < nsub) spec_fetch_b<S, PAD>(B1, 0, bb, R);  // ... the next sub-chunk's first
      }
      __syncthreads();
    }
    const float* Bp = Bs + (S::BFS ? pass * S::PW : 0);  // this pass's columns of the staged block
#pragma unroll
    for (int gi = 0; gi < S::GPW; ++gi) {
      const int g = w + gi * kWaves;
      if (g >= ngroups) continue;  // (no break: the loop must unroll so gi stays a constant)
      float* Aw = Aw0 + (S::RG > 1 ? gi : 0) * S::szA;
      if (S::NP == 1 || pass == 0) {
#pragma unroll
        for (int i = 0; i < S::K0T; ++i) {
          float2* dst = (float2*)(Aw + i16 * S::LDA + 4 * (kq + 4 * i));
          dst[0] = make_float2(av[gi][i].x, av[gi][i].y);
          dst[1] = make_float2(av[gi][i].z, av[gi][i].w);
        }
      }
      f32x4 acc[S::PNT];
      spec_gemm_x0<S, true>(Aw, Bp, acc);
      const int nrow = rec[gi].x;
      // Tail: lane (kq, i16) holds x_0[row i16][bl*R2 + h*16 + kq*4 + r] in acc[bl*HH + h][r]; its quarter's share of
      // out[lookup][a][bl][x] is the sum over its 4*HH values of kk; the four quarters are then summed by a reduce-scatter over
      // lane bits 32 and 16.  No LDS round trip of x_0 (round 1: 43 % of the LDS tail's cycles were bank conflicts), no
      // ds_bpermute, no select.
      constexpr int NVT = S::NVT, PERT = S::PERT;
      float v[NVT];
      if constexpr (S::FMT) {
        // ... on the matrix pipe (q0 = 4: the four lanes of a 4x4x1 block are the four rows a of ONE lookup):
        // D[lane 4b+j][reg i] += A[lane 4b+i] * B[lane 4b+j] with A = x_0 (row a = i), B = core_2[kk][4*xb + j]  ->  lane
        // (kq, jl, j = lane & 3) ends with out[jl][a = reg][bl][4*xb + j] over its quarter of kk: v[(a*BPP + bl)*(Q2/4) + xb].
        // BPP*HH*Q2 small MFMAs per pass for 4*BPP*HH*Q2 v_fma, and a quarter of the last-core registers.
#pragma unroll
        for (int bl = 0; bl < S::BPP; ++bl)
#pragma unroll
          for (int xb = 0; xb < S::Q2 / 4; ++xb) {
            f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int h = 0; h < S::HH; ++h)
#pragma unroll
              for (int r = 0; r < 4; ++r) o = mfma1(acc[bl * S::HH + h][r], c2[gi][(h * 4 + r) * (S::Q2 / 4) + xb], o);
#pragma unroll
            for (int i = 0; i < 4; ++i) v[(i * S::BPP + bl) * (S::Q2 / 4) + xb] = o[i];
          }
      } else {
#pragma unroll
        for (int bl = 0; bl < S::BPP; ++bl)
#pragma unroll
          for (int x = 0; x < S::Q2; ++x) {
            float sacc = 0.f;
#pragma unroll
            for (int h = 0; h < S::HH; ++h)
#pragma unroll
              for (int r = 0; r < 4; ++r) sacc = fmaf(acc[bl * S::HH + h][r], c2[gi][(h * 4 + r) * S::Q2 + x], sacc);
            v[bl * S::Q2 + x] = sacc;
          }
      }
      swap32_step<NVT>(v);
      swap16_step<NVT / 2>(v);
      // quarter kq ends with values kq*PERT .. kq*PERT + PERT-1 of the NVT
      if constexpr (S::FMT) {
        // value idx = (a*BPP + bl)*(Q2/4) + xb of lane (.., jl, j) is out[jl][a][pass*BPP + bl][4*xb + j]: the four lanes of a
        // block store 16 contiguous bytes per value
        if (nrow >= 0) {
#pragma unroll
          for (int u = 0; u < PERT; ++u) {
            const int idx = kq * PERT + u;
            const int ao = idx / (S::BPP * (S::Q2 / 4)), bl = (idx / (S::Q2 / 4)) % S::BPP, x = 4 * (idx % (S::Q2 / 4)) + t4;
            const int bq = pass * S::BPP + bl;
            if constexpr (PAD) {
              if (ao < R.q0 && bq < R.q1 && x < R.q2) rows[(size_t)nrow * R.D + (ao * R.q1 + bq) * R.q2 + x] = v[u];
            } else {
              spec_store_out<1, FUSE>(rows, rrows, (size_t)nrow * S::D + (ao * S::Q1 + bq) * S::Q2 + x, v + u);
            }
          }
        }
      } else if constexpr (PAD) {
        if (nrow >= 0 && a < R.q0) {
#pragma unroll
          for (int j = 0; j < PERT; ++j) {
            const int idx = kq * PERT + j;
            const int bq = pass * S::BPP + idx / S::Q2, x = idx % S::Q2;
            if (bq < R.q1 && x < R.q2) rows[(size_t)nrow * R.D + (a * R.q1 + bq) * R.q2 + x] = v[j];
          }
        }
      } else if (nrow >= 0) {
        // (the offset is a multiple of PERT floats and rows is 256-B aligned: vector stores are aligned)
        spec_store_out<PERT, FUSE>(rows, rrows, (size_t)nrow * S::D + (a * S::Q1 + pass * S::BPP) * S::Q2 + kq * PERT, v);
      }
    }
  }
  if constexpr (FUSE) pool_arrive<S::D>(F, rrows, bstart, blen, bag);
  if constexpr (MULTI) cur = nxt;
  } while (MULTI && ++sc < nsub);  // sub-chunks
}

template <bool NT>
__device__ __forceinline__ void spec_st(float v, float* p) {
  if (NT) __builtin_nontemporal_store(v, p); else *p = v;
}

template <bool NT>
__device__ __forceinline__ void spec_st4(const f32x4& v, float* p) {
  if (NT) __builtin_nontemporal_store(v, (f32x4*)p); else *(f32x4*)p = v;
}

// How a launch's 16-byte partial-gradient stores (Shape3::W16) leave the backward, chosen per LAUNCH by the host
// (partial_store_flavour): kernel-uniform, a scalar branch around each of the three store sites.
//   kStNt  non-temporal: no dirty line left for the end of the kernel, and the rows do not stay on-die either
//   kStWt  write-through (sc1): no dirty line, and reduce_apply -- the next launch -- finds the rows in the Infinity Cache
//   kStPl  plain (test library only, for the measurement)
// b0 / b1 / b2: bytes of pc[0], of ONE chunk's pc[1] slot, of pc[2] -- the write-through stores are buffer stores and are bounds-checked.
enum { kStNt = 0, kStWt = 1, kStPl = 2 };
struct PStore {
  int flav;
  unsigned b0, b1, b2;
};
// float4 `v` to float offset `at` of `base` (rs = the same buffer as a descriptor; FLAV is a constant at every call)
template <int FLAV>
__device__ __forceinline__ void st_part4(const f32x4& v, float* __restrict__ base, __amdgpu_buffer_rsrc_t rs, size_t at) {
  if constexpr (FLAV == kStWt) {
    __builtin_amdgcn_raw_buffer_store_b128((u32x4){__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])},
                                           rs, (int)(unsigned)(at * 4), 0, kAuxSc1);
  } else {
    spec_st4<FLAV == kStNt>(v, base + at);
  }
}
// the same call under the launch's flavour (CALL names the constant FLAV)
#define TTX_BY_FLAVOUR(flav, CALL)                                  \
  do {                                                              \
    if ((flav) == kStWt) { constexpr int FLAV = kStWt; CALL; }      \
    else if ((flav) == kStPl) { constexpr int FLAV = kStPl; CALL; } \
    else { constexpr int FLAV = kStNt; CALL; }                      \
  } while (0)
// The three store sites (Shape3::W16), a float4 per lane and store.
// d core_2 of a group: v[k][h][x4] = values 4*x4 .. +3 of row kk = h*16 + i16 of the partial of the lane's lookup k
template <class S, int FLAV>
__device__ __forceinline__ void st_pc2_rows(const f32x4 (&v)[S::LPR][S::HH][S::Q2 / 4], const bool (&live)[S::LPR], const int (&pos2)[S::LPR],
                                            float* __restrict__ pc2, __amdgpu_buffer_rsrc_t rs) {
  const int i16 = lane_id() & 15;
#pragma unroll
  for (int k = 0; k < S::LPR; ++k)
    if (live[k]) {
#pragma unroll
      for (int h = 0; h < S::HH; ++h)
#pragma unroll
        for (int x4 = 0; x4 < S::Q2 / 4; ++x4)
          st_part4<FLAV>(v[k][h][x4], pc2, rs, (size_t)pos2[k] * S::SL2 + (h * 16 + i16) * S::Q2 + 4 * x4);
    }
}
// d core_0 of a group, transposed accumulators: lane (kq, i16) holds columns y*16 + kq*4 .. +3 of tile row i16 = core-0 row
// i16 % Q0 of lookup i16 / Q0, whose partial is row `pos` (< 0: no such lookup)
template <class S, int FLAV>
__device__ __forceinline__ void st_pc0_rows(const f32x4 (&da)[S::K0T], int pos, float* __restrict__ pc0, __amdgpu_buffer_rsrc_t rs) {
  const int lane = lane_id(), i16 = lane & 15, kq = lane >> 4;
  if (pos < 0) return;
  const size_t at = (size_t)pos * S::SL0 + (i16 % S::Q0) * S::K0 + kq * 4;
#pragma unroll
  for (int y = 0; y < S::K0T; ++y) st_part4<FLAV>(da[y], pc0, rs, at + y * 16);
}
// the cooperative d core_1 of a pass, transposed accumulators: lane (kq, i16) holds columns kq*4 .. +3 of column tile w*TPW + x,
// row y*16 + i16 of the chunk's slot
template <class S, int FLAV>
__device__ __forceinline__ void st_pc1_tiles(const f32x4 (&acc)[S::K0T][S::TPW], float* __restrict__ pc1, __amdgpu_buffer_rsrc_t rs, int pass,
                                             int w) {
  const int lane = lane_id(), i16 = lane & 15, kq = lane >> 4;
#pragma unroll
  for (int y = 0; y < S::K0T; ++y)
#pragma unroll
    for (int x = 0; x < S::TPW; ++x)
      st_part4<FLAV>(acc[y][x], pc1, rs, (size_t)(y * 16 + i16) * S::N1 + pass * S::PW + (w * S::TPW + x) * 16 + kq * 4);
}

// everything the backward of one (sub-)chunk fetches from global memory, per wave -- issued in one go so that
// the dependent chain records -> operands is paid once (and, with sub-chunks, one sub-chunk ahead).
// Lane (quarter kq, i16) works for the LPR lookups kq*LPR + k of a group (the lookups of its four accumulator rows): it reads
// their records itself (lane_rec) and fetches ITS quarter's share of the group's core-0 slices and gradient rows -- float4s
// i16, i16 + 16, .. of the quarter's LPR*SL0 / LPR*D floats -- so no record has to cross lanes (round 3: ds_bpermute x 17 per group).
template <class S>
struct BwdLoads {
  static constexpr int NG4 = (S::LPR * S::D / 4 + 15) / 16;  // float4s of gradient rows per lane and group
  float4 av[S::GPW][S::K0T];                  // core_0 slices of the quarter's lookups
  float4 gv4[S::GPW][NG4];                    // their bags' gradient rows
  float gsw4[S::GPW][NG4];                    // ... and the per_sample_weight each is multiplied by on its way to LDS (bwd_put; 1
                                              // without weights: multiplied where it was loaded, the product and the plain value
                                              // met behind the branch -- a copy, i.e. a wait for the load, in front of the
                                              // last-core rows' requests)
  f32x4 c2q[S::GPW][S::LPR][S::HH][S::Q2 / 4];  // last-core rows of this lane's (lookup, kk) items: value x = c2q[..][x / 4][x % 4] (whole
                                              // float4s as they are loaded: four floats of one load in four unrelated registers were
                                              // copied there behind the load -- a wait for it in every sub-chunk's prologue)
  int4 myrec[S::GPW][S::LPR];                 // records of the lookup(s) of this lane's accumulator rows (Shape3::LPR)
  int pos0[S::GPW][S::LPR], pos2[S::GPW][S::LPR];  // rows of their d core_0 / d core_2 partials (Plan::ipos)
  // (Shape3::GPP) the lookup's gradient values are fetched per column pass: where pass 0's float4 of this lane lies (lane i16 <
  // BPP*Q2 of the quarter: values [a = i16 / (BPP*Q2/4)][block][x]; nullptr: nothing to fetch), and the lookup's per_sample_weight
  const float* gp[S::GPW][S::NPL];
  float gsw[S::GPW];
};
// which of the quarter's LPR lookups element e of its stacked block (LPR blocks of `per` floats) belongs to, as a value that
// is a compile-time constant wherever it can be.  (LPR == 2 only: a run-time k selects by ARITHMETIC between the two records'
// fields -- a select of two array elements becomes a dynamically indexed load, i.e. scratch.)
template <class S>
__device__ __forceinline__ int pick2(const int (&f)[S::LPR], int k) { return f[0] + (f[S::LPR - 1] - f[0]) * k; }
// stage 1 of the chain: the lookup records (and bag rows, when the plan carries them) of the lane's lookups
template <class S>
struct BwdRecs {
  int4 rec[S::GPW][S::LPR];
  int bagrow[S::GPW][S::LPR];
  int len;  // lookups of the sub-chunk the records belong to (a record at a position >= len is not one)
};
// (Round 6: nothing here may READ what it has just requested, and stage 2 requests nothing that depends on another of its requests.
//  `s_waitcnt vmcnt` counts every vector memory instruction in issue order: the fix-up of a record behind its load, the bag row
//  fetched under `rec.x >= 0`, a bag row from rowidx[] in stage 2 in front of the gradient rows' addresses -- each made the wave
//  wait for ALL the loads it had just issued for the NEXT sub-chunk, three trips to memory in a row in every sub-chunk's prologue.
//  The record is kept as loaded (RealDims::c2n is applied where it is read), the bag row is fetched by position, and only a plan
//  without bag rows pays a dependent load -- here, once.)
template <class S>
__device__ __forceinline__ void bwd_load_recs(BwdRecs<S>& Q, const Plan& P, int start, int len, int w, bool has_row,
                                              const int64_t* __restrict__ rowidx) {
  const int kq = lane_id() >> 4;
  Q.len = len;
  int at[S::GPW][S::LPR];
#pragma unroll
  for (int gi = 0; gi < S::GPW; ++gi)
#pragma unroll
    for (int k = 0; k < S::LPR; ++k) {
      // a lane behind the sub-chunk's end fetches the sub-chunk's first record (always there) and stage 2 discards it by POSITION:
      // a default value merged with the loaded one is a register copy of what has just been requested -- a wait for it
      const int pos = (w + gi * kWaves) * S::LPG + kq * S::LPR + k;
      at[gi][k] = start + (pos < len ? pos : 0);
      Q.rec[gi][k] = P.lrec[at[gi][k]];
    }
  // (the records in front of the branch, only the bag rows under it: where two paths meet, a value both define must sit in ONE
  //  register, and the copy that puts it there waits for its load)
  if (has_row) {
#pragma unroll
    for (int gi = 0; gi < S::GPW; ++gi)
#pragma unroll
      for (int k = 0; k < S::LPR; ++k) Q.bagrow[gi][k] = P.lrow[at[gi][k]];
  } else {
#pragma unroll
    for (int gi = 0; gi < S::GPW; ++gi)
#pragma unroll
      for (int k = 0; k < S::LPR; ++k) Q.bagrow[gi][k] = (int)rowidx[Q.rec[gi][k].x];
  }
}
// stage 2: everything the records address
// UNC (the single-sub-chunk kernels): core-0 slices and gradient rows are requested unconditionally (below).  The sub-chunk walk
// keeps the conditional form: there the allocator answers the unconditional one by copying two components of a slice load
// just requested into the registers `cur = nxt` will want -- a wait inside the prefetch block (tests/test_kernel_resources.py).
template <class S, bool PAD = false, bool UNC = false>
__device__ __forceinline__ void bwd_load(BwdLoads<S>& L, const BwdRecs<S>& Q, const Plan& P, const CorePtrs& C, const Partials& PC,
                                         bool has_row, int table, int B,
                                         const int64_t* __restrict__ rowidx, const float* __restrict__ d_output,
                                         const RealDims& R) {
  const int lane = lane_id(), i16 = lane & 15;
  int bagrow[S::GPW][S::LPR];
#pragma unroll
  for (int gi = 0; gi < S::GPW; ++gi)
#pragma unroll
    for (int k = 0; k < S::LPR; ++k) {
      const bool there = ((int)threadIdx.x / kWave + gi * kWaves) * S::LPG + (lane >> 4) * S::LPR + k < Q.len;
      L.myrec[gi][k] = there ? Q.rec[gi][k] : make_int4(-1, 0, 0, 0);
      if (R.c2n) L.myrec[gi][k].z = L.myrec[gi][k].x;  // (RealDims::c2n: the last core's slices are per LOOKUP -- M_n, ttx_tt.hip)
      bagrow[gi][k] = there ? Q.bagrow[gi][k] : 0;
      const int n = L.myrec[gi][k].x >= 0 ? L.myrec[gi][k].x : 0;
      L.pos0[gi][k] = P.ipos[0][n];
      L.pos2[gi][k] = R.c2n ? n : P.ipos[2][n];  // (c2n: d M goes by lookup)
    }
#pragma unroll
  for (int gi = 0; gi < S::GPW; ++gi) {
    int nn[S::LPR], s0[S::LPR];
#pragma unroll
    for (int k = 0; k < S::LPR; ++k) { nn[k] = L.myrec[gi][k].x; s0[k] = L.myrec[gi][k].y; }
#pragma unroll
    for (int i = 0; i < S::K0T; ++i) {  // core-0 slices: element e of the quarter's LPR stacked slices
      const int e = 4 * (i16 + 16 * i);
      const int k = e / S::SL0, rem = e % S::SL0;
      const int n = pick2<S>(nn, k);
      const size_t sid0 = (size_t)pick2<S>(s0, k);
      if constexpr (!PAD && UNC) {
        // (round 6) unconditional: a missing lookup's record is (-1, 0, 0, 0) -- slice 0, a valid address.  Its rows of A meet
        // rows of d x_0 that ARE zero (its gradient row below is) and nothing of it is stored, so what they hold does not
        // matter; `if (n >= 0)` over a zero default made the allocator copy one component of a load just requested into the
        // default's register -- a wait for every load issued so far in the middle of the operand requests (cfg2: a fourth trip)
        (void)n;
        L.av[gi][i] = *(const float4*)(C.c[0] + sid0 * S::SL0 + rem);
      } else if constexpr (!PAD) {
        L.av[gi][i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (n >= 0) L.av[gi][i] = *(const float4*)(C.c[0] + sid0 * S::SL0 + rem);
      } else {
        L.av[gi][i] = make_float4(0.f, 0.f, 0.f, 0.f);
        const int a = rem / S::K0, kc = rem % S::K0;  // (row a of the slice, columns kc .. kc+3 of its r1)
        L.av[gi][i] = ld4_guard(C.c[0] + sid0 * R.sl0 + a * R.r1 + kc, (n >= 0 && a < R.q0) ? R.r1 - kc : 0, C.c[0], (R.v4 & 1) != 0);
      }
    }
    if constexpr (S::GPP) {
      constexpr int NF = S::BPP * S::Q2;
      const size_t row = (size_t)table * B + (size_t)bagrow[gi][0];
#pragma unroll
      for (int j = 0; j < S::NPL; ++j) {  // float4 number i16 + 16 j of the lookup's NF pass values
        const int f = i16 + 16 * j;
        const int a = f / (NF / 4), rr = f % (NF / 4), bl = rr / (S::Q2 / 4), x = 4 * (rr % (S::Q2 / 4));
        L.gp[gi][j] = nullptr;
        if (nn[0] >= 0 && f < NF && (!PAD || (a < R.q0 && x < R.q2)))
          L.gp[gi][j] = PAD ? d_output + row * R.D + (a * R.q1 + bl) * R.q2 + x : d_output + row * S::D + (a * S::Q1 + bl) * S::Q2 + x;
      }
      L.gsw[gi] = (PC.psw && nn[0] >= 0) ? PC.psw[nn[0]] : 1.f;
    }
#pragma unroll
    for (int i = 0; i < (S::GPP ? 0 : BwdLoads<S>::NG4); ++i) {  // bag gradients: element e of the quarter's LPR stacked rows
      const int e = 4 * (i16 + 16 * i);
      const int k = (e / S::D) % S::LPR, rem = e % S::D;
      const int n = pick2<S>(nn, k);
      L.gv4[gi][i] = make_float4(0.f, 0.f, 0.f, 0.f);
      L.gsw4[gi][i] = 1.f;
      if constexpr (PAD) {  // padded element (a, q1 block bq, columns x .. x+3 of q2) of the bag's gradient row; no branches
        const bool ok = n >= 0 && ((S::LPR * S::D / 4) % 16 == 0 || e < S::LPR * S::D);
        const long long row = ok ? (long long)pick2<S>(bagrow[gi], k) : 0;
        const int a = rem / (S::Q1 * S::Q2), bq = (rem / S::Q2) % S::Q1, x = rem % S::Q2;
        L.gv4[gi][i] = ld4_guard(d_output + ((size_t)table * B + row) * R.D + (a * R.q1 + bq) * R.q2 + x,
                                 (ok && a < R.q0 && bq < R.q1) ? R.q2 - x : 0, d_output, (R.v4 & 4) != 0);
        const float w1 = ld_guard(PC.psw + (ok ? n : 0), PC.psw != nullptr && ok, d_output);
        const float sw = (PC.psw != nullptr && ok) ? w1 : 1.f;
        L.gv4[gi][i].x *= sw; L.gv4[gi][i].y *= sw; L.gv4[gi][i].z *= sw; L.gv4[gi][i].w *= sw;
      } else if constexpr (UNC) {
        // (round 6) unconditional, as the core-0 slices above: a missing lookup reads bag row 0 (a valid address) and bwd_put
        // writes zeros in its place -- `if (n >= 0)` over a zero default cost a wait in front of the last-core rows' requests
        const long long row = (long long)pick2<S>(bagrow[gi], k);
        L.gv4[gi][i] = *(const float4*)(d_output + ((size_t)table * B + row) * S::D + rem);
        if (PC.psw) L.gsw4[gi][i] = PC.psw[n >= 0 ? n : 0];
      } else if (n >= 0 && ((S::LPR * S::D / 4) % 16 == 0 || e < S::LPR * S::D)) {
        const long long row = (long long)pick2<S>(bagrow[gi], k);
        L.gv4[gi][i] = *(const float4*)(d_output + ((size_t)table * B + row) * S::D + rem);
        if (PC.psw) {
          const float sw = PC.psw[n];
          L.gv4[gi][i].x *= sw; L.gv4[gi][i].y *= sw; L.gv4[gi][i].z *= sw; L.gv4[gi][i].w *= sw;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < S::LPR; ++k)
#pragma unroll
      for (int h = 0; h < S::HH; ++h) {
        const int kk = h * 16 + i16;
        const size_t sid2 = (size_t)(L.myrec[gi][k].x >= 0 ? L.myrec[gi][k].z : 0);
        const float* cg = PAD ? C.c[2] + sid2 * R.sl2 + kk * R.q2 : C.c[2] + sid2 * S::SL2 + kk * S::Q2;
#pragma unroll
        for (int x4 = 0; x4 < S::Q2 / 4; ++x4) {
          if constexpr (!PAD) {
            L.c2q[gi][k][h][x4] = *(const f32x4*)(cg + 4 * x4);
          } else {
            const float4 t = ld4_guard(cg + 4 * x4, kk < R.r2 ? R.q2 - 4 * x4 : 0, C.c[2], (R.v4 & 4) != 0);
            L.c2q[gi][k][h][x4] = (f32x4){t.x, t.y, t.z, t.w};
          }
        }
      }
  }
}
// registers -> LDS: the quarter's rows kq*4 .. kq*4+3 of the wave's A tile (Aw[16 x LDA]) and its lookups' gradient rows
template <class S, bool UNC = false>
__device__ __forceinline__ void bwd_put(const BwdLoads<S>& L, int gi, float* Aw, float* Gw) {
  const int lane = lane_id(), i16 = lane & 15, kq = lane >> 4;
#pragma unroll
  for (int i = 0; i < S::K0T; ++i) {
    const int e = 4 * (i16 + 16 * i);  // element of the quarter's 4 x K0 block (its LPR slices stacked = 4 rows of the tile)
    float2* dst = (float2*)(Aw + (kq * 4 + e / S::K0) * S::LDA + e % S::K0);
    dst[0] = make_float2(L.av[gi][i].x, L.av[gi][i].y);
    dst[1] = make_float2(L.av[gi][i].z, L.av[gi][i].w);
  }
#pragma unroll
  for (int i = 0; i < (S::GPP ? 0 : BwdLoads<S>::NG4); ++i) {
    const int e = 4 * (i16 + 16 * i);
    if ((S::LPR * S::D / 4) % 16 == 0 || e < S::LPR * S::D) {
      if constexpr (UNC) {
        const float sw = L.gsw4[gi][i];
        int nn[S::LPR];
#pragma unroll
        for (int k = 0; k < S::LPR; ++k) nn[k] = L.myrec[gi][k].x;
        const bool there = pick2<S>(nn, (e / S::D) % S::LPR) >= 0;  // (a missing lookup's gradient row is zeros)
        *(float4*)(Gw + (kq * S::LPR + e / S::D) * S::GD + e % S::D) =
            there ? make_float4(L.gv4[gi][i].x * sw, L.gv4[gi][i].y * sw, L.gv4[gi][i].z * sw, L.gv4[gi][i].w * sw)
                  : make_float4(0.f, 0.f, 0.f, 0.f);
      } else {
        *(float4*)(Gw + (kq * S::LPR + e / S::D) * S::GD + e % S::D) = L.gv4[gi][i];
      }
    }
  }
}
// Shape3::GPP: the values (a, q1 block pass*BPP + bl, x) of the quarter's lookup, float4 number i16 + 16 j per lane (j < NPL)
// (BwdLoads::gp; zeros for a missing lookup) -- fetched one pass ahead -- and their place in the lookup's G rows [a][bl][x]
template <class S>
struct GPass { float4 v[S::NPL]; };
template <class S, bool PAD>
__device__ __forceinline__ GPass<S> bwd_fetch_g(const BwdLoads<S>& L, int gi, int pass, const RealDims& R) {
  constexpr int NF = S::BPP * S::Q2;  // float4s of one lookup's pass values
  static_assert(NF <= 16 * S::NPL, "NPL float4s per lane of the quarter");
  const int i16 = lane_id() & 15;
  const float sw = L.gsw[gi];
  GPass<S> out;
#pragma unroll
  for (int j = 0; j < S::NPL; ++j) {
    const int f = i16 + 16 * j;
    const int rr = f % (NF / 4), bl = rr / (S::Q2 / 4), x = 4 * (rr % (S::Q2 / 4));
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
    if (L.gp[gi][j]) {
      if constexpr (!PAD) {
        g = *(const float4*)(L.gp[gi][j] + pass * S::BPP * S::Q2);
      } else {
        g = ld4_guard(L.gp[gi][j] + pass * S::BPP * R.q2, (pass * S::BPP + bl < R.q1) ? R.q2 - x : 0, L.gp[gi][j], (R.v4 & 4) != 0);
      }
      g.x *= sw; g.y *= sw; g.z *= sw; g.w *= sw;
    }
    out.v[j] = g;
  }
  return out;
}
template <class S>
__device__ __forceinline__ void bwd_put_g(const GPass<S>& g, float* Gw) {
  constexpr int NF = S::BPP * S::Q2;
  const int lane = lane_id(), i16 = lane & 15, kq = lane >> 4;
#pragma unroll
  for (int j = 0; j < S::NPL; ++j) {
    const int f = i16 + 16 * j;
    if (f >= NF) continue;
    const int a = f / (NF / 4), rr = f % (NF / 4), bl = rr / (S::Q2 / 4), x = 4 * (rr % (S::Q2 / 4));
    *(float4*)(Gw + kq * S::GD + (a * S::BPP + bl) * S::Q2 + x) = g.v[j];
  }
}

// element (row k0 of r1, padded column colp) of a pivot partial -> where the real slice has it, or nowhere
template <class S, bool PAD, bool NT>
__device__ __forceinline__ void st_pc1(float v, float* __restrict__ pc1, int k0, int colp, const RealDims& R) {
  if constexpr (!PAD) {
    spec_st<NT>(v, pc1 + k0 * S::N1 + colp);
  } else {
    const int bq = colp / S::R2, kk = colp % S::R2;
    if (k0 < R.r1 && bq < R.q1 && kk < R.r2) spec_st<NT>(v, pc1 + (size_t)k0 * R.n1 + bq * R.r2 + kk);
  }
}

template <class S, bool MULTI, bool PAD = false>  // MULTI: a chunk of the plan holds several sub-chunks of S::MC lookups
__global__ __launch_bounds__(kThreads, (PAD && S::GPP) ? 2 : S::WGS) void spec_bwd_kernel(TTX_KHEAD_PARAMS Plan P, CorePtrs C, int B, int p1,
                                                             const int64_t* __restrict__ rowidx,
                                                             const float* __restrict__ d_output,
                                                             Partials PC, int dbg, long long* stamps, RealDims R, PStore PS) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  TTX_KHEAD_ADOPT(P, C);
  // 16-byte partial stores: d core_0 and the cooperative d core_1 come out transposed.  Not in the sub-chunk walk: its launches hand
  // over more than the Infinity Cache holds, so they stay non-temporal, and the 16-byte layout alone measured 0.2 % slower there
  // (cfg5shard 0.5590 / 0.5597 against 0.5570 / 0.5584 ms per step, profiles/partial_stores.md)
  constexpr bool W16 = S::W16 && !PAD && !MULTI;
  const int chunk = blockIdx.x;
#define SSTAMP(i) do { if (stamps && threadIdx.x == 0) stamps[(size_t)chunk * 16 + (i)] = wall_clock64(); } while (0)
  // (the sub-chunk walk enters as it always did: its entry is paid once per several sub-chunks)
  constexpr bool EARLY = !MULTI;
  if constexpr (!EARLY) {
    zero_hot_counters(PC);
    SSTAMP(0);
  }
  // (round 6) the plan header's "bag rows valid" word travels WITH the chunk record: read behind the early exit below it was a
  // trip to memory of its own between the chunk record and the bag rows (the branch on it sits in front of their requests)
  const int4 cr = EARLY ? chunk_record(P.chunk_rec, (unsigned)chunk) : P.chunk_rec[chunk];
  const int hdr3 = P.hdr[3];
  if constexpr (EARLY) {
    // Single sub-chunk: the chunk record is requested by the wave's first instructions -- its address arrives with the wave --
    // and UNDER its trip every argument that does not, in one round of the scalar cache.  Left to the compiler each was
    // fetched in front of its first use and waited for there: the hot counters' and the stamps' pointers in front of the chunk
    // record's request, the debug mask and then B / p_1 between the chunk record and the lookup records' requests -- four
    // dependent trips to the argument segment in a chain that holds three trips to memory.  (Stamp 0 is taken behind that round.)
    asm volatile("" ::"s"(B), "s"(rowidx), "s"(d_output), "s"(dbg), "s"(stamps), "s"(P.ipos[0]), "s"(P.ipos[2]), "s"(PC.pc[0]),
                 "s"(PC.pc[1]), "s"(PC.pc[2]), "s"(PC.psw), "s"(PC.tableidx), "s"(PC.hot_cnt), "s"(PC.n_hot_cnt), "s"(R.c2n),
                 "s"(R.tmul), "s"(R.tsh), "s"(PS.flav), "s"(PS.b0), "s"(PS.b1), "s"(PS.b2));
    zero_hot_counters_n<kThreads>(PC);
    SSTAMP(0);
  }
  asm volatile("" ::"v"(cr.x), "v"(cr.y), "v"(cr.z), "v"(cr.w), "v"(hdr3));
  const int s = cr.x, start0 = cr.y, len0 = cr.z;
  if (len0 == 0) return;
  SSTAMP(1);
  if (dbg & 16) { if (threadIdx.x == 0 && len0 < 0) PC.pc[0][0] = 0.f; return; }
  const int tid = threadIdx.x, lane = lane_id(), w = tid / kWave;
  const int i16 = lane & 15, kq = lane >> 4;
  float* Bs = smem + S::oB;
  float* Aw0 = smem + S::oA + w * S::RG * S::szA;  // this wave's resident regions, one set per group if RG > 1
  float* Xw0 = smem + S::oX + w * S::RG * S::szX;
  float* Gw0 = smem + S::oG + w * S::RG * S::szGb;
  // (single sub-chunk: s / p1 as the host's magic pair -- a multiply-high and a shift, 0 with one table -- RealDims::tmul)
  const int table = PC.tableidx ? (int)PC.tableidx[P.lrec[start0].x] : (MULTI ? s / p1 : (int)table_quot((unsigned)s, R.tmul, R.tsh));
  const bool has_row = hdr3 != 0;
  const float* B1 = C.c[1] + (size_t)s * (PAD ? R.sl1 : S::SL1);
  float* pc1 = PC.pc[1] + (size_t)cr.w * (PAD ? R.sl1 : S::SL1);  // .w = the chunk's partial slot
  // (W16) the partial buffers as descriptors, for the write-through flavour
  const __amdgpu_buffer_rsrc_t rp0 = make_rsrc(PC.pc[0], PS.b0), rp1 = make_rsrc(pc1, PS.b1), rp2 = make_rsrc(PC.pc[2], PS.b2);
  // A chunk of the plan may hold several sub-chunks of S::MC lookups (large batches: one 16 KB pivot partial
  // per 128 instead of per 16 lookups -- the partials, not the arithmetic, bound the kernel there).  The
  // work-group walks them; the cooperative d core_1 accumulates across sub-chunks in acc2p and is stored once.
  f32x4 acc2p[MULTI ? S::NP : 1][S::K0T][S::TPW];
  if (MULTI) {
#pragma unroll
    for (int pp = 0; pp < S::NP; ++pp)
#pragma unroll
      for (int y = 0; y < S::K0T; ++y)
#pragma unroll
        for (int x = 0; x < S::TPW; ++x) acc2p[pp][y][x] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }

  const int nsub = MULTI ? (len0 + S::MC - 1) / S::MC : 1;
  BwdRecs<S> rq;         // records in flight (MULTI: of the sub-chunk after the next)
  BwdLoads<S> cur, nxt;  // operands of this sub-chunk / (MULTI) in flight for the next
  BBlock<S> bb;          // core_1 block in flight
  if constexpr (MULTI) {
    bwd_load_recs<S>(rq, P, start0, min(S::MC, len0), w, has_row, rowidx);
    bwd_load<S, PAD>(cur, rq, P, C, PC, has_row, table, B, rowidx, d_output, R);
    if (nsub > 1) bwd_load_recs<S>(rq, P, start0 + S::MC, min(S::MC, len0 - S::MC), w, has_row, rowidx);
    spec_fetch_b<S, PAD>(B1, 0, bb, R);
    if constexpr (S::B1ONCE) {  // the slice is staged here, once, outside the walk (its registers are free inside)
      spec_zero_pads<S, true>(Bs, Aw0);
      spec_put_b<S>(bb, Bs);
      __syncthreads();
    }
  }
  int sc = 0;
  do {  // (a plain do-while: with MULTI == false there is no loop at all for the compiler to reason about)
  const int start = MULTI ? start0 + sc * S::MC : start0, len = MULTI ? min(S::MC, len0 - sc * S::MC) : len0;
  const int ngroups = (len + S::LPG - 1) / S::LPG;
  if (MULTI && sc > 0) __syncthreads();  // the previous sub-chunk's A / d x_0 regions are free
  SSTAMP(10);
  if (MULTI && sc < 4) SSTAMP(11 + sc);

  // ---- every global load of this wave is issued here, before any compute.  With sub-chunks (MULTI) the chain
  // records -> operands runs AHEAD of the arithmetic: this sub-chunk's operands were requested one iteration ago (`cur`), the
  // next one's are requested now from records that were requested an iteration ago (`rq`), and the records after those go out --
  // a wave no longer parks on two dependent trips to memory at the top of every sub-chunk (round 4; 2.1 of a sub-chunk's
  // 10.5 us at 327k lookups, scripts/phase_times_large.py).  Affordable since the tail left the VALU: the kernel holds 132
  // registers without, three work-groups per CU have 168.  (Round 2 tried it at 154: one wave per SIMD fewer, 341 -> 384 us.) ----
  if constexpr (!MULTI) {
    bwd_load_recs<S>(rq, P, start, len, w, has_row, rowidx);
#ifndef TTX_B1_LATE
    spec_fetch_b<S, PAD>(B1, 0, bb, R);  // (behind the records' requests, in front of the wait for them: the slice travels under it)
    // ... which the instruction scheduler has to be TOLD: the block's address needs nothing but the chunk record, and left alone
    // it sank all four loads behind the wait for the records, into the operand round -- 8 KB per work-group on top of the
    // burst that round already is.  Nothing crosses this line, so the requests stand where they are written.
    __builtin_amdgcn_sched_barrier(0);
#endif
    bwd_load<S, PAD, !PAD>(cur, rq, P, C, PC, has_row, table, B, rowidx, d_output, R);
  } else {
    if (sc + 1 < nsub) {
      bwd_load<S, PAD>(nxt, rq, P, C, PC, has_row, table, B, rowidx, d_output, R);
      if (sc + 2 < nsub) bwd_load_recs<S>(rq, P, start0 + (sc + 2) * S::MC, min(S::MC, len0 - (sc + 2) * S::MC), w, has_row, rowidx);
    }
  }
  float4 (&av)[S::GPW][S::K0T] = cur.av;
  float4 (&gv4)[S::GPW][BwdLoads<S>::NG4] = cur.gv4;
#define c2(GI, K, H, X) cur.c2q[GI][K][H][(X) / 4][(X) % 4]
  int4 (&myrec)[S::GPW][S::LPR] = cur.myrec;
  SSTAMP(3);
  if (dbg & 32) { if (myrec[0][0].x == -7 && myrec[S::GPW - 1][S::LPR - 1].y == -9) PC.pc[0][0] = 1.f; return; }
#ifdef TTX_B1_LATE
  if (!MULTI) spec_fetch_b<S, PAD>(B1, 0, bb, R);  // (MULTI: pass 0's block is in flight since the last put of the previous sub-chunk)
#endif
  if (!MULTI || (sc == 0 && !S::B1ONCE)) spec_zero_pads<S, true>(Bs, Aw0);
  if (S::COOP) {  // a group without lookups still lends its (zero) rows to the others' d core_1
#pragma unroll
    for (int gi = 0; gi < S::GPW; ++gi)
      if (w + gi * kWaves >= ngroups)
        for (int e = lane; e < S::szX; e += kWave) Xw0[gi * S::szX + e] = 0.f;
  }
  if (dbg & 64) {  // keep every prefetched value alive, then leave
    float keep = bb.v[0].x;
#pragma unroll
    for (int gi = 0; gi < S::GPW; ++gi) {
      keep += av[gi][0].x + av[gi][S::K0T - 1].w + gv4[gi][0].y + c2(gi, 0, 0, 0) + c2(gi, S::LPR - 1, S::HH - 1, S::Q2 - 1);
    }
    if (keep == 12345.678f) PC.pc[0][0] = keep;
    return;
  }

  // d core_2 partial of this lane's (lookup, kk) items: [.. h][x / 4] holds x = 4*(x/4) .. +3 of row kk = h*16 + i16
  f32x4 pc2v[S::GPW][S::LPR][S::HH][S::Q2 / 4];
  f32x4 da[S::GPW][S::K0T];          // d core_0 rows of the wave's groups
  float* scratch = smem + S::oX;     // cross-wave reduction area (the X regions, dead by then)
  GPass<S> gpass[S::GPP ? S::GPW : 1];  // (Shape3::GPP) the next column pass's gradient values in flight

#pragma unroll
  for (int pass = 0; pass < S::NP; ++pass) {
    // (the previous pass's d x_0 tiles -- read by every wave's cooperative d core_1 -- its core_1 block and the reduction
    //  scratch are free)
    if (pass > 0) __syncthreads();
    if (pass == 1) SSTAMP(6);
    // the staged core_1: a block per column pass -- or (Shape3::B1ONCE) the whole slice once per chunk
    if (S::B1ONCE ? (pass == 0 && !MULTI) : true) {
      spec_put_b<S>(bb, Bs);
      if (!S::B1ONCE && !(TTX_LATEB && S::GPP)) {
        if (pass + 1 < S::NP) spec_fetch_b<S, PAD>(B1, pass + 1, bb, R);  // next block in flight
        else if (MULTI && sc + 1 < nsub) spec_fetch_b<S, PAD>(B1, 0, bb, R);  // ... the next sub-chunk's first
      }
      __syncthreads();
    }
    const float* Bp = Bs + (S::BFS ? pass * S::PW : 0);  // this pass's columns of the staged block
    if (pass == 0) SSTAMP(2);
    f32x4 acc2[S::K0T][S::TPW];  // d core_1 of this pass: this wave's rows x all tiles, or (COOP) all rows x its tiles
#pragma unroll
    for (int y = 0; y < S::K0T; ++y)
#pragma unroll
      for (int x = 0; x < S::TPW; ++x) acc2[y][x] = (f32x4){0.f, 0.f, 0.f, 0.f};

#pragma unroll
    for (int gi = 0; gi < S::GPW; ++gi) {
      const int g = w + gi * kWaves;
      if (g >= ngroups) continue;  // (no break: the loop must unroll so gi stays a constant)
      bool live[S::LPR];
#pragma unroll
      for (int k = 0; k < S::LPR; ++k) live[k] = myrec[gi][k].x >= 0;
      float* Aw = Aw0 + (S::RG > 1 ? gi : 0) * S::szA;
      float* Xw = Xw0 + (S::RG > 1 ? gi : 0) * S::szX;
      float* Gw = Gw0 + (S::RG > 1 ? gi : 0) * S::szGb;
      if (S::NP == 1 || pass == 0) {
        bwd_put<S, !MULTI && !PAD>(cur, gi, Aw, Gw);
#pragma unroll
        for (int k = 0; k < S::LPR; ++k)
#pragma unroll
          for (int h = 0; h < S::HH; ++h)
#pragma unroll
            for (int xb = 0; xb < S::Q2 / 4; ++xb) pc2v[gi][k][h][xb] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int y = 0; y < S::K0T; ++y) da[gi][y] = (f32x4){0.f, 0.f, 0.f, 0.f};
      }
      if constexpr (S::GPP) {  // (wave-private rows: the wave's own LDS order is all the synchronisation there is)
        if (pass == 0) gpass[gi] = bwd_fetch_g<S, PAD>(cur, gi, 0, R);
        bwd_put_g<S>(gpass[gi], Gw);
        if (pass + 1 < S::NP) gpass[gi] = bwd_fetch_g<S, PAD>(cur, gi, pass + 1, R);
      }
      if (gi == 0 && pass == 0) SSTAMP(4);
      if (dbg & 8) continue;
      // ---- recompute x_0 (this pass's columns) into registers, fused tail on the registers ----
      f32x4 acc[S::PNT];
      spec_gemm_x0<S>(Aw, Bp, acc);
      {
        if constexpr (S::MT) {
          // Tail on the matrix pipe (round 4), v_mfma_f32_4x4x1 = sixteen 4 x 4 outer products per instruction, a block = four
          // consecutive lanes: D[lane 4b+j][reg i] += A[lane 4b+i] * B[lane 4b+j] (scripts/probes/mfma4x4.hip).  Both tail
          // contractions fit the registers as they are:
          //   d core_2[kk][x] += x_0[(a,b)][kk] * g[a][b][x]:  B = the accumulator register acc[bl*HH+h][a] (lane <-> kk),
          //     A = g[lookup][a][b][4*xb + (lane & 3)] (one ds_read_b32) -> reg i <-> x, the layout pc2v is stored from;
          //   d x_0[(a,b)][kk] = sum_x g[a][b][x] * core_2[kk][x]:  A = g[lookup][a = lane & 3][b][x], B = this lane's core_2 row
          //     value c2[h][x] -> reg i <-> a: exactly the accumulator layout spec_store_x writes out.
          // 2 * BPP*HH*Q2 small MFMAs per pass (8 cycles each) for the 2 * 4*BPP*HH*Q2 v_fma (4 cycles each) of rounds 1-3.
          const int t4 = lane & 3;
          const float* gl = Gw + kq * S::GD;
#pragma unroll
          for (int bl = 0; bl < S::BPP; ++bl) {
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
              for (int xb = 0; xb < S::Q2 / 4; ++xb) {
                const float gB = gl[(S::GPP ? a * S::BPP + bl : a * S::Q1 + pass * S::BPP + bl) * S::Q2 + xb * 4 + t4];
#pragma unroll
                for (int h = 0; h < S::HH; ++h) pc2v[gi][0][h][xb] = mfma1(gB, acc[bl * S::HH + h][a], pc2v[gi][0][h][xb]);
              }
            float gA[S::Q2];
#pragma unroll
            for (int x4 = 0; x4 < S::Q2 / 4; ++x4) {
              const float4 t = *(const float4*)(gl + (S::GPP ? t4 * S::BPP + bl : t4 * S::Q1 + pass * S::BPP + bl) * S::Q2 + 4 * x4);
              gA[4 * x4] = t.x; gA[4 * x4 + 1] = t.y; gA[4 * x4 + 2] = t.z; gA[4 * x4 + 3] = t.w;
            }
#pragma unroll
            for (int h = 0; h < S::HH; ++h) {
              f32x4 dx = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
              for (int x = 0; x < S::Q2; ++x) dx = mfma1(gA[x], c2(gi, 0, h, x), dx);
              acc[bl * S::HH + h] = dx;
            }
          }
        } else {
#pragma unroll
        for (int a = 0; a < 4; ++a) {  // accumulator row a: core-0 row a % Q0 of the lane's lookup a / Q0
          const float* gl = Gw + (kq * S::LPR + a / S::Q0) * S::GD;
#pragma unroll
          for (int bl = 0; bl < S::BPP; ++bl) {
            float gv[S::Q2];
#pragma unroll
            for (int x = 0; x < S::Q2; ++x) gv[x] = gl[((a % S::Q0) * S::Q1 + pass * S::BPP + bl) * S::Q2 + x];
#pragma unroll
            for (int h = 0; h < S::HH; ++h) {
              const float xv = acc[bl * S::HH + h][a];
              float dx = 0.f;
#pragma unroll
              for (int x = 0; x < S::Q2; ++x) {
                pc2v[gi][a / S::Q0][h][x / 4][x % 4] = fmaf(xv, gv[x], pc2v[gi][a / S::Q0][h][x / 4][x % 4]);
                dx = fmaf(gv[x], c2(gi, a / S::Q0, h, x), dx);
              }
              acc[bl * S::HH + h][a] = dx;
            }
          }
        }
        }
        if constexpr (W16) {  // a lane's Q2 values of row kk are consecutive floats of the partial: whole float4s
          if (pass == S::NP - 1 && !(dbg & 1)) TTX_BY_FLAVOUR(PS.flav, (st_pc2_rows<S, FLAV>(pc2v[gi], live, cur.pos2[gi], PC.pc[2], rp2)));
        } else if (pass == S::NP - 1 && !(dbg & 1)) {
#pragma unroll
          for (int k = 0; k < S::LPR; ++k)
            if (live[k]) {
#pragma unroll
              for (int h = 0; h < S::HH; ++h) {
                const int kk = h * 16 + i16;
                float* o = PAD ? PC.pc[2] + (size_t)cur.pos2[gi][k] * R.sl2 + kk * R.q2
                               : PC.pc[2] + (size_t)cur.pos2[gi][k] * S::SL2 + kk * S::Q2;
                if constexpr (!PAD) {
#pragma unroll
                  for (int x = 0; x < S::Q2; ++x) spec_st<S::NT>(pc2v[gi][k][h][x / 4][x % 4], o + x);
                } else if (R.v4 & 4) {  // (kernel-uniform) whole float4s of the real row
#pragma unroll
                  for (int x4 = 0; x4 < S::Q2 / 4; ++x4)
                    if (kk < R.r2 && 4 * x4 < R.q2) spec_st4<S::NT>(pc2v[gi][k][h][x4], o + 4 * x4);
                } else {  // (plain stores: the L2 merges a lane's 4-byte pieces before they leave for memory)
#pragma unroll
                  for (int x = 0; x < S::Q2; ++x)
                    if (kk < R.r2 && x < R.q2) o[x] = pc2v[gi][k][h][x / 4][x % 4];
                }
              }
            }
        }
      }
      spec_store_x<S>(acc, Xw);  // d x_0 -> LDS for the two operand layouts below
      if (gi == 0 && pass == 0) SSTAMP(7);
      if (dbg & 2) continue;
      // ---- d core_1 += Aw^T * dX0 over the 16 rows: 4 k-steps, rows {t, t+8 | t+4, t+12} ----
      TTX_PRIO(1);
      if constexpr (!S::COOP) {
        const int rbase = 8 * (kq & 1) + 4 * (kq >> 1);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int row = rbase + t;
          float avv[S::K0T], bv[S::PNT];
#pragma unroll
          for (int y = 0; y < S::K0T; ++y) avv[y] = Aw[row * S::LDA + y * 16 + i16];
#pragma unroll
          for (int x = 0; x < S::PNT; ++x) bv[x] = Xw[row * S::LD + x * 16 + i16];
#pragma unroll
          for (int y = 0; y < S::K0T; ++y)
#pragma unroll
            for (int x = 0; x < S::PNT; ++x) acc2[y][x] = mfma4(avv[y], bv[x], acc2[y][x]);
        }
      }
      // ---- d core_0 rows += dX0 * Bs^T: k-step columns {c..c+3} ----
      if constexpr (W16) {
        // The transposed product below leaves tile row i16 in lane i16, but the record of that row's lookup sits with the lanes of
        // quarter (i16 / Q0) / LPR.  The row of its d core_0 partial (-1: no lookup) crosses through LDS: column K0P of the wave's A
        // tile, row = lookup of the group -- a padding column (LDA >= K0P + 2) nothing else reads or writes.
        if (pass == S::NP - 1 && i16 == 0) {
#pragma unroll
          for (int k = 0; k < S::LPR; ++k) Aw[(kq * S::LPR + k) * S::LDA + S::K0P] = __int_as_float(live[k] ? cur.pos0[gi][k] : -1);
        }
      }
      {
        const float* xr = Xw + i16 * S::LD + kq;
        const float* br = Bp + i16 * S::LDB + kq;
        float ac[4], bc[4][S::K0T];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          ac[u] = xr[u * 4];
#pragma unroll
          for (int y = 0; y < S::K0T; ++y) bc[u][y] = br[y * 16 * S::LDB + u * 4];
        }
#pragma unroll
        for (int c = 0; c < S::PW; c += 16) {
          const int cn = (c + 16 < S::PW) ? c + 16 : 0;
          float an[4], bn[4][S::K0T];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            an[u] = xr[cn + u * 4];
#pragma unroll
            for (int y = 0; y < S::K0T; ++y) bn[u][y] = br[y * 16 * S::LDB + cn + u * 4];
          }
#pragma unroll
          for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int y = 0; y < S::K0T; ++y) da[gi][y] = W16 ? mfma4(bc[u][y], ac[u], da[gi][y]) : mfma4(ac[u], bc[u][y], da[gi][y]);
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            ac[u] = an[u];
#pragma unroll
            for (int y = 0; y < S::K0T; ++y) bc[u][y] = bn[u][y];
          }
          __builtin_amdgcn_sched_group_barrier(0x100, 2 + 2 * S::K0T, 0);
          __builtin_amdgcn_sched_group_barrier(0x008, 4 * S::K0T, 0);
        }
        TTX_PRIO(0);
        if (gi == 0 && pass == 0) SSTAMP(5);
        if constexpr (W16) {
          // transposed: this lane holds tile row i16 = (lookup i16 / Q0, core-0 row i16 % Q0), columns y*16 + kq*4 .. +3
          if (pass == S::NP - 1 && !(dbg & 1)) {
            const int p0 = __float_as_int(Aw[(i16 / S::Q0) * S::LDA + S::K0P]);
            TTX_BY_FLAVOUR(PS.flav, (st_pc0_rows<S, FLAV>(da[gi], p0, PC.pc[0], rp0)));
          }
        } else
        // rows kq*4 + r = (lookup kq*LPR + r / Q0, core-0 row r % Q0); columns y*16 + i16
        if (pass == S::NP - 1 && !(dbg & 1)) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (live[r / S::Q0]) {
              if constexpr (!PAD) {
                float* o = PC.pc[0] + (size_t)cur.pos0[gi][r / S::Q0] * S::SL0 + i16;
#pragma unroll
                for (int y = 0; y < S::K0T; ++y) spec_st<S::NT>(da[gi][y][r], o + (r % S::Q0) * S::K0 + y * 16);
              } else if (r % S::Q0 < R.q0) {
                float* o = PC.pc[0] + (size_t)cur.pos0[gi][r / S::Q0] * R.sl0 + (r % S::Q0) * R.r1;
#pragma unroll
                for (int y = 0; y < S::K0T; ++y)
                  if (y * 16 + i16 < R.r1) spec_st<S::NT>(da[gi][y][r], o + y * 16 + i16);
              }
            }
        }
      }
    }

    // ---- d core_1 partial of the chunk, columns of this pass: sum the four waves' accumulators
    // through LDS, one r1 tile row (PNT tiles) per round; scratch = the X regions ----
    if (pass == S::NP - 1) SSTAMP(8);
    if constexpr (TTX_LATEB && S::GPP && !S::B1ONCE) {
      if (pass + 1 < S::NP) spec_fetch_b<S, PAD>(B1, pass + 1, bb, R);
    }
    if (dbg & 4) continue;
    if constexpr (S::COOP) {
      __syncthreads();  // every wave's d x_0 block (and A) is in LDS
      const int rbase = 8 * (kq & 1) + 4 * (kq >> 1);
#pragma unroll
      for (int ws = 0; ws < kWaves * S::RG; ++ws) {  // every (wave, group) tile of the sub-chunk
        const float* As = smem + S::oA + ws * S::szA;
        const float* Xs = smem + S::oX + ws * S::szX;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const int row = rbase + t;
          float avv[S::K0T], bv[S::TPW];
#pragma unroll
          for (int y = 0; y < S::K0T; ++y) avv[y] = As[row * S::LDA + y * 16 + i16];
#pragma unroll
          for (int x = 0; x < S::TPW; ++x) bv[x] = Xs[row * S::LD + (w * S::TPW + x) * 16 + i16];
#pragma unroll
          for (int y = 0; y < S::K0T; ++y)
#pragma unroll
            for (int x = 0; x < S::TPW; ++x) acc2[y][x] = W16 ? mfma4(bv[x], avv[y], acc2[y][x]) : mfma4(avv[y], bv[x], acc2[y][x]);
        }
      }
      // (W16: transposed -- row (= core_1 row k0) = y*16 + i16, columns tile*16 + kq*4 .. +3)
      if constexpr (MULTI) {  // carried across the sub-chunks, stored once at the end
#pragma unroll
        for (int y = 0; y < S::K0T; ++y)
#pragma unroll
          for (int x = 0; x < S::TPW; ++x) acc2p[pass][y][x] += acc2[y][x];
      } else if constexpr (W16) {
        if (!(dbg & 128)) TTX_BY_FLAVOUR(PS.flav, (st_pc1_tiles<S, FLAV>(acc2, pc1, rp1, pass, w)));
      } else if (!(dbg & 128)) {  // single sub-chunk: this pass's block is final
#pragma unroll
        for (int y = 0; y < S::K0T; ++y)
#pragma unroll
          for (int x = 0; x < S::TPW; ++x)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr)
              st_pc1<S, PAD, S::NT>(acc2[y][x][rr], pc1, y * 16 + kq * 4 + rr, pass * S::PW + (w * S::TPW + x) * 16 + i16, R);
      }
      continue;
    }
#pragma unroll
    for (int y = 0; y < S::K0T; ++y) {
      __syncthreads();
#pragma unroll
      for (int x = 0; x < S::PNT; ++x)
#pragma unroll
        for (int r = 0; r < 4; ++r) scratch[((w * S::PNT + x) * 4 + r) * 64 + lane] = acc2[y][x][r];
      __syncthreads();
      for (int e = tid; e < S::PNT * 256; e += kThreads) {
        float v = 0.f;
#pragma unroll
        for (int ww = 0; ww < kWaves; ++ww) v += scratch[ww * S::PNT * 256 + e];
        const int x = e / 256, r = (e / 64) % 4, ln = e % 64;
        st_pc1<S, PAD, S::NT>(v, pc1, y * 16 + (ln >> 4) * 4 + r, pass * S::PW + x * 16 + (ln & 15), R);
      }
    }
  }
  if constexpr (MULTI) cur = nxt;
#undef c2
  } while (MULTI && ++sc < nsub);  // sub-chunks
  if constexpr (S::COOP && MULTI) {
    if constexpr (W16) {
      if (!(dbg & 4)) {
#pragma unroll
        for (int pass = 0; pass < S::NP; ++pass) TTX_BY_FLAVOUR(PS.flav, (st_pc1_tiles<S, FLAV>(acc2p[pass], pc1, rp1, pass, w)));
      }
    } else
    // C/D layout: row (= core_1 row k0) = y*16 + kq*4 + r, column = tile*16 + i16
    if (!(dbg & 4)) {
#pragma unroll
      for (int pass = 0; pass < S::NP; ++pass)
#pragma unroll
        for (int y = 0; y < S::K0T; ++y)
#pragma unroll
          for (int x = 0; x < S::TPW; ++x)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr)
              st_pc1<S, PAD, S::NT>(acc2p[pass][y][x][rr], pc1, y * 16 + kq * 4 + rr, pass * S::PW + (w * S::TPW + x) * 16 + i16, R);
    }
  }
  SSTAMP(9);
#undef SSTAMP
}

// ---- dispatch ---------------------------------------------------------------------------------
enum SpecId { SPEC_NONE = 0, SPEC_32_4_32_4, SPEC_16_4_16_4, SPEC_32_4_32_8, SPEC_16_4_16_8, SPEC_64_4_64_8, SPEC_64_4_64_4,
              SPEC2_32_4_32_4, SPEC2_16_4_16_4, SPEC2_64_4_64_4,
              SPEC_32_8_32_8, SPEC_64_8_64_8,
              SPEC2_32_2_32_4, SPEC2_64_2_64_4, SPEC2_16_2_16_4, SPEC_16_8_16_8,
              SPEC_128_4_128_4, SPEC_128_4_128_8, SPEC_128_8_128_8,
              SPEC_16_8_16_16, SPEC_32_8_32_16, SPEC_64_8_64_16,
              SPEC_16_16_16_16, SPEC_32_16_32_16,
              SPEC_16_4_16_32, SPEC_32_4_32_32, SPEC_16_8_16_32, SPEC_32_8_32_32, SPEC_64_16_64_16,
              SPEC_16_16_16_32, SPEC_32_16_32_32 };  // q = [4,16,32]: q1 = 16 AND a prime last factor (q = [1 | 2, 16, 23 .. 31])  // q2 up to 32 (round 5): a prime last factor 17 .. 31 -- the default factorings of D = 272 / 304 / 544 / 608 / 736 / 816 / 912 -- padded onto them  // q = [4,16,16] (round 5): q1 = 9 / 10 / 12 / 16 -- the default factorings of D = 720 / 800 / 864 / 880 / 960 / 1008 -- padded onto it  // q = [4,8,16] (round 4): with q0 = 8 as part lookups, the reference's default factorings of D = 640 / 768 / 1024  // r = 128 (round 3): one work-group per CU, 137 KB of LDS  // q = [2,2,4]: D = 16  // q = [4,8,8]: the reference's default factoring of D = 256  // SPEC2_*: q0 = 2 (the reference's default factoring of D = 32: q = [2,4,4])

// template (Q0, Q1, Q2, R) that holds the geometry: the exact shape, or -- round 3 -- the smallest template with
// q0 <= Q0, q1 <= Q1, q2 <= Q2, max(r1, r2) <= R, run through the PAD variants of the kernels (`*pad`).  A geometry that would
// use less than an eighth of the template's multiply-adds stays with the generic kernels (kMaxPadWaste).
constexpr long long kMaxPadWaste = 8;
static TTX_KNOB(int, g_disable_pad, 0);  // (debug: exact shapes only, ttx_debug_skip bit 15)
static SpecId spec_match(const Dims& d, bool* pad = nullptr) {
  if (pad) *pad = false;
  if (g_disable_spec || d.T != 3) return SPEC_NONE;
  const int q0 = d.q[0], r1 = d.r[1], q1 = d.q[1], r2 = d.r[2], q2 = d.q[2];
  if (q0 > 4 || q1 > 16 || q2 > 32 || r1 > 128 || r2 > 128) return SPEC_NONE;
  const int rmax = r1 > r2 ? r1 : r2;
  const int R = rmax <= 16 ? 16 : (rmax <= 32 ? 32 : (rmax <= 64 ? 64 : 128));
  struct Cand { int Q0, Q1, Q2; SpecId id[4]; };  // ids for R = 16, 32, 64, 128
  static const Cand cands[] = {
      {2, 2, 4, {SPEC2_16_2_16_4, SPEC2_32_2_32_4, SPEC2_64_2_64_4, SPEC_NONE}},
      {2, 4, 4, {SPEC2_16_4_16_4, SPEC2_32_4_32_4, SPEC2_64_4_64_4, SPEC_NONE}},
      {4, 4, 4, {SPEC_16_4_16_4, SPEC_32_4_32_4, SPEC_64_4_64_4, SPEC_128_4_128_4}},
      {4, 4, 8, {SPEC_16_4_16_8, SPEC_32_4_32_8, SPEC_64_4_64_8, SPEC_128_4_128_8}},
      {4, 8, 8, {SPEC_16_8_16_8, SPEC_32_8_32_8, SPEC_64_8_64_8, SPEC_128_8_128_8}},
      {4, 8, 16, {SPEC_16_8_16_16, SPEC_32_8_32_16, SPEC_64_8_64_16, SPEC_NONE}},  // (ranks <= 64: beyond, the backward's registers)
      {4, 4, 32, {SPEC_16_4_16_32, SPEC_32_4_32_32, SPEC_NONE, SPEC_NONE}},
      {4, 16, 16, {SPEC_16_16_16_16, SPEC_32_16_32_16, SPEC_64_16_64_16, SPEC_NONE}},  // (r = 64: gradient rows per pass, two work-groups)
      {4, 8, 32, {SPEC_16_8_16_32, SPEC_32_8_32_32, SPEC_NONE, SPEC_NONE}},
      {4, 16, 32, {SPEC_16_16_16_32, SPEC_32_16_32_32, SPEC_NONE, SPEC_NONE}},
  };
  const int ri = R == 16 ? 0 : (R == 32 ? 1 : (R == 64 ? 2 : 3));
  for (const Cand& c : cands) {  // (ordered by size: the first that holds the geometry is the smallest)
    if (q0 > c.Q0 || q1 > c.Q1 || q2 > c.Q2 || c.id[ri] == SPEC_NONE) continue;
    const bool exact = q0 == c.Q0 && q1 == c.Q1 && q2 == c.Q2 && r1 == R && r2 == R;
    if (exact) return c.id[ri];
    if (g_disable_pad) return SPEC_NONE;
    const long long real = (long long)q0 * r1 * q1 * r2 + (long long)q0 * q1 * r2 * q2;
    const long long padded = (long long)c.Q0 * R * c.Q1 * R + (long long)c.Q0 * c.Q1 * R * c.Q2;
    if (real * kMaxPadWaste < padded) return SPEC_NONE;
    if (pad) *pad = true;
    return c.id[ri];
  }
  return SPEC_NONE;
}

static RealDims real_dims(const Dims& d) {
  RealDims R;
  R.q0 = d.q[0]; R.q1 = d.q[1]; R.q2 = d.q[2]; R.r1 = d.r[1]; R.r2 = d.r[2];
  R.sl0 = d.slice[0]; R.sl1 = d.slice[1]; R.sl2 = d.slice[2];
  R.n1 = d.q[1] * d.r[2];
  R.D = d.D;
  R.c2n = 0;
  R.v4 = ((d.r[1] & 3) == 0 ? 1 : 0) | ((d.r[2] & 3) == 0 ? 2 : 0) | ((d.q[2] & 3) == 0 ? 4 : 0);  // (the launchers clear it
                                                                                         // when an array is not 16-byte aligned)
  const TableDiv td = table_div((unsigned)d.p[1], (unsigned long long)d.num_tables * (unsigned long long)d.p[1]);
  R.tmul = td.mul; R.tsh = td.sh;
  return R;
}

template <class S, bool MULTI, bool FUSE = false, bool PAD = false>
static int spec_launch_fwd_v(const Plan& P, const CorePtrs& C, float* rows, float* zout, long long nzero,
                             const PoolFuse& F, const RealDims& R, hipStream_t st) {
  const size_t lds = S::lds_floats_fwd * sizeof(float);
  if (lds > 64 * 1024) {
    const int rc = allow_dynamic_lds((const void*)spec_fwd_kernel<S, MULTI, FUSE, PAD>, (int)lds);
    if (rc) return rc;
  }
  RealDims Rv = R;
  if ((((uintptr_t)C.c[0]) | ((uintptr_t)C.c[1]) | ((uintptr_t)C.c[2])) & 15) Rv.v4 = 0;
  // (the grid IS P.max_chunks: the single-sub-chunk kernel zeroes `zout` with that stride -- zero_output(zout, nzero, P.max_chunks) --
  //  so a launch with fewer work-groups would leave part of it unzeroed)
  hipLaunchKernelGGL((spec_fwd_kernel<S, MULTI, FUSE, PAD>), dim3(P.max_chunks), dim3(kThreads), lds, st, TTX_KHEAD_ARGS(P, C) P, C, rows, zout, nzero,
                     F, Rv);
  TTX_HIP(hipGetLastError());
  return TTX_OK;
}

// Flavour of a launch's 16-byte partial stores (Shape3::W16), by the upper bound of the bytes it hands to reduce_apply.
// Write-through keeps them in the 256 MiB Infinity Cache for the next launch; past kPartialWtBytes they go non-temporal as before.
// Measured (profiles/partial_stores.md; rocprofv3 averages in us, non-temporal -> write-through, q = [4,4,4], ranks 32):
//   partial bytes (bound)          backward            reduce_apply
//   cfg2        10k lookups   23 MiB    16.02 ->  15.95      9.63 ->  7.82   wins 1.9 us
//   cfg5shard1  82k lookups  163 MiB    88.97 ->  91.04     34.57 -> 27.62   wins 4.9 us
//   cfg5shard  328k lookups  414 MiB   316.36 -> 315.91     83.13 -> 87.04   loses 3.5 us: they no longer fit
// Nothing was measured between 163 and 414 MiB; the switch sits at three quarters of the cache, above the largest measured win.
constexpr long long kPartialWtBytes = 192ll << 20;
// (test library: g_partial_flavour = 1 + a flavour forced for every launch, g_old_stores = OldStores<S>; ttx_tt_common.h)
template <class S>
static PStore partial_store_flavour(const Plan& P, long long nnz) {
  const long long b0 = nnz * S::SL0 * 4, b1 = (long long)S::SL1 * 4, b2 = nnz * S::SL2 * 4;
  PStore ps;
  ps.flav = b0 + b2 + (long long)P.max_chunks * b1 <= kPartialWtBytes ? kStWt : kStNt;
  if (g_partial_flavour) ps.flav = g_partial_flavour - 1;
  // (the write-through stores address with 32-bit byte offsets into bounds-checked descriptors)
  if (b0 > 0xffffffffll || b2 > 0xffffffffll) ps.flav = kStNt;
  ps.b0 = (unsigned)(b0 > 0xffffffffll ? 0 : b0); ps.b1 = (unsigned)b1; ps.b2 = (unsigned)(b2 > 0xffffffffll ? 0 : b2);
  return ps;
}

template <class S, bool MULTI, bool PAD = false>
static int spec_launch_bwd_v(const Dims& d, const Plan& P, const CorePtrs& C, int B, const int64_t* rowidx,
                             const float* d_output, const Partials& PC, const RealDims& R, long long nnz, hipStream_t st) {
  size_t lds = S::lds_floats_bwd * sizeof(float);
  // (debug: TTX_DEBUG_BWD_LDS=<bytes> asks for more LDS than the kernel uses -- fewer work-groups per CU, to time a work-group's
  //  own critical path without its neighbours, scripts/phase_times_large.py)
  static const long pad_to = getenv("TTX_DEBUG_BWD_LDS") ? atol(getenv("TTX_DEBUG_BWD_LDS")) : 0;
  if (pad_to > (long)lds && pad_to <= 160 * 1024) lds = (size_t)pad_to;
  if (lds > 64 * 1024) {
    const int rc = allow_dynamic_lds((const void*)spec_bwd_kernel<S, MULTI, PAD>, (int)lds);
    if (rc) return rc;
  }
  RealDims Rv = R;
  if ((((uintptr_t)C.c[0]) | ((uintptr_t)C.c[1]) | ((uintptr_t)C.c[2]) | ((uintptr_t)d_output) | ((uintptr_t)PC.pc[2])) & 15) Rv.v4 = 0;
  hipLaunchKernelGGL((spec_bwd_kernel<S, MULTI, PAD>), dim3(P.max_chunks), dim3(kThreads), lds, st, TTX_KHEAD_ARGS(P, C) P, C, B, d.p[1], rowidx,
                     d_output, PC, g_debug_skip, g_stamps, Rv, partial_store_flavour<S>(P, nnz));
  TTX_HIP(hipGetLastError());
  return TTX_OK;
}
// exact shapes: the kernel with 16-byte partial stores, or (test library, g_old_stores) the one with the stores as they were
template <class S, bool MULTI>
static int spec_launch_bwd_x(const Dims& d, const Plan& P, const CorePtrs& C, int B, const int64_t* rowidx,
                             const float* d_output, const Partials& PC, const RealDims& R, long long nnz, hipStream_t st) {
#ifdef TTX_TEST_HOOKS
  if constexpr (S::W16 && !MULTI) {  // (the sub-chunk walk stores as before either way)
    if (g_old_stores) return spec_launch_bwd_v<OldStores<S>, MULTI>(d, P, C, B, rowidx, d_output, PC, R, nnz, st);
  }
#endif
  return spec_launch_bwd_v<S, MULTI>(d, P, C, B, rowidx, d_output, PC, R, nnz, st);
}

// P.MC > S::MC: the plan's chunks hold several sub-chunks (only shapes with S::SUB are ever planned that way)
// *fused: in -> the caller offers fused pooling (F.arrive != NULL); out -> this variant did it (no pooling launch needed)
// pad: the geometry is smaller than the template (RealDims R says by how much)
template <class S>
static int spec_launch_fwd(const Plan& P, const CorePtrs& C, float* rows, float* zout, long long nzero,
                           const PoolFuse& F, bool* fused, bool pad, const RealDims& R, hipStream_t st) {
  const bool want = *fused;
  *fused = false;
  if constexpr (S::SUB) {
    static_assert(S::COOP, "sub-chunks need the cooperative d core_1");
    if (P.MC > S::MC)
      return pad ? spec_launch_fwd_v<S, true, false, true>(P, C, rows, zout, nzero, F, R, st)
                 : spec_launch_fwd_v<S, true>(P, C, rows, zout, nzero, F, R, st);
  }
  if (pad) return spec_launch_fwd_v<S, false, false, true>(P, C, rows, zout, nzero, F, R, st);
  if constexpr (S::D % 4 == 0) {
    if (want) {
      *fused = true;
      return spec_launch_fwd_v<S, false, true>(P, C, rows, zout, nzero, F, R, st);
    }
  }
  return spec_launch_fwd_v<S, false>(P, C, rows, zout, nzero, F, R, st);
}

template <class S>
static int spec_launch_bwd(const Dims& d, const Plan& P, const CorePtrs& C, int B, const int64_t* rowidx,
                           const float* d_output, const Partials& PC, bool pad, const RealDims& R, long long nnz, hipStream_t st) {
  if constexpr (S::SUB) {
    if (P.MC > S::MC)
      return pad ? spec_launch_bwd_v<S, true, true>(d, P, C, B, rowidx, d_output, PC, R, nnz, st)
                 : spec_launch_bwd_x<S, true>(d, P, C, B, rowidx, d_output, PC, R, nnz, st);
  }
  return pad ? spec_launch_bwd_v<S, false, true>(d, P, C, B, rowidx, d_output, PC, R, nnz, st)
             : spec_launch_bwd_x<S, false>(d, P, C, B, rowidx, d_output, PC, R, nnz, st);
}

// the benchmark shape: two column passes, 16 lookups per chunk (one M-tile per wave).  Measured against
// one pass x 32 lookups and two passes x 32 lookups at 10k and 327k lookups: fastest at both (the 16 KB pivot
// partial per 16 instead of 32 lookups costs reduce_apply +34 us at 327k lookups, the backward kernel gains 58).
#ifndef TTX_NP32
#define TTX_NP32 2
#endif
#ifndef TTX_MC32
#define TTX_MC32 16
#endif
using S_32_4_32_4 = Shape3<32, 4, 32, 4, TTX_NP32, TTX_MC32>;
using S_16_4_16_4 = Shape3<16, 4, 16, 4>;
using S_32_4_32_8 = Shape3<32, 4, 32, 8, 2, 16>;  // two column passes: measured 9 % faster than one (0.0805 -> 0.0735 ms/step)
using S_16_4_16_8 = Shape3<16, 4, 16, 8>;
using S_64_4_64_8 = Shape3<64, 4, 64, 8, 4, 16>;  // r = 64: four column passes, 16 lookups per chunk
using S_64_4_64_4 = Shape3<64, 4, 64, 4, 4, 16>;
// q0 = 2: a 16-row M tile is EIGHT lookups of two rows, a wave's group 8 lookups, a chunk 32
using S2_32_4_32_4 = Shape3<32, 4, 32, 4, 2, 32, 2>;
using S2_16_4_16_4 = Shape3<16, 4, 16, 4, 1, 32, 2>;
using S2_64_4_64_4 = Shape3<64, 4, 64, 4, 4, 32, 2>;
// D = 256 = [4,8,8]: x_0 has 8 column blocks; r = 32: four passes of two blocks, r = 64: eight of one
using S_32_8_32_8 = Shape3<32, 8, 32, 8, 4, 16>;
using S2_32_2_32_4 = Shape3<32, 2, 32, 4, 1, 32, 2>;  // D = 16 = [2,2,4]: one pass over the 64 columns of x_0
using S2_64_2_64_4 = Shape3<64, 2, 64, 4, 2, 32, 2>;
// r = 16 with 32-column passes: two column tiles per pass (the per-wave d core_1 with its cross-wave reduction; no sub-chunks)
using S2_16_2_16_4 = Shape3<16, 2, 16, 4, 1, 32, 2>;
using S_16_8_16_8 = Shape3<16, 8, 16, 8, 4, 16>;
using S_64_8_64_8 = Shape3<64, 8, 64, 8, 8, 16>;
// q2 = 16 (D = 512 per part lookup): r = 32 four passes of two q1 blocks, r = 16 four passes of 32 columns
using S_32_8_32_16 = Shape3<32, 8, 32, 16, 4, 16>;
using S_16_8_16_16 = Shape3<16, 8, 16, 16, 4, 16>;
using S_64_8_64_16 = Shape3<64, 8, 64, 16, 8, 16>;
// q1 = 16 (D = 1024 per part lookup): eight passes of two q1 blocks; gradient rows per pass, two float4 per lane (Shape3::GPP, NPL)
using S_32_16_32_16 = Shape3<32, 16, 32, 16, 8, 16>;
using S_16_16_16_16 = Shape3<16, 16, 16, 16, 8, 16>;
using S_64_16_64_16 = Shape3<64, 16, 64, 16, 16, 16>;  // (sixteen passes of one q1 block; gradient rows per pass, Shape3::GPP)
// q2 = 32: the last core's rows and the d core_2 partials are 2 x 64 registers of the backward at r = 32 -- 249 VGPRs, nothing in scratch
using S_32_4_32_32 = Shape3<32, 4, 32, 32, 2, 16>;
using S_16_4_16_32 = Shape3<16, 4, 16, 32, 1, 16>;
using S_32_8_32_32 = Shape3<32, 8, 32, 32, 4, 16>;
using S_16_8_16_32 = Shape3<16, 8, 16, 32, 4, 16>;
using S_32_16_32_32 = Shape3<32, 16, 32, 32, 8, 16>;  // (gradient rows per pass, four float4 per lane)
using S_16_16_16_32 = Shape3<16, 16, 16, 32, 8, 16>;
// r = 128: one q1 block (128 columns, 65 KB of core_1) per pass, 16 d core_1 accumulator tiles per wave; 137 KB of LDS and the
// register file of a SIMD per wave (Shape3::WGS = 1) -- instantiated to take ranks 65..128 off the generic block walk
using S_128_4_128_4 = Shape3<128, 4, 128, 4, 4, 16>;
using S_128_4_128_8 = Shape3<128, 4, 128, 8, 4, 16>;
using S_128_8_128_8 = Shape3<128, 8, 128, 8, 8, 16>;  // D = 256: eight passes, 150 KB of LDS

// ---- rank families: one translation unit each (ttx_tt_spec16.hip, ...32, ...64, ...128a/b/c define TTX_SPEC_GROUP and get the
// family's kernels instantiated; ttx_tt.hip includes this file for the host logic only and calls the entry points below) ----
#define TTX_SPEC_CASES_16(CALL)                      \
    case SPEC_16_4_16_4: return CALL(S_16_4_16_4);   \
    case SPEC_16_4_16_8: return CALL(S_16_4_16_8);   \
    case SPEC2_16_4_16_4: return CALL(S2_16_4_16_4); \
    case SPEC2_16_2_16_4: return CALL(S2_16_2_16_4); \
    case SPEC_16_8_16_8: return CALL(S_16_8_16_8);   \
    case SPEC_16_8_16_16: return CALL(S_16_8_16_16); \
    case SPEC_16_16_16_16: return CALL(S_16_16_16_16); \
    case SPEC_16_4_16_32: return CALL(S_16_4_16_32);   \
    case SPEC_16_8_16_32: return CALL(S_16_8_16_32);   \
    case SPEC_16_16_16_32: return CALL(S_16_16_16_32);
#define TTX_SPEC_CASES_32(CALL)                      \
    case SPEC_32_4_32_4: return CALL(S_32_4_32_4);   \
    case SPEC_32_4_32_8: return CALL(S_32_4_32_8);   \
    case SPEC2_32_4_32_4: return CALL(S2_32_4_32_4); \
    case SPEC_32_8_32_8: return CALL(S_32_8_32_8);   \
    case SPEC2_32_2_32_4: return CALL(S2_32_2_32_4); \
    case SPEC_32_8_32_16: return CALL(S_32_8_32_16);   \
    case SPEC_32_16_32_16: return CALL(S_32_16_32_16); \
    case SPEC_32_4_32_32: return CALL(S_32_4_32_32);   \
    case SPEC_32_8_32_32: return CALL(S_32_8_32_32);   \
    case SPEC_32_16_32_32: return CALL(S_32_16_32_32);
#define TTX_SPEC_CASES_64(CALL)                      \
    case SPEC_64_4_64_8: return CALL(S_64_4_64_8);   \
    case SPEC_64_4_64_4: return CALL(S_64_4_64_4);   \
    case SPEC2_64_4_64_4: return CALL(S2_64_4_64_4); \
    case SPEC_64_8_64_8: return CALL(S_64_8_64_8);   \
    case SPEC2_64_2_64_4: return CALL(S2_64_2_64_4); \
    case SPEC_64_8_64_16: return CALL(S_64_8_64_16); \
    case SPEC_64_16_64_16: return CALL(S_64_16_64_16);
// (r = 128: the kernels are thousands of unrolled instructions on 350+ registers and take minutes to compile -- a unit per shape)
#define TTX_SPEC_CASES_128a(CALL) case SPEC_128_4_128_4: return CALL(S_128_4_128_4);
#define TTX_SPEC_CASES_128b(CALL) case SPEC_128_4_128_8: return CALL(S_128_4_128_8);
#define TTX_SPEC_CASES_128c(CALL) case SPEC_128_8_128_8: return CALL(S_128_8_128_8);

constexpr int kSpecNotMine = -0x5bec;  // the id belongs to another family's translation unit
#define TTX_SPEC_FWD_ARGS                                                                                            \
  SpecId id, const Plan &P, const CorePtrs &C, float *rows, float *zout, long long nzero, const PoolFuse &F, bool *fused, \
      bool pad, const RealDims &R, hipStream_t st
#define TTX_SPEC_BWD_ARGS                                                                                             \
  SpecId id, const Dims &d, const Plan &P, const CorePtrs &C, int B, const int64_t *rowidx, const float *d_output,        \
      const Partials &PC, bool pad, const RealDims &R, long long nnz, hipStream_t st
#define TTX_SPEC_DECLARE(G)         \
  int spec_fwd_##G(TTX_SPEC_FWD_ARGS); \
  int spec_bwd_##G(TTX_SPEC_BWD_ARGS);
TTX_SPEC_DECLARE(16)
TTX_SPEC_DECLARE(32)
TTX_SPEC_DECLARE(64)
TTX_SPEC_DECLARE(128a)
TTX_SPEC_DECLARE(128b)
TTX_SPEC_DECLARE(128c)
#define TTX_SPEC_CALLF(S) spec_launch_fwd<S>(P, C, rows, zout, nzero, F, fused, pad, R, st)
#define TTX_SPEC_CALLB(S) spec_launch_bwd<S>(d, P, C, B, rowidx, d_output, PC, pad, R, nnz, st)
#define TTX_SPEC_DEFINE(G)                                                                 \
  int spec_fwd_##G(TTX_SPEC_FWD_ARGS) {                                                    \
    switch (id) { TTX_SPEC_CASES_##G(TTX_SPEC_CALLF) default: break; }                     \
    return kSpecNotMine;                                                                   \
  }                                                                                        \
  int spec_bwd_##G(TTX_SPEC_BWD_ARGS) {                                                    \
    switch (id) { TTX_SPEC_CASES_##G(TTX_SPEC_CALLB) default: break; }                     \
    return kSpecNotMine;                                                                   \
  }
#if defined(TTX_SPEC_GROUP)
#if TTX_SPEC_GROUP == 16
TTX_SPEC_DEFINE(16)
#elif TTX_SPEC_GROUP == 32
TTX_SPEC_DEFINE(32)
#elif TTX_SPEC_GROUP == 64
TTX_SPEC_DEFINE(64)
#elif TTX_SPEC_GROUP == 1281
TTX_SPEC_DEFINE(128a)
#elif TTX_SPEC_GROUP == 1282
TTX_SPEC_DEFINE(128b)
#elif TTX_SPEC_GROUP == 1283
TTX_SPEC_DEFINE(128c)
#endif
#endif

// ttx_magic.h -- table of a pivot slice, s / p_1, without a division in the kernel.  Plain C++ (no HIP, no other header of the
// library): the host computes the pair once per launch, the contraction kernels evaluate it, and tests/test_entry_chain_cpu.py
// compiles a stand-alone program from this file that checks it against s / p_1 over whole ranges.
//
// A pivot slice is s = table * p_1 + i_1 with 0 <= s < N = num_tables * p_1 < 2^31.  The quotient is
//   mul == 0:  s >> sh                        (p_1 a power of two; ONE table: sh = 31, the quotient is 0 whatever s)
//   mul != 0:  (s * mul) >> (32 + sh)         (one 32 x 32 -> high-32 multiply and a shift)
// For the second form, with k = 32 + sh and mul = floor(2^k / d) + 1, write e = mul * d - 2^k (0 < e <= d).  For n = q d + r:
//   n * mul / 2^k = q + r / d + e n / (d 2^k),   and   r / d + e n / (d 2^k) < 1   whenever   e n < 2^k   (r <= d - 1),
// so the pair is exact for every n < N as soon as e (N - 1) < 2^k.  The host takes the smallest sh for which that holds; the
// largest candidate, 2^sh < d < 2^(sh+1), always does: mul < 2^32 there and 2^k > 2^31 d >= e (N - 1).
#pragma once

#if defined(__HIPCC__)
#define TTX_MAGIC_HD __host__ __device__
#else
#define TTX_MAGIC_HD
#endif

namespace ttx {

struct TableDiv {
  unsigned mul;
  int sh;
};

// the pair for n / d, exact for every 0 <= n < N  (1 <= d, N <= 2^31)
inline TableDiv table_div(unsigned d, unsigned long long N) {
  TableDiv t;
  t.mul = 0;
  t.sh = 31;
  if (d == 0 || N <= d) return t;  // one table (or none): every n is below d
  if ((d & (d - 1)) == 0) {
    t.sh = 0;
    while ((1u << t.sh) < d) ++t.sh;
    return t;
  }
  for (int l = 0; l < 32 && (1ull << l) < d; ++l) {
    const unsigned long long k2 = 1ull << (32 + l);
    const unsigned long long m = k2 / d + 1;  // (< 2^32: 2^l < d)
    const unsigned long long e = m * d - k2;  // 0 < e <= d
    if (e * (N - 1) < k2) {                   // (e (N - 1) < 2^32 2^31: no overflow)
      t.mul = (unsigned)m;
      t.sh = l;
      return t;
    }
  }
  return t;  // (not reached: the last candidate holds, above)
}

TTX_MAGIC_HD inline unsigned table_quot(unsigned n, unsigned mul, int sh) {
  return mul ? (unsigned)(((unsigned long long)n * mul) >> 32) >> sh : n >> sh;
}

}  // namespace ttx

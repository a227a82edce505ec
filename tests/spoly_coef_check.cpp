// Stand-alone host program (tests/test_spoly_coef_cpu.py builds it with -fsanitize=address,undefined, together with
// bbx_ideals.cpp): the fast class's working form of a basis element's info word (bbx_ginfo_hot / bbx_ginfo_record,
// bbx_common.h: the statements the kernel uses) against the formulas the step used to evaluate for the two members of every
// selected pair,
//   a.c = tc ? tc / lc mod p : 0          b.c = tc ? -(tc / lc) mod p : 0
// with the products taken by the % operator here.  Every lead coefficient 1 .. p - 1 with 1/lc from the host's inverse
// (bbx::coef_inv, what the device table is filled from), tail coefficients 0, 1, 2, p - 2, p - 1 and 59 seeded values.
// Prints one line per property, `<name> cases <n> bad <n>`, and `bad <count>` (0 = all hold).
#include <stdio.h>

#include <vector>

#include "bbx_common.h"
#include "bbx_ideals.h"

int main() {
  const uint32_t P = BBX_P;
  std::vector<uint32_t> tcs = {0u, 1u, 2u, P - 2u, P - 1u};
  uint64_t z = 0x9E3779B97F4A7C15ull;
  while (tcs.size() < 64) { z ^= z << 13; z ^= z >> 7; z ^= z << 17; tcs.push_back((uint32_t)(z % P)); }
  std::vector<uint32_t> inv(P, 0u);
  long bad_inv = 0;
  for (uint32_t lc = 1; lc < P; lc++) {
    inv[lc] = (uint32_t)bbx::coef_inv((int)lc);
    bad_inv += !(inv[lc] >= 1u && inv[lc] < P && (uint64_t)inv[lc] * lc % P == 1u);
  }
  long cases = 0, bad_halves = 0, bad_range = 0, zero_cases = 0, bad_zero = 0, bad_round = 0, bad_mul = 0;
  for (uint32_t lc = 1; lc < P; lc++) {
    for (uint32_t tc : tcs) {
      const uint32_t rec_x = lc | (tc << 16);                        // the record's word
      const uint32_t hot = bbx_ginfo_hot(rec_x, inv[lc]);
      const uint32_t mt = hot & 0xffffu, nmt = hot >> 16;
      const uint32_t want_a = tc ? (uint32_t)((uint64_t)tc * inv[lc] % P) : 0u;
      const uint32_t want_b = tc ? (P - want_a) % P : 0u;
      cases++;
      bad_halves += !(mt == want_a && nmt == want_b);
      bad_range += !(mt < P && nmt < P);
      if (tc == 0) { zero_cases++; bad_zero += hot != 0u; }
      else bad_zero += (mt == 0u || nmt == 0u);                      // mt == 0 <=> tc == 0
      bad_round += bbx_ginfo_record(hot, rec_x) != rec_x;            // record word -> hot word + kept word -> record word
      bad_mul += bbx_coef_mulmod(tc, lc) != (uint32_t)((uint64_t)tc * lc % P);
    }
  }
  printf("inverse cases %u bad %ld\n", P - 1u, bad_inv);
  printf("halves cases %ld bad %ld\n", cases, bad_halves);
  printf("range cases %ld bad %ld\n", cases, bad_range);
  printf("zero cases %ld bad %ld\n", zero_cases, bad_zero);
  printf("roundtrip cases %ld bad %ld\n", cases, bad_round);
  printf("mulmod cases %ld bad %ld\n", cases, bad_mul);
  const long bad = bad_inv + bad_halves + bad_range + bad_zero + bad_round + bad_mul;
  printf("bad %ld\n", bad);
  return bad != 0;
}

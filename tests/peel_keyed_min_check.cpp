// Stand-alone host program (tests/test_peel_keyed_min_cpu.py builds it with -fsanitize=address,undefined): the fast class's
// Gebauer-Moeller peel by ONE wave minimum per bucket (add_poly, bbx_fast.h) — the keys are formed and taken apart by the
// statements the kernel uses (bbx_peel_key*, bbx_common.h) — against a direct statement of the rule for the new pairs (i, g):
//   L_i = lcm(LM G_i, LM f) is kept iff no L_j divides it properly; of every bucket of equal kept lcms the smallest index
//   is emitted, and nothing of the bucket if one of its members has LM G_i coprime to LM f.
// Cases: every multiset of 1..5 monomials with exponents 0..2 in 3 variables, in ascending and in descending arrangement,
// against every f of that box; seeded bases of 1..255 elements (every bank count) in four exponent regimes, the last with
// lcm degrees up to 65535 (the largest a key holds).
// Prints one line per property, `<name> cases <n> bad <n>`, and `bad <count>` (0 = all hold).
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "bbx_common.h"

struct Mon { uint32_t e[3]; };
static Mon lcm(const Mon& a, const Mon& b) { return Mon{{std::max(a.e[0], b.e[0]), std::max(a.e[1], b.e[1]), std::max(a.e[2], b.e[2])}}; }
static uint32_t deg(const Mon& a) { return a.e[0] + a.e[1] + a.e[2]; }
static bool divides(const Mon& a, const Mon& b) { return a.e[0] <= b.e[0] && a.e[1] <= b.e[1] && a.e[2] <= b.e[2]; }
static bool equal(const Mon& a, const Mon& b) { return a.e[0] == b.e[0] && a.e[1] == b.e[1] && a.e[2] == b.e[2]; }
static bool coprime(const Mon& a, const Mon& b) { return std::min(a.e[0], b.e[0]) + std::min(a.e[1], b.e[1]) + std::min(a.e[2], b.e[2]) == 0; }

static long g_bad_key = 0, g_iters = 0, g_max_buckets = 0, g_max_deg = 0, g_banks_seen[4] = {0, 0, 0, 0};

struct Set {                                                   // basis indices 0..255 (the kernel's emit masks, one word per bank)
  uint64_t w[4] = {0, 0, 0, 0};
  void add(int i) { w[i >> 6] |= 1ull << (i & 63); }
  bool operator!=(const Set& o) const { return w[0] != o.w[0] || w[1] != o.w[1] || w[2] != o.w[2] || w[3] != o.w[3]; }
};

// the kernel's loop: lane l of bank b holds basis element 64 b + l
static Set keyed_peel(const Mon* G, int n, const Mon& f) {
  Mon L[256]; uint32_t key[256]; bool cand[256], cp[256];
  for (int i = 0; i < n; i++) {
    L[i] = lcm(G[i], f); cp[i] = coprime(G[i], f); cand[i] = true;
    key[i] = bbx_peel_key(deg(L[i]), (uint32_t)i);
    g_bad_key += !(key[i] < BBX_PEEL_NO_KEY && bbx_peel_key_deg(key[i]) == deg(L[i]) && 64 * bbx_peel_key_bank(key[i]) + bbx_peel_key_lane(key[i]) == i);
    g_max_deg = std::max(g_max_deg, (long)deg(L[i]));
  }
  Set emit;
  long buckets = 0;
  for (;;) {
    uint32_t kmin = BBX_PEEL_NO_KEY;
    for (int i = 0; i < n; i++) if (cand[i]) kmin = std::min(kmin, key[i]);
    if (kmin == BBX_PEEL_NO_KEY) break;
    const int s = 64 * bbx_peel_key_bank(kmin) + bbx_peel_key_lane(kmin);
    g_banks_seen[bbx_peel_key_bank(kmin)]++;
    if (s >= n || !cand[s]) { g_bad_key++; break; }           // (the minimum names a candidate, or the loop would not end)
    bool bad = false;
    for (int i = 0; i < n; i++) {
      if (equal(L[i], L[s]) && cp[i]) bad = true;
      if (divides(L[s], L[i])) cand[i] = false;
    }
    if (!bad) emit.add(s);                                     // (a set: the pairs go out in ascending index whatever the order here)
    buckets++; g_iters++;
  }
  g_max_buckets = std::max(g_max_buckets, buckets);
  return emit;
}

static Set by_the_rule(const Mon* G, int n, const Mon& f) {
  Mon L[256];
  for (int i = 0; i < n; i++) L[i] = lcm(G[i], f);
  Set emit;
  for (int i = 0; i < n; i++) {
    bool keep = true;
    for (int j = 0; j < n && keep; j++) {
      if (divides(L[j], L[i]) && !equal(L[j], L[i])) keep = false;          // not minimal
      if (equal(L[j], L[i]) && (j < i || coprime(G[j], f))) keep = false;   // not its bucket's smallest index / a coprime member
    }
    if (keep) emit.add(i);
  }
  return emit;
}

int main() {
  long box_cases = 0, box_bad = 0, seeded_cases = 0, seeded_bad = 0;
  // every multiset of 1..5 monomials of the box {0,1,2}^3, both arrangements, every f of the box
  std::vector<Mon> box;
  for (uint32_t a = 0; a < 3; a++) for (uint32_t b = 0; b < 3; b++) for (uint32_t c = 0; c < 3; c++) box.push_back(Mon{{a, b, c}});
  for (int n = 1; n <= 5; n++) {
    int ix[5] = {0, 0, 0, 0, 0};
    for (;;) {
      Mon up[5], down[5];
      for (int i = 0; i < n; i++) { up[i] = box[ix[i]]; down[n - 1 - i] = box[ix[i]]; }
      for (const Mon& f : box) {
        box_cases += 2;
        box_bad += keyed_peel(up, n, f) != by_the_rule(up, n, f);
        box_bad += keyed_peel(down, n, f) != by_the_rule(down, n, f);
      }
      int k = n - 1;                                             // next non-decreasing index tuple
      while (k >= 0 && ix[k] == 26) k--;
      if (k < 0) break;
      ix[k]++;
      for (int j = k + 1; j < n; j++) ix[j] = ix[k];
    }
  }
  // seeded bases of 1..255 elements: exponents below 3 (many equal lcms), below 6, below 20, and up to 21845 with a tenth of
  // the elements at the corner (21845, 21845, 21845): lcm degree 65535
  uint64_t z = 0x9E3779B97F4A7C15ull;
  auto rnd = [&](uint32_t m) { z ^= z << 13; z ^= z >> 7; z ^= z << 17; return (uint32_t)((z >> 11) % m); };
  const uint32_t lim[4] = {3u, 6u, 20u, 21846u};
  for (int n = 1; n <= 255; n++) {
    for (int regime = 0; regime < 4; regime++) {
      for (int rep = 0; rep < 3; rep++) {
        std::vector<Mon> G(n);
        for (Mon& m : G) {
          m = Mon{{rnd(lim[regime]), rnd(lim[regime]), rnd(lim[regime])}};
          if (regime == 3 && rnd(10) == 0) m = Mon{{21845u, 21845u, 21845u}};
          if (regime == 3 && rnd(4) == 0) m.e[rnd(3)] = rnd(3);   // (small exponents among large ones: coprime members, divisors)
        }
        Mon f = Mon{{rnd(lim[regime]), rnd(lim[regime]), rnd(lim[regime])}};
        if (rnd(3) == 0) f.e[rnd(3)] = 0;
        seeded_cases++;
        seeded_bad += keyed_peel(G.data(), n, f) != by_the_rule(G.data(), n, f);
      }
    }
  }
  printf("box cases %ld bad %ld\n", box_cases, box_bad);
  printf("seeded cases %ld bad %ld\n", seeded_cases, seeded_bad);
  printf("keys cases %ld bad %ld\n", g_iters, g_bad_key);
  printf("reach: max_buckets %ld max_degree %ld bank0 %ld bank1 %ld bank2 %ld bank3 %ld\n", g_max_buckets, g_max_deg, g_banks_seen[0],
         g_banks_seen[1], g_banks_seen[2], g_banks_seen[3]);
  const long bad = box_bad + seeded_bad + g_bad_key;
  printf("bad %ld\n", bad);
  return bad != 0;
}

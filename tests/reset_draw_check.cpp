// Stand-alone host program (tests/test_reset_draw_cpu.py builds it with -fsanitize=address,undefined, together with
// bbx_ideals.cpp): the lane-parallel draw of a reset's ideal, as the fast class does it, against the sequential generator.
// The raws come from the table's jump-ahead multipliers, generator f is decoded by bbx_gen_decode (bbx_common.h: the
// statement the kernel uses) from the raws [f S, f S + S), and a deviation anywhere drops the batch for the sequential
// draw.  The reference is BinomialGen (bbx_ideals.cpp) seeded with the same engine state.  Prints, per distribution, how
// many ideals took the batch and how many fell back, the constructed rejection states, and `bad <count>` (0 = all equal).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>

#include <string>
#include <vector>

#include "bbx_common.h"
#include "bbx_ideals.h"

static const uint32_t M = 2147483647u;

struct HostAcc {
  const uint32_t* raws; const uint32_t* g;
  uint32_t raw(int i) const { return raws[i]; }
  double cp(int i) const { double v; memcpy(&v, g + BBX_GEN_CP + 2 * i, 8); return v; }
  BbxGenRow row(int d) const { const uint32_t* r = g + BBX_GEN_DEG + 8 * d; return BbxGenRow{r[0], r[2], r[3], r[4]}; }
  void mono(uint32_t j, uint32_t w[2]) const { w[0] = g[BBX_GEN_MONO + 2 * (size_t)j]; w[1] = g[BBX_GEN_MONO + 2 * (size_t)j + 1]; }
};

struct Drawn { std::vector<BbxGenDraw> gens; uint32_t x_after = 0; int first_deviation = -1; };

// what gen_ideal_lanes does, lane by lane; false: some generator deviated (x is then unchanged)
static bool draw_batch(const std::vector<uint32_t>& table, uint32_t x, Drawn* out) {
  const uint32_t* g = table.data();
  const uint32_t flags = g[3];
  const int npoly = (int)g[2], ncp = (int)g[4], S = bbx_gen_stride(flags, ncp);
  std::vector<uint32_t> raws(BBX_GEN_BATCH);
  for (int k = 0; k < BBX_GEN_BATCH; k++) raws[k] = bbx_gen_mulmod(g[BBX_GEN_JUMP + k], x);
  out->gens.clear(); out->first_deviation = -1;
  for (int f = 0; f < npoly; f++) {
    // (exactly the S raws of the window: a read beyond it is a heap overflow for the sanitizer)
    const std::vector<uint32_t> window(raws.begin() + f * S, raws.begin() + f * S + S);
    const HostAcc acc = {window.data(), g};
    out->gens.push_back(bbx_gen_decode(acc, flags, ncp));
    if (out->gens.back().deviated && out->first_deviation < 0) out->first_deviation = f;
  }
  out->x_after = raws[npoly * S - 1];
  return out->first_deviation < 0;
}

static void pack(const bbx::HTerm& t, uint32_t w[2]) {
  w[0] = (uint32_t)t.e[0] | ((uint32_t)t.e[1] << 16);
  w[1] = (uint32_t)t.e[2] | ((uint32_t)t.deg << 16);
}
static bool same(const std::vector<BbxGenDraw>& a, const bbx::HIdeal& F) {
  if (a.size() != F.size()) return false;
  for (size_t f = 0; f < a.size(); f++) {
    if (F[f].t.size() != 2 || F[f].t[0].c != 1 || (uint32_t)F[f].t[1].c != a[f].c) return false;
    uint32_t l[2], t[2];
    pack(F[f].t[0], l); pack(F[f].t[1], t);
    if (l[0] != a[f].lead[0] || l[1] != a[f].lead[1] || t[0] != a[f].tail[0] || t[1] != a[f].tail[1]) return false;
  }
  return true;
}

static uint32_t powmod(uint32_t a, uint32_t e) {
  uint32_t r = 1;
  for (; e; e >>= 1) { if (e & 1) r = bbx_gen_mulmod(r, a); a = bbx_gen_mulmod(a, a); }
  return r;
}

// Two ideals in a row from engine state x: the first by the batch (or, deviating, by the sequential generator), the second
// the same way from the state the first left — so a wrong state after the batch shows as a wrong second ideal.
// Returns 0 on equality; *path: 1 = the first ideal took the batch, 0 = it fell back.
static int check_state(const bbx::IdealGen& proto, const std::vector<uint32_t>& table, uint32_t x, int* path, int* first_deviation) {
  std::unique_ptr<bbx::IdealGen> ref = proto.clone();
  ref->seed((long long)x);
  bbx::HIdeal F1, F2;
  std::string err;
  // (a generator that fails — 1000 trials of two equal monomials, degree 0 twice under -consts — must deviate in the batch)
  const bool ok1 = ref->next(F1, &err), ok2 = ok1 && ref->next(F2, &err);
  Drawn d1;
  *path = draw_batch(table, x, &d1) ? 1 : 0;
  if (first_deviation) *first_deviation = d1.first_deviation;
  if (!*path) return 0;                                  // the fallback IS the sequential generator from x: nothing to compare
  if (!ok1 || !same(d1.gens, F1)) return 1;
  Drawn d2;
  if (draw_batch(table, d1.x_after, &d2)) return ok2 && same(d2.gens, F2) ? 0 : 1;
  if (!ok2) return 0;
  std::unique_ptr<bbx::IdealGen> again = proto.clone();  // the second ideal falls back: sequentially from the batch's state
  again->seed((long long)d1.x_after);
  bbx::HIdeal G;
  if (!again->next(G, &err)) return 1;
  Drawn want;                                            // compare G with F2 through the packed form
  for (auto& f : F2) { BbxGenDraw w; pack(f.t[0], w.lead); pack(f.t[1], w.tail); w.c = (uint32_t)f.t[1].c; w.deviated = false; want.gens.push_back(w); }
  return same(want.gens, G) ? 0 : 1;
}

int main(int argc, char** argv) {
  const int count = argc > 1 ? atoi(argv[1]) : 20000;
  int bad = 0;

  // the jump: A_k x_0 mod m is k engine steps
  {
    std::string err;
    std::vector<uint32_t> table;
    if (!bbx::parse_ideal_dist("3-20-10-weighted", &err)->device_table(2, &table)) { printf("no table\n"); return 2; }
    std::vector<uint32_t> starts = {1u, 2u, M - 1u};
    uint64_t z = 88172645463325252ull;
    for (int i = 0; i < 200; i++) { z ^= z << 13; z ^= z >> 7; z ^= z << 17; starts.push_back(1u + (uint32_t)(z % (M - 1u))); }
    int jump_bad = 0;
    for (uint32_t x0 : starts) {
      bbx::MinStd0 e; e.seed((long long)x0);
      for (int k = 1; k <= BBX_GEN_BATCH; k++) jump_bad += bbx_gen_mulmod(table[BBX_GEN_JUMP + k - 1], x0) != (uint32_t)e.next();
    }
    printf("jump starts %zu bad %d\n", starts.size(), jump_bad);
    bad += jump_bad;
  }

  const char* dists[] = {"3-20-10-weighted", "3-20-10-weighted-homog", "3-20-10-weighted-pure", "3-20-10-weighted-consts", "3-20-11-weighted",
                         "3-20-10-maximum", "3-2-10-uniform", "2-5-4-uniform"};
  for (const char* dist : dists) {
    std::string err;
    std::unique_ptr<bbx::IdealGen> proto = bbx::parse_ideal_dist(dist, &err);
    std::vector<uint32_t> table;
    if (!proto || !proto->device_table(2, &table)) { printf("no table for %s\n", dist); return 2; }
    const uint32_t flags = table[3];
    const int npoly = (int)table[2], ncp = (int)table[4], S = bbx_gen_stride(flags, ncp);
    int batch = 0, fallback = 0, mism = 0;
    uint64_t z = 0x9E3779B97F4A7C15ull ^ (uint64_t)strlen(dist);
    for (int i = 0; i < count; i++) {
      z ^= z << 13; z ^= z >> 7; z ^= z << 17;
      const uint32_t x = i < 64 ? (uint32_t)(i + 1) : 1u + (uint32_t)(z % (M - 1u));   // small seeds as the tests use them, then any state
      int path = 0;
      mism += check_state(*proto, table, x, &path, nullptr);
      if (path) batch++; else fallback++;
    }
    printf("dist %s stride %d batch %d fallback %d mismatches %d\n", dist, S, batch, fallback, mism);
    bad += mism;

    // constructed rejections: x_0 = t / A_k puts raw t at draw k (1-based).  t = m - 1 is past every distribution's `past`
    // (ret = 2^31 - 3 = the engine's range); for the coefficient draw also the two sides of its bound 2147462208.
    struct Case { const char* what; int k; uint32_t t; bool deviates; int gen; };
    std::vector<Case> cases;
    if (!(flags & 2u)) {
      cases.push_back({"coefficient", 2 * S + 1, M - 1u, true, 2});
      cases.push_back({"coefficient-at-past", 1, 2147462208u + 1u, true, 0});
      cases.push_back({"coefficient-below-past", 1, 2147462208u, false, -1});
    }
    cases.push_back({"choice", 3 * S + (S - 1), M - 1u, true, 3});
    cases.push_back({"last-draw", npoly * S, M - 1u, true, npoly - 1});
    for (const Case& c : cases) {
      const uint32_t inv = powmod(table[BBX_GEN_JUMP + c.k - 1], M - 2u);
      const uint32_t x = bbx_gen_mulmod(c.t, inv);
      int path = 0, dev = -1;
      const int m = check_state(*proto, table, x, &path, &dev);
      // the constructed draw should be the first to deviate; where an earlier generator deviates by chance (two equal monomials
      // are common in the small distributions) the case says nothing and is reported as such
      const bool placed = bbx_gen_mulmod(table[BBX_GEN_JUMP + c.k - 1], x) == c.t;
      const bool chance = c.deviates && dev >= 0 && dev < c.gen;
      const bool ok = m == 0 && placed && (c.deviates ? (path == 0 && dev == c.gen) : dev != 0);
      const bool fine = ok || (m == 0 && placed && chance);
      printf("reject %s %s state %u path %d generator %d %s\n", dist, c.what, x, path, dev, ok ? "ok" : fine ? "chance" : "BAD");
      bad += !fine;
    }
  }
  printf("bad %d\n", bad);
  return bad != 0;
}

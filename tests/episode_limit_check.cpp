// Host check of the episode step limit's rule (bbx_common.h: bbx_episode_end, bbx_episode_counted, bbx_episode_tlim), built by
// tests/test_episode_limit_cpu.py with -fsanitize=address,undefined and run on its own.
//   end      bbx_episode_end / bbx_episode_counted against a plain restatement, over nP x episode_steps x limit x auto_reset
//   walk     a counted walk (episode_steps counted step by step, as the general / binomial / wide classes do) against the fast
//            class's bookkeeping (t_ep0, t_lim, the test t_agent == t_lim, episode_steps = t_agent - t_ep0): every entry count
//            — below, at and past the limit —, every limit, with and without auto-reset, with resets behind ends, and split into
//            launches that re-enter from the stored count: same ends, same counters, same stored count at every step
//   off      with the limit off t_lim is never met and nothing is ever cut
// Prints "<name> cases N failures M" per section; exit status 1 on any failure.
#include <cstdio>
#include <cstdint>

#include "bbx_common.h"

static long cases, failures;
static void expect(bool ok, const char* what, long a, long b, long c, long d) {
  cases++;
  if (!ok) { if (failures++ < 20) printf("FAIL %s %ld %ld %ld %ld\n", what, a, b, c, d); }
}
static int section(const char* name) {
  printf("%s cases %ld failures %ld\n", name, cases, failures);
  const int bad = failures != 0;
  cases = failures = 0;
  return bad;
}

// the rule as the issue states it
static int plain_end(int nP, int steps, int limit) {
  if (nP == 0) return 1;
  if (limit > 0 && steps >= limit) return 2;
  return 0;
}
static bool plain_counted(int end, int steps, int limit, int auto_reset) {
  if (end == 0) return false;
  if (end == 1) return true;
  return auto_reset != 0 || steps == limit;
}

// a deterministic pair-set size behind step t of a walk: empty now and then (an ordinary end), every period-th step
static int pairs_after(int t, int period) { return (period > 0 && t % period == period - 1) ? 0 : 3; }

int main() {
  int bad = 0;
  for (int nP = 0; nP <= 3; nP++)
    for (int steps = 0; steps <= 12; steps++)
      for (int limit = 0; limit <= 12; limit++) {
        const int e = bbx_episode_end(nP, steps, limit);
        expect(e == plain_end(nP, steps, limit), "end", nP, steps, limit, e);
        for (int ar = 0; ar <= 1; ar++)
          for (int end = 0; end <= 2; end++)
            expect(bbx_episode_counted(end, steps, limit, ar) == plain_counted(end, steps, limit, ar), "counted", end, steps, limit, ar);
      }
  bad |= section("end");

  // t0: the agent step count at entry (also near the 32-bit wrap of the hash agent's counter)
  const int t0s[] = {0, 1, 63, 64, 1000, 0x7ffffff0};
  for (int t0 : t0s)
    for (int limit = 0; limit <= 9; limit++)
      for (int entry = 0; entry <= 12; entry++)              // episode_steps at entry: below, at and past the limit
        for (int ar = 0; ar <= 1; ar++)
          for (int period = 0; period <= 11; period++)        // 0: the pair set never empties
            for (int launch = 1; launch <= 7; launch += 3) {   // steps per launch: the fast class re-enters from the stored count
              // counted walk
              int c_steps = entry, c_ep = 0, c_tr = 0;
              // fast class
              uint32_t t_agent = (uint32_t)t0;
              int stored = entry, f_ep = 0, f_tr = 0;
              int t_ep0 = 0, t_lim = 0;
              bool alive = true;
              for (int i = 0; i < 40 && alive; i++) {
                if (i % launch == 0) {                        // kernel entry
                  t_ep0 = (int)(t_agent - (uint32_t)stored);
                  t_lim = bbx_episode_tlim(t_ep0, (int)t_agent, limit);
                }
                const int nP = pairs_after(i, period);
                // the step, counted
                c_steps++;
                const int c_end = bbx_episode_end(nP, c_steps, limit);
                if (bbx_episode_counted(c_end, c_steps, limit, ar)) { c_ep++; c_tr += c_end == 2; }
                // the step, fast class: one compare
                t_agent++;
                const bool f_done = (nP == 0) | ((int)t_agent == t_lim);
                expect(f_done == (c_end != 0), "walk done", limit, entry, i, period);
                const int f_steps = (int)(t_agent - (uint32_t)t_ep0);
                expect(f_steps == c_steps, "walk steps", limit, entry, i, f_steps);
                if (f_done) {
                  const int f_end = bbx_episode_end(nP, f_steps, limit);
                  expect(f_end == c_end, "walk end", limit, entry, i, f_end);
                  if (bbx_episode_counted(f_end, f_steps, limit, ar)) { f_ep++; f_tr += f_end == 2; }
                  if (!ar) t_lim = bbx_episode_tlim(t_ep0, (int)t_agent, limit);
                }
                stored = (int)(t_agent - (uint32_t)t_ep0);    // what a write-back here would store
                expect(stored == c_steps, "walk stored", limit, entry, i, stored);
                if (c_end != 0) {
                  if (ar) {                                   // the reset behind the end: a new episode, 0 steps
                    c_steps = 0;
                    t_ep0 = (int)t_agent; t_lim = bbx_episode_tlim(t_ep0, (int)t_agent, limit);
                    stored = 0;
                  } else if (nP == 0) alive = false;          // finished and left as it is: no further step
                }
                expect(f_ep == c_ep && f_tr == c_tr, "walk counters", limit, entry, i, f_ep * 1000 + f_tr);
              }
              if (!ar && limit > 0 && period == 0) expect(c_tr == (entry < limit ? 1 : 0), "walk counts once", limit, entry, c_tr, 0);
            }
  bad |= section("walk");

  for (int t0 : t0s) {
    uint32_t t_agent = (uint32_t)t0;
    const int t_lim = bbx_episode_tlim((int)t_agent - 5, (int)t_agent, 0);
    for (int i = 0; i < 100000; i++) { t_agent++; expect((int)t_agent != t_lim, "off", t0, i, 0, 0); }
    expect(bbx_episode_end(3, 1 << 30, 0) == 0, "off end", t0, 0, 0, 0);
  }
  bad |= section("off");
  return bad;
}

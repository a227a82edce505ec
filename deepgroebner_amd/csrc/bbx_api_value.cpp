// libbbx.so — LeadMonomialsEnv::value (buchberger.cpp:332-351): discounted returns of full Buchberger rollouts from clones of
// the current states (bbx_value, bbx_values, bbx_values_seeded of include/bbx.h), their asynchronous form (bbx_values_device)
// and the same rollouts behind every pair of every environment (bbx_action_values).
// All three run one pipeline — value_clone, value_resort, value_launch_rollouts, a collect that folds "did not finish" into a
// word pair — and read that word with one rule (classify).  They differ in three things.  Streams: the synchronous calls and
// bbx_action_values stay on the NULL stream, bbx_values_device clones on the caller's stream and runs the rest on the library's.
// The forced step: bbx_action_values steps every clone once with its own action between clone and re-sort.  After growth: both
// NULL-stream forms restart from fresh clones of the enlarged records (retry_growing), bbx_values_device carries its clones
// over to them and resumes (value_carry_over).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "bbx_batch.h"

using namespace bbx_host;

namespace {

int agent_of_strategy(const char* s) {   // unknown keys select First: std::map::operator[] default (buchberger.cpp:342-349)
  if (!strcmp(s, "degree")) return BBX_AGENT_DEGREE;
  if (!strcmp(s, "normal")) return BBX_AGENT_NORMAL;
  if (!strcmp(s, "sugar")) return BBX_AGENT_SUGAR;
  if (!strcmp(s, "random")) return BBX_AGENT_STDRANDOM;   // choice(P, rng) of a seeded std::default_random_engine (buchberger.cpp:200-203, 244)
  return BBX_AGENT_FIRST;
}

// std::default_random_engine::seed(s) (linear_congruential_engine<uint_fast32_t, 16807, 0, 2^31-1>, libstdc++ bits/random.tcc):
// the int seed converts to the unsigned result type first; x = s mod m, and 0 becomes 1
uint32_t minstd_state_of_seed(long long seed) {
  const uint32_t x = (uint32_t)((uint64_t)seed % 2147483647ull);
  return x ? x : 1u;
}

void free_dev(std::initializer_list<void*> dev) { for (void* q : dev) if (q) (void)hipFree(q); }
int launched(int lrc, const char* what) {   // what a bbx_launch_* returned -> the return code of the call
  return lrc ? fail(BBX_E_DEVICE, "%s launch failed: %s", what, hipGetErrorString((hipError_t)lrc)) : BBX_OK;
}

// the clone arrays of the synchronous calls and bbx_action_values: room for n clones in the batch's current layout (kept
// between calls; grow_records frees them, so a call after the records were enlarged makes them again)
int value_scratch_ensure(bbx_batch* b, int n) {
  if (n <= b->vcap) return BBX_OK;
  value_scratch_free(b);
  HIPCHK(hipMalloc((void**)&b->d_vrecs, (size_t)n * b->L.rec_bytes));
  HIPCHK(hipMalloc((void**)&b->d_vflags, (size_t)n));
  HIPCHK(hipMalloc((void**)&b->d_vsrc, (size_t)n * sizeof(int32_t)));
  HIPCHK(hipMalloc((void**)&b->d_vseeds, (size_t)n * sizeof(uint32_t)));
  HIPCHK(hipMalloc((void**)&b->d_vvals, ((size_t)n + 1) * sizeof(double)));   // the word pair, then a value per clone
  HIPCHK(hipMemsetAsync(b->d_vvals, 0, sizeof(double), 0));                   // (the word is clear whenever no attempt is under way)
  b->vcap = n;
  return BBX_OK;
}

// ---- the pipeline: n clones and the flags the clone kernel leaves for the re-sort (the scratch above, or a ring slot; flags
// may be null for clones that are only rolled out: value_clone writes them, value_resort reads them, nothing else) -----------
struct ValueClones { char* recs; uint8_t* flags; int n; };

// clones[k] <- environment d_src[k]; d_seeds != null: the engine states of the clones' seeded Random selection
int value_clone(bbx_batch* b, const ValueClones& c, const int32_t* d_src, const uint32_t* d_seeds, hipStream_t stream) {
  const int ngen = b->sort_reducers ? b->gens[0]->npolys() : 0;
  return launched(bbx_launch_clone(b->d_recs, c.recs, &b->L, d_src, nullptr, c.n, d_seeds, 0, 1, ngen, c.flags, stream), "clone");
}

// clones whose generator lead monomials tie get the reducer order buchberger()'s std::sort would give them (value() re-sorts
// the state it is called on; the flags are the clone's — a step in between leaves the generators alone)
int value_resort(bbx_batch* b, const ValueClones& c, hipStream_t stream) {
  return launched(bbx_launch_value_resort(c.recs, &b->L, c.n, c.flags, stream), "resort");
}

// what every launch on clones has in common: they are not the batch's environments (no status block, trace or accounting)
BbxParams clone_params(bbx_batch* b, const ValueClones& c, int nsteps, int agent) {
  BbxParams p; fill_params(b, &p);
  p.recs = c.recs; p.B = c.n; p.nsteps = nsteps; p.set_budget = 1; p.agent = agent; p.auto_reset = 0;
  p.trace = nullptr; p.accounting = 0; p.lite = nullptr;
  p.episode_limit = 0;                 // the value of a state is the return of the whole computation (bbx_episode_limit)
  return p;
}

// the kernels plan_launch gives a rollout of the class — the first kernel and those that take over what it hands on —, each
// with a budget of `budget` steps (0: p's own)
int launch_on_clones(bbx_batch* b, const BbxParams& p, bool resume, int budget, hipStream_t stream) {
  LaunchPlan pl = plan_launch(b, p, resume, true);
  int lrc = 0;
  for (int i = 0; i < pl.n && !lrc; i++) {
    if (budget) pl.pass[i].nsteps = budget;
    lrc = bbx_launch_step(&pl.pass[i], pl.kind[i], pl.waves[i], stream);
  }
  return launched(lrc, "kernel");
}

// The rollouts to completion (resume: clones carried over to enlarged records continue where they stopped).  3-variable binomial
// batches run on the register/LDS-resident class (bbx_fast_value_kernel: every selection strategy, f_select_ordered), clones that
// outgrow it and every other batch on the HBM-resident class of the batch, long-polynomial environments one workgroup per clone.
int value_launch_rollouts(bbx_batch* b, const ValueClones& c, int agent, double gamma, bool resume, hipStream_t stream) {
  BbxParams p = clone_params(b, c, 1 << 30, agent);
  p.value_mode = 1; p.gamma = gamma; p.values = nullptr;
  return launch_on_clones(b, p, resume, 0, stream);
}

// ---- a clone that did not finish -------------------------------------------------------------------------------------------
// The word pair a collect folds (bbx_unfinished_fold, bbx_aux.hip) on the host: bits = 1 << status of every clone that waits
// for room, bit 31 for anything else; env = the largest index reported (a collect that reports clones: mapped by the caller)
struct UnfinishedWord { unsigned bits; int env; };
UnfinishedWord word_of(const void* pair) { uint32_t w[2]; memcpy(w, pair, sizeof w); return {w[0], (int)w[1] - 1}; }
constexpr unsigned kCapacityBits = BBX_ST_CAPACITY_BITS;   // the statuses a larger record cures
constexpr int kGrowAttempts = 40;        // enlargements one call goes through before it gives up

// What a word means: nothing unfinished; clones wait for room and the records may grow; or the call fails with BBX_E_CAPACITY
// (recorded here) — pairs left, an error state, or capacities that are hard limits.  `what` names the call.
enum class Unfinished { none, grow, fail };
Unfinished classify(const bbx_batch* b, const UnfinishedWord& w, const char* what) {
  if (!w.bits) return Unfinished::none;
  if (!(w.bits & ~kCapacityBits) && !b->no_growth) return Unfinished::grow;
  fail(BBX_E_CAPACITY, "%s of environment %d did not finish: %s", what, w.env,
       (w.bits & kCapacityBits) ? status_name(__builtin_ctz(w.bits & kCapacityBits)) : "pairs left or a clone in an error state");
  return Unfinished::fail;
}
int kept_outgrowing(const char* what) { return fail(BBX_E_CAPACITY, "%ss kept outgrowing the records", what); }

// The restart policy: attempt(&w) runs the pipeline from fresh clones, reports its word and delivers its results when the word
// is clear; clones that wait for room enlarge the records of the whole batch (grow_records frees the clone scratch) and the
// attempt runs again — the results are those of a handle created with room to spare
template <class Attempt> int retry_growing(bbx_batch* b, const char* what, Attempt attempt) {
  for (int i = 0; i < kGrowAttempts; i++) {
    UnfinishedWord w{0, -1};
    if (int rc = attempt(&w)) return rc;
    const Unfinished u = classify(b, w, what);
    if (u != Unfinished::grow) return u == Unfinished::none ? BBX_OK : BBX_E_CAPACITY;
    if (int rc = grow_records(b, w.bits & kCapacityBits, w.env, 0)) return rc;
  }
  return kept_outgrowing(what);
}

// ---- bbx_value, bbx_values, bbx_values_seeded ------------------------------------------------------------------------------
// One rollout to completion per entry of src (indices into b), from clones of the current states; seeds != null: the engine
// states of the clones' seeded Random selection.  Everything runs on the default stream without a copy in between and with
// one wait: the word pair and the values behind it come back in one transfer at the end.  The word starts out clear and a call
// that finds it set clears it for the next (a clear per call costs: profiles/r24_value_calls_ab.txt); it sits in FRONT of the
// values so that its place does not move with n.
int value_rollouts(bbx_batch* b, const std::vector<int32_t>& src, int agent, const std::vector<uint32_t>* seeds, double gamma, double* out) {
  const int n = (int)src.size();
  if (int rc = settle(b)) return rc;
  std::vector<double> v((size_t)n + 1);
  return retry_growing(b, "value rollout", [&](UnfinishedWord* w) -> int {
    if (int rc = value_scratch_ensure(b, n)) return rc;
    const ValueClones c{b->d_vrecs, b->d_vflags, n};
    uint32_t* d_word = (uint32_t*)b->d_vvals;
    HIPCHK(hipMemcpyAsync(b->d_vsrc, src.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, 0));
    if (seeds) HIPCHK(hipMemcpyAsync(b->d_vseeds, seeds->data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, 0));
    if (int rc = value_clone(b, c, b->d_vsrc, seeds ? b->d_vseeds : nullptr, 0)) return rc;
    if (int rc = value_resort(b, c, 0)) return rc;
    if (int rc = value_launch_rollouts(b, c, agent, gamma, false, 0)) return rc;
    if (int rc = launched(bbx_launch_value_collect_device(c.recs, b->L.rec_bytes, n, b->d_vvals + 1, d_word, 0, 0), "collect")) return rc;
    HIPCHK(hipMemcpy(v.data(), b->d_vvals, v.size() * sizeof(double), hipMemcpyDeviceToHost));   // the only wait of the call
    *w = word_of(&v[0]);
    if (!w->bits) { memcpy(out, &v[1], (size_t)n * sizeof(double)); return BBX_OK; }
    w->env = src[(size_t)w->env];                               // (the collect reports a clone: "sample" has 100 per environment)
    HIPCHK(hipMemsetAsync(d_word, 0, sizeof(double), 0));
    return BBX_OK;
  });
}

// `seeds`: explicit seeds of the Random rollouts — [n] for "random", [n][100] for "sample" — or null: drawn from the
// handle's own stream (the reference seeds from std::random_device: ours starts from the handle's seed base, so a run is
// reproducible under BBX_DEFAULT_SEED)
int values_for(bbx_batch* b, const std::vector<int32_t>& envs, const char* strategy, double gamma, const int64_t* seeds, double* out) {
  const int n = (int)envs.size();
  auto draw = [b]() { return (long long)(b->value_rng() & 0x7fffffffull); };
  if (!strcmp(strategy, "sample")) {          // best of one Degree and 100 Random rollouts (buchberger.cpp:333-341)
    int rc = value_rollouts(b, envs, BBX_AGENT_DEGREE, nullptr, gamma, out);
    if (rc) return rc;
    std::vector<int32_t> src; std::vector<uint32_t> st;
    src.reserve((size_t)n * 100); st.reserve((size_t)n * 100);
    for (int k = 0; k < n; k++) for (int i = 0; i < 100; i++) { src.push_back(envs[k]); st.push_back(minstd_state_of_seed(seeds ? seeds[(size_t)k * 100 + i] : draw())); }
    std::vector<double> r(src.size());
    rc = value_rollouts(b, src, BBX_AGENT_STDRANDOM, &st, gamma, r.data());
    if (rc) return rc;
    for (int k = 0; k < n; k++) for (int i = 0; i < 100; i++) out[k] = std::max(out[k], r[(size_t)k * 100 + i]);
    return BBX_OK;
  }
  const int agent = agent_of_strategy(strategy);
  if (agent == BBX_AGENT_STDRANDOM) {
    std::vector<uint32_t> st(n);
    for (int k = 0; k < n; k++) st[k] = minstd_state_of_seed(seeds ? seeds[k] : draw());
    return value_rollouts(b, envs, agent, &st, gamma, out);
  }
  return value_rollouts(b, envs, agent, nullptr, gamma, out);
}

// ---- bbx_values_device: the same rollouts without the host in the loop -------------------------------------------------
// The clone is ordered in the caller's stream; resort, rollouts and collect run on a stream of the library's own, into one
// of v_depth clone arrays, so that the tail of a value launch (as long as its longest remaining episode) overlaps the
// steps queued behind the call and the next value launch.  Nothing here waits on the host side.

int value_ring_ensure(bbx_batch* b) {
  if (!b->v_stream) HIPCHK(hipStreamCreateWithFlags(&b->v_stream, hipStreamNonBlocking));   // (non-blocking: the NULL stream of the synchronous value calls does not serialise it)
  if (!b->d_vident) {
    HIPCHK(hipMalloc((void**)&b->d_vident, (size_t)b->B * sizeof(int32_t)));
    HIPCHK(hipMalloc((void**)&b->d_vwords, (size_t)BBX_VALUE_MAX_JOBS * 2 * sizeof(uint32_t)));
    HIPCHK(hipMemsetAsync(b->d_vwords, 0, (size_t)BBX_VALUE_MAX_JOBS * 2 * sizeof(uint32_t), b->v_stream));
    if (int rc = launched(bbx_launch_value_iota(b->d_vident, b->B, b->v_stream), "index")) return rc;
  }
  // the records were enlarged since the slots were made (no call is queued then: settle() resolved them all): made again
  if (!b->v_ring.empty() && memcmp(&b->v_L, &b->L, sizeof(BbxLayout)) != 0 && b->v_jobs.empty()) {
    HIPCHK(hipStreamSynchronize(b->v_stream));
    value_ring_free(b);
  }
  if (b->v_ring.empty()) {
    b->v_ring.resize((size_t)b->v_depth);
    b->v_L = b->L;
    for (bbx_vslot& s : b->v_ring) {
      HIPCHK(hipMalloc((void**)&s.recs, (size_t)b->B * b->L.rec_bytes));
      HIPCHK(hipMalloc((void**)&s.flags, (size_t)b->B));
      HIPCHK(hipMalloc((void**)&s.seeds, (size_t)b->B * sizeof(uint32_t)));
      HIPCHK(hipEventCreateWithFlags(&s.cloned, hipEventDisableTiming));
      HIPCHK(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
    }
  }
  return BBX_OK;
}

int values_device(bbx_batch* b, int agent, double gamma, const int64_t* d_seeds, double* d_values, hipStream_t stream) {
  if ((int)b->v_jobs.size() >= BBX_VALUE_MAX_JOBS)
    return fail(BBX_E_UNSUPPORTED, "%d bbx_values_device calls are queued on this handle: call bbx_sync before queueing more", BBX_VALUE_MAX_JOBS);
  // a running session owns the records on its own stream: closed first, `stream` ordered behind it (a mailbox session is
  // host-stepped, its flight is finished the usual way)
  if (b->ps_active) {
    int rc = b->ps_mbox ? settle(b) : session_close(b, true, stream, false);
    if (rc) return rc;
  }
  if (int rc = value_ring_ensure(b)) return rc;
  const int n = b->B;
  const int slot = (int)(b->v_calls % b->v_depth);
  bbx_vslot& s = b->v_ring[(size_t)slot];
  if (!s.used) HIPCHK(hipEventRecord(s.done, b->v_stream));    // (first use: behind the index array and the cleared words)
  HIPCHK(hipStreamWaitEvent(stream, s.done, 0));               // the slot's previous rollouts: a device-side wait
  if (int rc = d_seeds ? launched(bbx_launch_value_seeds(d_seeds, s.seeds, n, stream), "seed") : BBX_OK) return rc;
  const ValueClones c{s.recs, s.flags, n};
  if (int rc = value_clone(b, c, b->d_vident, d_seeds ? s.seeds : nullptr, stream)) return rc;
  HIPCHK(hipEventRecord(s.cloned, stream));
  HIPCHK(hipStreamWaitEvent(b->v_stream, s.cloned, 0));
  if (int rc = value_resort(b, c, b->v_stream)) return rc;
  if (int rc = value_launch_rollouts(b, c, agent, gamma, false, b->v_stream)) return rc;
  uint32_t* word = b->d_vwords + 2 * b->v_jobs.size();
  if (int rc = launched(bbx_launch_value_collect_device(s.recs, b->L.rec_bytes, n, d_values, word, 0, b->v_stream), "collect")) return rc;
  HIPCHK(hipEventRecord(s.done, b->v_stream));
  s.used = true;
  b->v_jobs.push_back(bbx_vjob{slot, d_values, b->L, agent, gamma});
  b->v_calls++;
  return BBX_OK;
}

// One queued call whose clones did not all finish (word: what its collect folded).  Clones that wait for room are carried over
// to records of the enlarged layout (bbx_relayout_kernel), finish there and fill the entries the collect left NaN.
int value_carry_over(bbx_batch* b, const bbx_vjob& j, size_t jix, const uint32_t* word) {
  const char* what = "value rollout";
  UnfinishedWord w = word_of(word);                                  // (clone k is environment k)
  bool owner = true;                                        // a later call has reused the slot: the waiting clones are gone
  for (size_t i = jix + 1; i < b->v_jobs.size(); i++) owner = owner && b->v_jobs[i].slot != j.slot;
  if (classify(b, w, what) == Unfinished::fail) return BBX_E_CAPACITY;
  const int n = b->B;
  char* src = b->v_ring[(size_t)j.slot].recs; char* tmp = nullptr;
  BbxLayout Ls = j.L;
  uint32_t* dw = b->d_vwords + 2 * jix;
  int rc = BBX_OK;
  for (int attempt = 0; attempt < kGrowAttempts && rc == BBX_OK; attempt++) {
    if (Ls.rec_bytes == b->L.rec_bytes) rc = grow_records(b, w.bits & kCapacityBits, w.env, 0);   // (else: an earlier call of this wait enlarged them already)
    if (rc) break;
    if (!owner) {
      rc = fail(BBX_E_CAPACITY, "value rollout of environment %d outgrew its records (%s) and %d later bbx_values_device calls reused its clone "
                                "before the wait; the records have been enlarged, later calls have room", w.env,
                status_name(__builtin_ctz(w.bits & kCapacityBits)), b->v_depth);
      break;
    }
    char* next = nullptr;
    if (hipMalloc((void**)&next, (size_t)n * b->L.rec_bytes) != hipSuccess) { (void)hipGetLastError(); rc = fail(BBX_E_CAPACITY, "no room for the clones of enlarged records"); break; }
    int lrc = bbx_launch_relayout(src, next, &Ls, &b->L, n, 0);
    if (tmp) { (void)hipStreamSynchronize(0); (void)hipFree(tmp); }
    tmp = next; src = next; Ls = b->L;
    if ((rc = launched(lrc, "relayout"))) break;
    if ((rc = value_launch_rollouts(b, ValueClones{tmp, nullptr, n}, j.agent, j.gamma, true, 0))) break;
    uint32_t h[2] = {0, 0};
    if (hipMemsetAsync(dw, 0, sizeof h, 0) != hipSuccess ||
        bbx_launch_value_collect_device(tmp, b->L.rec_bytes, n, j.d_values, dw, 1, 0) != 0 ||
        hipMemcpy(h, dw, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) { rc = fail(BBX_E_DEVICE, "collect of carried-over clones failed"); break; }
    w = word_of(h);
    const Unfinished u = classify(b, w, what);
    if (u == Unfinished::none) break;
    if (u == Unfinished::fail) rc = BBX_E_CAPACITY;
    else if (attempt == kGrowAttempts - 1) rc = kept_outgrowing(what);
  }
  if (tmp) { (void)hipStreamSynchronize(0); (void)hipFree(tmp); }
  return rc;
}

// ---- bbx_action_values: Q[e][a] = r + gamma * value of the state behind action a, for every pair of every environment ----
// What the reference's tree search does per expanded node (mcts.py:78-102,147; az.py:81-86: env.copy(), step(a), a rollout),
// for the whole batch: one clone per (environment, pair), the flat list cut into passes of at most av.chunk clones.  A pass
// is clone -> ONE step with the clone's own action -> resort -> the strategy's rollouts -> collect into [B][max_rows]
// staging blocks, all on the default stream; the host reads the offsets once before the first pass and the status word and
// the blocks once behind the last.

// the per-clone arrays of a pass and the staging blocks of a call (neither depends on the record layout)
int av_ensure(bbx_batch* b, int n, size_t cells) {
  bbx_avscratch& s = b->av;
  if (n > s.cap) {
    free_dev({s.d_act, s.d_rew, s.d_done});
    s.d_act = nullptr; s.d_rew = nullptr; s.d_done = nullptr; s.cap = 0;
    HIPCHK(hipMalloc((void**)&s.d_act, (size_t)n * sizeof(int32_t)));
    HIPCHK(hipMalloc((void**)&s.d_rew, (size_t)n * sizeof(double)));
    HIPCHK(hipMalloc((void**)&s.d_done, (size_t)n));
    s.cap = n;
  }
  if (cells > s.cells) {
    free_dev({s.d_q, s.d_r, s.d_d});
    s.d_q = nullptr; s.d_r = nullptr; s.d_d = nullptr; s.cells = 0;
    HIPCHK(hipMalloc((void**)&s.d_q, cells * sizeof(double)));
    HIPCHK(hipMalloc((void**)&s.d_r, cells * sizeof(double)));
    HIPCHK(hipMalloc((void**)&s.d_d, cells));
    s.cells = cells;
  }
  if (!s.d_word) HIPCHK(hipMalloc((void**)&s.d_word, 2 * sizeof(uint32_t)));
  return BBX_OK;
}

// The forced first step on the clones: one step with the actions of d_act, no auto-reset, no observation, rewards and done
// flags into per-clone arrays.  Planned as a rollout with a budget of one step: a clone that outgrows the LDS-resident class
// in this very step is continued by the kernel behind it, not left waiting for a host that polls.
int av_launch_first_step(bbx_batch* b, const ValueClones& c) {
  BbxParams p = clone_params(b, c, 2, BBX_AGENT_EXTERNAL);
  p.actions = b->av.d_act; p.rewards = b->av.d_rew; p.dones = b->av.d_done;
  return launch_on_clones(b, p, false, 1, 0);
}

// one pass: positions [first, first + n) of the flat list
int av_pass(bbx_batch* b, int first, int n, int agent, double gamma, int max_rows) {
  bbx_avscratch& s = b->av;
  if (int rc = value_scratch_ensure(b, n)) return rc;
  const ValueClones c{b->d_vrecs, b->d_vflags, n};
  if (int rc = launched(bbx_launch_av_expand(s.d_off, b->B, first, n, b->d_vsrc, s.d_act, 0), "expand")) return rc;
  if (int rc = value_clone(b, c, b->d_vsrc, nullptr, 0)) return rc;
  if (int rc = av_launch_first_step(b, c)) return rc;
  if (int rc = value_resort(b, c, 0)) return rc;                // (behind the step: value() re-sorts the state it is called on)
  if (int rc = value_launch_rollouts(b, c, agent, gamma, false, 0)) return rc;
  return launched(bbx_launch_av_collect(c.recs, b->L.rec_bytes, n, b->d_vsrc, s.d_act, s.d_rew, s.d_done, gamma, max_rows, s.d_q, s.d_r, s.d_d,
                                        s.d_word, 0), "collect");
}

int action_values(bbx_batch* b, int agent, double gamma, int max_rows, double* q, double* rewards, uint8_t* dones, int32_t* rows) {
  const int B = b->B;
  const size_t cells = (size_t)B * (size_t)max_rows;
  if (cells > 0x7fffffffull) return fail(BBX_E_ARG, "batch x max_rows = %zu: the flat clone list is indexed with 32 bits", cells);
  if (int rc = settle(b)) return rc;
  bbx_avscratch& s = b->av;
  if (!s.d_off) HIPCHK(hipMalloc((void**)&s.d_off, (2 * (size_t)B + 3) * sizeof(int32_t)));
  if (int rc = launched(bbx_launch_av_offsets(b->d_recs, b->L.rec_bytes, B, max_rows, s.d_off, 0), "offsets")) return rc;
  std::vector<int32_t> h(2 * (size_t)B + 3);
  HIPCHK(hipMemcpy(h.data(), s.d_off, h.size() * sizeof(int32_t), hipMemcpyDeviceToHost));   // all that visits the host of the states
  if (h[B + 1]) return fail(BBX_E_CAPACITY, "action values of environment %d: it is in an error state: %s", h[B + 1] - 1, status_name(h[B + 2]));
  memcpy(rows, &h[B + 3], (size_t)B * sizeof(int32_t));
  const int total = h[B];
  if (total == 0) {                                           // nothing to value: nothing launched
    for (size_t i = 0; i < cells; i++) q[i] = __builtin_nan("");
    if (rewards) for (size_t i = 0; i < cells; i++) rewards[i] = __builtin_nan("");
    if (dones) memset(dones, 0, cells);
    return BBX_OK;
  }
  std::vector<int32_t> counts(B), first((size_t)total / (size_t)s.chunk + 3);
  for (int e = 0; e < B; e++) counts[e] = h[e + 1] - h[e];
  int32_t npasses = 0;
  if (int rc = bbx_action_values_plan(counts.data(), B, s.chunk, first.data(), (int)first.size(), &npasses)) return rc;
  // (a forced step or a rollout that outgrows the records: ALL passes run again — one word per call does not say which pass)
  return retry_growing(b, "action-value rollout", [&](UnfinishedWord* w) -> int {
    if (int rc = av_ensure(b, std::min(total, s.chunk), cells)) return rc;
    if (int rc = launched(bbx_launch_av_fill(s.d_q, s.d_r, s.d_d, cells, s.d_word, 0), "fill")) return rc;
    for (int p = 0; p < npasses; p++)
      if (int rc = av_pass(b, first[p], first[p + 1] - first[p], agent, gamma, max_rows)) return rc;
    uint32_t word[2] = {0, 0};
    HIPCHK(hipMemcpy(word, s.d_word, sizeof word, hipMemcpyDeviceToHost));   // the wait of the call
    *w = word_of(word);                                  // (this collect reports environments)
    if (w->bits) return BBX_OK;
    HIPCHK(hipMemcpy(q, s.d_q, cells * sizeof(double), hipMemcpyDeviceToHost));
    if (rewards) HIPCHK(hipMemcpy(rewards, s.d_r, cells * sizeof(double), hipMemcpyDeviceToHost));
    if (dones) HIPCHK(hipMemcpy(dones, s.d_d, cells, hipMemcpyDeviceToHost));
    return BBX_OK;
  });
}

}  // namespace

int bbx_value_ring_from_env() {
  const char* s = getenv("BBX_VALUE_RING");
  const int d = s && *s ? atoi(s) : BBX_VALUE_RING_DEFAULT;
  return d < 1 ? 1 : (d > 16 ? 16 : d);
}

namespace bbx_host {
int value_wait(bbx_batch* b) {
  if (!b->v_jobs.empty()) HIPCHK(hipStreamSynchronize(b->v_stream));   // (it waited for every clone: the caller's streams are done with the records too)
  return BBX_OK;
}

int value_resolve(bbx_batch* b) {
  if (b->v_jobs.empty()) return BBX_OK;
  const size_t nj = b->v_jobs.size();
  std::vector<uint32_t> w(2 * nj);
  int err = BBX_OK; std::string msg;
  if (hipMemcpy(w.data(), b->d_vwords, w.size() * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) err = fail(BBX_E_DEVICE, "reading the value words failed");
  else for (size_t i = 0; i < nj; i++) {
    if (!w[2 * i]) continue;
    const int rc = value_carry_over(b, b->v_jobs[i], i, &w[2 * i]);   // (every call is served; the first error is the one reported)
    if (rc && !err) { err = rc; msg = bbx_last_error(); }
  }
  b->v_jobs.clear();
  (void)hipMemsetAsync(b->d_vwords, 0, 2 * nj * sizeof(uint32_t), b->v_stream);
  if (err && !msg.empty()) return fail(err, "%s", msg.c_str());
  return err;
}

void value_ring_free(bbx_batch* b) {
  for (bbx_vslot& s : b->v_ring) {
    free_dev({s.recs, s.flags, s.seeds});
    if (s.cloned) (void)hipEventDestroy(s.cloned);
    if (s.done) (void)hipEventDestroy(s.done);
  }
  b->v_ring.clear();
}

void value_scratch_free(bbx_batch* b) {
  free_dev({b->d_vrecs, b->d_vflags, b->d_vsrc, b->d_vseeds, b->d_vvals});
  b->d_vrecs = nullptr; b->d_vflags = nullptr; b->d_vsrc = nullptr; b->d_vseeds = nullptr; b->d_vvals = nullptr; b->vcap = 0;
}

void action_values_free(bbx_batch* b) {
  bbx_avscratch& s = b->av;
  free_dev({s.d_off, s.d_act, s.d_rew, s.d_done, s.d_q, s.d_r, s.d_d, s.d_word});
  const int chunk = s.chunk;
  s = bbx_avscratch{}; s.chunk = chunk;
}
}  // namespace bbx_host

extern "C" int bbx_values_device(bbx_batch* b, const char* strategy, double gamma, const int64_t* d_seeds, double* d_values, void* stream) {
  if (!b || !strategy || !d_values) return fail(BBX_E_ARG, "bad arguments");
  if (!strcmp(strategy, "sample")) return fail(BBX_E_UNSUPPORTED, "\"sample\" (101 rollouts per environment) has no asynchronous form: use bbx_values");
  const int agent = agent_of_strategy(strategy);
  if (agent == BBX_AGENT_STDRANDOM && !d_seeds) return fail(BBX_E_ARG, "\"random\" needs d_seeds (the handle's own seed stream lives on the host: bbx_values)");
  HIPCHK(hipSetDevice(b->device)); b->api_epoch++;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (stream != nullptr && hipStreamIsCapturing((hipStream_t)stream, &cap) != hipSuccess) { (void)hipGetLastError(); cap = hipStreamCaptureStatusNone; }
  if (cap != hipStreamCaptureStatusNone) return fail(BBX_E_UNSUPPORTED, "bbx_values_device cannot be captured into a graph (its clone ring is host bookkeeping)");
  return values_device(b, agent, gamma, agent == BBX_AGENT_STDRANDOM ? d_seeds : nullptr, d_values, (hipStream_t)stream);
}

extern "C" int bbx_gae_bootstrap_device(const double* d_rewards, const double* d_values, const uint8_t* d_dones, int nsteps, int batch,
                                        double gam, double lam, const double* d_last_values, double* d_returns, double* d_advantages,
                                        uint8_t* d_complete, double* d_lambda_returns, void* stream) {
  if (!d_rewards || !d_values || !d_dones || !d_returns || !d_advantages || !d_complete || nsteps < 0 || batch < 0) return fail(BBX_E_ARG, "bad arguments");
  if (nsteps == 0 || batch == 0) return BBX_OK;
  return launched(bbx_launch_gae(d_rewards, d_values, d_dones, nsteps, batch, gam, gam * lam, d_last_values, d_returns, d_advantages, d_complete,
                                 d_lambda_returns, (hipStream_t)stream), "GAE");
}

extern "C" int bbx_gae_device(const double* d_rewards, const double* d_values, const uint8_t* d_dones, int nsteps, int batch,
                              double gam, double lam, double* d_returns, double* d_advantages, uint8_t* d_complete, void* stream) {
  return bbx_gae_bootstrap_device(d_rewards, d_values, d_dones, nsteps, batch, gam, lam, nullptr, d_returns, d_advantages, d_complete, nullptr, stream);
}

// per-episode returns and lengths of a [nsteps][batch] block of rewards and dones (bbx_episodes_kernel): no handle, asynchronous.
// T == 0 with carries: nothing to add to them
extern "C" int bbx_episodes_device(const double* d_rewards, const uint8_t* d_dones, int nsteps, int batch, double* d_carry_return,
                                   int32_t* d_carry_len, int32_t* d_ep_count, double* d_ep_return, int32_t* d_ep_len, void* stream) {
  if (nsteps < 0 || batch < 1) return fail(BBX_E_ARG, "bad arguments (nsteps = %d, batch = %d)", nsteps, batch);
  if (nsteps == 0) return BBX_OK;
  if (!d_rewards || !d_dones || !d_ep_return || !d_ep_len) return fail(BBX_E_ARG, "null argument");
  return launched(bbx_launch_episodes(d_rewards, d_dones, nsteps, batch, d_carry_return, d_carry_len, d_ep_count, d_ep_return, d_ep_len, (hipStream_t)stream),
                  "episodes");
}

extern "C" int bbx_value(bbx_batch* b, int idx, const char* strategy, double gamma, double* out) {
  if (!b || !strategy || !out || idx < 0 || idx >= b->B) return fail(BBX_E_ARG, "bad arguments");
  HIPCHK(hipSetDevice(b->device)); b->api_epoch++;
  return values_for(b, std::vector<int32_t>{idx}, strategy, gamma, nullptr, out);
}

extern "C" int bbx_values_seeded(bbx_batch* b, const char* strategy, double gamma, const int64_t* seeds, double* out) {
  if (!b || !strategy || !out) return fail(BBX_E_ARG, "bad arguments");
  HIPCHK(hipSetDevice(b->device)); b->api_epoch++;
  std::vector<int32_t> envs(b->B);
  for (int e = 0; e < b->B; e++) envs[e] = e;
  return values_for(b, envs, strategy, gamma, seeds, out);
}

// The pass plan of bbx_action_values, on the host alone: the flat (environment, action) list — environment e contributes
// counts[e] positions — cut into contiguous ranges of at most `chunk`; first[p] is where pass p begins, first[npasses] the total
extern "C" int bbx_action_values_plan(const int32_t* counts, int B, int chunk, int32_t* first, int cap, int32_t* npasses) {
  if (!counts || !first || !npasses || B < 0 || chunk < 1 || cap < 0) return fail(BBX_E_ARG, "bad arguments");
  long long total = 0;
  for (int e = 0; e < B; e++) {
    if (counts[e] < 0) return fail(BBX_E_ARG, "counts[%d] = %d is negative", e, counts[e]);
    total += counts[e];
  }
  if (total > 0x7fffffffll) return fail(BBX_E_ARG, "%lld clones: the flat list is indexed with 32 bits", total);
  const long long n = (total + chunk - 1) / chunk;
  if (n + 1 > cap) return fail(BBX_E_CAPACITY, "%lld passes need %lld elements in first[], cap = %d", n, n + 1, cap);
  for (long long p = 0; p < n; p++) first[p] = (int32_t)(p * chunk);
  first[n] = (int32_t)total;
  *npasses = (int32_t)n;
  return BBX_OK;
}

extern "C" int bbx_action_values_chunk(bbx_batch* b, int clones) {
  if (!b) return fail(BBX_E_ARG, "null argument");
  const int before = b->av.chunk;
  b->av.chunk = clones <= 0 ? BBX_AV_CHUNK_DEFAULT : clones;
  return before;
}

extern "C" int bbx_action_values(bbx_batch* b, const char* strategy, double gamma, int max_rows, double* q, double* rewards, uint8_t* dones,
                                 int32_t* rows) {
  if (!b || !strategy || !q || !rows || max_rows < 1) return fail(BBX_E_ARG, "bad arguments");
  if (!strcmp(strategy, "random") || !strcmp(strategy, "sample"))
    return fail(BBX_E_UNSUPPORTED, "action values under \"%s\" need a seed stream per clone: not built (degree, normal, sugar, first)", strategy);
  HIPCHK(hipSetDevice(b->device)); b->api_epoch++;
  return action_values(b, agent_of_strategy(strategy), gamma, max_rows, q, rewards, dones, rows);
}

extern "C" int bbx_values(bbx_batch* b, const char* strategy, double gamma, double* out) {
  return bbx_values_seeded(b, strategy, gamma, nullptr, out);   // (no seeds: drawn from the handle's own stream)
}


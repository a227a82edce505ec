// libbbx.so — LeadMonomialsEnv::value (buchberger.cpp:332-351): discounted returns of full Buchberger rollouts from clones of
// the current states (bbx_value, bbx_values, bbx_values_seeded of include/bbx.h), their asynchronous form (bbx_values_device)
// and the same rollouts behind every pair of every environment (bbx_action_values).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "bbx_batch.h"

using namespace bbx_host;

// ---- value(): discounted return of full Buchberger rollouts from clones of the current states ---------------------
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

// One rollout to completion per entry of src (indices into b), from clones of the current states; seeds != null: the
// engine states of the clones' seeded Random selection.  Everything runs on the default stream without a copy in between
// and with one wait: values + completion marks come back in one transfer at the end (clones whose generator lead monomials
// tie get the reducer order buchberger()'s std::sort would give them from a kernel: bbx_value_resort_kernel).  3-variable binomial batches run on the register/LDS-resident class (bbx_fast_value_kernel),
// environments that outgrow it and every other batch on the HBM-resident class of the batch, long-polynomial
// environments one workgroup per clone.  A clone that runs out of room enlarges the records of the whole batch
// (grow_records) and the rollouts start again.
// the clone arrays of value() and bbx_action_values: room for n clones in the batch's current layout (kept between calls;
// grow_records frees them, so a call after the records were enlarged makes them again)
int value_scratch_ensure(bbx_batch* b, int n) {
  if (n <= b->vcap) return BBX_OK;
  void* old[] = {b->d_vrecs, b->d_vhdr, b->d_vsrc, b->d_vseeds, b->d_vvals};
  for (void* q : old) (void)hipFree(q);
  b->d_vrecs = nullptr; b->d_vhdr = nullptr; b->d_vsrc = nullptr; b->d_vseeds = nullptr; b->d_vvals = nullptr; b->vcap = 0;
  HIPCHK(hipMalloc((void**)&b->d_vrecs, (size_t)n * b->L.rec_bytes));
  HIPCHK(hipMalloc((void**)&b->d_vhdr, (size_t)n));                        // clone flags (u8)
  HIPCHK(hipMalloc((void**)&b->d_vsrc, (size_t)n * sizeof(int32_t)));
  HIPCHK(hipMalloc((void**)&b->d_vseeds, (size_t)n * sizeof(uint32_t)));
  HIPCHK(hipMalloc((void**)&b->d_vvals, (size_t)n * 2 * sizeof(double)));  // {value, completion mark} per clone
  b->vcap = n;
  return BBX_OK;
}

int value_rollouts(bbx_batch* b, const std::vector<int32_t>& src, int agent, const std::vector<uint32_t>* seeds, double gamma, double* out) {
  const int n = (int)src.size();
  if (int rc = settle(b)) return rc;
  for (int attempt = 0; attempt < 40; attempt++) {
    if (int rc = value_scratch_ensure(b, n)) return rc;
    HIPCHK(hipMemcpyAsync(b->d_vsrc, src.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, 0));
    if (seeds) HIPCHK(hipMemcpyAsync(b->d_vseeds, seeds->data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, 0));
    const int ngen = b->sort_reducers ? b->gens[0]->npolys() : 0;
    uint8_t* d_flags = (uint8_t*)b->d_vhdr;
    int lrc = bbx_launch_clone(b->d_recs, b->d_vrecs, &b->L, b->d_vsrc, nullptr, n, seeds ? b->d_vseeds : nullptr, 0, 1, ngen, d_flags, 0);
    if (lrc) return fail(BBX_E_DEVICE, "clone launch failed: %s", hipGetErrorString((hipError_t)lrc));
    lrc = bbx_launch_value_resort(b->d_vrecs, &b->L, n, d_flags, 0);   // (clones whose generators tie: std::sort's order)
    if (lrc) return fail(BBX_E_DEVICE, "resort launch failed: %s", hipGetErrorString((hipError_t)lrc));
    BbxParams p; fill_params(b, &p);
    p.recs = b->d_vrecs; p.B = n; p.nsteps = 1 << 30; p.set_budget = 1; p.agent = agent; p.auto_reset = 0;
    p.value_mode = 1; p.gamma = gamma; p.values = nullptr; p.trace = nullptr; p.accounting = 0;
    p.lite = nullptr;                                           // the clones are not the batch's environments
    const LaunchPlan pl = plan_launch(b, p, false, true);      // (the fast class: every selection strategy, bbx_fast.h f_select_ordered)
    for (int i = 0; i < pl.n && !lrc; i++) lrc = bbx_launch_step(&pl.pass[i], pl.kind[i], pl.waves[i], 0);
    if (lrc) return fail(BBX_E_DEVICE, "kernel launch failed: %s", hipGetErrorString((hipError_t)lrc));
    lrc = bbx_launch_value_collect(b->d_vrecs, b->L.rec_bytes, n, b->d_vvals, 0);
    if (lrc) return fail(BBX_E_DEVICE, "collect launch failed: %s", hipGetErrorString((hipError_t)lrc));
    std::vector<double> v2((size_t)n * 2);
    HIPCHK(hipMemcpy(v2.data(), b->d_vvals, v2.size() * sizeof(double), hipMemcpyDeviceToHost));   // the only wait of the call
    unsigned grow = 0; int grow_k = -1;
    for (int k = 0; k < n; k++) {
      const int st = (int)v2[2 * (size_t)k + 1];
      if (st == 0) continue;
      if (st > 0 && bbx_st_capacity(st) && !b->no_growth) { grow |= 1u << st; if (grow_k < 0) grow_k = k; continue; }
      return fail(BBX_E_CAPACITY, "value rollout of environment %d did not finish: %s", src[k], st > 0 ? status_name(st) : "pairs left");
    }
    if (!grow) {
      for (int k = 0; k < n; k++) out[k] = v2[2 * (size_t)k];
      return BBX_OK;
    }
    int rc = grow_records(b, grow, src[grow_k], 0);             // (frees the clones: sized by the old layout)
    if (rc) return rc;
  }
  return fail(BBX_E_CAPACITY, "value rollouts kept outgrowing the records");
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
    int lrc = bbx_launch_value_iota(b->d_vident, b->B, b->v_stream);
    if (lrc) return fail(BBX_E_DEVICE, "index launch failed: %s", hipGetErrorString((hipError_t)lrc));
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

// the rollout kernels of value() on `recs` (resume: clones carried over to enlarged records continue where they stopped)
int value_launch_rollouts(bbx_batch* b, char* recs, int n, int agent, double gamma, bool resume, hipStream_t stream) {
  BbxParams p; fill_params(b, &p);
  p.recs = recs; p.B = n; p.nsteps = 1 << 30; p.set_budget = 1; p.agent = agent; p.auto_reset = 0;
  p.value_mode = 1; p.gamma = gamma; p.values = nullptr; p.trace = nullptr; p.accounting = 0;
  p.lite = nullptr;                                           // the clones are not the batch's environments
  const LaunchPlan pl = plan_launch(b, p, resume, true);
  int lrc = 0;
  for (int i = 0; i < pl.n && !lrc; i++) lrc = bbx_launch_step(&pl.pass[i], pl.kind[i], pl.waves[i], stream);
  if (lrc) return fail(BBX_E_DEVICE, "kernel launch failed: %s", hipGetErrorString((hipError_t)lrc));
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
  if (s.used) HIPCHK(hipStreamWaitEvent(stream, s.done, 0));   // the slot's previous rollouts: a device-side wait
  else {                                                       // (first use: behind the index array and the cleared words)
    HIPCHK(hipEventRecord(s.done, b->v_stream));
    HIPCHK(hipStreamWaitEvent(stream, s.done, 0));
  }
  int lrc = 0;
  if (d_seeds) {
    lrc = bbx_launch_value_seeds(d_seeds, s.seeds, n, stream);
    if (lrc) return fail(BBX_E_DEVICE, "seed launch failed: %s", hipGetErrorString((hipError_t)lrc));
  }
  const int ngen = b->sort_reducers ? b->gens[0]->npolys() : 0;
  lrc = bbx_launch_clone(b->d_recs, s.recs, &b->L, b->d_vident, nullptr, n, d_seeds ? s.seeds : nullptr, 0, 1, ngen, s.flags, stream);
  if (lrc) return fail(BBX_E_DEVICE, "clone launch failed: %s", hipGetErrorString((hipError_t)lrc));
  HIPCHK(hipEventRecord(s.cloned, stream));
  HIPCHK(hipStreamWaitEvent(b->v_stream, s.cloned, 0));
  lrc = bbx_launch_value_resort(s.recs, &b->L, n, s.flags, b->v_stream);
  if (lrc) return fail(BBX_E_DEVICE, "resort launch failed: %s", hipGetErrorString((hipError_t)lrc));
  if (int rc = value_launch_rollouts(b, s.recs, n, agent, gamma, false, b->v_stream)) return rc;
  uint32_t* word = b->d_vwords + 2 * b->v_jobs.size();
  lrc = bbx_launch_value_collect_device(s.recs, b->L.rec_bytes, n, d_values, word, 0, b->v_stream);
  if (lrc) return fail(BBX_E_DEVICE, "collect launch failed: %s", hipGetErrorString((hipError_t)lrc));
  HIPCHK(hipEventRecord(s.done, b->v_stream));
  s.used = true;
  b->v_jobs.push_back(bbx_vjob{slot, d_values, b->L, agent, gamma});
  b->v_calls++;
  return BBX_OK;
}

// One queued call whose clones did not all finish (word: what its collect folded).  Clones that wait for room are carried over
// to records of the enlarged layout (bbx_relayout_kernel), finish there and fill the entries the collect left NaN.
int value_carry_over(bbx_batch* b, const bbx_vjob& j, size_t jix, const uint32_t* word) {
  const unsigned capmask = (1u << BBX_ST_G_FULL) | (1u << BBX_ST_P_FULL) | (1u << BBX_ST_ARENA_FULL) | (1u << BBX_ST_POLY_TOO_LONG);
  unsigned bits = word[0]; int env = (int)word[1] - 1;
  bool owner = true;                                        // a later call has reused the slot: the waiting clones are gone
  for (size_t i = jix + 1; i < b->v_jobs.size(); i++) owner = owner && b->v_jobs[i].slot != j.slot;
  if ((bits & ~capmask) || b->no_growth)
    return fail(BBX_E_CAPACITY, "value rollout of environment %d did not finish: %s", env,
                (bits & capmask) ? status_name(__builtin_ctz(bits & capmask)) : "pairs left or an environment in an error state");
  const int n = b->B;
  char* src = b->v_ring[(size_t)j.slot].recs; char* tmp = nullptr;
  BbxLayout Ls = j.L;
  uint32_t* dw = b->d_vwords + 2 * jix;
  int rc = BBX_OK;
  for (int attempt = 0; attempt < 40 && rc == BBX_OK; attempt++) {
    if (Ls.rec_bytes == b->L.rec_bytes) rc = grow_records(b, bits & capmask, env, 0);   // (else: an earlier call of this wait enlarged them already)
    if (rc) break;
    if (!owner) {
      rc = fail(BBX_E_CAPACITY, "value rollout of environment %d outgrew its records (%s) and %d later bbx_values_device calls reused its clone "
                                "before the wait; the records have been enlarged, later calls have room", env,
                status_name(__builtin_ctz(bits & capmask)), b->v_depth);
      break;
    }
    char* next = nullptr;
    if (hipMalloc((void**)&next, (size_t)n * b->L.rec_bytes) != hipSuccess) { (void)hipGetLastError(); rc = fail(BBX_E_CAPACITY, "no room for the clones of enlarged records"); break; }
    int lrc = bbx_launch_relayout(src, next, &Ls, &b->L, n, 0);
    if (tmp) { (void)hipStreamSynchronize(0); (void)hipFree(tmp); }
    tmp = next; src = next; Ls = b->L;
    if (lrc) { rc = fail(BBX_E_DEVICE, "relayout launch failed: %s", hipGetErrorString((hipError_t)lrc)); break; }
    if ((rc = value_launch_rollouts(b, tmp, n, j.agent, j.gamma, true, 0))) break;
    uint32_t w[2] = {0, 0};
    if (hipMemsetAsync(dw, 0, sizeof w, 0) != hipSuccess ||
        bbx_launch_value_collect_device(tmp, b->L.rec_bytes, n, j.d_values, dw, 1, 0) != 0 ||
        hipMemcpy(w, dw, sizeof w, hipMemcpyDeviceToHost) != hipSuccess) { rc = fail(BBX_E_DEVICE, "collect of carried-over clones failed"); break; }
    bits = w[0]; env = (int)w[1] - 1;
    if (!bits) break;
    if (bits & ~capmask) rc = fail(BBX_E_CAPACITY, "value rollout of environment %d did not finish: pairs left", env);
    else if (attempt == 39) rc = fail(BBX_E_CAPACITY, "value rollouts kept outgrowing the records");
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
    void* old[] = {s.d_act, s.d_rew, s.d_done};
    for (void* q : old) if (q) (void)hipFree(q);
    s.d_act = nullptr; s.d_rew = nullptr; s.d_done = nullptr; s.cap = 0;
    HIPCHK(hipMalloc((void**)&s.d_act, (size_t)n * sizeof(int32_t)));
    HIPCHK(hipMalloc((void**)&s.d_rew, (size_t)n * sizeof(double)));
    HIPCHK(hipMalloc((void**)&s.d_done, (size_t)n));
    s.cap = n;
  }
  if (cells > s.cells) {
    void* old[] = {s.d_q, s.d_r, s.d_d};
    for (void* q : old) if (q) (void)hipFree(q);
    s.d_q = nullptr; s.d_r = nullptr; s.d_d = nullptr; s.cells = 0;
    HIPCHK(hipMalloc((void**)&s.d_q, cells * sizeof(double)));
    HIPCHK(hipMalloc((void**)&s.d_r, cells * sizeof(double)));
    HIPCHK(hipMalloc((void**)&s.d_d, cells));
    s.cells = cells;
  }
  if (!s.d_word) HIPCHK(hipMalloc((void**)&s.d_word, 2 * sizeof(uint32_t)));
  return BBX_OK;
}

// The forced first step on the clones in `recs`: one step with the actions of d_act, no auto-reset, no observation, rewards
// and done flags into per-clone arrays.  The kernels are those plan_launch gives a rollout of the class — the first kernel and
// the one that takes over what it hands on: a clone that outgrows the LDS-resident class in this very step is continued, not
// left waiting for a host that polls —, each with a budget of one step.
int av_launch_first_step(bbx_batch* b, char* recs, int n) {
  BbxParams p; fill_params(b, &p);
  p.recs = recs; p.B = n; p.nsteps = 2; p.set_budget = 1; p.agent = BBX_AGENT_EXTERNAL; p.auto_reset = 0;
  p.actions = b->av.d_act; p.rewards = b->av.d_rew; p.dones = b->av.d_done;
  p.trace = nullptr; p.accounting = 0;
  p.lite = nullptr;                                           // the clones are not the batch's environments
  LaunchPlan pl = plan_launch(b, p, false, true);
  int lrc = 0;
  for (int i = 0; i < pl.n && !lrc; i++) { pl.pass[i].nsteps = 1; lrc = bbx_launch_step(&pl.pass[i], pl.kind[i], pl.waves[i], 0); }
  if (lrc) return fail(BBX_E_DEVICE, "kernel launch failed: %s", hipGetErrorString((hipError_t)lrc));
  return BBX_OK;
}

// one pass: positions [first, first + n) of the flat list
int av_pass(bbx_batch* b, int first, int n, int agent, double gamma, int max_rows) {
  bbx_avscratch& s = b->av;
  if (int rc = value_scratch_ensure(b, n)) return rc;
  int lrc = bbx_launch_av_expand(s.d_off, b->B, first, n, b->d_vsrc, s.d_act, 0);
  if (lrc) return fail(BBX_E_DEVICE, "expand launch failed: %s", hipGetErrorString((hipError_t)lrc));
  const int ngen = b->sort_reducers ? b->gens[0]->npolys() : 0;
  uint8_t* d_flags = (uint8_t*)b->d_vhdr;
  lrc = bbx_launch_clone(b->d_recs, b->d_vrecs, &b->L, b->d_vsrc, nullptr, n, nullptr, 0, 1, ngen, d_flags, 0);
  if (lrc) return fail(BBX_E_DEVICE, "clone launch failed: %s", hipGetErrorString((hipError_t)lrc));
  if (int rc = av_launch_first_step(b, b->d_vrecs, n)) return rc;
  // (behind the step: value() re-sorts the state it is called on; the flags are the clone's — a step leaves the generators alone)
  lrc = bbx_launch_value_resort(b->d_vrecs, &b->L, n, d_flags, 0);
  if (lrc) return fail(BBX_E_DEVICE, "resort launch failed: %s", hipGetErrorString((hipError_t)lrc));
  if (int rc = value_launch_rollouts(b, b->d_vrecs, n, agent, gamma, false, 0)) return rc;
  lrc = bbx_launch_av_collect(b->d_vrecs, b->L.rec_bytes, n, b->d_vsrc, s.d_act, s.d_rew, s.d_done, gamma, max_rows, s.d_q, s.d_r, s.d_d, s.d_word, 0);
  if (lrc) return fail(BBX_E_DEVICE, "collect launch failed: %s", hipGetErrorString((hipError_t)lrc));
  return BBX_OK;
}

int action_values(bbx_batch* b, int agent, double gamma, int max_rows, double* q, double* rewards, uint8_t* dones, int32_t* rows) {
  const int B = b->B;
  const size_t cells = (size_t)B * (size_t)max_rows;
  if (cells > 0x7fffffffull) return fail(BBX_E_ARG, "batch x max_rows = %zu: the flat clone list is indexed with 32 bits", cells);
  if (int rc = settle(b)) return rc;
  bbx_avscratch& s = b->av;
  if (!s.d_off) HIPCHK(hipMalloc((void**)&s.d_off, (2 * (size_t)B + 3) * sizeof(int32_t)));
  int lrc = bbx_launch_av_offsets(b->d_recs, b->L.rec_bytes, B, max_rows, s.d_off, 0);
  if (lrc) return fail(BBX_E_DEVICE, "offsets launch failed: %s", hipGetErrorString((hipError_t)lrc));
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
  const unsigned capmask = (1u << BBX_ST_G_FULL) | (1u << BBX_ST_P_FULL) | (1u << BBX_ST_ARENA_FULL) | (1u << BBX_ST_POLY_TOO_LONG);
  for (int attempt = 0; attempt < 40; attempt++) {
    if (int rc = av_ensure(b, std::min(total, s.chunk), cells)) return rc;
    lrc = bbx_launch_av_fill(s.d_q, s.d_r, s.d_d, cells, s.d_word, 0);
    if (lrc) return fail(BBX_E_DEVICE, "fill launch failed: %s", hipGetErrorString((hipError_t)lrc));
    for (int p = 0; p < npasses; p++)
      if (int rc = av_pass(b, first[p], first[p + 1] - first[p], agent, gamma, max_rows)) return rc;
    uint32_t w[2] = {0, 0};
    HIPCHK(hipMemcpy(w, s.d_word, sizeof w, hipMemcpyDeviceToHost));   // the wait of the call
    if (!w[0]) {
      HIPCHK(hipMemcpy(q, s.d_q, cells * sizeof(double), hipMemcpyDeviceToHost));
      if (rewards) HIPCHK(hipMemcpy(rewards, s.d_r, cells * sizeof(double), hipMemcpyDeviceToHost));
      if (dones) HIPCHK(hipMemcpy(dones, s.d_d, cells, hipMemcpyDeviceToHost));
      return BBX_OK;
    }
    const int env = (int)w[1] - 1;
    if ((w[0] & ~capmask) || b->no_growth)
      return fail(BBX_E_CAPACITY, "action-value rollout of environment %d did not finish: %s", env,
                  (w[0] & capmask) ? status_name(__builtin_ctz(w[0] & capmask)) : "pairs left or a clone in an error state");
    // a clone's forced step or rollout outgrew the records: those of the whole batch are enlarged (the clone arrays go with
    // the old layout) and the passes run again — the results are those of a handle created with room to spare
    if (int rc = grow_records(b, w[0] & capmask, env, 0)) return rc;
  }
  return fail(BBX_E_CAPACITY, "action-value rollouts kept outgrowing the records");
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
    void* dev[] = {s.recs, s.flags, s.seeds};
    for (void* q : dev) if (q) (void)hipFree(q);
    if (s.cloned) (void)hipEventDestroy(s.cloned);
    if (s.done) (void)hipEventDestroy(s.done);
  }
  b->v_ring.clear();
}

void action_values_free(bbx_batch* b) {
  bbx_avscratch& s = b->av;
  void* dev[] = {s.d_off, s.d_act, s.d_rew, s.d_done, s.d_q, s.d_r, s.d_d, s.d_word};
  for (void* q : dev) if (q) (void)hipFree(q);
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
  const int lrc = bbx_launch_gae(d_rewards, d_values, d_dones, nsteps, batch, gam, gam * lam, d_last_values, d_returns, d_advantages, d_complete,
                                 d_lambda_returns, (hipStream_t)stream);
  if (lrc) return fail(BBX_E_DEVICE, "GAE launch failed: %s", hipGetErrorString((hipError_t)lrc));
  return BBX_OK;
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
  const int lrc = bbx_launch_episodes(d_rewards, d_dones, nsteps, batch, d_carry_return, d_carry_len, d_ep_count, d_ep_return, d_ep_len, (hipStream_t)stream);
  if (lrc) return fail(BBX_E_DEVICE, "episodes launch failed: %s", hipGetErrorString((hipError_t)lrc));
  return BBX_OK;
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
  if (!b || !strategy || !out) return fail(BBX_E_ARG, "bad arguments");
  HIPCHK(hipSetDevice(b->device)); b->api_epoch++;
  std::vector<int32_t> envs(b->B);
  for (int e = 0; e < b->B; e++) envs[e] = e;
  return values_for(b, envs, strategy, gamma, nullptr, out);
}


// The batch handle of libbbx's C ABI and the internals its translation units share (bbx_api.cpp: creation, kernels of a
// launch, waits, stepping; bbx_api_session.cpp: what a call becomes — persistent / mailbox sessions, recorded steps;
// bbx_api_value.cpp: the value calls — one pipeline, one outgrow policy; bbx_api_policy.cpp: the PMLP policy calls — prepare,
// act, policy step, policy rollouts, and the training calls of policy and critic, one body per call for both depths;
// bbx_api_state.cpp: introspection, generators, text format).  The launchers of the kernel files they call are declared in
// bbx_launch.h, which the kernel files include as well.
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <random>
#include <string>
#include <deque>
#include <vector>

#include "bbx_host.h"
#include "bbx_ideals.h"
#include "bbx_launch.h"

// The call in flight: what finish() waits for, continues and reports on.  Formed in two places only — start_flight() (a
// call begins) and continue_session() (a closed session's closing kernels, bbx_api_session.cpp); grow_records moves its
// records; finish() ends it.  A recorded call (bbx_batch::cap) is the same record, restored by bbx_graph_replayed.
struct bbx_flight {
  bool active = false;                // finish() has not yet waited for it
  BbxParams p{};                      // its parameters, ctl and policy dropped (the policy is a host pointer of the caller's frame)
  hipStream_t stream = 0;             // where it runs (the session stream for a session's call)
  bool obs_external = false;          // writes observations into a caller-owned block: rows cut for lack of space are an error
                                      // the caller must hear about (bbx_sync)
  bool device_async = false;          // came through a *_device entry point (no host poll per step)
  bool policy_rollout = false;        // a policy rollout outside a session: what it left unfinished cannot be resumed
  bool poll = false;                  // its kernel signals completion through the pinned status words (enqueue -> read_lite)
  int async_chain = 0;                // asynchronous steps with caller-supplied actions queued since the last wait
};

// bbx_values_device (bbx_api_value.cpp): a ring of clone arrays, so that the rollouts of consecutive calls overlap each other
// and the steps that follow; a slot is reused behind a device-side wait for `done`.
struct bbx_vslot {
  char* recs = nullptr;               // [B] records in the layout of the batch when the slot was made
  uint8_t* flags = nullptr;           // clone flags (bbx_clone_kernel)
  uint32_t* seeds = nullptr;          // engine states of "random" rollouts
  hipEvent_t cloned = nullptr;        // the clone has run (the caller's stream) — what the rollouts wait for
  hipEvent_t done = nullptr;          // the collect has run (the library's stream) — what the next clone into the slot waits for
  bool used = false;                  // `done` has been recorded at least once
};
// One queued call: resolved by the next settle() (value_resolve)
struct bbx_vjob {
  int slot; double* d_values; BbxLayout L; int agent; double gamma;
};
constexpr int BBX_VALUE_RING_DEFAULT = 2;   // measured: 2, 4 and 8 are equal, 1 is 8 % slower
constexpr int BBX_VALUE_MAX_JOBS = 8192;    // calls between two waits (a word pair each)
int bbx_value_ring_from_env();        // BBX_VALUE_RING, clamped to 1..16

// bbx_action_values (bbx_api_value.cpp): what it keeps between calls besides the clone scratch it shares with value()
// (sized by the record layout: value_scratch_free).  Nothing here depends on the layout.
constexpr int BBX_AV_CHUNK_DEFAULT = 65536;   // clones in flight per pass (bbx_action_values_chunk)
struct bbx_avscratch {
  int chunk = BBX_AV_CHUNK_DEFAULT;
  int32_t* d_off = nullptr;           // [2 B + 3]: offsets, error pair, full pair counts (bbx_av_offsets_kernel)
  int32_t* d_act = nullptr; double* d_rew = nullptr; uint8_t* d_done = nullptr; int cap = 0;   // per clone: forced action, its reward and done flag
  double* d_q = nullptr; double* d_r = nullptr; uint8_t* d_d = nullptr; size_t cells = 0;      // [B][max_rows] staging blocks
  uint32_t* d_word = nullptr;         // the status word pair of the call (bbx_av_collect_kernel)
};

struct bbx_gen {
  std::unique_ptr<bbx::IdealGen> g;
  bbx::HIdeal last;
};

// The kernel class of a handle, chosen once by create_common; which kernels a launch of each is made of: plan_launch
// 
enum class BbxClass { FAST, BINOM_STAGED, GENERAL_STAGED, BINOM_HBM, GENERAL_HBM, GENERAL_TO_WIDE, WIDE };
inline bool lds_staged(BbxClass c) { return c == BbxClass::FAST || c == BbxClass::BINOM_STAGED || c == BbxClass::GENERAL_STAGED; }

// What create_common decides about a handle, and all of it that bbx_copy carries over.  L changes when the records grow
// (grow_records), accounting with bbx_accounting, policy_greedy with bbx_policy_greedy; nothing else changes after creation.
struct bbx_config {
  int B = 0, device = 0, k = 1, nvars = 0, W = 2;
  int elim = 0, rewards = 0, sort_input = 0, sort_reducers = 1;
  bool fixed = false, binom = false, listed = false;   // binom: the record format; listed: ideals of bbx_create_ideals
  BbxLayout L{}, LL{};                // the HBM record; the working copy of the LDS-staged classes
  BbxClass cls = BbxClass::GENERAL_HBM;
  uint32_t slot_words = 0, nslots = 0;   // ideal queue geometry
  int envs_per_block = 4;
  int fast_G = 0, fast_P = 0;          // capacities of the register/LDS-resident class (BbxParams::fast_G)
  int wide_waves = 0;                 // waves per environment of the wide kernel (WIDE, GENERAL_TO_WIDE)
  int wide_terms = 0;                 // forced LDS capacity of the wide class (caps.wide_lds_terms), 0 = automatic
  int ncu = 0;                        // compute units of the device
  bool no_growth = false;             // bbx_caps.no_growth: the configured capacities are hard limits (BBX_E_CAPACITY)
  bool accounting = true;             // count algorithmic bytes (bbx_accounting)
  bool policy_greedy = false;         // the policy calls on this handle take the argmax instead of drawing (bbx_policy_greedy)
  int episode_limit = 0;              // the episode step limit of every launch on this handle (bbx_episode_limit; 0: off)
};

struct bbx_batch : bbx_config {
  uint16_t* d_inv = nullptr;           // GF(32003) inverse table: one per device and process (bbx_host::inv_table), never freed
  std::vector<std::unique_ptr<bbx::IdealGen>> gens;   // one per environment (one shared when fixed)
  std::vector<uint32_t> h_q;          // host mirror of the ideal queue
  std::vector<int32_t> h_tail, h_head;
  std::vector<BbxHdr> h_hdr;
  std::vector<BbxLite> h_lite;        // the status block (bbx_common.h) as the last launch left it: take_lite
  bool q_dirty = true;
  std::vector<uint8_t> q_dirty_env;
  // ideals drawn on the device (binomial distributions): the table the kernels read, the per-environment engine state
  // lives in the record headers (BbxHdr.gen_rng); the host-side generators and the ideal queue are then unused
  uint32_t* d_gen = nullptr; size_t gen_words = 0; bool device_gen = false;
  std::shared_ptr<uint32_t> gen_owner;   // the table is immutable: copies of a handle share it (d_gen == gen_owner.get())
  std::vector<std::string> gen_error;   // per environment: a generator failure met while drawing ahead (see fill_queues)
  // device
  char* d_recs = nullptr;
  uint32_t* d_q = nullptr;
  int32_t* d_tail = nullptr;
  // one device block polled after every launch (bbx_out_layout, bbx_common.h: status block | rewards | rows | dones); the
  // kernels write it themselves, the host fetches it with ONE copy into pinned memory
  char* d_out = nullptr; int32_t* d_lite = nullptr; double* d_rewards = nullptr; int32_t* d_rows = nullptr; uint8_t* d_dones = nullptr;
  char* h_io = nullptr; size_t io_bytes = 0;      // pinned mirror of d_out
  int32_t* h_act = nullptr;                       // pinned staging of host actions
  // small batches (the single-environment drop-in): the kernels read the actions from and write their outputs and the
  // observation straight into pinned host memory — no copy calls on the latency path, one stream synchronisation per step
  // (whether the outputs of the call in flight are in the pinned block is a property of that call: outputs_pinned())
  bool zero_copy = false;
  int poll_seq = 0, poll_misses = 0; unsigned polled_launches = 0;   // completion through h_io (done_seq): bbx_flight::poll
  char* zc_io_dev = nullptr; int32_t* zc_act_dev = nullptr;     // device-side addresses of h_io / h_act
  int32_t* h_zobs = nullptr; int32_t* zc_obs_dev = nullptr; size_t zobs_rows_cap = 0;
  // ragged observations (bbx_step_obs): device offsets [B+1] + packed rows, and their pinned mirror handed to the caller
  int32_t* d_obs_off = nullptr; int32_t* d_obs_packed = nullptr; int32_t* h_obs = nullptr; size_t obs_packed_cap = 0;
  uint32_t* h_stage = nullptr; uint32_t* d_stage = nullptr; size_t stage_words = 0;   // queue refill staging (pinned / device)
  int32_t* d_actions = nullptr; uint8_t* d_mask = nullptr; uint32_t* d_seeds = nullptr;
  int32_t* d_obs = nullptr; size_t obs_rows_cap = 0;
  BbxTraceRec* d_trace = nullptr; int trace_cap = 0;
  BbxHdr* d_hdr = nullptr;            // compact header copy (bbx_gather_hdr_kernel)
  // clone scratch of value() and bbx_action_values, [vcap] each (value_scratch_free): cloned records, the clone kernel's flags
  // for the re-sort (u8), source indices, agent seeds; [1 + vcap] results: the "did not finish" word pair, then a value per clone
  char* d_vrecs = nullptr; uint8_t* d_vflags = nullptr; int32_t* d_vsrc = nullptr; uint32_t* d_vseeds = nullptr; double* d_vvals = nullptr;
  int vcap = 0;
  // bbx_values_device: the ring (depth read from BBX_VALUE_RING when the handle is made), the stream its rollouts run on,
  // the identity source indices, a word pair per queued call, and the calls queued since the last wait
  int v_depth = bbx_value_ring_from_env();
  std::vector<bbx_vslot> v_ring; BbxLayout v_L{};
  hipStream_t v_stream = nullptr;
  int32_t* d_vident = nullptr; uint32_t* d_vwords = nullptr;
  std::vector<bbx_vjob> v_jobs;
  long long v_calls = 0;              // calls so far (slot = v_calls % v_depth)
  bbx_avscratch av;                   // bbx_action_values
  // HIP-event timing of the step-kernel launches (bbx_timing)
  bool timing = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_open;
  double kernel_ms = 0.0; int kernel_launches = 0;
  std::vector<char> h_out;
  bbx_flight flight;                  // the call in flight (so bbx_sync can finish environments that waited for ideals)
  bbx_flight cap; bool cap_valid = false;   // the last call recorded into a HIP graph (bbx_graph_replayed)
  bool cap_stale = false; std::vector<void*> retired;   // the records were enlarged after the recording: the old arrays stay allocated (replays write there)
  int32_t* d_wide_done = nullptr;     // wide class: workgroups that have left the launch's first kernel (BbxParams::wide_tail)
  // persistent sessions (bbx_persistent): see BbxParams::ctl
  bool ps_enabled = false, ps_active = false;
  // host mailbox sessions (BbxParams::mbox): host-driven steps of small zero-copy batches on the register/LDS-resident class
  bool ps_mbox = false;                 // the session in progress is one
  unsigned long long* h_mbox = nullptr; // its control word, in pinned host memory, and the device's address of it
  unsigned long long* mbox_dev = nullptr;
  unsigned long long api_epoch = 0, mbox_epoch = ~0ull;   // launches / waits on the handle so far; the count as the last host step left it
  int mbox_streak = 0;                  // host steps in a row with nothing else on the handle in between (a loop: worth a session)
  int mbox_misses = 0;                  // steps whose result did not arrive through the mailbox in time (three in a row: no more mailbox sessions)
  unsigned long long* d_ctl = nullptr;
  hipStream_t ps_stream = nullptr, ps_ctl_stream = nullptr;   // the session's kernel / the writes to its control word
  hipEvent_t ps_ev = nullptr;
  long long ps_target = 0;            // steps issued since the session began
  std::deque<std::pair<double, long long>> ps_recent;   // (host time in ms, steps) of the latest calls: how much may still be owed when the session closes
  BbxParams ps_p{};                   // the parameters of the call that began it (later calls must match to join)
  BbxPolicy ps_pol{};                 // ... and its policy arguments (ps_p.policy points here), when it is a session of policy steps
  int ps_sessions = 0, ps_joined = 0, ps_kernels = 0; // statistics: sessions begun, calls that joined a running one, kernels
  int32_t* d_clone_idx = nullptr; int clone_cap = 0;   // bbx_clone_envs: source / destination indices on the device
  std::mt19937_64 value_rng;          // seeds of value("random") / value("sample") rollouts when the caller gives none
  int grow_events = 0;                // times the records were enlarged (bbx_capacities)
  bool steps_uncounted = false;       // a headline-shaped kernel has run since the limit was last set: BbxHdr.episode_steps is out of date
  long long step_kernels = 0;         // kernels enqueue() has launched for this handle (bbx_kernels_launched: what a call costs in launches)
  bbx_batch() = default;
  bbx_batch(const bbx_batch&) = delete;
  bbx_batch& operator=(const bbx_batch&) = delete;
  ~bbx_batch();                       // frees every device / pinned allocation (also on half-built handles)
};


namespace bbx_host {
// wait for the launch in flight, serve environments that need the host (queued ideals, larger records, the kernels of a
// session), surface errors; the handle is left with nothing in flight
int finish(bbx_batch* b, hipStream_t stream);
int settle(bbx_batch* b);            // finish() whatever is in flight (the entry of every call that needs the batch quiet)
int quiesce(bbx_batch* b);           // the read-only introspection calls: close a session and wait, WITHOUT finishing
// the outputs and status words of the call in flight are in the pinned block (zero-copy host steps, a mailbox session)
inline bool outputs_pinned(const bbx_batch* b) { return b->zero_copy && b->flight.p.lite == (int32_t*)b->zc_io_dev; }
// The status block in pinned memory (bbx_common.h BbxLite), as the host watches it while a kernel may still be writing
inline volatile BbxLite* pinned_lite(const bbx_batch* b) { return (volatile BbxLite*)b->h_io; }
// Its status words against sequence number `want`: all — every one carries it; trouble — one that carries it reports a
// status other than OK, or one of the bits `flags`.
struct SeqScan { bool all, trouble; };
inline SeqScan scan_seq(const bbx_batch* b, int want, int32_t flags) {
  const volatile BbxLite* w = pinned_lite(b);
  SeqScan s{true, false};
  for (int e = 0; e < b->B; e++) {
    const int32_t v = w[e].word0;
    if (bbx_lite_seq(v) != want) s.all = false;
    else if (bbx_lite_status(v) != BBX_ST_OK || (v & flags)) s.trouble = true;
  }
  return s;
}
// the words the host is going to watch start out cleared (no step has sequence number 0)
inline void clear_pinned_seq(const bbx_batch* b) { for (int e = 0; e < b->B; e++) pinned_lite(b)[e].word0 = 0; }
inline bool traced(const bbx_batch* b) { return b->d_trace && b->trace_cap >= 1; }
// the register/LDS-resident class, lean and untraced: what sessions, mailboxes and the fused policy step run on
inline bool lean_fast(const bbx_batch* b) { return b->cls == BbxClass::FAST && !b->accounting && !traced(b); }
// The kernels of one launch (plan_launch): kind[i] with parameters pass[i], waves[i] environments per workgroup (wide: waves per environment)
struct LaunchPlan {
  int n = 0;
  BbxKernel kind[3];
  int waves[3];
  BbxParams pass[3];
  bool wide_tail = false;             // the last kernel is the tail of a two-kernel wide launch (BbxParams::wide_tail)
  bool poll = false;                  // bbx_flight::poll
};
LaunchPlan plan_launch(const bbx_batch* b, const BbxParams& p0, bool resume, bool value);
int read_headers(bbx_batch* b, hipStream_t stream = 0);
void fill_params(bbx_batch* b, BbxParams* p);
int grow_records(bbx_batch* b, unsigned need, int env, hipStream_t stream);
const char* status_name(int s);
// bbx_api.cpp
void take_lite(bbx_batch* b);         // the pinned block's status records -> h_lite, the queue heads they report -> h_head
int fill_queues(bbx_batch* b, int min_avail = 1, hipStream_t stream = 0);
int enqueue(bbx_batch* b, const BbxParams& p0, bool resume, hipStream_t stream);   // the kernels of one logical launch
int step_device(bbx_batch* b, const int32_t* d_actions, double* d_rewards, uint8_t* d_dones, int32_t* d_rows, int32_t* d_obs, int obs_rows,
                int obs_fill, void* stream, int auto_reset);   // bbx_step_device[_autoreset]
// bbx_api_value.cpp: the calls bbx_values_device queued — value_wait: the host waits for their device work (before anything
// moves or frees records); value_resolve: after that, read their words, carry waiting clones over to enlarged records,
// report; value_ring_free, value_scratch_free: the ring's memory, the clone scratch (the device must be idle)
int value_wait(bbx_batch* b);
int value_resolve(bbx_batch* b);
void value_ring_free(bbx_batch* b);
void value_scratch_free(bbx_batch* b);
void action_values_free(bbx_batch* b);   // what bbx_action_values keeps between calls (the device must be idle)
// bbx_api_session.cpp
int launch(bbx_batch* b, BbxParams& p, hipStream_t stream, bool obs_external = false, bool device_async = false);
void start_flight(bbx_batch* b, const BbxParams& p, hipStream_t stream, bool obs_external, bool device_async);
void continue_session(bbx_batch* b);
int ensure_session_streams(bbx_batch* b);
int ps_write_ctl(bbx_batch* b, bool stop);
int ps_behind_ctl(bbx_batch* b);                                         // the session stream waits for the control word's last write
int session_kernel(bbx_batch* b, bool first, hipStream_t after, bool sliced, bool behind_after = false);   // behind_after: ordered behind what `after` (possibly the NULL stream) holds
int session_close(bbx_batch* b, bool wait, hipStream_t then, bool sliced);
bool session_same_call(const BbxParams& a, const BbxParams& c);
bool mbox_eligible(const bbx_batch* b);
int mbox_step(bbx_batch* b, BbxParams& p, bool* used);
}  // namespace bbx_host

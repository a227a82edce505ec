// Shared between the host side of libbbx (bbx_api.cpp) and the HIP kernels (bbx_*.hip, bbx_device.h).
//
// HBM layout
// ----------
// A batch is B independent Buchberger environments.  Each environment owns one
// contiguous *record* in HBM (rec_bytes, 256-B aligned) holding everything the
// step path touches; records never reference each other, so a batch shards
// across wavefronts / GPUs with no exchange.  Inside a record every array is
// 16-B aligned so monomials can be moved with 8-/16-byte loads:
//
//   hdr     BbxHdr                      counters, sizes, status
//   lm      Mono[maxG]                  lead monomial of G[i]      (G order; pair criteria, lcm)
//   slm     Mono[maxG]                  lead monomials in REDUCER order (ascending grevlex; the
//                                       first-divisor scan reads this coalesced, lane k <- slm[k])
//   lcm     Mono[maxG]                  scratch: lcm(LM G[i], LM f) during the Gebauer-Moeller update
//   am      Mono[arena]                 term arena: monomials of all basis polynomials, append-only
//   hm      Mono[5*maxT]                scratch polynomials: h ping/pong, r, merge staging (2*maxT)
//   poff    u32[maxG]                   arena offset of G[i]
//   pairs   u32[maxP]                   pair set P in reference order, i | j<<16
//   sidx    u16[maxG]                   reducer r -> index into G
//   plen    u16[maxG]                   #terms of G[i]       psug u16[maxG] sugar   pinv u16[maxG] 1/LC
//   ac      u16[arena]                  arena coefficients   hc u16[5*maxT] scratch coefficients
//   cp      u8[maxG]                    scratch: G[i] coprime to f
//
// Mono is W 32-bit words of packed u16 pairs (v_pk_max_u16 / v_pk_add_u16 / v_pk_sub_u16 clamp
// operate on it directly): slot s (= variable s) lives in word s/2, half s%2; the LAST slot holds
// the total degree.  W=2 serves n<=3 variables (8 B / monomial), W=4 serves n<=7 (16 B).
#pragma once
#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#define BBX_P 32003u
#define BBX_POLICY_MAX_ROWS 2048    /* rows (pairs) per environment the policy kernels score: their logits live in LDS */
#define BBX_MAXVARS 8
#ifdef __HIPCC__                    /* functions the host side and the kernels share */
#define BBX_HD __host__ __device__
#else
#define BBX_HD
#endif

// per-environment status (sticky except STARVED)
enum {
  BBX_ST_OK = 0,
  BBX_ST_G_FULL = 1,        // basis capacity exceeded
  BBX_ST_P_FULL = 2,        // pair capacity exceeded
  BBX_ST_ARENA_FULL = 3,    // term arena exhausted
  BBX_ST_POLY_TOO_LONG = 4, // an intermediate polynomial exceeded maxT terms
  BBX_ST_DEG_OVERFLOW = 5,  // total degree above 65535
  BBX_ST_STARVED = 6,       // ideal queue empty: the environment waits for the host to refill
  BBX_ST_BAD_ACTION = 7,    // action index outside [0, |P|)
  BBX_ST_RUNAWAY = 9,       // a reduction exceeded 2^24 rounds (corrupt state guard; never seen in practice)
  BBX_ST_GEN_FAIL = 10,     // the ideal generator failed (no two distinct monomials after 1000 trials: the reference throws)
  BBX_ST_GEN_ZERO = 11,     // a random polynomial cancelled to zero (undefined in the reference)
  BBX_ST_POLY_LIMIT = 12,   // a basis element would have more than 65535 terms (plen[] is 16 bits): a hard limit
  BBX_ST_TIMESLICE = 14,    // transient: a kernel of a persistent session ended its time slice with steps still owed (a kernel
                            // that runs longer than ~100 ms is clocked down to half speed; sessions run in slices of 10 ms:
                            // PS_SLICE_TICKS, bbx_api_session.cpp)
  BBX_ST_SPILL = 8,         // transient: the state outgrew the LDS-resident class; the HBM-resident pass of the
                            // same launch sequence continues this environment
};

// Capacity statuses are not failures: the kernels leave the record consistent (the step that did not fit has not been
// started: nothing persistent is modified before its last capacity check), the host enlarges the record layout
// (bbx_api.cpp grow_records) and the environment continues.  A launch that finds an environment waiting like that adds
// its steps to the environment's budget instead of replacing it, so no step is lost across asynchronous launches.
static inline BBX_HD int bbx_st_capacity(int st) { return st == BBX_ST_G_FULL || st == BBX_ST_P_FULL || st == BBX_ST_ARENA_FULL || st == BBX_ST_POLY_TOO_LONG; }
// the same set as bits of a word of `1 << status` (the "did not finish" word of the value calls, bbx_api_value.cpp)
#define BBX_ST_CAPACITY_BITS ((1u << BBX_ST_G_FULL) | (1u << BBX_ST_P_FULL) | (1u << BBX_ST_ARENA_FULL) | (1u << BBX_ST_POLY_TOO_LONG))
// Transient statuses say "steps are still owed, somebody else (the host's refill, the follow-up pass, the session's next
// kernel) has to act first": every step kernel clears them on entry and tries again.
static inline BBX_HD int bbx_st_transient(int st) { return st == BBX_ST_STARVED || st == BBX_ST_SPILL || st == BBX_ST_TIMESLICE; }
// A follow-up pass (BbxParams::pass == 1) serves an environment only when it has something to do: a pending reset or owed steps
static inline BBX_HD bool bbx_pass_has_work(int st, int need_reset, int budget, int nP) { return st == BBX_ST_OK && (need_reset || (budget > 0 && nP > 0)); }
// The `dones` output: the last step taken ended an episode, or the episode is over and no reset is pending (a finished
// environment stepped without auto-reset stays done)
static inline BBX_HD int bbx_done_flag(int done_last, int nP, int need_reset) { return (done_last || (nP == 0 && !need_reset)) ? 1 : 0; }
// The episode step limit (bbx_episode_limit; 0: off), stated once for every step kernel and the host.  How the step that has
// just been accounted ends its episode — nP, episode_steps: the state and the episode's step count AFTER it:
//   1  the pair set is empty: an ordinary end (also when this was the limit-th step)
//   2  pairs are left and the episode has its `limit` steps: it is CUT
//   0  the episode goes on
// Wherever a kernel says `done` (dones, done_last, the trace record, the mailbox publication, need_reset under auto-reset, the
// hand-back to a session) it means end != 0; the bytes it writes stay 0 / 1.
static inline BBX_HD int bbx_episode_end(int nP, int episode_steps, int limit) { return nP == 0 ? 1 : ((limit > 0 && episode_steps >= limit) ? 2 : 0); }
// ... and whether that end moves the counters (BbxHdr.episodes, and BbxHdr.truncations when it is a cut).  Without auto-reset a
// cut environment is left as it is: further steps are taken and each reports done, but only the limit-th one counted.
static inline BBX_HD bool bbx_episode_counted(int end, int episode_steps, int limit, int auto_reset) {
  return end == 1 || (end == 2 && (auto_reset || episode_steps == limit));
}
// The fast class (bbx_fast.h) counts no steps of an episode: it keeps t_ep0, the agent step count at which the running episode
// began (episode_steps = t_agent - t_ep0, formed where it is wanted), and tests one event per step, t_agent == t_lim: the agent
// step count at which the episode is cut.  t_lim as of agent step count t_agent (kernel entry, behind a reset, behind a cut
// that no reset follows): the episode's limit-th step, or the very next one where it already has them (a limit lowered under a
// running episode; an environment stepped on without auto-reset) — t_agent + max(limit - episode_steps, 1).  Limit off: a
// count t_agent, which only goes up, does not reach.
static inline BBX_HD int bbx_episode_tlim(int t_ep0, int t_agent, int limit) {
  if (limit <= 0) return (int)((uint32_t)t_agent - 1u);
  const int left = limit - (int)((uint32_t)t_agent - (uint32_t)t_ep0);
  return (int)((uint32_t)t_agent + (uint32_t)(left > 1 ? left : 1));
}

// The user priority (s_setprio, 0..3) of a wave of the register/LDS-resident step kernels (fast_body, bbx_fast.h): a slot of
// 2^BBX_PRIO_TICK_SHIFT ticks of the 100 MHz clock every wave reads alike (its low 32 bits: 2^32 is a whole number of cycles of
// four slots, the wrap is no seam), offset by the wave's rank among those it shares a SIMD with.  At any tick the four ranks
// hold the four priorities, and over a cycle of four slots every rank holds each priority for one slot
// (tests/prio_phase_check.cpp).  The slot length is held between two demands that pull apart: several looks long (a wave looks
// every 64 steps, ~10.5 k ticks — until its next look it keeps the last slot's priority, which another wave may hold by then)
// and short enough that a launch of 1024 steps (~200 k ticks) holds a whole cycle.  Measured (profiles/r17_bench_ab.txt, plain
// bench.py against the rotation keyed on steps): shift 13 -1.9 %, 14 -0.1 %, 15 +1.5 %.
#ifndef BBX_PRIO_TICK_SHIFT
#define BBX_PRIO_TICK_SHIFT 15
#endif
static_assert(BBX_PRIO_TICK_SHIFT >= 0 && BBX_PRIO_TICK_SHIFT <= 30, "2^32 ticks must hold a whole number of cycles of four slots");
static inline BBX_HD int bbx_prio_phase(uint32_t ticks, int rank) { return (int)(((ticks >> BBX_PRIO_TICK_SHIFT) + (uint32_t)rank) & 3u); }

// The status block ("lite"): what every step kernel leaves per environment and the host reads after every launch.
//   word0   bits 0..15 the status (BBX_ST_*), bit 16 BBX_LITE_OBS_TRUNC (BbxHdr.obs_trunc != 0), bits 17.. a sequence number
//   budget  the steps still owed; BBX_LITE_GONE on top of it once a mailbox session's wave has left
// No sequence number (the host waits through the runtime): ONE 16-byte store.  With one (BbxParams::done_seq, mailbox sessions:
// the block is pinned host memory the host spins on) word0 goes LAST: the other three words and every output (rewards, dones,
// rows, observation) as plain stores, __threadfence_system(), then word0 as a system-scope release store.  Step or launch n
// carries bbx_lite_seq_of(n): never 0, which is what the host clears the words to before it watches them.
// The gone mark says "this wave has stored its environment and left": what the host waits for when it closes a mailbox session,
// instead of the runtime's completion signal.  A release store of its own, the wave's last, behind word0: the host, seeing it,
// may begin the next session at once, and a word0 arriving behind the mark carried this session's last sequence number into
// the next one (whose first step then returned the OLD step's outputs: found by scripts/fuzz_gym.py, round 4).
struct BbxLite { int32_t word0, q_head, budget, nP; };
static_assert(sizeof(BbxLite) == 16, "the kernels store a BbxLite as one int4");
#define BBX_LITE_STATUS_MASK 0xffff
#define BBX_LITE_OBS_TRUNC 0x10000
#define BBX_LITE_SEQ_SHIFT 17
#define BBX_LITE_SEQ_MOD 16000       /* sequence numbers are 1..16000: (16000 + 1) << 17 must stay below 2^31 (a round number under 16383) */
#define BBX_LITE_GONE 0x40000000     /* on the budget word */
#define BBX_LITE_BUDGET_BOUND (1 << 30)   /* a session issues fewer steps than this in all (launch_kind, mbox_step) */
static_assert(((long long)(BBX_LITE_SEQ_MOD + 1) << BBX_LITE_SEQ_SHIFT) <= 0x7fffffffll, "word0 stays a positive int32_t");
static_assert(BBX_LITE_GONE >= BBX_LITE_BUDGET_BOUND && BBX_LITE_GONE > 0, "the gone mark lies above every session budget");
static inline BBX_HD int32_t bbx_lite_word0(int status, int trunc, int seq) { return status | (trunc ? BBX_LITE_OBS_TRUNC : 0) | (seq << BBX_LITE_SEQ_SHIFT); }
static inline BBX_HD int bbx_lite_status(int32_t w) { return w & BBX_LITE_STATUS_MASK; }
static inline BBX_HD int bbx_lite_seq(int32_t w) { return (int)((uint32_t)w >> BBX_LITE_SEQ_SHIFT); }
static inline BBX_HD int bbx_lite_seq_of(int n) { return (n % BBX_LITE_SEQ_MOD) + 1; }   // n >= 0

// The host API's output block, on the device and in its pinned mirror: BbxLite[B] | rewards f64[B] | rows i32[B] | dones u8[B]
// (16 | 8 | 4 | 1 bytes per environment: every array aligned to its element for any B); byte offsets and the total
struct BbxOutLayout { size_t lite, rewards, rows, dones, bytes; };
static inline BBX_HD BbxOutLayout bbx_out_layout(size_t B) {
  const size_t rw = B * sizeof(BbxLite), ro = rw + B * sizeof(double), dn = ro + B * sizeof(int32_t);
  return {0, rw, ro, dn, dn + B};
}

struct BbxHdr {             // 128 bytes
  int32_t nG, nP, arena_used, status;
  int32_t need_reset, q_head, t, episode_steps;
  int64_t total_steps, total_additions;
  int32_t episodes, zero_reductions;
  uint32_t agent_seed;
  int32_t steps_done;       // steps completed in the last launch
  int32_t budget;           // steps still owed in the current rollout (survives queue starvation)
  int32_t rollout_pos;      // steps completed in the current rollout (trace slot)
  int32_t done_last;        // the last executed step ended an episode
  uint32_t std_rng;         // state of the minstd_rand0 engine behind the reference's seeded Random selection (buchberger.cpp:200-206)
  int64_t alg_bytes;        // algorithmic bytes moved so far (SURVEY.md 8d formula), for the roofline figure
  double vret, vdisc;       // value() rollouts: discounted return so far and the current discount (buchberger.cpp:248-252)
  uint32_t gen_rng;         // state of this environment's ideal generator engine (minstd_rand0) when ideals are drawn
                            // on the device (BbxParams.gen != null); the host-side generators then stay unused
  int32_t obs_trunc;        // != 0: during the current rollout an observation had more rows than the caller's block holds
                            // (rows beyond obs_rows were not written); reported by bbx_sync as BBX_E_CAPACITY
  int32_t sess_done;        // persistent sessions (bbx_persistent): steps of the session's total this environment has taken
  int32_t truncations;      // episodes cut by the episode step limit (bbx_episode_end == 2), counted like `episodes`
  int32_t reserved[2];
};
static_assert(sizeof(BbxHdr) == 128, "BbxHdr: the record arrays start at byte 128");

struct BbxLayout {
  uint32_t W;               // words per monomial (2 or 4)
  uint32_t maxG, maxP, arena, maxT;
  uint32_t off_lm, off_slm, off_lcm, off_am, off_hm, off_poff, off_pairs;
  uint32_t off_sidx, off_plen, off_psug, off_pinv, off_ac, off_hc, off_cp;
  uint32_t rec_bytes;
  // binomial class (kind == 1): every basis polynomial has <= 2 terms, so there is no arena; the
  // record holds, in BASIS order, lm[] / tm[] (lead and tail monomial) and ginfo[] = {lc | tc<<16,
  // 1/lc | sugar<<16}, and in REDUCER order slm[] / stm[] and sinfo[] = {tc | (-tc/lc mod p)<<16, sugar | g<<16},
  // so that one reduction round needs the scan of slm[] plus two independent loads.  tc == 0: no tail.
  uint32_t kind;
  uint32_t off_tm, off_stm, off_ginfo, off_sinfo;
};

// Ideal queue: per environment a ring of `nslots` ideals (or ONE shared slot when fixed != 0).
// Slot words: [npolys, then per polynomial: nterms, sugar, then nterms x (coef, mono W words)].
struct BbxQueue {
  const uint32_t* words;
  uint32_t env_stride;      // words per environment (0 when fixed)
  uint32_t slot_words;
  uint32_t nslots;
  uint32_t fixed;
  uint32_t no_redraw;       // ideal lists (bbx_create_ideals): an ideal whose pair set starts empty IS the episode (buchberger() of it
                            // returns at once, make_strat.cpp:62-66); BuchbergerEnv::reset would draw another (buchberger.cpp:313-314)
  const int32_t* tail;      // [B] ideals produced so far per environment (host-written)
};

struct BbxTraceRec {        // one per environment per step when tracing (tests / parity)
  int32_t action, nP, nG, done;
  double reward;
  uint64_t obs_hash, pairs_hash, newpoly_hash;
};

enum { BBX_AGENT_EXTERNAL = 0, BBX_AGENT_HASH = 1, BBX_AGENT_DEGREE = 2, BBX_AGENT_FIRST = 3, BBX_AGENT_NORMAL = 4, BBX_AGENT_SUGAR = 5,
       // the reversed orders of buchberger.cpp:207-240 and the seeded std::default_random_engine choice of :200-206,244
       BBX_AGENT_LAST = 6, BBX_AGENT_CODEGREE = 7, BBX_AGENT_STRANGE = 8, BBX_AGENT_SPICE = 9, BBX_AGENT_STDRANDOM = 10 };
enum { BBX_ELIM_GM = 0, BBX_ELIM_LCM = 1, BBX_ELIM_NONE = 2 };
enum { BBX_REW_ADDITIONS = 0, BBX_REW_REDUCTIONS = 1 };

// one-hidden-layer PMLP policy (networks.py:49-95, 414-460) for the policy + step launch: device pointers
struct BbxPolicy {
  const float* wp; int32_t hidden;     // prepared weights (bbx_pmlp_prepare) of a [cols] -> [hidden] -> 1 network
  // != 0: the kernels take the row of the largest logit (the first on ties) instead of drawing; u is not read and may be null
  // (bbx_policy_greedy).  By value, like everything here: a recorded graph keeps the mode it was captured with.  (In the four
  // bytes between `hidden` and the next pointer: the struct, and with it the kernels' argument block, is as large as it was)
  int32_t greedy;
  const float* u;                      // [B] uniforms in [0, 1) for the inverse-CDF draw
  int32_t* actions; float* logprobs;   // [B] outputs: the sampled row and its log-probability
  // policy ROLLOUT (nsteps > 1 inside one launch): the arrays above are [nsteps][B] and so are these; the observation
  // the policy saw at step t goes to obs + t * obs_tstride (0: one block, overwritten every step)
  int32_t rollout;                     // 0: per-step call; 1: rollout, register/LDS-resident kernel first; 2: rollout, HBM-resident kernel only
  double* rewards_t; uint8_t* dones_t; int32_t* rows_t; long long obs_tstride;
  // calls of bbx_policy_step_device served by a persistent session: u is [steps][B] (call t reads slice t), every other
  // array is the [B] array of the calls, rewritten at each step (stride_out = 0), and the observation block and row
  // counts describe the state AFTER the step, as that call leaves them (post_obs = 1).  Rollouts: stride_out = B, post_obs = 0.
  int32_t stride_out, post_obs;
  // 0: the network above.  > 0: two hidden layers (bbx_policy2_rollout_device, networks.py:562-571) of `hidden` and `hidden2`
  // units, wp as bbx_pmlp2_prepare leaves it; rollouts only
  int32_t hidden2;
};
// workgroup of the register/LDS-resident kernel of a two-layer policy rollout: 16 waves, one workgroup per CU, sharing one
// LDS copy of the layers behind the first (fast_body POL2, bbx_fast.h)
enum { BBX_POL2_WAVES = 16 };
struct BbxParams {
  char* recs;
  BbxLayout L;              // layout of the records in HBM
  BbxLayout LL;             // layout of the LDS-resident working copy (staged kernel only)
  int32_t fast_G, fast_P;   // capacities of the register/LDS-resident class (bbx_fast.h; its kernels clamp them to what they hold)
  BbxQueue q;
  int32_t B;
  int32_t nsteps;
  int32_t set_budget;       // 1: start a rollout of nsteps steps; 0: continue the one in progress
  int32_t agent;
  int32_t auto_reset;
  int32_t elim, rewards_mode, sort_reducers, k, nvars;
  const struct BbxPolicy* policy;   // HOST pointer or null: a PMLP policy evaluated inside the step kernel (fast class only)
  int32_t sort_input;       // device-drawn ideals: the generators of a new ideal enter in ascending lead-monomial order
                            // (BuchbergerEnv::reset, buchberger.cpp:299-303; at most 16 generators: see gen_sorted_rank)
  const int32_t* actions;   // [B], agent == EXTERNAL
  double* rewards;          // [B] reward of the last executed step
  uint8_t* dones;           // [B]
  int32_t* rows;            // [B] |P| after the step
  int32_t* obs;             // [B, obs_rows, 2*n*k] int32 or null
  int32_t obs_rows;         // row capacity per environment in obs
  int32_t obs_fill;         // 1: pad rows [nP, obs_rows) with -1
  int32_t obs_every_step;   // 1: materialise the observation after every step (what a policy consumes),
                            // 0: only for the state the caller sees when the launch ends
  int32_t value_mode;       // 1: accumulate the discounted return of the rollout (value(), buchberger.cpp:332-351)
  double gamma;
  double* values;           // [B] discounted return when value_mode
  int32_t accounting;       // 1: count algorithmic bytes per step (BbxHdr.alg_bytes); the lean fast kernel omits it
  int32_t pass;             // 0: primary launch; 1: follow-up launch serving only environments with work left
  const uint16_t* inv_table; // [32003] inverses in GF(32003) (L2-resident), binomial class
  const uint32_t* gen;      // device-side generator table (BBX_GEN_* layout below) or null: ideals come from the queue
  int32_t* lite;            // BbxLite[B] (above), as words: what the host polls after a launch, or null
  int32_t done_seq;         // != 0: lite lives in host memory and the host spins on it — word0 carries this sequence number
  BbxTraceRec* trace;       // [B, trace_stride] or null
  int32_t trace_stride;
  // persistent sessions (bbx_persistent; register/LDS-resident class): asynchronous rollouts queued behind each other do not
  // become one kernel each — the first starts a kernel whose waves keep their environments, and every further call only
  // raises the step total in a device-visible control word the waves look at when they have taken all steps issued so far
  const unsigned long long* ctl;   // control word {bits 0..31: steps issued since the session began, bit 32: stop} or null
  unsigned long long* ctl_stats;   // statistics: steps the closing launches had to take (null: not counted)
  int32_t sess_target;      // != 0: every environment owes sess_target - BbxHdr.sess_done steps (later slices of a session, and
                            // the launch of the HBM-resident class behind them)
  int32_t spill_terms;      // general class, != 0: a merge of more than this many terms hands the environment (untouched: the
                            // step is restartable) to the wide class — one workgroup per environment — launched right behind
  uint32_t slice_ticks;     // persistent kernels: leave after this many ticks of the 100 MHz clock (0: no limit)
  int32_t mbox;             // persistent kernels, != 0: a host MAILBOX session — the control word and the action buffer live in
                            // pinned host memory and are written by the host itself (no launch per step), and every step publishes
                            // its outputs (rewards / dones / rows / observation block, then the status word with the step's
                            // sequence number) to the pinned block the host spins on: bbx_step / bbx_step_obs of small batches
  int32_t wide_hc, wide_fc, wide_rc, wide_sc;   // wide class: LDS capacities (terms) of the polynomial being reduced, the
                                       // reducer-tail window, the reducer table and the accumulator; wide_hc == 0: chosen by the launcher
  // wide class, batches of more than one workgroup per CU: the launch is two kernels.  The first (wide_tail == 1, two
  // workgroups per CU, 128 registers) counts the workgroups that have left in *wide_done; once those still at work would fit
  // one per CU (wide_ncu) each of them stops at its next step boundary (BBX_ST_TIMESLICE, budget kept), and the second
  // (wide_tail == 2: the variant without the register cap, 160 KB of LDS) takes what they owe — a rollout of T steps per
  // environment ends with its slowest environments, and those then run at the speed of a workgroup that has a CU to itself
  int32_t wide_tail, wide_ncu;
  int32_t* wide_done;
  int32_t episode_limit;    // the episode step limit (bbx_episode_end above; 0: off).  By value: a recorded graph keeps the limit
                            // it was captured with.  The clone pipelines of the value calls run with 0
};
// The launch shape bbx_fast_headline[_persistent]_kernel are specialised for (bbx_fast.hip picks them by this; a session's
// launches, p.ctl, are lean and untraced by admission).  They know no episode limit and do not keep BbxHdr.episode_steps.
static inline BBX_HD bool bbx_headline_shape(const BbxParams& p) {
  return !p.policy && !p.value_mode && (p.ctl || (!p.trace && !p.accounting)) && p.agent == BBX_AGENT_HASH && p.nvars == 3 && p.k == 2 &&
         p.obs && p.obs_every_step && !p.obs_fill && p.auto_reset && p.episode_limit == 0;
}
// ... and every launch of the register/LDS-resident class whose kernel leaves BbxHdr.episode_steps alone: those, and the two-layer
// policy rollout launched without a limit (bbx_fast.h, NOLIM).  The host notes them (bbx_batch::steps_uncounted)
static inline BBX_HD bool bbx_fast_keeps_no_count(const BbxParams& p) {
  return bbx_headline_shape(p) || (p.policy && p.policy->rollout && p.policy->hidden2 > 0 && p.episode_limit == 0);
}

// The step kernels a launch is made of (bbx_launch_step): HBM-resident, LDS-staged, aux (reset / observation only), the
// hand-tuned register/LDS-resident kernel (bbx_fast.h), wide (one workgroup per environment, bbx_wide.h)
enum BbxKernel { BBX_K_HBM = 0, BBX_K_STAGED = 1, BBX_K_AUX = 2, BBX_K_FAST = 3, BBX_K_WIDE = 4 };

// Device-side ideal generation (RandomBinomialIdealGenerator, ideals.cpp:156-201): one immutable table per batch, words:
//   [0] n  [1] d  [2] s  [3] flags (1 homogeneous, 2 pure, 4 polynomial distribution = RandomIdealGenerator, ideals.cpp:203-231)
//   [4] #cumulative probabilities (0: degree is always 0)  [5] W  [6..7] exp(-lambda) of the polynomial distribution (double)
//   [BBX_GEN_CP + 2 i]      cumulative probability i of the degree distribution (double, 64 entries, padded with +inf)
//   [BBX_GEN_DEG + 8 i]     per degree i: offset of its monomials (in monomials), their number, the two constants of
//                           libstdc++'s uniform_int_distribution(0, number - 1) — scaling, past — and floor(2^32 / scaling)
//   [BBX_GEN_JUMP + k]      16807^(k + 1) mod (2^31 - 1), k < BBX_GEN_BATCH: the engine's jump-ahead multipliers (lane-parallel draw)
//   [BBX_GEN_MONO + W j]    monomial j, packed (with degree slot), in the reference's enumeration order (ideals.cpp:39-64)
#define BBX_GEN_CP 8
#define BBX_GEN_DEG (BBX_GEN_CP + 128)
#define BBX_GEN_JUMP (BBX_GEN_DEG + 512)
#define BBX_GEN_BATCH 128
#define BBX_GEN_MONO (BBX_GEN_JUMP + BBX_GEN_BATCH)
#define BBX_GEN_MAXDEG 63

#ifdef __cplusplus
// ------------------------------------------------------------------ one generator of a binomial ideal from a batch of raws
// The lane-parallel draw of the fast class (gen_ideal_lanes, bbx_device.h) computes the engine's next BBX_GEN_BATCH outputs
// at once (x_k = 16807^k x_0 mod (2^31 - 1)) and lets lane f decode generator f from the raws a sequential draw WITHOUT
// rejections and retrials would have given it: bbx_gen_stride of them.  The decode is stated once, here, for the kernel and
// for the host check (tests/reset_draw_check.cpp): the operations of gen_binomial (bbx_device.h) / BinomialGen
// (bbx_ideals.cpp) in their order.  A generator whose sequential draw would have used another number of raws — a uniform draw
// at or past `past`, or two equal monomials — reports `deviated`; the caller then drops the whole batch and draws one by one.
// Acc supplies the data, each its own way (registers and cross-lane reads on the device, plain arrays on the host):
//   uint32_t raw(int i)         raw i of this generator's window          double cp(int i)          cumulative probability i
//   BbxGenRow row(int d)        the per-degree row of degree d            void mono(j, uint32_t w[2])   monomial j (W = 2)
static inline BBX_HD uint32_t bbx_gen_mulmod(uint32_t a, uint32_t x) {      // a x mod (2^31 - 1); a, x in [1, 2^31 - 1)
  const uint64_t pr = (uint64_t)a * x;
  uint32_t s = (uint32_t)(pr & 0x7fffffffu) + (uint32_t)(pr >> 31);        // 2^31 = 1 (mod 2^31 - 1); below 2 (2^31 - 1)
  if (s >= 2147483647u) s -= 2147483647u;
  return s;
}
// ret / scaling for ret < 2^31 with magic = floor(2^32 / scaling): the estimate is at most one too small
static inline BBX_HD uint32_t bbx_gen_div(uint32_t ret, uint32_t scaling, uint32_t magic) {
  uint32_t q = (uint32_t)(((uint64_t)ret * magic) >> 32);
  if (ret - q * scaling >= scaling) q++;
  return q;
}
static inline BBX_HD double bbx_gen_canonical(uint32_t r1, uint32_t r2) {   // random.tcc generate_canonical, k = 2
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double R = 2147483646.0;
  double sum = (double)(r1 - 1u);
  sum = sum + (double)(r2 - 1u) * R;
  double ret = sum / (R * R);
  if (ret >= 1.0) ret = 0x1.fffffffffffffp-1;                               // nextafter(1, 0)
  return ret;
}
static inline BBX_HD int bbx_gen_stride(uint32_t flags, int ncp) {          // raws of one generator: [c] [degrees] m1 m2
  return ((flags & 2u) ? 0 : 1) + (ncp == 0 ? 0 : ((flags & 1u) ? 2 : 4)) + 2;
}
#define BBX_GEN_BATCH_MAXPOLY 11                                            /* 11 generators x 7 raws <= BBX_GEN_BATCH */
struct BbxGenRow { uint32_t off, scaling, past, magic; };
struct BbxGenDraw { uint32_t lead[2], tail[2], c; bool deviated; };
template <class Acc>
static inline BBX_HD BbxGenDraw bbx_gen_decode(const Acc& acc, uint32_t flags, int ncp) {
  BbxGenDraw r;
  bool dev = false;
  int at = 0;
  // (a rejected draw decodes as 0: whatever follows is dropped with the batch, but stays inside the table)
  auto uniform = [&](uint32_t scaling, uint32_t past, uint32_t magic) {
    uint32_t ret = acc.raw(at++) - 1u;
    if (ret >= past) { dev = true; ret = 0; }
    return bbx_gen_div(ret, scaling, magic);
  };
  auto degree = [&]() {                                                     // std::lower_bound(cp, cp + ncp, pr) - cp
    const uint32_t r1 = acc.raw(at), r2 = acc.raw(at + 1);
    at += 2;
    const double pr = bbx_gen_canonical(r1, r2);
    int d = 0;
    for (int i = 0; i < ncp; i++) d += acc.cp(i) < pr ? 1 : 0;
    return d;
  };
  r.c = (flags & 2u) ? BBX_P - 1u : 1u + uniform(67104u, 2147462208u, 64004u);
  int d1 = 0, d2 = 0;
  if (ncp != 0) {
    d1 = degree();
    d2 = (flags & 1u) ? d1 : degree();
  }
  const BbxGenRow row1 = acc.row(d1), row2 = acc.row(d2);
  const uint32_t j1 = row1.off + uniform(row1.scaling, row1.past, row1.magic);
  const uint32_t j2 = row2.off + uniform(row2.scaling, row2.past, row2.magic);
  uint32_t m1[2], m2[2];
  acc.mono(j1, m1); acc.mono(j2, m2);                                       // (both loads in flight)
  // grevlex as one unsigned compare: m_gt for W = 2 (bbx_device.h)
  const uint64_t k1 = (((uint64_t)m1[1] << 32) | m1[0]) ^ 0x0000FFFFFFFFFFFFull;
  const uint64_t k2 = (((uint64_t)m2[1] << 32) | m2[0]) ^ 0x0000FFFFFFFFFFFFull;
  const bool second = k2 > k1;
  r.lead[0] = second ? m2[0] : m1[0]; r.lead[1] = second ? m2[1] : m1[1];
  r.tail[0] = second ? m1[0] : m2[0]; r.tail[1] = second ? m1[1] : m2[1];
  r.deviated = dev || k1 == k2;                                             // equal: the trial loop would go round
  return r;
}
#endif

// ------------------------------------------------------------------ the fast class's working copy of a basis element's info
// The record keeps, per basis element, ginfo = { lc | tc << 16 , 1/lc | sugar << 16 } (tc: the tail coefficient, 0 = no tail).
// The only thing a step of the fast class ever wants of the first word is the tail coefficient of the MONIC element, with
// either sign — the two coefficients of an S-polynomial —, so its LDS copy (bbx_fast.h) holds those instead, formed once when
// the element enters, and the record's word aside in an array nothing hot reads:
//   hot word  mt | nmt << 16,  mt = tc / lc mod p,  nmt = -mt mod p  (both 0 iff tc == 0; nmt is the reducer word's upper half)
// Stated once, here, for the kernel and for the host check (tests/spoly_coef_check.cpp).
static inline BBX_HD uint32_t bbx_coef_mulmod(uint32_t a, uint32_t b) {      // a b mod p for a, b < p: mulmod of bbx_device.h
  const uint32_t x = a * b;
  const uint32_t q = (uint32_t)(((uint64_t)x * 1099408559ull) >> 45);
  return x - q * BBX_P;
}
static inline BBX_HD uint32_t bbx_ginfo_hot(uint32_t rec_x, uint32_t inv) {  // record word, 1/lc -> hot word
  const uint32_t mt = bbx_coef_mulmod(rec_x >> 16, inv);
  return mt | ((mt ? BBX_P - mt : 0u) << 16);
}
// hot word + the word kept aside -> record word.  (The hot word alone does not determine it — lc is gone —, which is why the
// record's word is kept; the function is where a layout that packs the two differently would say so.)
static inline BBX_HD uint32_t bbx_ginfo_record(uint32_t hot_x, uint32_t kept) { (void)hot_x; return kept; }

// ------------------------------------------------------------------ the fast class's Gebauer-Moeller peel: the key of a candidate
// A candidate lcm of the peel (add_poly, bbx_fast.h) is named by ONE word, degree above basis index: the wave minimum of the
// keys is the smallest index among the candidates of minimal degree — which bucket is next and which member stands for it —,
// and lane and register bank fall out of its low byte.  The lcm's degree is a 16-bit slot and the class holds at most 256
// basis elements (index = 64 bank + lane), so a key has 24 bits and 0xFFFFFFFF (no candidate) is above every one of them.
// Stated once, here, for the kernel and for the host check (tests/peel_keyed_min_check.cpp).
#define BBX_PEEL_NO_KEY 0xFFFFFFFFu
static inline BBX_HD uint32_t bbx_peel_key(uint32_t deg, uint32_t index) { return (deg << 8) | index; }   // deg < 2^16, index < 2^8
static inline BBX_HD uint32_t bbx_peel_key_deg(uint32_t key) { return key >> 8; }
static inline BBX_HD int bbx_peel_key_lane(uint32_t key) { return (int)(key & 63u); }
static inline BBX_HD int bbx_peel_key_bank(uint32_t key) { return (int)((key >> 6) & 3u); }

// position-keyed commutative hash used for parity traces (same definition in oracle/trace.py)
static inline BBX_HD uint64_t bbx_mix64(uint64_t idx, uint32_t word) {
  uint64_t z = ((idx << 32) | (uint64_t)word) + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// counter-based action hash of the built-in random agent (same in oracle/ffi.py, oracle/*.c*)
static inline BBX_HD uint32_t bbx_agent_hash32(uint32_t seed, uint32_t t) {
  return (uint32_t)(bbx_mix64((uint64_t)seed, t) >> 32);
}
// the row the built-in random agent picks among `rows`: multiply-shift range reduction (one mul_hi on the device)
static inline BBX_HD uint32_t bbx_agent_action32(uint32_t seed, uint32_t t, uint32_t rows) {
  return (uint32_t)(((uint64_t)bbx_agent_hash32(seed, t) * rows) >> 32);
}

/* bbx — MI355X-native BuchbergerEnv step path: the C ABI of libbbx.so
 *
 * This is the drop-in boundary for the one hot path of dylanpeifer/deepgroebner that this
 * project replaces: everything the reference's Cython binding (deepgroebner/wrapped.pyx:11-38,
 * declared in deepgroebner/buchberger.pxd:8-18) calls on the C++ class LeadMonomialsEnv
 * (deepgroebner/buchberger.h:224-257, buchberger.cpp:373-408) — generalised from one
 * environment per object to a batch of independent environments per handle, because the device
 * wants thousands of them per launch.  batch == 1 is exactly the reference's single env.
 *
 * Conventions: plain C, caller-allocated outputs, every entry point returns 0 or a negative
 * bbx_status; nothing throws across the ABI; bbx_last_error() (thread-local) explains the last
 * failure.  One host thread per handle.  The library owns all device memory.  It fails loudly
 * (BBX_E_DEVICE) when no HIP device is usable: there is no CPU fallback in the product.
 */
#ifndef BBX_H
#define BBX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bbx_batch bbx_batch;

enum bbx_status {
  BBX_OK = 0,
  BBX_E_ARG = -1,         /* bad argument / unparsable distribution string */
  BBX_E_DEVICE = -2,      /* HIP error or no device */
  BBX_E_CAPACITY = -3,    /* an environment exceeded its configured capacity (see bbx_env_status) */
  BBX_E_GENERATOR = -4,   /* the ideal generator failed (the reference would have thrown) */
  BBX_E_UNSUPPORTED = -5, /* the library has no code for the request (e.g. more than 8 variables, a policy shape or kernel class without a built-in policy) */
  BBX_E_ACTION = -6       /* an action index was outside [0, rows) */
};

/* elimination / reward selectors (reference enums buchberger.h:58 and :93) */
enum { BBX_GEBAUERMOELLER = 0, BBX_LCM = 1, BBX_NONE = 2 };
enum { BBX_ADDITIONS = 0, BBX_REDUCTIONS = 1 };
/* built-in device-side agents for bbx_rollout (0 = actions supplied by the caller) */
enum { BBX_EXTERNAL = 0, BBX_RANDOM_HASH = 1, BBX_DEGREE = 2, BBX_FIRST = 3, BBX_NORMAL = 4, BBX_SUGAR = 5,
       /* the remaining SelectionType values of buchberger.h:111 / buchberger.cpp:200-240: the reversed orders, and
          Random as the reference draws it from a seeded std::default_random_engine (see bbx_seed_strategy) */
       BBX_LAST = 6, BBX_CODEGREE = 7, BBX_STRANGE = 8, BBX_SPICE = 9, BBX_RANDOM_STD = 10 };

/* Per-environment capacities; 0 picks a default suited to the distribution.  Hard limits that remain: 65534 basis
 * elements (pairs are two 16-bit indices), 65535 terms per BASIS element, 2^22 terms per intermediate polynomial. */
typedef struct bbx_caps {
  int32_t max_basis;      /* |G|  (<= 65535) */
  int32_t max_pairs;      /* |P| */
  int32_t arena_terms;    /* total terms of all basis polynomials */
  int32_t max_poly_terms; /* longest intermediate polynomial during spoly/reduce; basis elements hold <= 65535 terms */
  int32_t queue_slots;    /* pre-generated ideals buffered per environment for device-side resets */
  int32_t lds_max_basis;  /* |G| up to which a small (3-variable binomial) environment is kept register/LDS-resident
                             for a whole launch; 0 = default (256 for the class of the reference's C++ LeadMonomialsEnv —
                             Gebauer-Moeller, sorted reducers —, its policy kernels and the other eliminations: 128),
                             negative = never */
  int32_t wide_waves;     /* fixed ideals (long polynomials): waves of the workgroup that serves ONE environment;
                             0 = default (8 when batch <= 4096, else one wave per environment), negative = never */
  int32_t general_class;  /* non-zero: never use the binomial kernel class (term arena + general merges even for
                             binomial ideals); for testing the general path on the same inputs */
  int32_t wide_lds_terms; /* wide class (fixed ideals, one workgroup per environment): terms of the polynomial being
                             reduced kept in LDS (also sizes the reducer window and table); 0 = as much as the LDS
                             holds.  Longer polynomials continue on HBM-resident buffers, so this only affects speed */
  int32_t no_growth;      /* 0 (default): max_basis / max_pairs / arena_terms / max_poly_terms are STARTING sizes — an
                             environment that outgrows one stops before the step that does not fit, the library doubles
                             that array for the whole batch (device memory permitting) and the environment continues, as
                             the reference's heap vectors would (polynomials.h:71-94): capacity costs time, never results.
                             Non-zero: they are hard limits and exceeding one is BBX_E_CAPACITY */
} bbx_caps;

/* One record per environment per step of a traced rollout (parity tests). */
typedef struct bbx_trace_rec {
  int32_t action, rows, basis_size, done;
  double reward;
  uint64_t obs_hash, pairs_hash, newpoly_hash;
} bbx_trace_rec;

/* ---- construction ------------------------------------------------------------------------------
 * Replaces LeadMonomialsEnv::LeadMonomialsEnv(ideal_dist, sort_input, sort_reducers, k)
 * (buchberger.cpp:373-381; reached from wrapped.pyx:14-16) and, for the options the Cython class
 * ignores but the Python class honours, BuchbergerEnv's constructor (buchberger.cpp:269-276;
 * buchberger.py:320-326).  ideal_dist uses the reference grammar (ideals.cpp:103-143). */
int bbx_create(const char* ideal_dist, int elimination, int rewards, int sort_input, int sort_reducers,
               int k, int batch, int device, const bbx_caps* caps, bbx_batch** out);
/* Same over a fixed ideal (FixedIdealGenerator, ideals.h:116-138): polynomial p has nterms[p] terms,
 * coefs/exps (8 ints per term) are concatenated.  nvars_obs <= 0 reproduces the reference's
 * "largest variable index" quirk (ideals.cpp:146-154). */
int bbx_create_fixed(int npolys, const int32_t* nterms, const int32_t* coefs, const int32_t* exps, int nvars_obs,
                     int elimination, int rewards, int sort_input, int sort_reducers,
                     int k, int batch, int device, const bbx_caps* caps, bbx_batch** out);
/* A list of ideals instead of one (what scripts/make_strat.cpp:12-72 iterates over): environment e is reset to ideals
 * e, e + batch, e + 2*batch, ... (wrapping around).  npolys[nideals]; nterms per polynomial, coefs, exps concatenated.
 * Together with bbx_rollout(agent, huge nsteps, auto_reset = 0) and bbx_stats this yields the reference's
 * ZeroReductions / NonzeroReductions / PolynomialAdditions columns per ideal and strategy. */
int bbx_create_ideals(int nideals, const int32_t* npolys, const int32_t* nterms, const int32_t* coefs, const int32_t* exps,
                      int nvars_obs, int elimination, int rewards, int sort_input, int sort_reducers,
                      int k, int batch, int device, const bbx_caps* caps, bbx_batch** out);
void bbx_destroy(bbx_batch* b);
/* LeadMonomialsEnv copy constructor (buchberger.pxd:11, wrapped.pyx:35-38): deep clone incl. the
 * generators' RNG state. */
int bbx_copy(const bbx_batch* b, bbx_batch** out);

/* In-batch clones for tree search (the reference's mcts.py:89,96,147 / az.py:82 copy the env per expanded node):
 * environment src[i] overwrites environment dst[i] — device record, queued ideals and generator RNG state — with no
 * allocation, so a batch can serve as a pool of search nodes.  src and dst must not overlap. */
int bbx_clone_envs(bbx_batch* b, int n, const int32_t* src, const int32_t* dst);

/* ---- LeadMonomialsEnv::seed (buchberger.h:243, wrapped.pyx:28-30): one seed per environment ---- */
int bbx_seed(bbx_batch* b, const int64_t* seeds);
/* seeds of the built-in BBX_RANDOM_HASH agent: action = bbx_agent_action(seed, t, rows), t = steps taken so far */
int bbx_seed_agent(bbx_batch* b, const uint32_t* seeds);
/* seeds of the BBX_RANDOM_STD agent: rng.seed(seed) of buchberger(..., SelectionType::Random, ..., seed)
 * (buchberger.cpp:200-203); every pick is choice(P.begin(), P.end(), rng) (buchberger.cpp:244, ideals.h:68-73).
 * scripts/make_strat.cpp:66 passes the same seed for every ideal. */
int bbx_seed_strategy(bbx_batch* b, const int64_t* seeds);

/* ---- LeadMonomialsEnv::reset (buchberger.cpp:384-395, wrapped.pyx:18-21) ----------------------
 * mask == NULL resets every environment, else those with mask[e] != 0.  rows[e] = |P|. */
int bbx_reset(bbx_batch* b, const uint8_t* mask, int32_t* rows);

/* ---- LeadMonomialsEnv::step (buchberger.cpp:398-408, wrapped.pyx:23-26) -----------------------
 * actions[e] indexes the rows of environment e's observation.  Environments that are done are
 * left untouched (reward 0).  rewards/dones/rows may be NULL.
 * Small batches (<= 8 environments) on the class of the reference's C++ LeadMonomialsEnv: the step calls of a loop (from
 * the fifth call in a row on: bbx_step, bbx_step_autoreset, bbx_step_obs) feed one resident kernel through pinned host memory
 * instead of launching one each — a host mailbox session; any other call on the handle ends it first.
 * Results are those of one launch per step.  Batches of up to 64
 * environments read the actions from and write outputs and observation rows to pinned host memory (no copy calls). */
int bbx_step(bbx_batch* b, const int32_t* actions, double* rewards, uint8_t* dones, int32_t* rows);

/* The vectorised-environment convention: an environment whose episode ends with this step is reset inside the same
 * launch (dones[e] = 1, rows[e] / the next bbx_obs describe the NEW episode), saving the separate bbx_reset call. */
int bbx_step_autoreset(bbx_batch* b, const int32_t* actions, double* rewards, uint8_t* dones, int32_t* rows);

/* nsteps steps per environment in one go with a device-side agent, optionally re-drawing a new
 * ideal whenever an episode ends (what the reference's scripts/random_episodes.cpp:13-29 loop does
 * on the host).  rewards/dones/rows describe the LAST step. */
int bbx_rollout(bbx_batch* b, int agent, int nsteps, int auto_reset, double* rewards, uint8_t* dones, int32_t* rows);

/* ---- the observation: `state` of LeadMonomialsEnv (buchberger.h:247-248; wrapped.pyx:20,25) ---
 * out is int32 [batch, max_rows, cols], cols = 2*nvars*k; rows beyond |P| are filled with -1 when
 * fill != 0 (the padding the reference's agents apply, pg.py:217-226). */
int bbx_obs(bbx_batch* b, int32_t* out, int max_rows, int fill);
/* One call per vector step of the Gym-style loop: the step (actions != NULL; NULL = only refresh the observation), its
 * outputs, and the observation of every environment as a RAGGED block: *offsets -> int32 [batch + 1] row offsets,
 * *obs -> int32 [offsets[batch], cols], environment e owning rows offsets[e] .. offsets[e+1]-1 (exactly the `state`
 * matrices wrapped.pyx:20,25 returns, back to back, no padding).  Both point into pinned memory owned by the handle and
 * stay valid until the next call on it.  One kernel launch for the step, two small ones to pack, two device-to-host
 * copies sized by what the pair sets actually hold (3-4 MB instead of a 25 MB padded block at batch 4096). */
int bbx_step_obs(bbx_batch* b, const int32_t* actions, int auto_reset, double* rewards, uint8_t* dones, int32_t* rows,
                 const int32_t** obs, const int32_t** offsets);
int bbx_cols(const bbx_batch* b);
int bbx_nvars(const bbx_batch* b);
int bbx_batch_size(const bbx_batch* b);

/* ---- LeadMonomialsEnv::value (buchberger.h:245, buchberger.cpp:332-351, wrapped.pyx:32-33) ----
 * discounted return of a full Buchberger rollout from environment idx's current state.
 * Unknown strategies select First, as the reference's std::map lookup does. */
int bbx_value(bbx_batch* b, int idx, const char* strategy, double gamma, double* out);
/* the same for every environment of the batch at once: out[batch].  "random" and "sample" roll out under
 * buchberger(..., SelectionType::Random, ..., seed) (buchberger.cpp:200-203, 244: a std::default_random_engine seeded per
 * rollout, every pick choice(P.begin(), P.end(), rng)); the reference seeds each rollout from std::random_device, here the
 * seeds come from a stream of the handle's own (started from its seed base: reproducible under BBX_DEFAULT_SEED). */
int bbx_values(bbx_batch* b, const char* strategy, double gamma, double* out);
/* ... with the seeds of the Random rollouts given: seeds[batch] for "random", seeds[batch][100] for "sample" (the 100
 * Random rollouts of environment e; its Degree rollout needs none); other strategies ignore them.  Equal to the
 * reference's buchberger(G, P, Random, ..., seed).discounted_return per rollout, bit for bit. */
int bbx_values_seeded(bbx_batch* b, const char* strategy, double gamma, const int64_t* seeds, double* out);
/* Action values: what each pair of each environment is worth under a fixed strategy — the node expansion of the reference's
 * tree search (mcts.py:78-102,147; az.py:81-86: env.copy(), step(a), a rollout, once per action) for the whole batch in one
 * call.  For environment e with n_e pairs and a < n_e:
 *     c = copy of environment e;  (r, done) = c.step(a)      (no auto-reset; rewards as the handle was created)
 *     q[e][a] = r + gamma * c.value(strategy, gamma)          (the value of a finished environment is 0.0)
 * formed in double with one rounded product and one rounded sum: == on doubles to bbx_copy, bbx_step and bbx_values done one
 * after another (NOT the single-rollout sum r0 + gamma r1 + ..., which rounds differently).
 *   q [batch][max_rows], NaN at a >= min(rows[e], max_rows); rewards (or NULL) the same shape: r, NaN padding; dones (or NULL):
 *   the forced step ended the episode, 0 padding; rows [batch]: the FULL pair count — an environment with more than max_rows
 *   pairs has its first max_rows actions valued and shows the cut here.  An environment without pairs (finished, or waiting
 *   for its reset): rows[e] = 0 and an all-NaN row; a batch with nothing to value launches nothing.
 *   "random" / "sample": BBX_E_UNSUPPORTED (per-clone seed streams are not built); any other unknown name selects First, as in
 *   bbx_values.  NULL b / strategy / q / rows or max_rows < 1: BBX_E_ARG.  An environment in an error state fails the call
 *   like bbx_values.  Waits on the host; the call in flight, sessions and queued bbx_values_device calls are settled first.
 *   The handle's environments, counters, bbx_stats and pinned outputs are untouched.
 * One clone per (environment, action), bbx_action_values_chunk of them in flight per pass (default 65536; <= 0 restores it;
 * returns the previous value); a pass is clone, one forced step, resort, the strategy's rollouts, collect.  Clones that
 * outgrow the records enlarge those of the batch (bbx_capacities) and the passes run again: same doubles.
 * bbx_action_values_plan is the pass plan, on the host alone: the flat (environment, action) list with counts[e] positions
 * for environment e, cut into contiguous ranges of at most chunk; first[p] = where pass p begins, first[*npasses] = the
 * total; cap = elements first[] holds (too few: BBX_E_CAPACITY). */
int bbx_action_values(bbx_batch* b, const char* strategy, double gamma, int max_rows, double* q, double* rewards, uint8_t* dones,
                      int32_t* rows);
int bbx_action_values_chunk(bbx_batch* b, int clones);
int bbx_action_values_plan(const int32_t* counts, int B, int chunk, int32_t* first, int cap, int32_t* npasses);

/* ---- same calls on caller-owned DEVICE buffers (e.g. torch tensors), asynchronous on `stream` ----
 * (hipStream_t passed as void*; NULL = the default stream).  obs may be NULL.
 * obs_fill: 0 = rows beyond |P| are left alone; 1 = they are padded with -1 (pg.py:217-226); 2 = incremental padding:
 * the caller vouches that d_obs and d_rows still hold what the previous call on this handle wrote, so only the rows
 * that stopped being valid are re-padded (classes without the incremental path pad everything, like 1).
 * Any number of these calls may be queued before a bbx_sync.  An environment that outgrows a capacity stops at that step:
 * with one step between two waits bbx_sync enlarges the records and takes the step (nothing to see); with several, the
 * environment has sat out the later ones and d_actions meanwhile holds a later step's actions, so bbx_sync enlarges the
 * records and returns BBX_E_CAPACITY naming the environment — its steps of that chain are missing, later calls proceed. */
int bbx_step_device(bbx_batch* b, const int32_t* d_actions, double* d_rewards, uint8_t* d_dones, int32_t* d_rows,
                    int32_t* d_obs, int obs_rows, int obs_fill, void* stream);
/* the same with the vectorised-environment convention of bbx_step_autoreset (finished episodes restart inside the call) */
int bbx_step_device_autoreset(bbx_batch* b, const int32_t* d_actions, double* d_rewards, uint8_t* d_dones, int32_t* d_rows,
                              int32_t* d_obs, int obs_rows, int obs_fill, void* stream);
/* ---- the consumer of the padded observation block: the reference's default policy network on the device ----------
 * ParallelMultilayerPerceptron([hidden]) (networks.py:522-571: ParallelEmbeddingLayer :49-95 with one dense relu layer,
 * ParallelDecidingLayer :414-460) evaluated on d_obs [batch, obs_rows, cols] over the d_rows[e] valid rows of each
 * environment (the -1 padding is masked out there, plays no part here), log-softmax over the rows and ONE action drawn
 * by inverse CDF from the uniform number d_u[e] in [0, 1) — the step of pg.py:451-503's run_episode that used to cross to
 * the host every step.  fp32, the hidden layer on the matrix cores (exact f32 MFMA); cols <= 64, hidden <= 256, at most
 * 2048 rows per environment (obs_rows > 2048: BBX_E_UNSUPPORTED; a policy rollout without an observation block whose pair
 * set outgrows 2048 rows: BBX_E_CAPACITY from bbx_sync — never a silent cut).  exp / log of the softmax are the
 * hardware's fast forms (__expf / __logf).  Against a float64 evaluation a log-probability is held to
 * |error| <= C_L 2^-24 (S + |logZ| + 1), S the network evaluated with |W|, |b|, |x| (tests/policy_cases.py, tests/test_policy_parity.py;
 * C_L = 64 is a ceiling, not yet a measurement: about 4e-6 (S + |logZ| + 1)).
 * The weights are handed over PREPARED: bbx_pmlp_prepare copies d_w1 [cols][hidden] (the layout of
 * torch.nn.Linear(...).weight.t()), d_b1 [hidden], d_w2 [hidden], b2 into d_prepared (bbx_pmlp_prepared_floats(cols,
 * hidden) floats, 16-byte aligned) zero-padded to the kernels' tile sizes; call it again whenever the weights change.
 * d_actions[e] in [0, rows), d_logprobs[e] = its log-probability. */
int bbx_pmlp_prepared_floats(int cols, int hidden);        /* < 0: shape not supported */
int bbx_pmlp_prepare(const float* d_w1, const float* d_b1, const float* d_w2, float b2, int cols, int hidden, float* d_prepared, void* stream);
int bbx_pmlp_act(const int32_t* d_obs, const int32_t* d_rows, int batch, int obs_rows, int cols, const float* d_prepared, int hidden,
                 const float* d_u, int32_t* d_actions, float* d_logprobs, void* stream);
/* ---- the same policy as a differentiable function of its weights: what the reference's update (pg.py _fit_policy_model)
 * needs per recorded state.  No handle: device pointers and a stream; asynchronous on `stream`, recordable into a HIP graph,
 * no host read-back and no allocation inside the calls.  One hidden layer here; two: bbx_pmlp2_logprob / bbx_pmlp2_grad below.
 * bbx_pmlp_logprob: d_logprobs[s] = log pi(d_actions[s] | state s) and d_entropy[s] (may be NULL) = the entropy of pi(. | state s)
 * for n recorded states d_obs [n][obs_rows][cols] under the weights d_prepared (as bbx_pmlp_prepare leaves them).
 *   Shapes: exactly those of bbx_pmlp_act (cols <= 64, hidden <= 256, obs_rows <= BBX_POLICY_MAX_ROWS); anything else:
 *     BBX_E_UNSUPPORTED with a message, before anything is queued.  n == 0 is legal (bbx_pmlp_grad then only zeroes its outputs).
 *   Rows: the row COUNT masks, n_s = clamp(d_rows[s], 0, min(obs_rows, 2048)); what lies beyond the live rows, -1 padding or
 *     garbage, plays no part.
 *   n_s <= 0: logprob = 0.0f, entropy = 0.0f, no contribution to any gradient.
 *   n_s == 1: logprob = 0, entropy = 0, and a gradient contribution that is exactly zero (delta - p = 0).
 *   An action outside [0, n_s) on a state with n_s > 0: logprob = NaN (never a silently wrong number); its entropy is still
 *     computed; in bbx_pmlp_grad such a state contributes NOTHING (its d_glogp / d_gent entries are not read into any sum).
 *   exp / log are the fast forms of bbx_pmlp_act; the logits come from the same tile code, the maximum and the sum in the same
 *     order: for an action bbx_pmlp_act has just sampled from the same block and weights, d_logprobs equals that call's bit for bit.
 *   Entropy: log(se) - (sum_r e_r (z_r - m)) / se with m = max_r z_r, e_r = exp(z_r - m), se = sum_r e_r (= logZ - sum_r p_r z_r).
 *   Against a float64 evaluation (tests/policy_grad_cases.py): the log-probability as for bbx_pmlp_act; the entropy within
 *     C_H 2^-24 (S + |logZ| + 1)(1 + log n_s).
 * bbx_pmlp_grad: dL/dW1 -> d_gw1 [cols][hidden], dL/db1 -> d_gb1 [hidden], dL/dw2 -> d_gw2 [hidden], dL/db2 -> d_gb2 [1] of
 *     L = sum_s d_glogp[s] logprob_s + d_gent[s] entropy_s          (d_gent may be NULL = zeros)
 *   in the layouts bbx_pmlp_prepare READS (not the padded ones).  The outputs are overwritten, not accumulated into.
 *   The hidden activations are recomputed, never stored: d_workspace holds bbx_pmlp_grad_workspace_floats(n, obs_rows, cols,
 *   hidden) floats (16-byte aligned), which does not grow with obs_rows and is bounded in n (at most 1024 partial sums per output).
 *   Deterministic: no floating-point atomics; every wave's partial sums go to the workspace and a second kernel of the same
 *   call adds them in a fixed order; the partition depends on (n, cols, hidden) alone, not on the device: two calls on the same
 *   inputs return the same bits.  Against float64 every entry is held to C_G 2^-24 sum_s K_s A_s (K_s = S + |logZ_s| + 1, A_s the
 *   state's contribution with every term replaced by its absolute value: tests/policy_grad_cases.py). */
int bbx_pmlp_logprob(const int32_t* d_obs, const int32_t* d_rows, const int32_t* d_actions, int n, int obs_rows, int cols,
                     const float* d_prepared, int hidden, float* d_logprobs, float* d_entropy, void* stream);
int bbx_pmlp_grad_workspace_floats(int n, int obs_rows, int cols, int hidden);   /* < 0: shape not supported */
int bbx_pmlp_grad(const int32_t* d_obs, const int32_t* d_rows, const int32_t* d_actions, int n, int obs_rows, int cols,
                  const float* d_prepared, int hidden, const float* d_glogp, const float* d_gent, float* d_workspace,
                  float* d_gw1, float* d_gb1, float* d_gw2, float* d_gb2, void* stream);
/* The same for ParallelMultilayerPerceptron(hidden_layers=[hidden1, hidden2]) (networks.py:562-571: two dense layers in the
 * embedding): logit_r = w3 . relu(W2^T relu(W1^T x_r + b1) + b2) + b3, both layers on the matrix cores in exact f32, the
 * second layer's weights staged in LDS once per workgroup (bbx_pmlp2.hip); cols <= 64, hidden1, hidden2 <= 128, at most 2048
 * rows per environment.  d_w1 [cols][hidden1], d_b1 [hidden1], d_w2 [hidden1][hidden2], d_b2 [hidden2], d_w3 [hidden2],
 * d_b3 [1] (the transposed layouts of torch.nn.Linear weights; every argument on the device: preparing never reads back).
 * Stands alone in front of bbx_step_device_autoreset (two launches per vector step, both recordable into a HIP graph);
 * the fused per-step and session forms exist for one hidden layer only, the rollout form also for two
 * (bbx_policy2_rollout_device). */
int bbx_pmlp2_prepared_floats(int cols, int hidden1, int hidden2);   /* < 0: shape not supported */
int bbx_pmlp2_prepare(const float* d_w1, const float* d_b1, const float* d_w2, const float* d_b2, const float* d_w3, const float* d_b3,
                      int cols, int hidden1, int hidden2, float* d_prepared, void* stream);
int bbx_pmlp2_act(const int32_t* d_obs, const int32_t* d_rows, int batch, int obs_rows, int cols, const float* d_prepared, int hidden1, int hidden2,
                  const float* d_u, int32_t* d_actions, float* d_logprobs, void* stream);
/* The two-layer policy as a differentiable function of its weights: bbx_pmlp_logprob / bbx_pmlp_grad for
 * ParallelMultilayerPerceptron([hidden1, hidden2]), with the same conventions word for word — no handle, asynchronous on `stream`,
 * no host read-back, no allocation; n == 0 is legal (bbx_pmlp2_grad then only zeroes its outputs); the row count masks,
 * n_s = clamp(d_rows[s], 0, min(obs_rows, 2048)); n_s <= 0: 0.0f / 0.0f and no gradient; n_s == 1: 0 / 0 and an exactly zero
 * contribution; an action outside [0, n_s): logprob NaN, the entropy still computed, nothing contributed to any gradient (its
 * d_glogp / d_gent are not read into any sum); entropy = log(se) - (sum_r e_r (z_r - m)) / se; the relu derivative is
 * [pre-activation > 0] in both layers; L = sum_s d_glogp[s] logprob_s + d_gent[s] entropy_s (d_gent may be NULL = zeros).
 *   d_prepared: exactly what bbx_pmlp2_prepare leaves.  Shapes: those of bbx_pmlp2_act (cols <= 64, hidden1, hidden2 <= 128,
 *     obs_rows <= BBX_POLICY_MAX_ROWS); anything else: BBX_E_UNSUPPORTED naming the number, before anything is queued and
 *     without a device.  A device with less LDS per workgroup than the staged second layer needs: BBX_E_UNSUPPORTED.
 *   The logits come from the tile code of bbx_pmlp2_act, maximum and sum in its order: for an action bbx_pmlp2_act has just
 *     drawn from the same block and prepared weights, d_logprobs equals that call's log-probability bit for bit.
 *   Outputs in the layouts bbx_pmlp2_prepare READS: d_gw1 [cols][hidden1], d_gb1 [hidden1], d_gw2 [hidden1][hidden2],
 *     d_gb2 [hidden2], d_gw3 [hidden2], d_gb3 [1]; overwritten, not accumulated into; nothing outside them is written.
 *   Both hidden tiles are recomputed, never stored: d_workspace holds bbx_pmlp2_grad_workspace_floats(n, obs_rows, cols, hidden1,
 *     hidden2) floats (16-byte aligned), which does not depend on obs_rows, stops growing with n (at most 512 partial sums per
 *     output) and is at most 2^24 floats.  Deterministic: no floating-point atomics; every workgroup's partial sums go to the
 *     workspace and a second kernel of the same call adds them in a fixed order; the partition depends on (n, cols, hidden1,
 *     hidden2) alone: two calls on the same inputs return the same bits.  Against float64 (tests/policy2_grad_cases.py): the
 *     log-probability as for bbx_pmlp2_act, the entropy within C_H2 2^-24 K_s (1 + log n_s), every gradient entry within
 *     C_G2 2^-24 sum_s K_s A_s. */
int bbx_pmlp2_logprob(const int32_t* d_obs, const int32_t* d_rows, const int32_t* d_actions, int n, int obs_rows, int cols,
                      const float* d_prepared, int hidden1, int hidden2, float* d_logprobs, float* d_entropy, void* stream);
int bbx_pmlp2_grad_workspace_floats(int n, int obs_rows, int cols, int hidden1, int hidden2);   /* < 0: not supported */
int bbx_pmlp2_grad(const int32_t* d_obs, const int32_t* d_rows, const int32_t* d_actions, int n, int obs_rows, int cols,
                   const float* d_prepared, int hidden1, int hidden2, const float* d_glogp, const float* d_gent, float* d_workspace,
                   float* d_gw1, float* d_gb1, float* d_gw2, float* d_gb2, float* d_gw3, float* d_gb3, void* stream);
/* The four calls above, INDEXED: position k in [0, n) of the call is about recorded state s = d_index[k] of n_src recorded ones —
 * d_obs [n_src][obs_rows][cols], d_rows [n_src] and d_actions [n_src] are read at s, nothing is gathered or copied; d_index,
 * d_logprobs, d_entropy, d_glogp and d_gent have length n and are addressed by k.  What a training epoch over a trajectory buffer
 * needs: its minibatches are slices of one int32 list of step numbers over the arrays as the rollout kernels left them, a
 * shuffle is a permutation of that list.  All offsets are 64-bit (n_src obs_rows cols may exceed 2^31).
 *   Every convention is that of the call without _at, word for word: shapes and refusals (before anything is queued; the
 *     two-layer pair without a device), n == 0 (the grad entries then only zero their outputs), NULL d_entropy / d_gent, no
 *     allocation, no read-back, recordable into a HIP graph, deterministic.  The workspace of the grad entries holds
 *     bbx_pmlp_grad_workspace_floats(n, ...) / bbx_pmlp2_grad_workspace_floats(n, ...) floats for THIS n (not n_src).
 *   In addition: n_src < 0, or a NULL d_index with n > 0: BBX_E_ARG.
 *   An index outside [0, n_src): logprob = NaN and entropy = NaN at its position; it contributes NOTHING to any gradient (its
 *     d_glogp / d_gent are not read into any sum), and nothing is read from d_obs, d_rows or d_actions at that index.
 *   Repeated indices are legal; every occurrence counts.
 *   For every index in range the outputs equal, bit for bit, those of the call without _at on the gathered contiguous arrays
 *     d_obs[d_index], d_rows[d_index], d_actions[d_index]: the same tile code, the same order of maximum and sum, the same partition
 *     of the n positions over waves and workgroups, the same second kernel. */
int bbx_pmlp_logprob_at(const int32_t* d_obs, const int32_t* d_rows, const int32_t* d_actions, int n_src, const int32_t* d_index, int n,
                        int obs_rows, int cols, const float* d_prepared, int hidden, float* d_logprobs, float* d_entropy, void* stream);
int bbx_pmlp_grad_at(const int32_t* d_obs, const int32_t* d_rows, const int32_t* d_actions, int n_src, const int32_t* d_index, int n,
                     int obs_rows, int cols, const float* d_prepared, int hidden, const float* d_glogp, const float* d_gent,
                     float* d_workspace, float* d_gw1, float* d_gb1, float* d_gw2, float* d_gb2, void* stream);
int bbx_pmlp2_logprob_at(const int32_t* d_obs, const int32_t* d_rows, const int32_t* d_actions, int n_src, const int32_t* d_index, int n,
                         int obs_rows, int cols, const float* d_prepared, int hidden1, int hidden2, float* d_logprobs, float* d_entropy,
                         void* stream);
int bbx_pmlp2_grad_at(const int32_t* d_obs, const int32_t* d_rows, const int32_t* d_actions, int n_src, const int32_t* d_index, int n,
                      int obs_rows, int cols, const float* d_prepared, int hidden1, int hidden2, const float* d_glogp, const float* d_gent,
                      float* d_workspace, float* d_gw1, float* d_gb1, float* d_gw2, float* d_gb2, float* d_gw3, float* d_gb3, void* stream);
/* One call per PPO minibatch: from the recorded states, the rollout's log-probabilities and the advantages to the weight gradients
 * of the PPO objective and the numbers a training loop watches — the forward kernel of bbx_pmlp[2]_logprob[_at] with a loss
 * epilogue, a statistics kernel, and the gradient and reduce kernels of bbx_pmlp[2]_grad[_at], queued from here: no autograd, no
 * elementwise pass over the n positions in between, no host wait.
 *   Per position k, with new = logprob_k, old = d_old_logprobs[k], A = d_advantages[k], in float32 and in this order
 *   (exp is the fast form of the kernels; no fused multiply-adds):
 *       d = new - old            r = exp(d)                   sA = scale * A
 *       mode 0 (policy gradient):   u = new * A                      gl = -sA
 *       mode 1 (PPO-clip):          a = r * A;  b = fminf(fmaxf(r, lo), hi) * A      (lo = 1.f - eps, hi = 1.f + eps)
 *                                   u = fminf(a, b)                  gl = (a <= b) ? -(sA * r) : 0.f         "clipped" iff a > b
 *       mode 2 (PPO-penalty):       u = r * A - c_kl * (old - new)   gl = -(sA * r) - scale * c_kl
 *       every mode:                 ge = -(scale * ent_coef)
 *   gl = dL/dlogprob_k and ge = dL/dH_k of the objective L = -scale sum_k u_k - scale ent_coef sum_k H_k over the counted positions
 *   (mode 1: what autograd gives for -(min(r A, clamp(r, lo, hi) A)).sum() * scale, ties inside the clip range included).  The
 *   caller passes scale (1 / n for means): nothing is counted in a pass of its own.
 *   d_coef [2 n] receives gl at k and ge at n + k.  THE GRADIENTS ARE, BIT FOR BIT, THOSE OF bbx_pmlp_grad[_at] (bbx_pmlp2_grad[_at])
 *   CALLED WITH d_glogp = d_coef, d_gent = d_coef + n ON THE SAME INPUTS; d_logprobs and d_entropy (either may be NULL) are those of
 *   bbx_pmlp[2]_logprob[_at], bit for bit.
 *   Positions that do not count: a NaN log-probability (an index out of range, an action outside the live rows): gl = ge = 0.f,
 *   u left out of every sum.  A state without live rows counts, with logprob = 0 and H = 0 (the gradient kernel skips it, as
 *   always).  What the caller puts into d_old_logprobs / d_advantages is not checked.
 *   d_stats, double [6]: counted positions, sum u_k, sum H_k, sum (old_k - new_k), positions clipped (mode 1; else 0), positions
 *   not counted — sums in double over the float32 terms by one workgroup, thread t adding positions t, t + 1024, ..., then lanes,
 *   then waves in a fixed order: no floating-point atomics, a partition that depends on n alone, the same bits on any device.
 *   (loss = -scale (stats[1] + ent_coef stats[2]); approximate KL = stats[3] / stats[0]; clip fraction = stats[4] / stats[0].)
 *   d_workspace holds bbx_pmlp_ppo_workspace_floats(n, ...) floats (16-byte aligned): the gradient kernels' workspace, then
 *   u | H | old - new | flags, n each.
 *   Every convention of the logprob / grad entries holds word for word: shapes and refusals before anything is queued (the
 *   two-layer entries without a device), n == 0 (gradients zeroed, d_stats zeros; the arrays of length n may be NULL), outputs
 *   overwritten, no allocation, no read-back, asynchronous on `stream`, recordable into a HIP graph, deterministic, 64-bit offsets;
 *   _at: position k is about recorded state d_index[k] of n_src, the per-call arrays (d_old_logprobs, d_advantages, d_logprobs,
 *   d_entropy, d_coef) are addressed by k.  In addition BBX_E_ARG for: mode outside 0..2, eps < 0, a NULL d_coef / d_stats /
 *   d_old_logprobs / d_advantages with n > 0, an n whose workspace size does not fit an int. */
int bbx_pmlp_ppo_workspace_floats(int n, int obs_rows, int cols, int hidden);   /* < 0: shape not supported */
int bbx_pmlp_ppo_grad(const int32_t* d_obs, const int32_t* d_rows, const int32_t* d_actions, int n, int obs_rows, int cols,
                      const float* d_prepared, int hidden, const float* d_old_logprobs, const float* d_advantages, int mode, float scale,
                      float eps, float ent_coef, float c_kl, float* d_logprobs, float* d_entropy, float* d_coef, double* d_stats,
                      float* d_workspace, float* d_gw1, float* d_gb1, float* d_gw2, float* d_gb2, void* stream);
int bbx_pmlp_ppo_grad_at(const int32_t* d_obs, const int32_t* d_rows, const int32_t* d_actions, int n_src, const int32_t* d_index, int n,
                         int obs_rows, int cols, const float* d_prepared, int hidden, const float* d_old_logprobs, const float* d_advantages,
                         int mode, float scale, float eps, float ent_coef, float c_kl, float* d_logprobs, float* d_entropy, float* d_coef,
                         double* d_stats, float* d_workspace, float* d_gw1, float* d_gb1, float* d_gw2, float* d_gb2, void* stream);
int bbx_pmlp2_ppo_workspace_floats(int n, int obs_rows, int cols, int hidden1, int hidden2);   /* < 0: not supported */
int bbx_pmlp2_ppo_grad(const int32_t* d_obs, const int32_t* d_rows, const int32_t* d_actions, int n, int obs_rows, int cols,
                       const float* d_prepared, int hidden1, int hidden2, const float* d_old_logprobs, const float* d_advantages, int mode,
                       float scale, float eps, float ent_coef, float c_kl, float* d_logprobs, float* d_entropy, float* d_coef, double* d_stats,
                       float* d_workspace, float* d_gw1, float* d_gb1, float* d_gw2, float* d_gb2, float* d_gw3, float* d_gb3, void* stream);
int bbx_pmlp2_ppo_grad_at(const int32_t* d_obs, const int32_t* d_rows, const int32_t* d_actions, int n_src, const int32_t* d_index, int n,
                          int obs_rows, int cols, const float* d_prepared, int hidden1, int hidden2, const float* d_old_logprobs,
                          const float* d_advantages, int mode, float scale, float eps, float ent_coef, float c_kl, float* d_logprobs,
                          float* d_entropy, float* d_coef, double* d_stats, float* d_workspace, float* d_gw1, float* d_gb1, float* d_gw2,
                          float* d_gb2, float* d_gw3, float* d_gb3, void* stream);
/* Cross-entropy against a target distribution over each state's rows (a softmax of action values, a search's visit counts, an
 * expert's pick as a one-hot row): the loss alone (bbx_pmlp[2]_xent[_at], for held-out data), and one call per training minibatch
 * (bbx_pmlp[2]_xent_grad[_at]) — the forward kernel of bbx_pmlp[2]_logprob[_at] with a cross-entropy epilogue, a statistics kernel,
 * a gradient kernel whose head forms dL/dz from the targets, and the reduce kernel of bbx_pmlp[2]_grad, queued from here.
 *   d_targets is float32 [n_src][obs_rows] (plain forms: n_src == n) and, like d_actions, addressed by the RECORDED STATE; d_weights
 *   (NULL: every weight 1), d_losses, d_entropy and d_coef are addressed by the position k.
 *   Per position k about state s, with n = clamp(d_rows[s], 0, min(obs_rows, 2048)) live rows, logits z_r, mx / se / logz as the
 *   log-probability kernels form them, p_r = exp(z_r - mx) (1.f / se), t_r = d_targets[s][r] for r < n, w = d_weights[k], in float32
 *   and in this order (no fused multiply-adds but the one named):
 *       T = sum_r t_r        sd = sum_r t_r (z_r - mx)        (lane t adds rows t, t + 64, ... in order, then the wave's 64 sums)
 *       l = T * log(se) - sd                  = -sum_r t_r log p_r       H = the entropy of bbx_pmlp[2]_logprob        c = scale * w
 *       g_r = c * fma(T * (1.f / se), exp(z_r - mx), -t_r)               = dL/dz_r of L = scale sum_k w_k l_k
 *   What lies in d_targets[s][r] for r >= n is never read into anything (the NaN padding of bbx_action_values included).  Targets
 *   need not sum to one.  A one-hot row (t = e_a, w = 1) gives, bit for bit, the gradients of bbx_pmlp[2]_grad with d_glogp[k] =
 *   -scale and d_gent = NULL.
 *   Positions that do not count — l = NaN, c = 0, nothing in any sum or gradient: an index out of range (H = NaN too), a live t_r
 *   that is negative or not finite, a w that is not finite.  Counted, with zero loss and no gradient: no live row (l = H = 0), one
 *   live row (l = 0 exactly), T = 0.
 *   d_losses [n] receives l, d_entropy [n] H (bbx_pmlp[2]_xent: d_losses is owed when n > 0; bbx_pmlp[2]_xent_grad: either may be
 *   NULL); d_coef [2 n] receives c at k and T at n + k (zeros where the position is not counted).
 *   d_stats, double [6]: counted positions, sum w l, sum w T, sum H, sum w, positions not counted — sums in double over the float32
 *   terms, in the order of bbx_pmlp_ppo_grad's.  (the weighted mean loss = stats[1] / stats[4].)
 *   d_workspace holds bbx_pmlp[2]_xent_workspace_floats(n, ...) floats (16-byte aligned): the gradient kernels' workspace, then
 *   w l | w T | H | w | flags, n each.
 *   Every convention of the bbx_pmlp[2]_ppo_grad entries holds word for word (shapes and refusals before anything is queued, n == 0,
 *   outputs overwritten, no allocation, no read-back, asynchronous on `stream`, recordable into a HIP graph, deterministic, 64-bit
 *   offsets, _at addressing).  In addition BBX_E_ARG for: a NULL d_targets (bbx_pmlp[2]_xent_grad: d_coef, d_stats too) with
 *   n > 0, a scale that is not finite, an n whose workspace size does not fit an int. */
int bbx_pmlp_xent(const int32_t* d_obs, const int32_t* d_rows, const float* d_targets, int n, int obs_rows, int cols, const float* d_prepared,
                  int hidden, const float* d_weights, float scale, float* d_losses, float* d_entropy, void* stream);
int bbx_pmlp_xent_at(const int32_t* d_obs, const int32_t* d_rows, const float* d_targets, int n_src, const int32_t* d_index, int n, int obs_rows,
                     int cols, const float* d_prepared, int hidden, const float* d_weights, float scale, float* d_losses, float* d_entropy,
                     void* stream);
int bbx_pmlp_xent_workspace_floats(int n, int obs_rows, int cols, int hidden);   /* < 0: shape not supported */
int bbx_pmlp_xent_grad(const int32_t* d_obs, const int32_t* d_rows, const float* d_targets, int n, int obs_rows, int cols, const float* d_prepared,
                       int hidden, const float* d_weights, float scale, float* d_losses, float* d_entropy, float* d_coef, double* d_stats,
                       float* d_workspace, float* d_gw1, float* d_gb1, float* d_gw2, float* d_gb2, void* stream);
int bbx_pmlp_xent_grad_at(const int32_t* d_obs, const int32_t* d_rows, const float* d_targets, int n_src, const int32_t* d_index, int n,
                          int obs_rows, int cols, const float* d_prepared, int hidden, const float* d_weights, float scale, float* d_losses,
                          float* d_entropy, float* d_coef, double* d_stats, float* d_workspace, float* d_gw1, float* d_gb1, float* d_gw2,
                          float* d_gb2, void* stream);
int bbx_pmlp2_xent(const int32_t* d_obs, const int32_t* d_rows, const float* d_targets, int n, int obs_rows, int cols, const float* d_prepared,
                   int hidden1, int hidden2, const float* d_weights, float scale, float* d_losses, float* d_entropy, void* stream);
int bbx_pmlp2_xent_at(const int32_t* d_obs, const int32_t* d_rows, const float* d_targets, int n_src, const int32_t* d_index, int n, int obs_rows,
                      int cols, const float* d_prepared, int hidden1, int hidden2, const float* d_weights, float scale, float* d_losses,
                      float* d_entropy, void* stream);
int bbx_pmlp2_xent_workspace_floats(int n, int obs_rows, int cols, int hidden1, int hidden2);   /* < 0: not supported */
int bbx_pmlp2_xent_grad(const int32_t* d_obs, const int32_t* d_rows, const float* d_targets, int n, int obs_rows, int cols,
                        const float* d_prepared, int hidden1, int hidden2, const float* d_weights, float scale, float* d_losses, float* d_entropy,
                        float* d_coef, double* d_stats, float* d_workspace, float* d_gw1, float* d_gb1, float* d_gw2, float* d_gb2, float* d_gw3,
                        float* d_gb3, void* stream);
int bbx_pmlp2_xent_grad_at(const int32_t* d_obs, const int32_t* d_rows, const float* d_targets, int n_src, const int32_t* d_index, int n,
                           int obs_rows, int cols, const float* d_prepared, int hidden1, int hidden2, const float* d_weights, float scale,
                           float* d_losses, float* d_entropy, float* d_coef, double* d_stats, float* d_workspace, float* d_gw1, float* d_gb1,
                           float* d_gw2, float* d_gb2, float* d_gw3, float* d_gb3, void* stream);
/* A learned value baseline (critic) over recorded states: ONE hidden layer with exactly the parameters, layouts and prepared
 * weights of the one-layer policy (bbx_pmlp_prepare, unchanged) and the shapes of bbx_pmlp_logprob (cols <= 64, hidden <= 256,
 * obs_rows <= BBX_POLICY_MAX_ROWS).  The row score z_r = w2 . relu(W1^T x_r + b1) + b2 comes from the policy kernels' tile code
 * (for the same block and weights: the same bits as their logits); the live rows are n_s = clamp(d_rows[s], 0, min(obs_rows, 2048));
 * the value is V(s) = pool over the live rows of z_r, float32:
 *   BBX_POOL_SUM   lane t of the state's wave adds z_t, z_{t+64}, ... in increasing row order from 0.f, the 64 lanes are then added
 *                  in the fixed order of the policy kernels' wave sum.             dV/dz_r = 1
 *   BBX_POOL_MEAN  that sum divided by (float)n_s (an IEEE division).             dV/dz_r = 1 / (float)n_s   (g_r = g / (float)n_s)
 *   BBX_POOL_LSE   the log-partition of the policy kernels (max + log sum exp, their order and fast exp / log).
 *                  g_r = g * (exp(z_r - max) * (1.f / se)): the probability expression of bbx_pmlp_grad.
 *   n_s <= 0: V = 0.0f and no gradient (a finished state is worth nothing: what GAE assumes behind a done flag).  A state with ONE
 *   live row contributes to the gradients like any other (bbx_pmlp_grad skips such states; these calls do not).  Rows beyond the
 *   live rows play no part, whether they hold -1 padding or anything else.
 * Every convention of bbx_pmlp_logprob[_at] / bbx_pmlp_grad[_at] / bbx_pmlp_ppo_grad[_at] holds word for word: no handle,
 * asynchronous on `stream`, no allocation, no read-back, 64-bit offsets, refusals before anything is queued and without a device
 * (BBX_E_UNSUPPORTED for shapes; BBX_E_ARG for a pool outside 0..2 and the NULLs named here), n == 0 legal (gradients zeroed, stats
 * zeros), outputs overwritten, deterministic (no floating-point atomics; the partition depends on the shape and n alone); _at:
 * position k is about recorded state d_index[k] of n_src, repeated indices count every time, an index outside [0, n_src) gives NaN at
 * its position, reads nothing at that index and contributes nothing to any gradient.
 * bbx_pmlp_value[_at]: d_values [n] float and d_values64 [n] (the same number widened: the [nsteps][batch] double array
 *   bbx_gae_device reads can be filled directly) — either may be NULL, both NULL with n > 0: BBX_E_ARG.
 * bbx_pmlp_value_grad[_at]: the gradients of L = sum_k d_gvalue[k] V_k in the layouts bbx_pmlp_prepare reads; d_workspace holds
 *   bbx_pmlp_value_grad_workspace_floats(n, ...) = bbx_pmlp_grad_workspace_floats(n, ...) floats (the policy gradient's partition
 *   and second kernel).  A state without live rows or an index out of range: its d_gvalue is not read.
 * bbx_pmlp_value_fit[_at]: one call per minibatch of the squared-error fit, L = scale 1/2 sum_k d_k^2.  Per position, in float32
 *   and in this order, no fused multiply-adds:   d = V - target   u = d * d   coef = scale * d.   d_coef [n] receives coef; THE
 *   GRADIENTS ARE, BIT FOR BIT, THOSE OF bbx_pmlp_value_grad[_at] CALLED WITH d_gvalue = d_coef; d_values (may be NULL) is, bit for
 *   bit, that of bbx_pmlp_value[_at].  A NaN value (an index out of range): coef = 0, left out of every sum.  A state without live
 *   rows counts, with V = 0.  d_stats, double [6]: counted positions, sum d^2, sum V, sum target, sum target^2 (the float32 product),
 *   positions not counted — in double over the float32 terms, by one workgroup in the thread, lane and wave order of the PPO
 *   statistics.  (loss = scale stats[1] / 2; explained variance = 1 - (stats[1] / c) / (stats[4] / c - (stats[3] / c)^2), c = stats[0].)
 *   d_workspace holds bbx_pmlp_value_fit_workspace_floats(n, ...) floats (16-byte aligned): the gradient workspace, then
 *   d^2 | V | target | flags, n each.  d_targets, d_coef or d_stats NULL with n > 0: BBX_E_ARG. */
enum { BBX_POOL_SUM = 0, BBX_POOL_MEAN = 1, BBX_POOL_LSE = 2 };
int bbx_pmlp_value(const int32_t* d_obs, const int32_t* d_rows, int n, int obs_rows, int cols, const float* d_prepared, int hidden, int pool,
                   float* d_values, double* d_values64, void* stream);
int bbx_pmlp_value_at(const int32_t* d_obs, const int32_t* d_rows, int n_src, const int32_t* d_index, int n, int obs_rows, int cols,
                      const float* d_prepared, int hidden, int pool, float* d_values, double* d_values64, void* stream);
int bbx_pmlp_value_grad_workspace_floats(int n, int obs_rows, int cols, int hidden);   /* < 0: shape not supported */
int bbx_pmlp_value_grad(const int32_t* d_obs, const int32_t* d_rows, int n, int obs_rows, int cols, const float* d_prepared, int hidden, int pool,
                        const float* d_gvalue, float* d_workspace, float* d_gw1, float* d_gb1, float* d_gw2, float* d_gb2, void* stream);
int bbx_pmlp_value_grad_at(const int32_t* d_obs, const int32_t* d_rows, int n_src, const int32_t* d_index, int n, int obs_rows, int cols,
                           const float* d_prepared, int hidden, int pool, const float* d_gvalue, float* d_workspace, float* d_gw1, float* d_gb1,
                           float* d_gw2, float* d_gb2, void* stream);
int bbx_pmlp_value_fit_workspace_floats(int n, int obs_rows, int cols, int hidden);   /* < 0: shape not supported */
int bbx_pmlp_value_fit(const int32_t* d_obs, const int32_t* d_rows, int n, int obs_rows, int cols, const float* d_prepared, int hidden, int pool,
                       const float* d_targets, float scale, float* d_values, float* d_coef, double* d_stats, float* d_workspace, float* d_gw1,
                       float* d_gb1, float* d_gw2, float* d_gb2, void* stream);
int bbx_pmlp_value_fit_at(const int32_t* d_obs, const int32_t* d_rows, int n_src, const int32_t* d_index, int n, int obs_rows, int cols,
                          const float* d_prepared, int hidden, int pool, const float* d_targets, float scale, float* d_values, float* d_coef,
                          double* d_stats, float* d_workspace, float* d_gw1, float* d_gb1, float* d_gw2, float* d_gb2, void* stream);
/* The critic over TWO hidden layers: the block above word for word — pools, live rows n_s = clamp(d_rows[s], 0, min(obs_rows, 2048)),
 * n_s <= 0: V = 0.0f and no gradient, ONE live row contributes, rows beyond the live ones play no part, _at: an index outside
 * [0, n_src) gives NaN, reads nothing there and contributes nothing, n == 0 legal, the fit's float32 recipe, d_stats and workspace
 * tail — with the parameters, layouts and prepared weights of the two-layer policy (bbx_pmlp2_prepare, unchanged:
 * bbx_pmlp2_prepared_floats) and the shapes of bbx_pmlp2_logprob (1 <= cols <= 64, 1 <= hidden1, hidden2 <= 128, 1 <= obs_rows <=
 * BBX_POLICY_MAX_ROWS; anything else: BBX_E_UNSUPPORTED before a device is asked for anything; a device with too little LDS per
 * workgroup: BBX_E_UNSUPPORTED as well).  The row score z_r = w3 . relu(W2^T relu(W1^T x_r + b1) + b2) + b3 comes from the two-layer
 * policy kernels' tile code: for the same block and weights, the bits of their logits.
 * bbx_pmlp2_value[_at]: d_values / d_values64 as bbx_pmlp_value's (either may be NULL, both NULL with n > 0: BBX_E_ARG).
 * bbx_pmlp2_value_grad[_at]: the gradients of L = sum_k d_gvalue[k] V_k in the six layouts bbx_pmlp2_prepare reads; d_workspace holds
 *   bbx_pmlp2_value_grad_workspace_floats(n, ...) = bbx_pmlp2_grad_workspace_floats(n, ...) floats: the partition, the float64
 *   recomputation of both pre-activations and the second kernel are bbx_pmlp2_grad's (no floating-point atomics; the partition
 *   depends on n and the shape alone).  A state without live rows or an index out of range: its d_gvalue is not read.
 * bbx_pmlp2_value_fit[_at]: forward with the squared-error epilogue, statistics, gradients; THE GRADIENTS ARE, BIT FOR BIT, THOSE OF
 *   bbx_pmlp2_value_grad[_at] CALLED WITH d_gvalue = d_coef, d_values (may be NULL) that of bbx_pmlp2_value[_at].  d_workspace holds
 *   bbx_pmlp2_value_fit_workspace_floats(n, ...) floats (16-byte aligned): the gradient workspace, then d^2 | V | target | flags, n
 *   each.  d_targets or d_coef NULL with n > 0: BBX_E_ARG; d_stats may be NULL (no statistics kernel is queued; everything else as with it). */
int bbx_pmlp2_value(const int32_t* d_obs, const int32_t* d_rows, int n, int obs_rows, int cols, const float* d_prepared, int hidden1, int hidden2,
                    int pool, float* d_values, double* d_values64, void* stream);
int bbx_pmlp2_value_at(const int32_t* d_obs, const int32_t* d_rows, int n_src, const int32_t* d_index, int n, int obs_rows, int cols,
                       const float* d_prepared, int hidden1, int hidden2, int pool, float* d_values, double* d_values64, void* stream);
int bbx_pmlp2_value_grad_workspace_floats(int n, int obs_rows, int cols, int hidden1, int hidden2);   /* < 0: shape not supported */
int bbx_pmlp2_value_grad(const int32_t* d_obs, const int32_t* d_rows, int n, int obs_rows, int cols, const float* d_prepared, int hidden1, int hidden2,
                         int pool, const float* d_gvalue, float* d_workspace, float* d_gw1, float* d_gb1, float* d_gw2, float* d_gb2, float* d_gw3,
                         float* d_gb3, void* stream);
int bbx_pmlp2_value_grad_at(const int32_t* d_obs, const int32_t* d_rows, int n_src, const int32_t* d_index, int n, int obs_rows, int cols,
                            const float* d_prepared, int hidden1, int hidden2, int pool, const float* d_gvalue, float* d_workspace, float* d_gw1,
                            float* d_gb1, float* d_gw2, float* d_gb2, float* d_gw3, float* d_gb3, void* stream);
int bbx_pmlp2_value_fit_workspace_floats(int n, int obs_rows, int cols, int hidden1, int hidden2);   /* < 0: shape not supported */
int bbx_pmlp2_value_fit(const int32_t* d_obs, const int32_t* d_rows, int n, int obs_rows, int cols, const float* d_prepared, int hidden1, int hidden2,
                        int pool, const float* d_targets, float scale, float* d_values, float* d_coef, double* d_stats, float* d_workspace, float* d_gw1,
                        float* d_gb1, float* d_gw2, float* d_gb2, float* d_gw3, float* d_gb3, void* stream);
int bbx_pmlp2_value_fit_at(const int32_t* d_obs, const int32_t* d_rows, int n_src, const int32_t* d_index, int n, int obs_rows, int cols,
                           const float* d_prepared, int hidden1, int hidden2, int pool, const float* d_targets, float scale, float* d_values,
                           float* d_coef, double* d_stats, float* d_workspace, float* d_gw1, float* d_gb1, float* d_gw2, float* d_gb2, float* d_gw3,
                           float* d_gb3, void* stream);
/* ... and for three hidden layers (hidden_layers=[hidden1, hidden2, hidden3], each <= 128): the same kernel with a middle layer
 * whose output stays in registers as the next layer's B operands; d_w3 [hidden2][hidden3], d_b3 [hidden3], d_w4 [hidden3],
 * d_b4 [1].  All three layers are padded to the widest one's tile size (64 or 128 units). */
int bbx_pmlp3_prepared_floats(int cols, int hidden1, int hidden2, int hidden3);   /* < 0: shape not supported */
int bbx_pmlp3_prepare(const float* d_w1, const float* d_b1, const float* d_w2, const float* d_b2, const float* d_w3, const float* d_b3,
                      const float* d_w4, const float* d_b4, int cols, int hidden1, int hidden2, int hidden3, float* d_prepared, void* stream);
int bbx_pmlp3_act(const int32_t* d_obs, const int32_t* d_rows, int batch, int obs_rows, int cols, const float* d_prepared, int hidden1, int hidden2,
                  int hidden3, const float* d_u, int32_t* d_actions, float* d_logprobs, void* stream);
/* One vector step with the policy in the loop: bbx_pmlp_act on the block the previous call left in d_obs / d_rows, then
 * bbx_step_device_autoreset with the sampled rows as actions, which rewrites d_obs / d_rows (the inner loop of
 * pg.py:451-503 run_episode, batched).  Where the step kernel has the policy built in (the register/LDS-resident class
 * with accounting off, 33..128 hidden units) this is ONE kernel launch; otherwise the two calls it stands for.
 * d_actions and d_logprobs receive what was sampled; arguments as in those two calls. */
int bbx_policy_step_device(bbx_batch* b, const float* d_prepared, int hidden, const float* d_u, int32_t* d_actions, float* d_logprobs,
                           double* d_rewards, uint8_t* d_dones, int32_t* d_rows, int32_t* d_obs, int obs_rows, int obs_fill, void* stream);
/* nsteps vector steps in ONE launch with the policy inside the step kernel (pg.py:451-503 run_episode for a whole batch, no
 * host in the loop and no waiting between environments): at step t every environment writes the observation the policy
 * is about to see to d_obs + t * obs_step_stride (int32 elements; 0 = a single block overwritten every step; rows beyond
 * d_rows[t][e] are not written) and its row count to d_rows[t][e], evaluates the policy, draws the action with d_u[t][e]
 * -> d_actions[t][e], d_logprobs[t][e], takes the step -> d_rewards[t][e], d_dones[t][e]; finished episodes restart
 * (auto-reset).  All per-step arrays are [nsteps][batch]; d_rewards / d_dones / d_rows / d_obs may be null.  Built into the
 * binomial kernel classes (binomial ideals in up to 7 variables, 2nk <= 12 observation columns — <= 20 with more than 3
 * variables —, accounting off, 33..128 hidden units); other batches: BBX_E_UNSUPPORTED (use bbx_policy_step_device).
 * 3 variables with k = 2 run in the register/LDS-resident kernel; environments that outgrow it inside the rollout
 * (|G| > 128 or |P| > 256) are continued, policy included, by the HBM-resident kernel launched right behind, which is
 * also the rollout kernel of every other admitted shape.
 * Batches whose ideals come from the host-side queue (BBX_HOST_GEN, sort_input with more than 16 generators) must hold
 * enough queued ideals for the episodes that end inside the launch (bbx_caps.queue_slots, bbx_prefetch): the host cannot
 * refill in the middle of a launch, and an environment left waiting makes bbx_sync report BBX_E_CAPACITY.
 * Asynchronous like bbx_rollout_device. */
int bbx_policy_rollout_device(bbx_batch* b, const float* d_prepared, int hidden, int nsteps, const float* d_u, int32_t* d_actions,
                              float* d_logprobs, double* d_rewards, uint8_t* d_dones, int32_t* d_rows, int32_t* d_obs, int obs_rows,
                              long long obs_step_stride, void* stream);
/* The same with ParallelMultilayerPerceptron(hidden_layers=[hidden1, hidden2]) (networks.py:562-571: two dense layers in the
 * embedding) choosing every action: d_prepared as bbx_pmlp2_prepare leaves it; arguments and outputs exactly those of
 * bbx_policy_rollout_device, and the draws those of bbx_pmlp2_act in front of bbx_step_device_autoreset (the logits come from the
 * same tile code).  Built into the binomial kernel classes (8-byte monomials with 2nk <= 12 columns, 16-byte ones with 2nk <= 32;
 * at most 128 units per layer); other shapes and classes, accounting on, traced handles or obs_rows > BBX_POLICY_MAX_ROWS:
 * BBX_E_UNSUPPORTED.  3 variables with k = 2 run in the register/LDS-resident kernel (workgroups of 16 waves sharing one LDS
 * copy of the second layer), continued by the HBM-resident kernel as for one layer.  Asynchronous like bbx_rollout_device. */
int bbx_policy2_rollout_device(bbx_batch* b, const float* d_prepared, int hidden1, int hidden2, int nsteps, const float* d_u, int32_t* d_actions,
                               float* d_logprobs, double* d_rewards, uint8_t* d_dones, int32_t* d_rows, int32_t* d_obs, int obs_rows,
                               long long obs_step_stride, void* stream);
/* value() of every environment (bbx_values) on caller-owned device memory, asynchronous: d_values[batch]
 * (double) is valid after the next bbx_sync.  d_seeds: int64 [batch] on the device, needed by "random" only.
 * The baseline of the reference's training loop (pg.py:451-475 with --value_model degree: env.value('degree', gamma) before every
 * step; buchberger.cpp:332-351) without the host in the loop.  The doubles are those of bbx_values_seeded for the same states,
 * bit for bit ("random": seed -> engine state on the device, as std::default_random_engine::seed; d_seeds == NULL with "random":
 * BBX_E_ARG; "sample": BBX_E_UNSUPPORTED, use bbx_values; unknown names select First).
 * The states valued are those of this call's place in `stream` order: behind every *_device call queued before it on that
 * stream, before any queued after it; environments, generator streams, bbx_stats and bbx_kernels_launched are untouched.
 * Only the clone is ordered in `stream`: the rollouts run on a stream of the library's own, in one of BBX_VALUE_RING clone
 * arrays (default 2, read when the handle is created; each costs batch x record bytes of device memory; 1 = no overlap), so
 * they overlap the steps queued behind the call and each other.  A slot is reused behind a device-side wait; the host never
 * waits here.  Any number of calls (at most 8192) may be queued between two bbx_sync, interleaved with the other *_device calls.
 * An environment that sits out a chain of asynchronous steps (bbx_step_device above) is valued in the state it stopped in:
 * bbx_sync returns that chain's error, and its values of the chain are not to be used.
 * A clone that runs out of room stops with its partial return; bbx_sync (or any call that settles the handle) enlarges the
 * records, carries the waiting clones over, finishes them and writes their values — nothing to see, same doubles — as long as
 * no later call has reused its slot (more than BBX_VALUE_RING calls behind it before the wait: BBX_E_CAPACITY naming the
 * environment, NaN in its entry, records enlarged for later calls).  With bbx_caps.no_growth: BBX_E_CAPACITY and NaN.  Never a
 * silently wrong value.  A running persistent session is closed first (device-side); a mailbox session is finished.  While
 * `stream` is capturing: BBX_E_UNSUPPORTED (the ring is host bookkeeping). */
int bbx_values_device(bbx_batch* b, const char* strategy, double gamma, const int64_t* d_seeds,
                      double* d_values, void* stream);
/* GAE over a [nsteps][batch] trajectory block: what DeviceTrajectoryBuffer.finish() computes (pg.py:20-76 per trajectory, episodes
 * end where d_dones is set).  ret = r + gam*nret; adv = ((r - v) + gam*nval) + (gam*lam)*nadv, every product rounded before it
 * is added; d_complete[t] = an episode ends at or after t.  One kernel, one thread per environment; needs no handle;
 * asynchronous on `stream`. */
int bbx_gae_device(const double* d_rewards, const double* d_values, const uint8_t* d_dones, int nsteps, int batch,
                   double gam, double lam, double* d_returns, double* d_advantages, uint8_t* d_complete, void* stream);
/* bbx_gae_device over a block whose episodes the end of the block may have cut (environments stepping in lockstep for a fixed
 * nsteps): truncated-horizon GAE, the same scan in the same kernel body, operation for operation, started from a value of the state
 * BEHIND step nsteps - 1 instead of from zero.
 *   d_last_values [batch] (or NULL): nret = nval = d_last_values[e], nadv = 0, and every step counts as complete (d_complete all
 *     ones).  A done flag clears the carries as before, so the entry of an environment whose last recorded step ended its episode
 *     is never used (under auto-reset its current state belongs to the next episode) — a NaN there reaches no output.  NULL: the
 *     scan starts from zero and d_complete is bbx_gae_device's.
 *   d_lambda_returns [nsteps][batch] (or NULL): adv + v, one rounded sum — the TD(lambda) target of a value fit; with bootstrapped
 *     tails the discounted return d_returns is no longer a pure Monte-Carlo target, and callers have the choice.
 * bbx_gae_device is this call with both NULL: the same bits.  A NULL among the other pointers, nsteps < 0 or batch < 0: BBX_E_ARG;
 * nsteps == 0 or batch == 0: BBX_OK, nothing launched.  One kernel, one thread per environment; needs no handle; asynchronous on
 * `stream`. */
int bbx_gae_bootstrap_device(const double* d_rewards, const double* d_values, const uint8_t* d_dones, int nsteps, int batch,
                             double gam, double lam, const double* d_last_values, double* d_returns, double* d_advantages,
                             uint8_t* d_complete, double* d_lambda_returns, void* stream);
/* Evaluation (run_episodes(..., greedy=True), pg.py; scripts/eval.py): the policy takes the row of the largest logit at every
 * step instead of drawing one.
 * The greedy forms of bbx_pmlp_act, bbx_pmlp2_act and bbx_pmlp3_act: the same arguments without d_u, the same shape refusals, the
 * same row-count convention (n = clamp(d_rows[e], 0, min(obs_rows, BBX_POLICY_MAX_ROWS)); n == 0: action 0, log-probability 0),
 * asynchronous on `stream`.  d_actions[e] = the smallest row whose logit equals the maximum bit for bit; d_logprobs[e] = its
 * log-probability, from the sampler's reductions in the sampler's order: the same bits *_act and *_logprob give for that action. */
int bbx_pmlp_act_greedy(const int32_t* d_obs, const int32_t* d_rows, int batch, int obs_rows, int cols, const float* d_prepared, int hidden,
                        int32_t* d_actions, float* d_logprobs, void* stream);
int bbx_pmlp2_act_greedy(const int32_t* d_obs, const int32_t* d_rows, int batch, int obs_rows, int cols, const float* d_prepared, int hidden1,
                         int hidden2, int32_t* d_actions, float* d_logprobs, void* stream);
int bbx_pmlp3_act_greedy(const int32_t* d_obs, const int32_t* d_rows, int batch, int obs_rows, int cols, const float* d_prepared, int hidden1,
                         int hidden2, int hidden3, int32_t* d_actions, float* d_logprobs, void* stream);
/* A switch of the handle, like bbx_accounting: while it is on, bbx_policy_step_device, bbx_policy_rollout_device and
 * bbx_policy2_rollout_device take the argmax (as the *_act_greedy calls do) and ignore d_u, which may then be NULL; where
 * bbx_policy_step_device stands for two calls, the first is the greedy act.  Nothing else about those calls changes: same
 * outputs, same auto-reset, same step loop.  The mode travels with each launch by value, so a recorded graph keeps the mode it
 * was captured with.  A running persistent session or mailbox session is ended first.  Off when a handle is created. */
int bbx_policy_greedy(bbx_batch* b, int enable);
/* The episode step limit (the reference's max_episode_length).  A switch of the handle, like bbx_policy_greedy: limit = 0 is off
 * (the default), limit < 0 is BBX_E_ARG.  With a limit every call that steps environments ends an episode that has taken `limit`
 * steps and still has pairs: that step reports done = 1 like an ordinary end (dones, the trace record, a mailbox step), under
 * auto-reset the next episode begins as behind an ordinary end, and the episode is counted as an episode and as a truncation
 * (bbx_episode_counts).  An episode whose limit-th step empties the pair set ends ordinarily.  Without auto-reset the environment
 * is left as it is: further steps are taken, each reports done while the episode has `limit` steps or more, and none counts
 * again.  Lowering the limit below a running episode's step count cuts that episode at its next step.  Every reset starts the
 * count at 0; bbx_copy and bbx_clone_envs carry the count (bbx_copy the limit as well).  The value calls (bbx_value, bbx_values,
 * bbx_values_seeded, bbx_values_device, bbx_action_values) ignore the limit: the value of a state is the return of the whole
 * computation.  The limit travels with each launch by value, so a recorded graph keeps the limit it was captured with.  A
 * running persistent session or mailbox session is ended first.  KNOWN LIMITATION, a deviation from "the
 * count travels with the record": the kernels of the headline rollout shape (and the two-layer policy rollout) run the code
 * they ran before the limit existed while it is off, and keep no step count per episode; when a limit is set after such a
 * launch, the episodes under way in the WHOLE batch count from there (count 0).  Replays of a recorded headline launch are
 * noted by bbx_graph_replayed, which does the same on its stream when a limit has been set meanwhile; a recorded two-layer
 * policy rollout replayed under a limit set later is not noted: record it again after setting the limit. */
int bbx_episode_limit(bbx_batch* b, int limit);
/* [batch] each, either may be NULL: episodes ended so far (column 2 of bbx_stats) and how many of them the limit cut.  Ends a
 * running session the way bbx_stats does. */
int bbx_episode_counts(bbx_batch* b, int64_t* episodes, int64_t* truncations);
/* Per-episode returns and lengths from the [nsteps][batch] d_rewards and d_dones a rollout leaves on the device (one return and
 * one length per episode: what run_episodes logs).  Per environment e: acc = d_carry_return[e], len = d_carry_len[e]; for
 * t = 0 .. nsteps - 1: acc += r[t][e] (a plain double add, in step order), len += 1; where d_dones[t][e] is set:
 * d_ep_return[t][e] = acc, d_ep_len[t][e] = len, d_ep_count[e] += 1, acc = len = 0; elsewhere d_ep_return[t][e] = 0.0 and
 * d_ep_len[t][e] = 0.  The carries are written back, so a long evaluation is a chain of chunks.  NULL carries: start from zero,
 * nothing written back; d_ep_count may be NULL.  nsteps == 0 is legal (nothing happens).  nsteps < 0, batch < 1, or NULL
 * d_rewards / d_dones / d_ep_return / d_ep_len with nsteps > 0: BBX_E_ARG.  One kernel, one thread per environment; needs no
 * handle; asynchronous on `stream`. */
int bbx_episodes_device(const double* d_rewards, const uint8_t* d_dones, int nsteps, int batch, double* d_carry_return,
                        int32_t* d_carry_len, int32_t* d_ep_count, double* d_ep_return, int32_t* d_ep_len, void* stream);
/* obs_every_step != 0 materialises the observation in d_obs after every step (what a device-side policy
 * would consume), otherwise only the state at the end of the rollout is written */
int bbx_rollout_device(bbx_batch* b, int agent, int nsteps, int auto_reset, double* d_rewards, uint8_t* d_dones,
                       int32_t* d_rows, int32_t* d_obs, int obs_rows, int obs_fill, int obs_every_step, void* stream);
/* after asynchronous rollouts: waits, refills the ideal queues, finishes environments that had to
 * wait for ideals; returns BBX_E_CAPACITY etc. if any environment failed */
int bbx_sync(bbx_batch* b);

/* ---- persistent sessions ---------------------------------------------------------------------------------------------
 * A launch of K steps ends with its slowest environment (an episode reset costs as much as several steps), so K-step
 * rollouts queued one kernel each leave most of the device idle at the end of every launch: 115 us per 20-step launch for
 * 68 us of work.  With bbx_persistent(b, 1), the first asynchronous bbx_rollout_device call on the register/LDS-resident
 * class (3-variable binomial distributions drawn on the device, Gebauer-Moeller, sorted reducers; built-in agent,
 * auto-reset, lean, untraced, batch <= 4096) starts ONE kernel whose waves keep their environments, and every further
 * call with the same arguments only raises the step total in a device-visible control word; a wave that has taken every
 * step issued so far looks at the word and carries on — environments never wait for each other between calls.  The
 * session ends (its kernel is told to stop after the steps issued, a closing launch takes whatever an environment still
 * owes) with bbx_sync, bbx_join or any other call on the handle; results are those of the same calls as separate
 * launches, bit for bit.  Outputs (rewards / dones / rows / observation block: those of the LAST step) are ready for the
 * caller's stream after bbx_join(b, stream) — device-side: `stream` waits, the host does not — or after bbx_sync.
 * A wave that sees no news for 20 ms leaves by itself (a session never outlives an idle host by more than that). */
int bbx_persistent(bbx_batch* b, int enable);
int bbx_join(bbx_batch* b, void* stream);
/* out5 = {sessions begun, calls that joined a running session, env-steps taken by later kernels of sessions, kernels,
 *         environments that left the register/LDS-resident class (basis beyond 256 elements / 512 pairs) and were continued
 *         by the HBM-resident pass: counted while sessions are enabled} */
int bbx_session_stats(bbx_batch* b, int64_t* out5);
/* Step / reset / observation kernels launched for the handle so far (the kernels of one call: the class's kernel, the
 * continuation pass behind it where the class has one, the second kernel of a wide-class launch of more workgroups than CUs):
 * what a call costs in launches, for tests and for callers who budget them.  No reference counterpart. */
int bbx_kernels_launched(bbx_batch* b, int64_t* out);

/* ---- HIP graphs ---------------------------------------------------------------------------------------------------------
 * The asynchronous device calls (bbx_step_device[_autoreset], bbx_rollout_device, bbx_policy_step_device,
 * bbx_policy_rollout_device) on a batch whose ideals are drawn on the device (or a fixed ideal) only enqueue kernels whose
 * arguments do not depend on host-side counters, so they may be recorded while `stream` is capturing
 * (hipStreamBeginCapture / torch.cuda.graph) together with whatever produces the actions — e.g. a policy of any depth as
 * library GEMMs — and replayed as one graph launch per vector step: the reference's loop `action = policy(state);
 * state, reward, done, _ = env.step(action)` (pg.py:451-465) without a host call per operation.  Launches that would need
 * the host (ideals drawn on the host, persistent sessions, kernel timing) return BBX_E_UNSUPPORTED while capturing.
 * Replays bypass the library, so tell it before the next bbx_sync: bbx_graph_replayed(b, stream) marks the handle as
 * having work in flight on `stream` (the one the graph was replayed on); bbx_sync then waits for it, reports what the
 * replayed steps reported (BBX_E_ACTION, capacities, ...) and continues environments that had to stop, exactly as after
 * the same calls made directly.  One thing invalidates a recording: records enlarged by bbx_sync (an environment outgrew a
 * capacity) live at a new address; the old arrays are kept so that further replays stay harmless, and the next
 * bbx_graph_replayed returns BBX_E_CAPACITY — the steps replayed since did not reach the batch; record the step again. */
int bbx_graph_replayed(bbx_batch* b, void* stream);

/* Algorithmic-byte accounting (stats column 6, the roofline numerator) is on by default; the hand-tuned kernel
 * has a leaner variant without it, selected by bbx_accounting(b, 0).  The count is a property of the workload:
 * bench.py times the lean variant and takes the bytes from an accounting run over a bbx_copy of the same batch. */
int bbx_accounting(bbx_batch* b, int enable);

/* Tops every environment's ring of pre-generated ideals up to queue_slots and uploads them, so that the
 * following rollouts find their inputs resident in HBM (launches themselves only refill EMPTY rings). */
int bbx_prefetch(bbx_batch* b);

/* HIP-event timing of the step-kernel launches on their own stream: returns the milliseconds and launch
 * count accumulated since the previous call, then enables/disables further collection */
int bbx_timing(bbx_batch* b, int enable, double* kernel_ms, int32_t* launches);

/* ---- introspection (tests, checkpoints) -------------------------------------------------------- */
/* per environment 8 values: total_steps, total_additions, episodes, zero_reductions, status,
 * ideals_consumed, algorithmic_bytes (the roofline numerator), basis_size */
int bbx_stats(bbx_batch* b, int64_t* out8);
int bbx_env_status(bbx_batch* b, int32_t* status);
/* the current per-environment capacities (they grow on demand, see bbx_caps.no_growth) and how often they grew:
 * out5 = {max_basis, max_pairs, arena_terms, max_poly_terms, times enlarged} */
int bbx_capacities(bbx_batch* b, int32_t* out5);
int bbx_state_sizes(bbx_batch* b, int idx, int32_t* basis_size, int32_t* npairs, int32_t* nterms_total);
/* G[0..basis_size): nterms[i], then concatenated coefs and exps (8 ints per term); pairs as (i,j);
 * order[r] = index into G of the r-th reducer */
int bbx_state_get(bbx_batch* b, int idx, int32_t* nterms, int32_t* coefs, int32_t* exps, int32_t* pairs, int32_t* order);
/* interreduce(minimalize(G)) of environment idx's basis — the reduced Groebner basis buchberger() returns
 * (buchberger.cpp:102-122, 265) once the environment's pair set is empty; computed on the device (bbx_alg_*).  Call with
 * nterms == NULL for the sizes, then with buffers (nterms[basis_size], coefs/exps[nterms_total(*8)]). */
int bbx_reduced_basis(bbx_batch* b, int idx, int32_t* basis_size, int32_t* nterms_total, int32_t* nterms, int32_t* coefs, int32_t* exps);
int bbx_trace_enable(bbx_batch* b, int capacity_steps);  /* 0 disables */
int bbx_trace_read(bbx_batch* b, int env, int first, int count, bbx_trace_rec* out);

/* ---- ideal generators on their own (reference deepgroebner/ideals.{h,cpp}; host only) ---------- */
typedef struct bbx_gen bbx_gen;
int bbx_gen_create(const char* ideal_dist, bbx_gen** out);
void bbx_gen_destroy(bbx_gen* g);
int bbx_gen_seed(bbx_gen* g, int64_t seed);
int bbx_gen_nvars(const bbx_gen* g);
/* bbx_gen_next draws the next ideal (IdealGenerator::next) and reports its size; bbx_gen_get copies
 * the ideal drawn last: nterms[npolys], coefs[nterms_total], exps[nterms_total*8]; sugars may be NULL */
int bbx_gen_next(bbx_gen* g, int32_t* npolys, int32_t* nterms_total);
int bbx_gen_get(const bbx_gen* g, int32_t* nterms, int32_t* coefs, int32_t* exps, int32_t* sugars);

/* ---- ideals as text (data/stats/<dist>/<dist>.csv lines) ------------------------------------------
 * bbx_parse_ideal reads polynomials such as "413*a^2*b^5*c+32*d^2-5" joined by '|' (parse_polynomial,
 * polynomials.cpp:226-300; parse_ideal_string, scripts/make_strat.cpp:12-19) into the flat layout bbx_create_ideals
 * takes.  It always reports the sizes; with nterms == coefs == exps == NULL it only does that.  Inputs on which the
 * reference has undefined behaviour (variable beyond 'h', zero coefficients, empty polynomials) are BBX_E_ARG.
 * bbx_format_ideal writes the same format (coefficients as signed representatives, the way Macaulay2's make_dist.m2
 * prints them) and returns the length needed excluding the terminator; nothing is written when cap is too small. */
int bbx_parse_ideal(const char* text, int32_t cap_polys, int32_t cap_terms, int32_t* npolys, int32_t* nterms_total,
                    int32_t* nterms, int32_t* coefs, int32_t* exps);
int bbx_format_ideal(int npolys, const int32_t* nterms, const int32_t* coefs, const int32_t* exps, char* out, int cap);

/* ---- the reference's free functions on device-resident lists of polynomials -----------------------------------------
 * spoly / reduce / update (buchberger.cpp:18-99; buchberger.py:11-147), minimalize / interreduce (buchberger.cpp:102-122;
 * buchberger.py:150-166) and Polynomial +, -, * (polynomials.cpp:148-210), batched: a bbx_alg holds `nlists` independent
 * std::vector<Polynomial>s in HBM (flat input like bbx_create_ideals: npolys[nlists], nterms per polynomial, coefs, exps
 * with 8 ints per term; a polynomial may have 0 terms), every call runs one kernel over all lists (one wavefront each) and
 *   - binop / reduce APPEND their result to every list (G.push_back): read it back with bbx_alg_sizes + bbx_alg_get;
 *   - update treats the LAST element of every list as f and the elements before it as G, and rewrites the pair sets;
 *   - minimalize / interreduce REPLACE every list by the result.
 * Records grow on demand.  GF(32003), grevlex, up to 8 variables, polynomials of at most 65535 terms, degrees and sugars of at
 * most 65535.  A call that one list makes fail (a result beyond those limits: BBX_E_CAPACITY) leaves THAT list as it was;
 * the other lists of a binop / reduce may already hold their results — bbx_alg_sizes / bbx_alg_get report every list as it
 * is on the device, and the handle stays usable. */
typedef struct bbx_alg bbx_alg;
int bbx_alg_create(int device, int nlists, const int32_t* npolys, const int32_t* nterms, const int32_t* coefs, const int32_t* exps, bbx_alg** out);
void bbx_alg_destroy(bbx_alg* a);
/* the bases of n environments of a batch (envs == NULL: environments 0..n-1) as n polynomial lists, copied on the device:
 * with bbx_alg_minimalize + bbx_alg_interreduce the reduced Groebner bases of a whole batch of finished runs
 * (scripts/make_strat.cpp of the reference prints their sizes) without the polynomials visiting the host */
int bbx_alg_from_envs(bbx_batch* b, int n, const int32_t* envs, bbx_alg** out);
/* op: 0 = f + g, 1 = f - g, 2 = f * g, 3 = spoly(f, g); ij[nlists][2] = the elements f, g of every list */
int bbx_alg_binop(bbx_alg* a, int op, const int32_t* ij);
/* reduce(g, F) (buchberger.cpp:24-49): dividend_and_ndivisors[nlists][2] = {index of g, n: F = the list's elements 0..n-1 in list
 * order}; the remainder is appended, steps[nlists] (may be NULL) = successful reductions */
int bbx_alg_reduce(bbx_alg* a, const int32_t* dividend_and_ndivisors, int32_t* steps);
/* update(G, P, f, elimination) (buchberger.cpp:52-99): npairs[nlists] + concatenated pairs (i, j) in; npairs_out[nlists] +
 * pairs_out (room for pairs_cap pairs; may be NULL) = the new pair sets in the reference's order */
int bbx_alg_update(bbx_alg* a, int elimination, const int32_t* npairs, const int32_t* pairs, int32_t* npairs_out, int32_t* pairs_out, int pairs_cap);
int bbx_alg_minimalize(bbx_alg* a);
int bbx_alg_interreduce(bbx_alg* a);
int bbx_alg_sizes(bbx_alg* a, int32_t* npolys, int32_t* nterms_total);          /* per list */
int bbx_alg_get(bbx_alg* a, int list, int32_t* nterms, int32_t* coefs, int32_t* exps, int32_t* sugars);   /* sugars may be NULL */

uint32_t bbx_agent_hash(uint32_t seed, uint32_t t);
uint32_t bbx_agent_action(uint32_t seed, uint32_t t, uint32_t rows);   /* (hash * rows) >> 32 */
const char* bbx_last_error(void);
const char* bbx_version(void);

#ifdef __cplusplus
}
#endif
#endif

// libbbx.so — the PMLP policy calls of include/bbx.h: prepared weights, the stand-alone act kernels (one, two and three hidden
// layers), the training calls of policy and critic, policy + step in one call, and policy rollouts inside the step kernels.  Which shapes the kernels are built for is
// stated once, in bbx_pmlp_shape.h: a call is admitted here by the predicates the launchers pick an instantiation with.
#include "bbx_batch.h"
#include "bbx_pmlp_shape.h"

using namespace bbx_host;

namespace {

// what every policy call refuses first: a null argument, arguments out of range (the call's own text), a block taller than
// the kernels score (obs_rows: 0 where the call has none)
int refuse_args(bool null_arg, bool bad, const char* bad_text, int obs_rows) {
  if (null_arg) return fail(BBX_E_ARG, "null argument");
  if (bad) return fail(BBX_E_ARG, "%s", bad_text);
  if (obs_rows > BBX_POLICY_MAX_ROWS) return fail(BBX_E_UNSUPPORTED, "the policy kernels score at most %d rows per environment (obs_rows = %d)", BBX_POLICY_MAX_ROWS, obs_rows);
  return BBX_OK;
}

int launched(int lrc) { return lrc ? fail(BBX_E_DEVICE, "policy launch failed: %s", hipGetErrorString((hipError_t)lrc)) : BBX_OK; }

// the current device, with what the launchers of the deep kernels size themselves by: its CU count and its LDS per workgroup
// (cached: this sits on the per-step path of a policy rollout)
struct Device { int id = 0; DeviceInfo info{}; };
int current_device(Device* d) { HIPCHK(hipGetDevice(&d->id)); HIPCHK(device_info(d->id, &d->info)); return BBX_OK; }
// (hipErrorInvalidValue from such a launcher: the shape needs more LDS than the device has)
int launched_lds(int lrc, const Device& d) {
  if (lrc == (int)hipErrorInvalidValue)
    return fail(BBX_E_UNSUPPORTED, "the policy kernel needs more LDS than device %d has (%d bytes per workgroup)", d.id, d.info.max_lds);
  return launched(lrc);
}

int pmlp_deep_floats(int cols, int h1, int hm, int h2, bool three) {
  if (cols < 1 || cols > 64 || h1 < 1 || h1 > 128 || h2 < 1 || h2 > 128 || (three && (hm < 1 || hm > 128)))
    return three ? fail(BBX_E_UNSUPPORTED, "policy shape %d x %d x %d x %d is not built into the three-layer policy kernel", cols, h1, hm, h2)
                 : fail(BBX_E_UNSUPPORTED, "policy shape %d x %d x %d is not built into the two-layer policy kernel", cols, h1, h2);
  const Pmlp2Pads pd = pmlp2_pads(h1, three ? hm : 0, h2);
  return pmlp2_prepared_floats(cols, pd.hp1, pd.hpm, pd.hp2);
}

int pmlp_deep_act(const int32_t* d_obs, const int32_t* d_rows, int batch, int obs_rows, int cols, const float* d_prepared, int h1, int hm, int h2,
                  bool three, const float* d_u, int32_t* d_actions, float* d_logprobs, void* stream, bool greedy = false) {
  // (greedy: the argmax in place of the draw — d_u is not read)
  if (int rc = refuse_args(!d_obs || !d_rows || !d_prepared || (!d_u && !greedy) || !d_actions || !d_logprobs, batch < 1 || obs_rows < 1, "bad policy shape", obs_rows)) return rc;
  if (pmlp_deep_floats(cols, h1, hm, h2, three) < 0) return BBX_E_UNSUPPORTED;
  Device d;
  if (int rc = current_device(&d)) return rc;
  return launched_lds(bbx_launch_pmlp2_act(d_obs, d_rows, batch, obs_rows, cols, d_prepared, h1, three ? hm : 0, h2, d_u, d_actions, d_logprobs, greedy ? 1 : 0,
                                           d.info.cus, d.info.max_lds, (hipStream_t)stream), d);
}

int pmlp_act(const int32_t* d_obs, const int32_t* d_rows, int batch, int obs_rows, int cols, const float* d_prepared, int hidden, const float* d_u,
             int32_t* d_actions, float* d_logprobs, void* stream, bool greedy) {
  if (int rc = refuse_args(!d_obs || !d_rows || !d_prepared || (!d_u && !greedy) || !d_actions || !d_logprobs, batch < 1 || obs_rows < 1, "bad policy shape", obs_rows)) return rc;
  if (bbx_pmlp_prepared_floats(cols, hidden) < 0) return BBX_E_UNSUPPORTED;
  return launched(bbx_launch_pmlp_act(d_obs, d_rows, batch, obs_rows, cols, d_prepared, hidden, d_u, d_actions, d_logprobs, greedy ? 1 : 0, (hipStream_t)stream));
}

// ---- the training calls of policy and critic: one body per call, for one hidden layer and two, plain and indexed.  What a call
// is about comes as the records of bbx_pmlp_shape.h (PmlpStates, PmlpNet, PmlpGrads); net.layers picks the launcher.

// the shape of a two-layer training call, naming the number that is out of range, then its rows
int refuse_pmlp2_shape(int obs_rows, int cols, int h1, int h2) {
  if (cols < 1 || cols > 64) return fail(BBX_E_UNSUPPORTED, "the two-layer policy kernels take 1..64 columns (cols = %d)", cols);
  if (h1 < 1 || h1 > 128) return fail(BBX_E_UNSUPPORTED, "the two-layer policy kernels take 1..128 units per layer (hidden1 = %d)", h1);
  if (h2 < 1 || h2 > 128) return fail(BBX_E_UNSUPPORTED, "the two-layer policy kernels take 1..128 units per layer (hidden2 = %d)", h2);
  return refuse_args(false, false, "", obs_rows);
}
static_assert(BBX_POOL_SUM == PMLP_POOL_SUM && BBX_POOL_MEAN == PMLP_POOL_MEAN && BBX_POOL_LSE == PMLP_POOL_LSE, "include/bbx.h and bbx_pmlp_shape.h disagree");
// What every training call and workspace query refuses, and in which order: the one statement of it.  null_arg: a pointer the
// call cannot do without is null (its own expression: the arrays of length n may be null when n == 0); pool: a critic's.
//   two layers: the shape — rows above BBX_POLICY_MAX_ROWS, or a cols / hidden1 / hidden2 out of range, the message naming the number:
//               it needs no device and outranks a null pointer, since a caller sizing buffers asks with none; then the index of an
//               _at call (n_src < 0; no index with n > 0); a null argument; "bad policy shape" (n < 0, obs_rows < 1); the pool
//   one layer:  the index of an _at call; a null argument; "bad policy shape"; rows above the limit; the shape
//               (bbx_pmlp_prepared_floats' message); the pool
// so the one-layer workspace query looks at n and obs_rows before the shape, the two-layer one at the shape first.  The PPO and fit
// calls go on from here, alike for both depths: the PPO arguments (refuse_ppo: mode, eps, then the epilogue's null arrays), the
// fit's null arrays, a workspace that would not fit an int.  Nothing is queued before all of it has passed.
int refuse_training(const PmlpStates& s, const PmlpNet& net, bool null_arg, int pool = BBX_POOL_SUM) {
  const bool two = net.layers == 2;
  if (two) { if (int rc = refuse_pmlp2_shape(s.obs_rows, s.cols, net.h1, net.h2)) return rc; }
  if (s.at && s.n_src < 0) return fail(BBX_E_ARG, "bad policy shape (n_src = %d)", s.n_src);
  if (s.at && s.n > 0 && !s.index) return fail(BBX_E_ARG, "null argument");
  if (int rc = refuse_args(null_arg, s.n < 0 || s.obs_rows < 1, "bad policy shape", s.obs_rows)) return rc;
  if (!two && bbx_pmlp_prepared_floats(s.cols, net.h1) < 0) return BBX_E_UNSUPPORTED;
  return pool < BBX_POOL_SUM || pool > BBX_POOL_LSE ? fail(BBX_E_ARG, "bad pool %d (0: sum, 1: mean, 2: log-sum-exp)", pool) : BBX_OK;
}
// the null-argument expressions the calls are made of: the weights and the states' arrays, the gradient outputs
bool no_inputs(const PmlpStates& s, const PmlpNet& net) { return !net.prepared || (s.n > 0 && (!s.obs || !s.rows)); }
bool no_grads(const PmlpNet& net, const PmlpGrads& g) {
  return !g.workspace || !g.gw1 || !g.gb1 || !g.gw2 || !g.gb2 || (net.layers == 2 && (!g.gw3 || !g.gb3));
}
// the floats of the gradient kernels' workspace: of an admitted call, and as the workspace queries answer (or refuse)
int grad_floats(const PmlpStates& s, const PmlpNet& net) {
  return net.layers == 2 ? pmlp2_grad_workspace_floats(s.n, s.cols, net.h1, net.h2) : pmlp_grad_workspace_floats(s.n, s.cols, net.h1);
}
int grad_workspace(int n, int obs_rows, int cols, const PmlpNet& net) {
  const PmlpStates s{nullptr, nullptr, n, nullptr, n, obs_rows, cols, false};
  if (int rc = refuse_training(s, net, false)) return rc;
  return grad_floats(s, net);
}

// The forward and the gradient calls.  Two layers ask for the device (their launchers size themselves by it), and their forward
// calls with n == 0 return before they do; the gradient calls with n == 0 still zero their outputs.
// (loss: the forward kernel of a PPO call, which may leave d_logprobs out)
int pmlp_logprob(const PmlpStates& s, const PmlpNet& net, const int32_t* actions, float* logprobs, float* entropy, void* stream, const PmlpLoss* loss = nullptr) {
  if (int rc = refuse_training(s, net, no_inputs(s, net) || (s.n > 0 && (!actions || (!logprobs && !loss))))) return rc;
  if (net.layers == 1) return launched(bbx_launch_pmlp_logprob(s, net, actions, logprobs, entropy, loss, (hipStream_t)stream));
  if (s.n == 0) return BBX_OK;
  Device d;
  if (int rc = current_device(&d)) return rc;
  return launched_lds(bbx_launch_pmlp2_logprob(s, net, actions, logprobs, entropy, loss, d.info.cus, d.info.max_lds, (hipStream_t)stream), d);
}
int pmlp_grad(const PmlpStates& s, const PmlpNet& net, const int32_t* actions, const float* glogp, const float* gent, const PmlpGrads& g, void* stream) {
  if (int rc = refuse_training(s, net, no_inputs(s, net) || no_grads(net, g) || (s.n > 0 && (!actions || !glogp)))) return rc;
  if (net.layers == 1) return launched(bbx_launch_pmlp_grad(s, net, actions, glogp, gent, g, (hipStream_t)stream));
  Device d;
  if (int rc = current_device(&d)) return rc;
  return launched_lds(bbx_launch_pmlp2_grad(s, net, actions, glogp, gent, g, d.info.max_lds, (hipStream_t)stream), d);
}
// (fit: the forward kernel of a fit call, which may leave both value outputs out)
int pmlp_value(const PmlpStates& s, const PmlpNet& net, int pool, float* values, double* values64, void* stream, const PmlpFit* fit = nullptr) {
  if (int rc = refuse_training(s, net, no_inputs(s, net) || (s.n > 0 && !values && !values64 && !fit), pool)) return rc;
  if (net.layers == 1) return launched(bbx_launch_pmlp_value(s, net, pool, values, values64, fit, (hipStream_t)stream));
  if (s.n == 0) return BBX_OK;
  Device d;
  if (int rc = current_device(&d)) return rc;
  return launched_lds(bbx_launch_pmlp2_value(s, net, pool, values, values64, fit, d.info.cus, d.info.max_lds, (hipStream_t)stream), d);
}
int pmlp_value_grad(const PmlpStates& s, const PmlpNet& net, int pool, const float* gvalue, const PmlpGrads& g, void* stream) {
  if (int rc = refuse_training(s, net, no_inputs(s, net) || no_grads(net, g) || (s.n > 0 && !gvalue), pool)) return rc;
  if (net.layers == 1) return launched(bbx_launch_pmlp_value_grad(s, net, pool, gvalue, g, (hipStream_t)stream));
  Device d;
  if (int rc = current_device(&d)) return rc;
  return launched_lds(bbx_launch_pmlp2_value_grad(s, net, pool, gvalue, g, d.info.max_lds, (hipStream_t)stream), d);
}

// ---- the PPO call: the forward body with the loss epilogue, the statistics kernel, the gradient body on the coefficients the
// epilogue wrote.  Everything either body would refuse is refused here first, before anything is queued
struct PpoArgs {
  const float* old_logprobs; const float* advantages; int mode; float scale, eps, ent_coef, c_kl;
  float* logprobs; float* entropy; float* coef; double* stats;
};
int refuse_ppo(const PpoArgs& a, int n) {
  if (a.mode < 0 || a.mode > 2) return fail(BBX_E_ARG, "bad loss mode %d (0: policy gradient, 1: PPO-clip, 2: PPO-penalty)", a.mode);
  if (!(a.eps >= 0.f)) return fail(BBX_E_ARG, "bad clip range (eps = %g)", (double)a.eps);
  if (n > 0 && (!a.coef || !a.stats || !a.old_logprobs || !a.advantages)) return fail(BBX_E_ARG, "null argument");
  return BBX_OK;
}
int ppo_workspace(int n, int grad_floats) {
  const int fl = pmlp_ppo_workspace_floats(n, grad_floats);
  return fl < 0 ? fail(BBX_E_ARG, "bad policy shape (n = %d: the workspace would not fit an int)", n) : fl;
}
int pmlp_ppo(const PmlpStates& s, const PmlpNet& net, const int32_t* actions, const PpoArgs& a, const PmlpGrads& g, void* stream) {
  if (int rc = refuse_training(s, net, no_inputs(s, net) || no_grads(net, g) || (s.n > 0 && !actions))) return rc;
  if (int rc = refuse_ppo(a, s.n)) return rc;
  const int gfl = grad_floats(s, net);
  if (ppo_workspace(s.n, gfl) < 0) return BBX_E_ARG;
  const PmlpLoss loss{a.old_logprobs, a.advantages, a.coef, g.workspace + gfl, s.n, a.mode, a.scale, a.eps, a.ent_coef, a.c_kl};
  if (int rc = pmlp_logprob(s, net, actions, a.logprobs, a.entropy, stream, &loss)) return rc;
  if (a.stats) { if (int rc = launched(bbx_launch_pmlp_ppo_stats(loss.tail, s.n, a.stats, (hipStream_t)stream))) return rc; }   // (null: n == 0 and none wanted)
  return pmlp_grad(s, net, actions, a.coef, a.coef ? a.coef + s.n : nullptr, g, stream);
}

// ---- cross-entropy against per-row target distributions: the forward body with the cross-entropy epilogue (alone: bbx_pmlp[2]_xent),
// the statistics kernel, the gradient body on the coefficients the epilogue wrote.  What the PPO call refuses is refused here in its
// order; the call's own: a null d_targets (d_coef, d_stats) with n > 0, a scale that is not finite, the workspace's size
struct XentArgs {
  const float* targets; const float* weights; float scale;
  float* losses; float* entropy; float* coef; double* stats;
};
int refuse_xent(const XentArgs& a, int n, bool grad) {
  if (n > 0 && (!a.targets || (grad && (!a.coef || !a.stats)))) return fail(BBX_E_ARG, "null argument");
  if (!(a.scale - a.scale == 0.f)) return fail(BBX_E_ARG, "bad scale (%g: not finite)", (double)a.scale);
  return BBX_OK;
}
int xent_workspace(int n, int grad_floats) {
  const int fl = pmlp_xent_workspace_floats(n, grad_floats);
  return fl < 0 ? fail(BBX_E_ARG, "bad policy shape (n = %d: the workspace would not fit an int)", n) : fl;
}
// (admitted already: the forward launch of either call)
int xent_forward(const PmlpStates& s, const PmlpNet& net, const PmlpXent& x, float* losses, float* entropy, void* stream) {
  if (net.layers == 1) return launched(bbx_launch_pmlp_xent(s, net, x, losses, entropy, (hipStream_t)stream));
  if (s.n == 0) return BBX_OK;
  Device d;
  if (int rc = current_device(&d)) return rc;
  return launched_lds(bbx_launch_pmlp2_xent(s, net, x, losses, entropy, d.info.cus, d.info.max_lds, (hipStream_t)stream), d);
}
int pmlp_xent(const PmlpStates& s, const PmlpNet& net, const XentArgs& a, void* stream) {
  if (int rc = refuse_training(s, net, no_inputs(s, net) || (s.n > 0 && !a.losses))) return rc;
  if (int rc = refuse_xent(a, s.n, false)) return rc;
  return xent_forward(s, net, PmlpXent{a.targets, a.weights, nullptr, nullptr, s.n, a.scale}, a.losses, a.entropy, stream);
}
int pmlp_xent_grad(const PmlpStates& s, const PmlpNet& net, const XentArgs& a, const PmlpGrads& g, void* stream) {
  if (int rc = refuse_training(s, net, no_inputs(s, net) || no_grads(net, g))) return rc;
  if (int rc = refuse_xent(a, s.n, true)) return rc;
  const int gfl = grad_floats(s, net);
  if (xent_workspace(s.n, gfl) < 0) return BBX_E_ARG;
  const PmlpXent x{a.targets, a.weights, a.coef, g.workspace + gfl, s.n, a.scale};
  if (s.n > 0) { if (int rc = xent_forward(s, net, x, a.losses, a.entropy, stream)) return rc; }
  if (a.stats) { if (int rc = launched(bbx_launch_pmlp_xent_stats(x.tail, s.n, a.stats, (hipStream_t)stream))) return rc; }   // (null: n == 0 and none wanted)
  if (net.layers == 1) return launched(bbx_launch_pmlp_xent_grad(s, net, a.targets, a.coef, g, (hipStream_t)stream));
  Device d;
  if (int rc = current_device(&d)) return rc;
  return launched_lds(bbx_launch_pmlp2_xent_grad(s, net, a.targets, a.coef, g, d.info.max_lds, (hipStream_t)stream), d);
}

// ---- the critic's fit call: the forward body with the squared-error epilogue, the statistics kernel, the gradient body on the
// coefficients the epilogue wrote; everything either body would refuse is refused here first
int fit_workspace(int n, int grad_floats) {
  const int fl = pmlp_fit_workspace_floats(n, grad_floats);
  return fl < 0 ? fail(BBX_E_ARG, "bad policy shape (n = %d: the workspace would not fit an int)", n) : fl;
}
int pmlp_value_fit(const PmlpStates& s, const PmlpNet& net, int pool, const float* targets, float scale, float* values, float* coef, double* stats,
                   const PmlpGrads& g, void* stream) {
  if (int rc = refuse_training(s, net, no_inputs(s, net) || no_grads(net, g), pool)) return rc;
  // (one layer owes d_stats; two take a null one for "no statistics wanted" and skip the statistics kernel: include/bbx.h)
  if (s.n > 0 && (!targets || !coef || (net.layers == 1 && !stats))) return fail(BBX_E_ARG, "null argument");
  const int gfl = grad_floats(s, net);
  if (fit_workspace(s.n, gfl) < 0) return BBX_E_ARG;
  const PmlpFit fit{targets, coef, g.workspace + gfl, s.n, scale};
  if (int rc = pmlp_value(s, net, pool, values, nullptr, stream, &fit)) return rc;
  if (stats) { if (int rc = launched(bbx_launch_pmlp_value_stats(fit.tail, s.n, stats, (hipStream_t)stream))) return rc; }
  return pmlp_value_grad(s, net, pool, coef, g, stream);
}

// A policy rollout inside the step kernels, one hidden layer (hidden2 == 0) or two; admit: the call's shape test and its refusals
int policy_rollout(bbx_batch* b, const float* d_prepared, int hidden, int hidden2, int (*admit)(const bbx_batch*, int cols, int h1, int h2),
                   int nsteps, const float* d_u, int32_t* d_actions, float* d_logprobs, double* d_rewards, uint8_t* d_dones, int32_t* d_rows,
                   int32_t* d_obs, int obs_rows, long long obs_step_stride, void* stream) {
  if (int rc = refuse_args(!b || !d_prepared || (!d_u && !b->policy_greedy) || !d_actions || !d_logprobs, nsteps < 1 || (d_obs && obs_rows < 1) || obs_step_stride < 0,
                           "bad rollout arguments", d_obs ? obs_rows : 0)) return rc;
  const int cols = 2 * b->nvars * b->k;
  if (int rc = admit(b, cols, hidden, hidden2)) return rc;
  if (b->accounting) return fail(BBX_E_UNSUPPORTED, "policy rollouts run the lean kernel: call bbx_accounting(b, 0) first");
  if (traced(b)) return fail(BBX_E_UNSUPPORTED, "policy rollouts are not traced");
  if (d_obs && obs_step_stride != 0 && obs_step_stride < (long long)b->B * obs_rows * cols) return fail(BBX_E_ARG, "obs_step_stride smaller than one block");
  HIPCHK(hipSetDevice(b->device)); b->api_epoch++;
  const int greedy = b->policy_greedy ? 1 : 0;
  BbxPolicy pol{d_prepared, hidden, greedy, d_u, d_actions, d_logprobs, 1, d_rewards, d_dones, d_rows, obs_step_stride, b->B, 0, hidden2};
  BbxParams p; fill_params(b, &p);
  p.nsteps = nsteps; p.set_budget = 1; p.agent = BBX_AGENT_EXTERNAL; p.auto_reset = 1;
  p.obs = d_obs; p.obs_rows = d_obs ? obs_rows : 0; p.obs_fill = 0;   // (no block: the kernels size their logits for every row they score)
  p.trace = nullptr; p.policy = &pol;
  // the register/LDS-resident kernel has the policy for 3 variables and k = 2; every other admitted shape runs in the
  // HBM-resident binomial kernel from the start
  pol.rollout = (lean_fast(b) && b->nvars == 3 && b->k == 2) ? 1 : 2;
  return launch(b, p, (hipStream_t)stream, true, true);   // (rows the policy could not score — more than the block or the kernel holds — are an error)
}

// the shape tests: the prepared-weights range, then whether the step kernels of this batch have the policy (bbx_pmlp_shape.h)
int admit_rollout(const bbx_batch* b, int cols, int hidden, int) {
  if (bbx_pmlp_prepared_floats(cols, hidden) < 0) return BBX_E_UNSUPPORTED;
  if (!b->binom || !pmlp_step_has(b->W, cols, hidden))
    return fail(BBX_E_UNSUPPORTED, "policy rollouts are built into the binomial kernel classes only (<= 7 variables, 2nk <= 12 columns, or <= 20 with "
                                   "more than 3 variables; 33..128 hidden units); drive this batch with bbx_policy_step_device");
  return BBX_OK;
}
int admit_rollout2(const bbx_batch* b, int cols, int hidden1, int hidden2) {
  if (bbx_pmlp2_prepared_floats(cols, hidden1, hidden2) < 0) return BBX_E_UNSUPPORTED;
  if (!b->binom || !pmlp2_step_has(b->W, cols, hidden1, hidden2))
    return fail(BBX_E_UNSUPPORTED, "two-layer policy rollouts are built into the binomial kernel classes only (<= 7 variables, 2nk <= 12 columns, or <= 32 with "
                                   "more than 3 variables; <= 128 units per layer); drive this batch with bbx_pmlp2_act and bbx_step_device_autoreset");
  return BBX_OK;
}

}  // namespace

extern "C" {

int bbx_pmlp_prepared_floats(int cols, int hidden) {
  if (cols < 1 || cols > 64 || hidden < 1 || hidden > 256) return fail(BBX_E_UNSUPPORTED, "policy shape %d x %d is not built into the policy kernel", cols, hidden);
  return pmlp_prepared_floats(cols, hidden);
}

int bbx_pmlp_prepare(const float* d_w1, const float* d_b1, const float* d_w2, float b2, int cols, int hidden, float* d_prepared, void* stream) {
  if (!d_w1 || !d_b1 || !d_w2 || !d_prepared) return fail(BBX_E_ARG, "null argument");
  if (bbx_pmlp_prepared_floats(cols, hidden) < 0) return BBX_E_UNSUPPORTED;
  return launched(bbx_launch_pmlp_prepare(d_w1, d_b1, d_w2, b2, cols, hidden, d_prepared, (hipStream_t)stream));
}

int bbx_pmlp_act(const int32_t* d_obs, const int32_t* d_rows, int batch, int obs_rows, int cols, const float* d_prepared, int hidden,
                 const float* d_u, int32_t* d_actions, float* d_logprobs, void* stream) {
  return pmlp_act(d_obs, d_rows, batch, obs_rows, cols, d_prepared, hidden, d_u, d_actions, d_logprobs, stream, false);
}
int bbx_pmlp_act_greedy(const int32_t* d_obs, const int32_t* d_rows, int batch, int obs_rows, int cols, const float* d_prepared, int hidden,
                        int32_t* d_actions, float* d_logprobs, void* stream) {
  return pmlp_act(d_obs, d_rows, batch, obs_rows, cols, d_prepared, hidden, nullptr, d_actions, d_logprobs, stream, true);
}

// ---- the training calls, one hidden layer: fill the records, call the body.  A plain call is about its n states in order; an _at
// call about state d_index[k] of n_src at position k
// the policy as a differentiable function of its weights (bbx_pmlp_grad.h)
int bbx_pmlp_logprob(const int32_t* d_obs, const int32_t* d_rows, const int32_t* d_actions, int n, int obs_rows, int cols, const float* d_prepared,
                     int hidden, float* d_logprobs, float* d_entropy, void* stream) {
  return pmlp_logprob(PmlpStates{d_obs, d_rows, n, nullptr, n, obs_rows, cols}, PmlpNet{d_prepared, 1, hidden}, d_actions, d_logprobs, d_entropy, stream);
}
int bbx_pmlp_logprob_at(const int32_t* d_obs, const int32_t* d_rows, const int32_t* d_actions, int n_src, const int32_t* d_index, int n, int obs_rows,
                        int cols, const float* d_prepared, int hidden, float* d_logprobs, float* d_entropy, void* stream) {
  return pmlp_logprob(PmlpStates{d_obs, d_rows, n_src, d_index, n, obs_rows, cols, true}, PmlpNet{d_prepared, 1, hidden}, d_actions, d_logprobs, d_entropy,
                      stream);
}
int bbx_pmlp_grad_workspace_floats(int n, int obs_rows, int cols, int hidden) { return grad_workspace(n, obs_rows, cols, PmlpNet{nullptr, 1, hidden}); }
int bbx_pmlp_grad(const int32_t* d_obs, const int32_t* d_rows, const int32_t* d_actions, int n, int obs_rows, int cols, const float* d_prepared,
                  int hidden, const float* d_glogp, const float* d_gent, float* d_workspace, float* d_gw1, float* d_gb1, float* d_gw2, float* d_gb2,
                  void* stream) {
  return pmlp_grad(PmlpStates{d_obs, d_rows, n, nullptr, n, obs_rows, cols}, PmlpNet{d_prepared, 1, hidden}, d_actions, d_glogp, d_gent,
                   PmlpGrads{d_workspace, d_gw1, d_gb1, d_gw2, d_gb2}, stream);
}
int bbx_pmlp_grad_at(const int32_t* d_obs, const int32_t* d_rows, const int32_t* d_actions, int n_src, const int32_t* d_index, int n, int obs_rows,
                     int cols, const float* d_prepared, int hidden, const float* d_glogp, const float* d_gent, float* d_workspace, float* d_gw1,
                     float* d_gb1, float* d_gw2, float* d_gb2, void* stream) {
  return pmlp_grad(PmlpStates{d_obs, d_rows, n_src, d_index, n, obs_rows, cols, true}, PmlpNet{d_prepared, 1, hidden}, d_actions, d_glogp, d_gent,
                   PmlpGrads{d_workspace, d_gw1, d_gb1, d_gw2, d_gb2}, stream);
}

// forward, PPO loss and gradients in one call
int bbx_pmlp_ppo_workspace_floats(int n, int obs_rows, int cols, int hidden) {
  const int gfl = bbx_pmlp_grad_workspace_floats(n, obs_rows, cols, hidden);
  return gfl < 0 ? gfl : ppo_workspace(n, gfl);
}
int bbx_pmlp_ppo_grad(const int32_t* d_obs, const int32_t* d_rows, const int32_t* d_actions, int n, int obs_rows, int cols, const float* d_prepared,
                      int hidden, const float* d_old_logprobs, const float* d_advantages, int mode, float scale, float eps, float ent_coef, float c_kl,
                      float* d_logprobs, float* d_entropy, float* d_coef, double* d_stats, float* d_workspace, float* d_gw1, float* d_gb1, float* d_gw2,
                      float* d_gb2, void* stream) {
  return pmlp_ppo(PmlpStates{d_obs, d_rows, n, nullptr, n, obs_rows, cols}, PmlpNet{d_prepared, 1, hidden}, d_actions,
                  PpoArgs{d_old_logprobs, d_advantages, mode, scale, eps, ent_coef, c_kl, d_logprobs, d_entropy, d_coef, d_stats},
                  PmlpGrads{d_workspace, d_gw1, d_gb1, d_gw2, d_gb2}, stream);
}
int bbx_pmlp_ppo_grad_at(const int32_t* d_obs, const int32_t* d_rows, const int32_t* d_actions, int n_src, const int32_t* d_index, int n, int obs_rows,
                         int cols, const float* d_prepared, int hidden, const float* d_old_logprobs, const float* d_advantages, int mode, float scale,
                         float eps, float ent_coef, float c_kl, float* d_logprobs, float* d_entropy, float* d_coef, double* d_stats, float* d_workspace,
                         float* d_gw1, float* d_gb1, float* d_gw2, float* d_gb2, void* stream) {
  return pmlp_ppo(PmlpStates{d_obs, d_rows, n_src, d_index, n, obs_rows, cols, true}, PmlpNet{d_prepared, 1, hidden}, d_actions,
                  PpoArgs{d_old_logprobs, d_advantages, mode, scale, eps, ent_coef, c_kl, d_logprobs, d_entropy, d_coef, d_stats},
                  PmlpGrads{d_workspace, d_gw1, d_gb1, d_gw2, d_gb2}, stream);
}

// cross-entropy against per-row target distributions: the loss alone, and forward, loss, statistics and gradients in one call
int bbx_pmlp_xent(const int32_t* d_obs, const int32_t* d_rows, const float* d_targets, int n, int obs_rows, int cols, const float* d_prepared, int hidden,
                  const float* d_weights, float scale, float* d_losses, float* d_entropy, void* stream) {
  return pmlp_xent(PmlpStates{d_obs, d_rows, n, nullptr, n, obs_rows, cols}, PmlpNet{d_prepared, 1, hidden},
                   XentArgs{d_targets, d_weights, scale, d_losses, d_entropy, nullptr, nullptr}, stream);
}
int bbx_pmlp_xent_at(const int32_t* d_obs, const int32_t* d_rows, const float* d_targets, int n_src, const int32_t* d_index, int n, int obs_rows, int cols,
                     const float* d_prepared, int hidden, const float* d_weights, float scale, float* d_losses, float* d_entropy, void* stream) {
  return pmlp_xent(PmlpStates{d_obs, d_rows, n_src, d_index, n, obs_rows, cols, true}, PmlpNet{d_prepared, 1, hidden},
                   XentArgs{d_targets, d_weights, scale, d_losses, d_entropy, nullptr, nullptr}, stream);
}
int bbx_pmlp_xent_workspace_floats(int n, int obs_rows, int cols, int hidden) {
  const int gfl = bbx_pmlp_grad_workspace_floats(n, obs_rows, cols, hidden);
  return gfl < 0 ? gfl : xent_workspace(n, gfl);
}
int bbx_pmlp_xent_grad(const int32_t* d_obs, const int32_t* d_rows, const float* d_targets, int n, int obs_rows, int cols, const float* d_prepared,
                       int hidden, const float* d_weights, float scale, float* d_losses, float* d_entropy, float* d_coef, double* d_stats,
                       float* d_workspace, float* d_gw1, float* d_gb1, float* d_gw2, float* d_gb2, void* stream) {
  return pmlp_xent_grad(PmlpStates{d_obs, d_rows, n, nullptr, n, obs_rows, cols}, PmlpNet{d_prepared, 1, hidden},
                        XentArgs{d_targets, d_weights, scale, d_losses, d_entropy, d_coef, d_stats}, PmlpGrads{d_workspace, d_gw1, d_gb1, d_gw2, d_gb2}, stream);
}
int bbx_pmlp_xent_grad_at(const int32_t* d_obs, const int32_t* d_rows, const float* d_targets, int n_src, const int32_t* d_index, int n, int obs_rows,
                          int cols, const float* d_prepared, int hidden, const float* d_weights, float scale, float* d_losses, float* d_entropy,
                          float* d_coef, double* d_stats, float* d_workspace, float* d_gw1, float* d_gb1, float* d_gw2, float* d_gb2, void* stream) {
  return pmlp_xent_grad(PmlpStates{d_obs, d_rows, n_src, d_index, n, obs_rows, cols, true}, PmlpNet{d_prepared, 1, hidden},
                        XentArgs{d_targets, d_weights, scale, d_losses, d_entropy, d_coef, d_stats}, PmlpGrads{d_workspace, d_gw1, d_gb1, d_gw2, d_gb2}, stream);
}

// the critic: a pooled value of the row scores, its weight gradients, the squared-error fit (bbx_pmlp_value.h)
int bbx_pmlp_value(const int32_t* d_obs, const int32_t* d_rows, int n, int obs_rows, int cols, const float* d_prepared, int hidden, int pool,
                   float* d_values, double* d_values64, void* stream) {
  return pmlp_value(PmlpStates{d_obs, d_rows, n, nullptr, n, obs_rows, cols}, PmlpNet{d_prepared, 1, hidden}, pool, d_values, d_values64, stream);
}
int bbx_pmlp_value_at(const int32_t* d_obs, const int32_t* d_rows, int n_src, const int32_t* d_index, int n, int obs_rows, int cols,
                      const float* d_prepared, int hidden, int pool, float* d_values, double* d_values64, void* stream) {
  return pmlp_value(PmlpStates{d_obs, d_rows, n_src, d_index, n, obs_rows, cols, true}, PmlpNet{d_prepared, 1, hidden}, pool, d_values, d_values64, stream);
}
int bbx_pmlp_value_grad_workspace_floats(int n, int obs_rows, int cols, int hidden) { return bbx_pmlp_grad_workspace_floats(n, obs_rows, cols, hidden); }
int bbx_pmlp_value_grad(const int32_t* d_obs, const int32_t* d_rows, int n, int obs_rows, int cols, const float* d_prepared, int hidden, int pool,
                        const float* d_gvalue, float* d_workspace, float* d_gw1, float* d_gb1, float* d_gw2, float* d_gb2, void* stream) {
  return pmlp_value_grad(PmlpStates{d_obs, d_rows, n, nullptr, n, obs_rows, cols}, PmlpNet{d_prepared, 1, hidden}, pool, d_gvalue,
                         PmlpGrads{d_workspace, d_gw1, d_gb1, d_gw2, d_gb2}, stream);
}
int bbx_pmlp_value_grad_at(const int32_t* d_obs, const int32_t* d_rows, int n_src, const int32_t* d_index, int n, int obs_rows, int cols,
                           const float* d_prepared, int hidden, int pool, const float* d_gvalue, float* d_workspace, float* d_gw1, float* d_gb1,
                           float* d_gw2, float* d_gb2, void* stream) {
  return pmlp_value_grad(PmlpStates{d_obs, d_rows, n_src, d_index, n, obs_rows, cols, true}, PmlpNet{d_prepared, 1, hidden}, pool, d_gvalue,
                         PmlpGrads{d_workspace, d_gw1, d_gb1, d_gw2, d_gb2}, stream);
}
int bbx_pmlp_value_fit_workspace_floats(int n, int obs_rows, int cols, int hidden) {
  const int gfl = bbx_pmlp_grad_workspace_floats(n, obs_rows, cols, hidden);
  return gfl < 0 ? gfl : fit_workspace(n, gfl);
}
int bbx_pmlp_value_fit(const int32_t* d_obs, const int32_t* d_rows, int n, int obs_rows, int cols, const float* d_prepared, int hidden, int pool,
                       const float* d_targets, float scale, float* d_values, float* d_coef, double* d_stats, float* d_workspace, float* d_gw1,
                       float* d_gb1, float* d_gw2, float* d_gb2, void* stream) {
  return pmlp_value_fit(PmlpStates{d_obs, d_rows, n, nullptr, n, obs_rows, cols}, PmlpNet{d_prepared, 1, hidden}, pool, d_targets, scale, d_values,
                        d_coef, d_stats, PmlpGrads{d_workspace, d_gw1, d_gb1, d_gw2, d_gb2}, stream);
}
int bbx_pmlp_value_fit_at(const int32_t* d_obs, const int32_t* d_rows, int n_src, const int32_t* d_index, int n, int obs_rows, int cols,
                          const float* d_prepared, int hidden, int pool, const float* d_targets, float scale, float* d_values, float* d_coef,
                          double* d_stats, float* d_workspace, float* d_gw1, float* d_gb1, float* d_gw2, float* d_gb2, void* stream) {
  return pmlp_value_fit(PmlpStates{d_obs, d_rows, n_src, d_index, n, obs_rows, cols, true}, PmlpNet{d_prepared, 1, hidden}, pool, d_targets, scale, d_values,
                        d_coef, d_stats, PmlpGrads{d_workspace, d_gw1, d_gb1, d_gw2, d_gb2}, stream);
}

// ---- two and three hidden layers (bbx_pmlp2.hip)
int bbx_pmlp2_prepared_floats(int cols, int hidden1, int hidden2) { return pmlp_deep_floats(cols, hidden1, 0, hidden2, false); }
int bbx_pmlp3_prepared_floats(int cols, int hidden1, int hidden2, int hidden3) { return pmlp_deep_floats(cols, hidden1, hidden2, hidden3, true); }

int bbx_pmlp2_prepare(const float* d_w1, const float* d_b1, const float* d_w2, const float* d_b2, const float* d_w3, const float* d_b3,
                      int cols, int hidden1, int hidden2, float* d_prepared, void* stream) {
  if (!d_w1 || !d_b1 || !d_w2 || !d_b2 || !d_w3 || !d_b3 || !d_prepared) return fail(BBX_E_ARG, "null argument");
  if (bbx_pmlp2_prepared_floats(cols, hidden1, hidden2) < 0) return BBX_E_UNSUPPORTED;
  return launched(bbx_launch_pmlp2_prepare(d_w1, d_b1, nullptr, nullptr, d_w2, d_b2, d_w3, d_b3, cols, hidden1, 0, hidden2, d_prepared, (hipStream_t)stream));
}

int bbx_pmlp2_act(const int32_t* d_obs, const int32_t* d_rows, int batch, int obs_rows, int cols, const float* d_prepared, int hidden1, int hidden2,
                  const float* d_u, int32_t* d_actions, float* d_logprobs, void* stream) {
  return pmlp_deep_act(d_obs, d_rows, batch, obs_rows, cols, d_prepared, hidden1, 0, hidden2, false, d_u, d_actions, d_logprobs, stream);
}
int bbx_pmlp2_act_greedy(const int32_t* d_obs, const int32_t* d_rows, int batch, int obs_rows, int cols, const float* d_prepared, int hidden1, int hidden2,
                         int32_t* d_actions, float* d_logprobs, void* stream) {
  return pmlp_deep_act(d_obs, d_rows, batch, obs_rows, cols, d_prepared, hidden1, 0, hidden2, false, nullptr, d_actions, d_logprobs, stream, true);
}

// ---- the training calls, two hidden layers (bbx_pmlp2_grad.h, bbx_pmlp2_value.h): the same bodies on the weights
// bbx_pmlp2_prepare leaves.  Shapes: those of bbx_pmlp2_act, refused before a device is asked for anything
int bbx_pmlp2_logprob(const int32_t* d_obs, const int32_t* d_rows, const int32_t* d_actions, int n, int obs_rows, int cols, const float* d_prepared,
                      int hidden1, int hidden2, float* d_logprobs, float* d_entropy, void* stream) {
  return pmlp_logprob(PmlpStates{d_obs, d_rows, n, nullptr, n, obs_rows, cols}, PmlpNet{d_prepared, 2, hidden1, hidden2}, d_actions, d_logprobs, d_entropy, stream);
}
int bbx_pmlp2_logprob_at(const int32_t* d_obs, const int32_t* d_rows, const int32_t* d_actions, int n_src, const int32_t* d_index, int n, int obs_rows,
                         int cols, const float* d_prepared, int hidden1, int hidden2, float* d_logprobs, float* d_entropy, void* stream) {
  return pmlp_logprob(PmlpStates{d_obs, d_rows, n_src, d_index, n, obs_rows, cols, true}, PmlpNet{d_prepared, 2, hidden1, hidden2}, d_actions, d_logprobs,
                      d_entropy, stream);
}
int bbx_pmlp2_grad_workspace_floats(int n, int obs_rows, int cols, int hidden1, int hidden2) {
  return grad_workspace(n, obs_rows, cols, PmlpNet{nullptr, 2, hidden1, hidden2});
}
int bbx_pmlp2_grad(const int32_t* d_obs, const int32_t* d_rows, const int32_t* d_actions, int n, int obs_rows, int cols, const float* d_prepared,
                   int hidden1, int hidden2, const float* d_glogp, const float* d_gent, float* d_workspace, float* d_gw1, float* d_gb1, float* d_gw2,
                   float* d_gb2, float* d_gw3, float* d_gb3, void* stream) {
  return pmlp_grad(PmlpStates{d_obs, d_rows, n, nullptr, n, obs_rows, cols}, PmlpNet{d_prepared, 2, hidden1, hidden2}, d_actions, d_glogp, d_gent,
                   PmlpGrads{d_workspace, d_gw1, d_gb1, d_gw2, d_gb2, d_gw3, d_gb3}, stream);
}
int bbx_pmlp2_grad_at(const int32_t* d_obs, const int32_t* d_rows, const int32_t* d_actions, int n_src, const int32_t* d_index, int n, int obs_rows,
                      int cols, const float* d_prepared, int hidden1, int hidden2, const float* d_glogp, const float* d_gent, float* d_workspace,
                      float* d_gw1, float* d_gb1, float* d_gw2, float* d_gb2, float* d_gw3, float* d_gb3, void* stream) {
  return pmlp_grad(PmlpStates{d_obs, d_rows, n_src, d_index, n, obs_rows, cols, true}, PmlpNet{d_prepared, 2, hidden1, hidden2}, d_actions, d_glogp, d_gent,
                   PmlpGrads{d_workspace, d_gw1, d_gb1, d_gw2, d_gb2, d_gw3, d_gb3}, stream);
}

int bbx_pmlp2_ppo_workspace_floats(int n, int obs_rows, int cols, int hidden1, int hidden2) {
  const int gfl = bbx_pmlp2_grad_workspace_floats(n, obs_rows, cols, hidden1, hidden2);
  return gfl < 0 ? gfl : ppo_workspace(n, gfl);
}
int bbx_pmlp2_ppo_grad(const int32_t* d_obs, const int32_t* d_rows, const int32_t* d_actions, int n, int obs_rows, int cols, const float* d_prepared,
                       int hidden1, int hidden2, const float* d_old_logprobs, const float* d_advantages, int mode, float scale, float eps, float ent_coef,
                       float c_kl, float* d_logprobs, float* d_entropy, float* d_coef, double* d_stats, float* d_workspace, float* d_gw1, float* d_gb1,
                       float* d_gw2, float* d_gb2, float* d_gw3, float* d_gb3, void* stream) {
  return pmlp_ppo(PmlpStates{d_obs, d_rows, n, nullptr, n, obs_rows, cols}, PmlpNet{d_prepared, 2, hidden1, hidden2}, d_actions,
                  PpoArgs{d_old_logprobs, d_advantages, mode, scale, eps, ent_coef, c_kl, d_logprobs, d_entropy, d_coef, d_stats},
                  PmlpGrads{d_workspace, d_gw1, d_gb1, d_gw2, d_gb2, d_gw3, d_gb3}, stream);
}
int bbx_pmlp2_ppo_grad_at(const int32_t* d_obs, const int32_t* d_rows, const int32_t* d_actions, int n_src, const int32_t* d_index, int n, int obs_rows,
                          int cols, const float* d_prepared, int hidden1, int hidden2, const float* d_old_logprobs, const float* d_advantages, int mode,
                          float scale, float eps, float ent_coef, float c_kl, float* d_logprobs, float* d_entropy, float* d_coef, double* d_stats,
                          float* d_workspace, float* d_gw1, float* d_gb1, float* d_gw2, float* d_gb2, float* d_gw3, float* d_gb3, void* stream) {
  return pmlp_ppo(PmlpStates{d_obs, d_rows, n_src, d_index, n, obs_rows, cols, true}, PmlpNet{d_prepared, 2, hidden1, hidden2}, d_actions,
                  PpoArgs{d_old_logprobs, d_advantages, mode, scale, eps, ent_coef, c_kl, d_logprobs, d_entropy, d_coef, d_stats},
                  PmlpGrads{d_workspace, d_gw1, d_gb1, d_gw2, d_gb2, d_gw3, d_gb3}, stream);
}

int bbx_pmlp2_xent(const int32_t* d_obs, const int32_t* d_rows, const float* d_targets, int n, int obs_rows, int cols, const float* d_prepared, int hidden1,
                   int hidden2, const float* d_weights, float scale, float* d_losses, float* d_entropy, void* stream) {
  return pmlp_xent(PmlpStates{d_obs, d_rows, n, nullptr, n, obs_rows, cols}, PmlpNet{d_prepared, 2, hidden1, hidden2},
                   XentArgs{d_targets, d_weights, scale, d_losses, d_entropy, nullptr, nullptr}, stream);
}
int bbx_pmlp2_xent_at(const int32_t* d_obs, const int32_t* d_rows, const float* d_targets, int n_src, const int32_t* d_index, int n, int obs_rows, int cols,
                      const float* d_prepared, int hidden1, int hidden2, const float* d_weights, float scale, float* d_losses, float* d_entropy,
                      void* stream) {
  return pmlp_xent(PmlpStates{d_obs, d_rows, n_src, d_index, n, obs_rows, cols, true}, PmlpNet{d_prepared, 2, hidden1, hidden2},
                   XentArgs{d_targets, d_weights, scale, d_losses, d_entropy, nullptr, nullptr}, stream);
}
int bbx_pmlp2_xent_workspace_floats(int n, int obs_rows, int cols, int hidden1, int hidden2) {
  const int gfl = bbx_pmlp2_grad_workspace_floats(n, obs_rows, cols, hidden1, hidden2);
  return gfl < 0 ? gfl : xent_workspace(n, gfl);
}
int bbx_pmlp2_xent_grad(const int32_t* d_obs, const int32_t* d_rows, const float* d_targets, int n, int obs_rows, int cols, const float* d_prepared,
                        int hidden1, int hidden2, const float* d_weights, float scale, float* d_losses, float* d_entropy, float* d_coef, double* d_stats,
                        float* d_workspace, float* d_gw1, float* d_gb1, float* d_gw2, float* d_gb2, float* d_gw3, float* d_gb3, void* stream) {
  return pmlp_xent_grad(PmlpStates{d_obs, d_rows, n, nullptr, n, obs_rows, cols}, PmlpNet{d_prepared, 2, hidden1, hidden2},
                        XentArgs{d_targets, d_weights, scale, d_losses, d_entropy, d_coef, d_stats},
                        PmlpGrads{d_workspace, d_gw1, d_gb1, d_gw2, d_gb2, d_gw3, d_gb3}, stream);
}
int bbx_pmlp2_xent_grad_at(const int32_t* d_obs, const int32_t* d_rows, const float* d_targets, int n_src, const int32_t* d_index, int n, int obs_rows,
                           int cols, const float* d_prepared, int hidden1, int hidden2, const float* d_weights, float scale, float* d_losses,
                           float* d_entropy, float* d_coef, double* d_stats, float* d_workspace, float* d_gw1, float* d_gb1, float* d_gw2, float* d_gb2,
                           float* d_gw3, float* d_gb3, void* stream) {
  return pmlp_xent_grad(PmlpStates{d_obs, d_rows, n_src, d_index, n, obs_rows, cols, true}, PmlpNet{d_prepared, 2, hidden1, hidden2},
                        XentArgs{d_targets, d_weights, scale, d_losses, d_entropy, d_coef, d_stats},
                        PmlpGrads{d_workspace, d_gw1, d_gb1, d_gw2, d_gb2, d_gw3, d_gb3}, stream);
}

int bbx_pmlp2_value(const int32_t* d_obs, const int32_t* d_rows, int n, int obs_rows, int cols, const float* d_prepared, int hidden1, int hidden2, int pool,
                    float* d_values, double* d_values64, void* stream) {
  return pmlp_value(PmlpStates{d_obs, d_rows, n, nullptr, n, obs_rows, cols}, PmlpNet{d_prepared, 2, hidden1, hidden2}, pool, d_values, d_values64, stream);
}
int bbx_pmlp2_value_at(const int32_t* d_obs, const int32_t* d_rows, int n_src, const int32_t* d_index, int n, int obs_rows, int cols,
                       const float* d_prepared, int hidden1, int hidden2, int pool, float* d_values, double* d_values64, void* stream) {
  return pmlp_value(PmlpStates{d_obs, d_rows, n_src, d_index, n, obs_rows, cols, true}, PmlpNet{d_prepared, 2, hidden1, hidden2}, pool, d_values, d_values64,
                    stream);
}
int bbx_pmlp2_value_grad_workspace_floats(int n, int obs_rows, int cols, int hidden1, int hidden2) {
  return bbx_pmlp2_grad_workspace_floats(n, obs_rows, cols, hidden1, hidden2);
}
int bbx_pmlp2_value_grad(const int32_t* d_obs, const int32_t* d_rows, int n, int obs_rows, int cols, const float* d_prepared, int hidden1, int hidden2,
                         int pool, const float* d_gvalue, float* d_workspace, float* d_gw1, float* d_gb1, float* d_gw2, float* d_gb2, float* d_gw3,
                         float* d_gb3, void* stream) {
  return pmlp_value_grad(PmlpStates{d_obs, d_rows, n, nullptr, n, obs_rows, cols}, PmlpNet{d_prepared, 2, hidden1, hidden2}, pool, d_gvalue,
                         PmlpGrads{d_workspace, d_gw1, d_gb1, d_gw2, d_gb2, d_gw3, d_gb3}, stream);
}
int bbx_pmlp2_value_grad_at(const int32_t* d_obs, const int32_t* d_rows, int n_src, const int32_t* d_index, int n, int obs_rows, int cols,
                            const float* d_prepared, int hidden1, int hidden2, int pool, const float* d_gvalue, float* d_workspace, float* d_gw1,
                            float* d_gb1, float* d_gw2, float* d_gb2, float* d_gw3, float* d_gb3, void* stream) {
  return pmlp_value_grad(PmlpStates{d_obs, d_rows, n_src, d_index, n, obs_rows, cols, true}, PmlpNet{d_prepared, 2, hidden1, hidden2}, pool, d_gvalue,
                         PmlpGrads{d_workspace, d_gw1, d_gb1, d_gw2, d_gb2, d_gw3, d_gb3}, stream);
}
int bbx_pmlp2_value_fit_workspace_floats(int n, int obs_rows, int cols, int hidden1, int hidden2) {
  const int gfl = bbx_pmlp2_grad_workspace_floats(n, obs_rows, cols, hidden1, hidden2);
  return gfl < 0 ? gfl : fit_workspace(n, gfl);
}
int bbx_pmlp2_value_fit(const int32_t* d_obs, const int32_t* d_rows, int n, int obs_rows, int cols, const float* d_prepared, int hidden1, int hidden2,
                        int pool, const float* d_targets, float scale, float* d_values, float* d_coef, double* d_stats, float* d_workspace, float* d_gw1,
                        float* d_gb1, float* d_gw2, float* d_gb2, float* d_gw3, float* d_gb3, void* stream) {
  return pmlp_value_fit(PmlpStates{d_obs, d_rows, n, nullptr, n, obs_rows, cols}, PmlpNet{d_prepared, 2, hidden1, hidden2}, pool, d_targets, scale, d_values,
                        d_coef, d_stats, PmlpGrads{d_workspace, d_gw1, d_gb1, d_gw2, d_gb2, d_gw3, d_gb3}, stream);
}
int bbx_pmlp2_value_fit_at(const int32_t* d_obs, const int32_t* d_rows, int n_src, const int32_t* d_index, int n, int obs_rows, int cols,
                           const float* d_prepared, int hidden1, int hidden2, int pool, const float* d_targets, float scale, float* d_values,
                           float* d_coef, double* d_stats, float* d_workspace, float* d_gw1, float* d_gb1, float* d_gw2, float* d_gb2, float* d_gw3,
                           float* d_gb3, void* stream) {
  return pmlp_value_fit(PmlpStates{d_obs, d_rows, n_src, d_index, n, obs_rows, cols, true}, PmlpNet{d_prepared, 2, hidden1, hidden2}, pool, d_targets, scale,
                        d_values, d_coef, d_stats, PmlpGrads{d_workspace, d_gw1, d_gb1, d_gw2, d_gb2, d_gw3, d_gb3}, stream);
}

int bbx_pmlp3_prepare(const float* d_w1, const float* d_b1, const float* d_w2, const float* d_b2, const float* d_w3, const float* d_b3,
                      const float* d_w4, const float* d_b4, int cols, int hidden1, int hidden2, int hidden3, float* d_prepared, void* stream) {
  if (!d_w1 || !d_b1 || !d_w2 || !d_b2 || !d_w3 || !d_b3 || !d_w4 || !d_b4 || !d_prepared) return fail(BBX_E_ARG, "null argument");
  if (bbx_pmlp3_prepared_floats(cols, hidden1, hidden2, hidden3) < 0) return BBX_E_UNSUPPORTED;
  return launched(bbx_launch_pmlp2_prepare(d_w1, d_b1, d_w2, d_b2, d_w3, d_b3, d_w4, d_b4, cols, hidden1, hidden2, hidden3, d_prepared, (hipStream_t)stream));
}

int bbx_pmlp3_act(const int32_t* d_obs, const int32_t* d_rows, int batch, int obs_rows, int cols, const float* d_prepared, int hidden1, int hidden2,
                  int hidden3, const float* d_u, int32_t* d_actions, float* d_logprobs, void* stream) {
  return pmlp_deep_act(d_obs, d_rows, batch, obs_rows, cols, d_prepared, hidden1, hidden2, hidden3, true, d_u, d_actions, d_logprobs, stream);
}
int bbx_pmlp3_act_greedy(const int32_t* d_obs, const int32_t* d_rows, int batch, int obs_rows, int cols, const float* d_prepared, int hidden1, int hidden2,
                         int hidden3, int32_t* d_actions, float* d_logprobs, void* stream) {
  return pmlp_deep_act(d_obs, d_rows, batch, obs_rows, cols, d_prepared, hidden1, hidden2, hidden3, true, nullptr, d_actions, d_logprobs, stream, true);
}

// the handle's policy calls (bbx_policy_step_device, bbx_policy_rollout_device, bbx_policy2_rollout_device) take the argmax
// instead of drawing while this is on: BbxPolicy.greedy of every launch they make.  A running session was begun in the other
// mode: it ends here
int bbx_policy_greedy(bbx_batch* b, int enable) {
  if (!b) return fail(BBX_E_ARG, "null argument");
  HIPCHK(hipSetDevice(b->device)); b->api_epoch++;
  if (b->ps_active) { if (int rc = session_close(b, true, nullptr, false)) return rc; }
  b->policy_greedy = enable != 0;
  return BBX_OK;
}

int bbx_policy_step_device(bbx_batch* b, const float* d_prepared, int hidden, const float* d_u, int32_t* d_actions, float* d_logprobs,
                           double* d_rewards, uint8_t* d_dones, int32_t* d_rows, int32_t* d_obs, int obs_rows, int obs_fill, void* stream) {
  if (int rc = refuse_args(!b || !d_prepared || (!d_u && !b->policy_greedy) || !d_actions || !d_logprobs || !d_rows || !d_obs, obs_rows < 1, "obs_rows must be positive", obs_rows)) return rc;
  HIPCHK(hipSetDevice(b->device)); b->api_epoch++;
  const int cols = 2 * b->nvars * b->k;
  if (bbx_pmlp_prepared_floats(cols, hidden) < 0) return BBX_E_UNSUPPORTED;
  // one launch for policy + step where the step kernel has the policy built in (the register/LDS-resident class, lean
  // variant, 33..128 hidden units, at most 12 columns); everywhere else the two launches it replaces
  if (!(lean_fast(b) && pmlp_fused_step_has(cols, hidden))) {
    int rc = pmlp_act(d_obs, d_rows, b->B, obs_rows, cols, d_prepared, hidden, d_u, d_actions, d_logprobs, stream, b->policy_greedy);
    if (rc) return rc;
    return step_device(b, d_actions, d_rewards, d_dones, d_rows, d_obs, obs_rows, obs_fill, stream, 1);
  }
  HIPCHK(hipSetDevice(b->device)); b->api_epoch++;
  // persistent sessions: the call joins (or begins) a session whose kernel has the policy inside its step loop — the
  // uniforms of consecutive calls must then be consecutive [B] slices of one array (what a rollout loop that draws its
  // random numbers a chunk of steps at a time passes), every other argument the same from call to call
  const bool session = b->ps_enabled && b->nvars == 3 && b->k == 2 && b->device_gen;
  const int greedy = b->policy_greedy ? 1 : 0;
  BbxPolicy pol = session ? BbxPolicy{d_prepared, hidden, greedy, d_u, d_actions, d_logprobs, 1, d_rewards, d_dones, d_rows, 0, 0, 1}
                          : BbxPolicy{d_prepared, hidden, greedy, d_u, d_actions, d_logprobs, 0, nullptr, nullptr, nullptr, 0, 0, 0};
  BbxParams p; fill_params(b, &p);
  p.nsteps = 1; p.set_budget = 1; p.agent = BBX_AGENT_EXTERNAL; p.auto_reset = 1;
  p.obs = d_obs; p.obs_rows = obs_rows; p.obs_fill = obs_fill; p.trace = nullptr;
  if (!session) { p.actions = d_actions; p.rewards = d_rewards; p.dones = d_dones; p.rows = d_rows; }   // (actions: the follow-up pass reads them)
  p.policy = &pol;
  return launch(b, p, (hipStream_t)stream, true, true);
}

int bbx_policy_rollout_device(bbx_batch* b, const float* d_prepared, int hidden, int nsteps, const float* d_u, int32_t* d_actions,
                              float* d_logprobs, double* d_rewards, uint8_t* d_dones, int32_t* d_rows, int32_t* d_obs, int obs_rows,
                              long long obs_step_stride, void* stream) {
  return policy_rollout(b, d_prepared, hidden, 0, admit_rollout, nsteps, d_u, d_actions, d_logprobs, d_rewards, d_dones, d_rows, d_obs, obs_rows,
                        obs_step_stride, stream);
}

// two hidden layers inside the step loop (ParallelMultilayerPerceptron([h1, h2]), networks.py:562-571): the same call with the
// weights bbx_pmlp2_prepare leaves
int bbx_policy2_rollout_device(bbx_batch* b, const float* d_prepared, int hidden1, int hidden2, int nsteps, const float* d_u, int32_t* d_actions,
                               float* d_logprobs, double* d_rewards, uint8_t* d_dones, int32_t* d_rows, int32_t* d_obs, int obs_rows,
                               long long obs_step_stride, void* stream) {
  return policy_rollout(b, d_prepared, hidden1, hidden2, admit_rollout2, nsteps, d_u, d_actions, d_logprobs, d_rewards, d_dones, d_rows, d_obs, obs_rows,
                        obs_step_stride, stream);
}

}  // extern "C"

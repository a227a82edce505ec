// Shapes of the PMLP policy kernels, stated once: the prepared-weight geometry, and which (columns, hidden units) the step kernels
// have a policy built in for.  Plain C++: the host API (bbx_api_policy.cpp) admits a call by the functions the launchers
// (bbx_fast.hip, bbx_binom.hip, bbx_aux.hip, bbx_pmlp2.hip; declared in bbx_launch.h) pick their kernel by (bbx_pick) and the
// kernels (bbx_pmlp.h) are sized with.
#pragma once
#include "bbx_common.h"

// ---- one hidden layer (bbx_pmlp.h: pmlp_tile).  KS = k-steps of two columns built in (>= ceil(cols / 2)), NB = blocks of 32
// hidden units (>= ceil(hidden / 32), a power of two)
BBX_HD constexpr int pmlp_ks_for(int cols) { const int ks = (cols + 1) / 2; return ks <= 3 ? 3 : ks <= 6 ? 6 : ks <= 10 ? 10 : ks <= 16 ? 16 : 32; }
BBX_HD constexpr int pmlp_nb_for(int hidden) { const int nb = (hidden + 31) / 32; return nb <= 1 ? 1 : nb <= 2 ? 2 : nb <= 4 ? 4 : 8; }
// prepared weights (floats): W1p [2 KS][32 NB] | b1p [32 NB] | w2p [32 NB] | b2 | pad to a multiple of 4
BBX_HD constexpr int pmlp_prepared_floats(int cols, int hidden) { return (2 * pmlp_ks_for(cols) + 2) * 32 * pmlp_nb_for(hidden) + 4; }

// ---- one hidden layer, gradients (bbx_pmlp_grad.h).  A wave accumulates dW1 for PMLP_GRAD_UBW unit blocks x CB column blocks
// of 32 (64 accumulator registers at the most); the NB / UBW unit groups are separate waves (blockIdx.y).  The states are
// dealt to pmlp_grad_waves(n) waves per group, wave p taking states p, p + waves, ...: a function of n alone, never of the device.
constexpr int PMLP_GRAD_STATES_PER_WAVE = 4;      // a further wave per this many states ...
constexpr int PMLP_GRAD_MAX_WAVES = 1024;         // ... up to this many per unit group
BBX_HD constexpr int pmlp_grad_cb(int cols) { return pmlp_ks_for(cols) == 32 ? 2 : 1; }
BBX_HD constexpr int pmlp_grad_ubw(int cols, int hidden) {
  const int nb = pmlp_nb_for(hidden), most = pmlp_grad_cb(cols) == 2 ? 2 : 4;
  return nb < most ? nb : most;
}
BBX_HD constexpr int pmlp_grad_waves(int n) {
  const int w = (n + PMLP_GRAD_STATES_PER_WAVE - 1) / PMLP_GRAD_STATES_PER_WAVE;
  return w < 1 ? 1 : w > PMLP_GRAD_MAX_WAVES ? PMLP_GRAD_MAX_WAVES : w;
}
// one wave's partial sums (floats): dW1 [32 CB][32 UBW] | db1 [32 UBW] | dw2 [32 UBW] | db2, pad to a multiple of 4
BBX_HD constexpr int pmlp_grad_partial_floats(int cols, int hidden) { return 32 * pmlp_grad_ubw(cols, hidden) * (32 * pmlp_grad_cb(cols) + 2) + 4; }
BBX_HD constexpr int pmlp_grad_workspace_floats(int n, int cols, int hidden) {
  return pmlp_grad_waves(n) * (pmlp_nb_for(hidden) / pmlp_grad_ubw(cols, hidden)) * pmlp_grad_partial_floats(cols, hidden);
}

// ---- two and three hidden layers (bbx_pmlp.h: pmlp2_tile; bbx_pmlp2.hip)
// prepared weights (floats): W1p [4 KS][HP1] | b1p [HP1] | [AM [HPM / 16][HP1 / 16][64][4]] | A2 [HP2 / 16][HPI / 16][64][4] | [bMp [HPM]] |
// b2p [HP2] | wdp [HP2] | bd, pad          (bracketed: the optional middle hidden layer; HPI = HPM if there is one, else HP1)
// HP = the layer padded to 64 or 128 units, KS = k-steps of four columns built in
BBX_HD constexpr int pmlp2_hp_for(int hidden) { return hidden <= 64 ? 64 : 128; }
BBX_HD constexpr int pmlp2_ks_for(int cols) { const int ks = (cols + 3) / 4; return ks <= 3 ? 3 : ks <= 8 ? 8 : 16; }
BBX_HD constexpr int pmlp2_prepared_floats(int cols, int hp1, int hpm, int hp2) {   // (padded sizes; hpm = 0: two hidden layers)
  return (4 * pmlp2_ks_for(cols) + 1) * hp1 + hp1 * hpm + (hpm ? hpm : hp1) * hp2 + hpm + 2 * hp2 + 4;
}
// padded layer sizes: two hidden layers are padded one by one; with a middle layer all three take the size of the widest
// (one kernel per size instead of eight)
struct Pmlp2Pads { int hp1, hpm, hp2; };
BBX_HD constexpr Pmlp2Pads pmlp2_pads(int h1, int hm, int h2) {
  if (hm == 0) return {pmlp2_hp_for(h1), 0, pmlp2_hp_for(h2)};
  const int hp = pmlp2_hp_for(h1 > hm ? (h1 > h2 ? h1 : h2) : (hm > h2 ? hm : h2));
  return {hp, hp, hp};
}

// ---- two hidden layers, gradients (bbx_pmlp2_grad.h).  A workgroup of pmlp2_grad_waves waves accumulates all six gradients for
// the states p, p + groups, ...; wave w owns units 32 w .. 32 w + 31 of both layers.  pmlp2_grad_groups(n) workgroups, each with
// one slot of partial sums in the workspace: a function of n alone, never of the device.
constexpr int PMLP2_GRAD_STATES_PER_GROUP = 4;    // a further workgroup per this many states ...
constexpr int PMLP2_GRAD_MAX_GROUPS = 512;        // ... up to this many (64 x 128 x 128: 512 slots of 24964 floats, 12.8 M <= 2^24)
BBX_HD constexpr int pmlp2_grad_cb(int cols) { return pmlp2_ks_for(cols) == 16 ? 2 : 1; }   // blocks of 32 columns
BBX_HD constexpr int pmlp2_grad_waves(int hp1, int hp2) { return (hp1 > hp2 ? hp1 : hp2) / 32; }
BBX_HD constexpr int pmlp2_grad_groups(int n) {
  const int g = (n + PMLP2_GRAD_STATES_PER_GROUP - 1) / PMLP2_GRAD_STATES_PER_GROUP;
  return g < 1 ? 1 : g > PMLP2_GRAD_MAX_GROUPS ? PMLP2_GRAD_MAX_GROUPS : g;
}
// one workgroup's partial sums (float offsets; padded sizes, kp = 32 pmlp2_grad_cb(cols)):
// dW1 [kp][hp1] | db1 [hp1] | dW2 [hp1][hp2] | db2 [hp2] | dw3 [hp2] | db3 [4: one per wave]
struct Pmlp2GradLayout { int w1, b1, w2, b2, w3, b3, total; };
BBX_HD constexpr Pmlp2GradLayout pmlp2_grad_layout(int kp, int hp1, int hp2) {
  const int b1 = kp * hp1, w2 = b1 + hp1, b2 = w2 + hp1 * hp2, w3 = b2 + hp2, b3 = w3 + hp2;
  return {0, b1, w2, b2, w3, b3, b3 + 4};
}
BBX_HD constexpr int pmlp2_grad_workspace_floats(int n, int cols, int h1, int h2) {
  return pmlp2_grad_groups(n) * pmlp2_grad_layout(32 * pmlp2_grad_cb(cols), pmlp2_hp_for(h1), pmlp2_hp_for(h2)).total;
}

// ---- the PPO loss between the forward and the gradient kernels (bbx_pmlp.h: pmlp_loss_lane0; bbx_pmlp_ppo_grad of include/bbx.h).
// What the forward kernels' loss epilogue reads and writes, all of length n and addressed by the position k of the call:
// coef [2n] = glogp | gent (what the gradient kernels take), tail [4n] = u | H | old - new | flags (int32: PMLP_LOSS_*), which
// lies in the call's workspace behind the gradient kernels' partial sums and is what the statistics kernel adds up.
struct PmlpLoss {
  const float* old_logprobs; const float* advantages; float* coef; float* tail;
  int n, mode;                                     // mode: 0 policy gradient, 1 PPO-clip, 2 PPO-penalty
  float scale, eps, ent_coef, c_kl;
};
constexpr int PMLP_LOSS_COUNTED = 1, PMLP_LOSS_CLIPPED = 2;
constexpr int PMLP_PPO_TAIL = 4;                  // floats per position behind the gradient workspace
// the statistics kernel: ONE workgroup of this many threads, thread t adding positions t, t + threads, ... in double, then the
// lanes of a wave, then the waves in order: a function of n alone
constexpr int PMLP_PPO_STAT_THREADS = 1024;
// floats of a PPO call's workspace (grad_floats: the gradient kernels' own, a multiple of 4); -1: more than an int holds
BBX_HD constexpr int pmlp_ppo_workspace_floats(int n, int grad_floats) {
  const long long t = (long long)grad_floats + (long long)PMLP_PPO_TAIL * n;
  return t > 0x7fffffffLL ? -1 : (int)t;
}

// ---- cross-entropy against per-row target distributions (bbx_pmlp.h: pmlp_xent_wave; bbx_pmlp_xent[_grad] of include/bbx.h).
// What the forward kernels' cross-entropy epilogue reads and writes: targets [n_src][obs_rows] addressed by the recorded state,
// everything else of length n and addressed by the position k of the call: weights (null: 1), coef [2n] = c | T (what the gradient
// kernels take), tail [5n] = w l | w T | H | w | flags (int32: PMLP_LOSS_COUNTED), which lies in the call's workspace behind the
// gradient kernels' partial sums and is what the statistics kernel adds up.  coef == null (bbx_pmlp_xent, forward only): losses
// and entropy alone.
struct PmlpXent {
  const float* targets; const float* weights; float* coef; float* tail;
  int n;
  float scale;
};
constexpr int PMLP_XENT_TAIL = 5;                 // floats per position behind the gradient workspace
BBX_HD constexpr int pmlp_xent_workspace_floats(int n, int grad_floats) {   // -1: more than an int holds
  const long long t = (long long)grad_floats + (long long)PMLP_XENT_TAIL * n;
  return t > 0x7fffffffLL ? -1 : (int)t;
}
// which epilogue a forward kernel's LOSS instantiation runs: the PPO loss from logprob_k and H_k (lane 0), or the cross-entropy
// over the wave's scores
template <class E> struct PmlpEpilogue { static constexpr bool xent = false; };
template <> struct PmlpEpilogue<PmlpXent> { static constexpr bool xent = true; };

// ---- the critic (bbx_pmlp_value.h; bbx_pmlp_value / bbx_pmlp_value_grad / bbx_pmlp_value_fit of include/bbx.h): the one-layer
// policy's weights and gradient partition, a pool over a state's row scores in place of the softmax (BBX_POOL_* of include/bbx.h)
constexpr int PMLP_POOL_SUM = 0, PMLP_POOL_MEAN = 1, PMLP_POOL_LSE = 2;
// what the forward kernel's fit epilogue reads and writes, all of length n and addressed by the position k of the call:
// coef [n] = scale (V - target) (what the gradient kernel takes), tail [4n] = d^2 | V | target | flags (int32: PMLP_LOSS_COUNTED),
// which lies in the call's workspace behind the gradient kernel's partial sums and is what the statistics kernel adds up
struct PmlpFit {
  const float* targets; float* coef; float* tail;
  int n;
  float scale;
};
constexpr int PMLP_FIT_TAIL = 4;                  // floats per position behind the gradient workspace
BBX_HD constexpr int pmlp_fit_workspace_floats(int n, int grad_floats) {   // -1: more than an int holds
  const long long t = (long long)grad_floats + (long long)PMLP_FIT_TAIL * n;
  return t > 0x7fffffffLL ? -1 : (int)t;
}

// ---- what a training call is about (bbx_pmlp[2]_{logprob, grad, ppo_grad, value, value_grad, value_fit}[_at] of include/bbx.h):
// host-side records, filled by the entry points (bbx_api_policy.cpp) and taken by the training launchers (bbx_launch.h;
// bbx_aux.hip, bbx_pmlp2.hip) — a field has a name where a place in a list of eight float* had none.  What belongs to one head stays an
// argument: actions, glogp, gent (policy); pool, gvalue (critic); PmlpLoss, PmlpFit, PmlpXent (the epilogues)
struct PmlpStates {                                // the recorded states
  const int32_t* obs; const int32_t* rows;         // [n_src] blocks of obs_rows x cols, and their row counts
  int n_src; const int32_t* index;                 // index == null: position k of the call is state k and n_src == n; else state index[k]
  int n, obs_rows, cols;                           // n positions
  bool at;                                         // an _at call, which owes an index when n > 0 (what is refused, never what is launched)
};
struct PmlpNet {                                   // the network: bbx_pmlp_prepare's weights, or bbx_pmlp2_prepare's
  const float* prepared;
  int layers, h1, h2;                              // layers: 1 or 2 (stated, not read off h2: hidden2 = 0 is a two-layer shape to refuse); one layer: h2 = 0
};
struct PmlpGrads {                                 // the gradient outputs
  float* workspace;                                // the partial sums (pmlp[2]_grad_workspace_floats)
  float *gw1, *gb1, *gw2, *gb2, *gw3, *gb3;        // (gw3, gb3: null with one layer)
};

// ---- the policies built into the step kernels
// a rollout with one hidden layer, step kernels of W-word monomials (bbx_binom_policy_kernel; 8-byte monomials with 3 variables
// and k = 2 also bbx_fast_policy_rollout_kernel): 33..128 hidden units, 6 k-steps, or 10 with 16-byte monomials
BBX_HD constexpr bool pmlp_step_has(int W, int cols, int hidden) {
  return (W == 2 || W == 4) && (pmlp_nb_for(hidden) == 2 || pmlp_nb_for(hidden) == 4) && (pmlp_ks_for(cols) == 6 || (W == 4 && pmlp_ks_for(cols) == 10));
}
// ... with two (bbx_binom_policy2_kernel, bbx_fast_policy2_rollout_kernel): <= 128 units per layer, 3 k-steps, or 8 with 16-byte monomials
BBX_HD constexpr bool pmlp2_step_has(int W, int cols, int h1, int h2) {
  return h1 >= 1 && h1 <= 128 && h2 >= 1 && h2 <= 128 && (((W == 2 || W == 4) && pmlp2_ks_for(cols) == 3) || (W == 4 && pmlp2_ks_for(cols) == 8));
}
// policy + one step in one launch, the register/LDS-resident class (bbx_fast_policy_kernel): 33..128 hidden units, <= 12 columns
BBX_HD constexpr bool pmlp_fused_step_has(int cols, int hidden) { return (pmlp_nb_for(hidden) == 2 || pmlp_nb_for(hidden) == 4) && cols >= 1 && cols <= 12; }

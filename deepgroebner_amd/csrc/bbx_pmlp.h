// PMLP policy on the observation block (included by the binomial / fast / aux translation units: the step kernels of
// the binomial classes have the policy built in).
#pragma once
#include "bbx_pmlp_shape.h"

// ------------------------------------------------------------------ the consumer of the observation block: PMLP policy
// The reference's default policy (ParallelMultilayerPerceptron, networks.py:522-571 = ParallelEmbeddingLayer :49-95 with
// one dense layer + ParallelDecidingLayer :414-460) evaluated on the padded observation block and sampled, without the
// block leaving the device:   logit_r = w2 . relu(W1^T x_r + b1) + b2   over the |P| rows of an environment,
// log-softmax over them, and one action drawn by inverse CDF from a caller-supplied uniform number u (so that the
// torch module of deepgroebner_amd/rollout.py reproduces the draw).  fp32 throughout.  One wavefront per environment.
// Padded rows (beyond rows[e]) never reach a logit: the -1 padding the reference masks out (networks.py:94-95, 456-457)
// plays no part.
constexpr int PMLP_MAXROWS = BBX_POLICY_MAX_ROWS;
// logits per wave in LDS: what the caller's block can hold, at most PMLP_MAXROWS
// (no block, obs_rows <= 0 — a policy rollout that keeps no observations: every row the kernels score)
__host__ __device__ constexpr int pmlp_lgcap(int obs_rows) { return obs_rows > 0 && obs_rows < PMLP_MAXROWS ? obs_rows : PMLP_MAXROWS; }
__device__ __forceinline__ float wave_sum_f32(float x) {    // sum over the 64 lanes, valid in lane 63
#define BBX_DPPADD(ctrl, rmask) x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), ctrl, rmask, 0xF, false));
  BBX_DPPADD(0x111, 0xF) BBX_DPPADD(0x112, 0xF) BBX_DPPADD(0x114, 0xF) BBX_DPPADD(0x118, 0xF) BBX_DPPADD(0x142, 0xA) BBX_DPPADD(0x143, 0xC)
#undef BBX_DPPADD
  return x;
}
// inclusive prefix sum over the lanes (every lane; the wave total in lane 63) and the wave maximum (lane 63): the DPP
// doubling sequence — lanes without a source keep `old`, the identity of the operation
__device__ __forceinline__ float wave_max_f32(float x) {
#define BBX_DPPMAX(ctrl, rmask) { const float t_ = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, x), __builtin_bit_cast(int, x), ctrl, rmask, 0xF, false)); x = t_ > x ? t_ : x; }
  BBX_DPPMAX(0x111, 0xF) BBX_DPPMAX(0x112, 0xF) BBX_DPPMAX(0x114, 0xF) BBX_DPPMAX(0x118, 0xF) BBX_DPPMAX(0x142, 0xA) BBX_DPPMAX(0x143, 0xC)
#undef BBX_DPPMAX
  return x;
}
__device__ __forceinline__ float lane63_f32(float x) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 63)); }
// log-softmax over the n logits of one environment (in LDS) and the inverse-CDF draw; lane 0 writes action and
// log-probability; returns the sampled row (wave-uniform)
__device__ __forceinline__ int pmlp_sample(const float* lg, int n, int env, float uu, int32_t* __restrict__ actions, float* __restrict__ logprobs) {
  const int lane = lane_id();
  wave_sync();
  float mx = -3.0e38f;
  for (int r = lane; r < n; r += WAVE) { const float t = lg[r]; mx = t > mx ? t : mx; }
  mx = lane63_f32(wave_max_f32(mx));
  float se = 0.f;
  for (int r = lane; r < n; r += WAVE) se += __expf(lg[r] - mx);
  se = lane63_f32(wave_sum_f32(se));
  const float logz = mx + __logf(se);
  // inverse CDF over the rows in order: the first row whose cumulative probability exceeds u (the last one on round-off)
  const float target = uu * se;
  float run = 0.f; int pick = -1;
  for (int base = 0; base < n; base += WAVE) {
    const int r = base + lane;
    const float e = r < n ? __expf(lg[r] - mx) : 0.f;
    const float c = wave_sum_f32(e);                         // inclusive prefix within the wave
    const uint64_t hit = ballot64(r < n && run + c > target);
    if (hit) { pick = base + (int)__builtin_ctzll(hit); break; }
    run += lane63_f32(c);
  }
  if (pick < 0) pick = n - 1;
  if (lane == 0) { actions[env] = pick; logprobs[env] = lg[pick] - logz; }
  return uni(pick);
}

// maximum, sum of exponentials and log-partition of the n > 0 logits in lg: pmlp_sample's reductions in pmlp_sample's order
struct PmlpSoftmax { float mx, se, logz; };
__device__ __forceinline__ PmlpSoftmax pmlp_softmax_wave(const float* lg, int n, int lane) {
  float mx = -3.0e38f;
  for (int r = lane; r < n; r += WAVE) { const float t = lg[r]; mx = t > mx ? t : mx; }
  mx = lane63_f32(wave_max_f32(mx));
  float se = 0.f;
  for (int r = lane; r < n; r += WAVE) se += __expf(lg[r] - mx);
  se = lane63_f32(wave_sum_f32(se));
  const float logz = mx + __logf(se);
  return {mx, se, logz};
}
// The greedy pick in place of the draw (evaluation: run_episodes(greedy=True), pg.py): the row of the largest logit, the first
// one on ties.  The same reductions in the same order as pmlp_sample, so lg[pick] - logz is, for that action, what the sampler
// and the log-probability kernels give, bit for bit.  The row is found by comparing BITS with the maximum (which is one of the
// logits, carried through compares and selects only): lane-strided, one ballot per 64 rows, the first group that hits ends the
// search; nothing is recomputed in floating point.  Lane 0 writes action and log-probability; returns the row (wave-uniform).
__device__ __forceinline__ int pmlp_greedy(const float* lg, int n, int env, int32_t* __restrict__ actions, float* __restrict__ logprobs) {
  const int lane = lane_id();
  wave_sync();
  if (n <= 0) { if (lane == 0) { actions[env] = 0; logprobs[env] = 0.f; } return 0; }
  const PmlpSoftmax sm = pmlp_softmax_wave(lg, n, lane);
  const uint32_t mxb = __builtin_bit_cast(uint32_t, sm.mx);
  int pick = 0;                                              // (no row matches: every logit is a NaN)
  for (int base = 0; base < n; base += WAVE) {
    const int r = base + lane;
    const uint64_t hit = ballot64(r < n && __builtin_bit_cast(uint32_t, lg[r]) == mxb);
    if (hit) { pick = base + (int)__builtin_ctzll(hit); break; }
  }
  if (lane == 0) { actions[env] = pick; logprobs[env] = lg[pick] - sm.logz; }
  return uni(pick);
}
// what every policy kernel ends with: the draw from uu, or (greedy != 0, wave-uniform: a kernel argument or BbxPolicy.greedy,
// so it travels by value and a recorded graph keeps the mode it was captured with) the argmax, which does not look at uu
__device__ __forceinline__ int pmlp_pick(const float* lg, int n, int env, float uu, int greedy, int32_t* __restrict__ actions, float* __restrict__ logprobs) {
  return greedy ? pmlp_greedy(lg, n, env, actions, logprobs) : pmlp_sample(lg, n, env, uu, actions, logprobs);
}
// H = log(se) - (sum_r e_r (z_r - mx)) / se
__device__ __forceinline__ float pmlp_entropy_wave(const float* lg, int n, int lane, const PmlpSoftmax& sm) {
  float sd = 0.f;
  for (int r = lane; r < n; r += WAVE) { const float d = lg[r] - sm.mx; sd += __expf(d) * d; }
  sd = lane63_f32(wave_sum_f32(sd));
  return __logf(sm.se) - sd / sm.se;
}
// the policy gradient's coefficient of row r in dL/dz:   g_r = gl (delta_{r,a} - p_r) - ge p_r (log p_r + H)
// with t = z_r, p_r = exp(t - mx) rse (rse = 1.f / se) and log p_r = t - logz; the one- and the two-layer gradient kernels write it
// over the logits in LDS
__device__ __forceinline__ float pmlp_policy_coef(float t, bool is_a, const PmlpSoftmax& sm, float H, float gl, float ge, float rse) {
  const float pr = __expf(t - sm.mx) * rse;
  return gl * ((is_a ? 1.f : 0.f) - pr) - ge * pr * ((t - sm.logz) + H);
}

// The loss epilogue of the forward kernels (their LOSS instantiations: bbx_pmlp_ppo_grad, bbx_pmlp2_ppo_grad), called by lane 0
// once a wave has logprob_k and H_k of position k: the coefficients dL/dlogprob_k, dL/dH_k of
//   L = -scale sum_k u_k - scale ent_coef sum_k H_k
// for the gradient kernels, and u_k, H_k, old_k - new_k and the flags for the statistics kernel.  float32, in this order, no
// contraction into fused multiply-adds: the same inputs give the same bits whatever the compiler makes of the callers.
// A NaN log-probability (index out of range, action outside the live rows) is not counted: zeros everywhere.
__device__ __forceinline__ void pmlp_loss_lane0(const PmlpLoss& L, int k, float logprob, float H) {
#pragma clang fp contract(off)
  const size_t n = (size_t)L.n;
  float gl = 0.f, ge = 0.f, u = 0.f, h = 0.f, dk = 0.f;
  int flags = 0;
  if (logprob == logprob) {
    const float nw = logprob, old = L.old_logprobs[k], A = L.advantages[k];
    const float d = nw - old, r = __expf(d), sA = L.scale * A;
    flags = PMLP_LOSS_COUNTED;
    dk = old - nw;
    h = H;
    if (L.mode == 0) { u = nw * A; gl = -sA; }
    else if (L.mode == 1) {
      const float lo = 1.f - L.eps, hi = 1.f + L.eps;
      const float a = r * A, b = fminf(fmaxf(r, lo), hi) * A;
      u = fminf(a, b);
      if (a <= b) gl = -(sA * r); else flags |= PMLP_LOSS_CLIPPED;
    } else { u = r * A - L.c_kl * dk; gl = -(sA * r) - L.scale * L.c_kl; }
    ge = -(L.scale * L.ent_coef);
  }
  L.coef[k] = gl; L.coef[n + k] = ge;
  L.tail[k] = u; L.tail[n + k] = h; L.tail[2 * n + k] = dk; ((int*)L.tail)[3 * n + k] = flags;
}
// ... with the kernels' own two outputs, either of which a PPO call may leave out
__device__ __forceinline__ void pmlp_loss_out(const PmlpLoss& L, float* logprobs, float* entropy, int k, float logprob, float H) {
  if (logprobs) logprobs[k] = logprob;
  if (entropy) entropy[k] = H;
  pmlp_loss_lane0(L, k, logprob, H);
}

// The cross-entropy epilogue of the forward kernels (their PmlpXent instantiations: bbx_pmlp_xent[_grad], bbx_pmlp2_xent[_grad]):
// position k of the call against the target row t_r = targets[s][r] of its recorded state, r < n alone (what lies beyond the live
// rows, the NaN padding of action values included, is never read into anything):
//   T = sum_r t_r    sd = sum_r t_r (z_r - mx)    l = T log(se) - sd  (= -sum_r t_r log p_r)    c = scale w_k
// float32, lane-strided and then the wave sum (pmlp_entropy_wave's pattern), no contraction into fused multiply-adds.  What lane 0
// writes: losses[k] = l, entropy[k] = H (either may be null), and for the gradient and the statistics kernels coef[k] = c,
// coef[n + k] = T, tail = w l | w T | H | w | flags.  NOT COUNTED — zeros everywhere, l = NaN: an index out of range (H = NaN
// too), a live t_r that is negative or not finite, a weight that is not finite.  No live row: counted, l = H = T = 0.
__device__ __forceinline__ void pmlp_xent_lane0(const PmlpXent& X, float* losses, float* entropy, int k, bool in_src, bool bad, float T, float l, float H) {
#pragma clang fp contract(off)
  const size_t n = (size_t)X.n;
  const float w = X.weights ? X.weights[k] : 1.f;
  const bool counted = in_src && !bad && (__builtin_bit_cast(uint32_t, w) & 0x7f800000u) != 0x7f800000u;
  if (losses) losses[k] = counted ? l : __builtin_nanf("");
  if (entropy) entropy[k] = in_src ? H : __builtin_nanf("");
  if (!X.coef) return;
  float c = 0.f, tt = 0.f, wl = 0.f, wt = 0.f, h = 0.f, ww = 0.f;
  int flags = 0;
  if (counted) { c = X.scale * w; tt = T; wl = w * l; wt = w * T; h = H; ww = w; flags = PMLP_LOSS_COUNTED; }
  X.coef[k] = c; X.coef[n + k] = tt;
  X.tail[k] = wl; X.tail[n + k] = wt; X.tail[2 * n + k] = h; X.tail[3 * n + k] = ww; ((int*)X.tail)[4 * n + k] = flags;
}
// ... behind the n > 0 scores of the wave's state in lg; tg: the state's target row
__device__ __forceinline__ void pmlp_xent_wave(const PmlpXent& X, float* losses, float* entropy, int k, const float* __restrict__ tg, const float* lg, int n,
                                               int lane, const PmlpSoftmax& sm) {
#pragma clang fp contract(off)
  float T = 0.f, sd = 0.f;
  bool bad = false;
  for (int r = lane; r < n; r += WAVE) {
    const float t = tg[r];
    bad |= !(t >= 0.f && t < __builtin_inff());
    T += t; sd += t * (lg[r] - sm.mx);
  }
  T = lane63_f32(wave_sum_f32(T));
  sd = lane63_f32(wave_sum_f32(sd));
  const bool anybad = ballot64(bad) != 0;
  const float H = pmlp_entropy_wave(lg, n, lane, sm);
  const float l = T * __logf(sm.se) - sd;
  if (lane == 0) pmlp_xent_lane0(X, losses, entropy, k, true, anybad, T, l, H);
}
// the cross-entropy's coefficient of row r in dL/dz:   g_r = c (T p_r - t_r),   p_r = __expf(z_r - mx) rse, with trse = T * rse (one
// rounded product per state) and T p_r - t_r as ONE fused multiply-add of trse and the exponential.  That is how the policy's
// delta_{r,a} - p_r comes out of pmlp_policy_coef (the compiler contracts its product into the subtraction), so a one-hot target
// row (T = 1.f exactly, trse = rse) leaves the policy gradient's (-c) (delta_{r,a} - p_r) bit for bit; nothing else is contracted
__device__ __forceinline__ float pmlp_xent_coef(float z, float t, const PmlpSoftmax& sm, float c, float trse) {
#pragma clang fp contract(off)
  return c * __builtin_fmaf(trse, __expf(z - sm.mx), -t);
}

// The hidden layer on the matrix cores, exact f32 (v_mfma_f32_32x32x2_f32 = an fmaf chain), everything in registers: a
// tile is 32 hidden units x 32 rows of the block, D[unit][row] = sum_k W1[k][unit] x[row][k] + b1[unit]:
//   A operand  lane l: W1[2s + (l >> 5)][unit = 32 nb + (l & 31)]        (coalesced loads, the same for every wave: L1)
//   B operand  lane l: x[row = r0 + (l & 31)][2s + (l >> 5)]             (KS loads per lane)
//   C / D      lane l, register v: unit 32 nb + (v & 3) + 8 (v >> 2) + 4 (l >> 5), row r0 + (l & 31); starts at b1[unit]
// so that a ROW's hidden vector lies along the registers of the two lanes l and l + 32: relu and the dot with w2 are
// in-lane multiply-adds over the accumulator registers and one exchange between the wave's halves finishes the logit —
// no cross-lane reduction tree, no LDS staging, no barrier.  The weights come PREPARED (bbx_pmlp_prepare: zero-padded to
// 2 KS x 32 NB, so every load is unconditional at a compile-time offset), and nothing the first tile needs depends on
// another load: row count, uniform number, rows (read without knowing the count: the block holds obs_rows rows whatever
// it means) and weights are all requested before the first wait — at four waves per SIMD a dependent trip to memory
// costs more than the arithmetic of a tile.
// KS = k-steps built in (>= ceil(cols / 2)), NB = unit blocks (>= ceil(hidden / 32), a power of two).
typedef float bbx_f32x16 __attribute__((ext_vector_type(16)));
typedef float bbx_f32x4 __attribute__((ext_vector_type(4)));
// (the built-in k-step and unit-block counts and the prepared layout: bbx_pmlp_shape.h)
// one tile: the logit (without b2) of row (lane & 31) from the lane's B operands xa[]; G unit blocks in flight together
// (registers: 32 G + G KS)
// (WP: where the prepared weights live — `const float*` in memory, or an LDS pointer when a rollout kernel has staged them
// once per launch)
template <int NB, int KS, int G, class WP = const float*>
__device__ __forceinline__ float pmlp_tile(const float (&xa)[KS], WP wp, int lr, int lk) {
  constexpr int HP = 32 * NB;
  const WP b1p = wp + 2 * KS * HP;
  const WP w2p = b1p + HP;
  const WP wl = wp + lk * HP + lr;                          // my A-operand column: + 2 s HP + 32 nb
  float part = 0.f;
#pragma clang loop unroll(disable)
  for (int g0 = 0; g0 < NB; g0 += G) {
    bbx_f32x16 acc[G];
    bbx_f32x4 wv[G][4];
    float wa[G][KS];
#pragma unroll
    for (int j = 0; j < G; j++) {
      const int ub = (g0 + j) * 32 + 4 * lk;                 // + (v & 3) + 8 (v >> 2): the units of my accumulator registers
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const WP bp = b1p + ub + 8 * q, vp = w2p + ub + 8 * q;
        acc[j][4 * q] = bp[0]; acc[j][4 * q + 1] = bp[1]; acc[j][4 * q + 2] = bp[2]; acc[j][4 * q + 3] = bp[3];   // (one 16-byte load)
        bbx_f32x4 w4; w4.x = vp[0]; w4.y = vp[1]; w4.z = vp[2]; w4.w = vp[3];
        wv[j][q] = w4;
      }
#pragma unroll
      for (int s2 = 0; s2 < KS; s2++) wa[j][s2] = wl[2 * s2 * HP + (g0 + j) * 32];
    }
#pragma unroll
    for (int s2 = 0; s2 < KS; s2++)
#pragma unroll
      for (int j = 0; j < G; j++) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[j][s2], xa[s2], acc[j], 0, 0, 0);
#pragma unroll
    for (int j = 0; j < G; j++)
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const bbx_f32x4 w = wv[j][q];
        const float h0 = acc[j][4 * q], h1 = acc[j][4 * q + 1], h2 = acc[j][4 * q + 2], h3 = acc[j][4 * q + 3];
        part = fmaf(h0 > 0.f ? h0 : 0.f, w.x, part); part = fmaf(h1 > 0.f ? h1 : 0.f, w.y, part);
        part = fmaf(h2 > 0.f ? h2 : 0.f, w.z, part); part = fmaf(h3 > 0.f ? h3 : 0.f, w.w, part);
      }
  }
  return part + __shfl_xor(part, 32, WAVE);                  // the other half of the row's units
}
// the logits of one state or environment into lg (the wave's LDS array); returns the live row count.  The one row loop of every
// one-layer kernel: the stand-alone and built-in policies (pmlp_act_wave) and the log-probability, value and gradient kernels
// (bbx_pmlp_grad.h, bbx_pmlp_value.h) score a block with the same bits.  nraw = rows[...] as loaded: the caller requests it (and
// whatever else it needs from memory) in front of the call, and the count is first looked at behind the first tile
template <int NB, int KS>
__device__ __forceinline__ int pmlp_logits_wave(float* lg, const int32_t* __restrict__ ob, int nraw, int obs_rows, int cols, const float* __restrict__ wp,
                                                int lr, int lk) {
  constexpr int HP = 32 * NB;
  constexpr int G = (KS <= 10 ? 2 : 1) < NB ? (KS <= 10 ? 2 : 1) : NB;   // unit blocks in flight together
  const float b2 = wp[(size_t)(2 * KS + 2) * HP];
  int n = 0;
  for (int r0 = 0;; r0 += 32) {
    int r = r0 + lr; r = r < obs_rows ? r : obs_rows - 1;    // inside the block whatever the row count is
    const int32_t* xr = ob + (size_t)r * cols;
    float xa[KS];
#pragma unroll
    for (int s2 = 0; s2 < KS; s2++) {
      const int k = 2 * s2 + lk;
      const int32_t xi = xr[k < cols ? k : 0];
      xa[s2] = k < cols ? (float)xi : 0.f;
    }
    const float logit = pmlp_tile<NB, KS, G>(xa, wp, lr, lk);
    if (r0 == 0) { n = uni(nraw); n = n < obs_rows ? n : obs_rows; n = n < PMLP_MAXROWS ? n : PMLP_MAXROWS; }
    if (lk == 0 && r0 + lr < n) lg[r0 + lr] = logit + b2;
    if (r0 + 32 >= n) break;
  }
  return n;
}
template <int NB, int KS>
__device__ __forceinline__ int pmlp_act_wave(char* smem, int env, bool live, const int32_t* __restrict__ obs, const int32_t* __restrict__ rows,
                                             int obs_rows, int cols, const float* __restrict__ wp, const float* __restrict__ u,
                                             int32_t* __restrict__ actions, float* __restrict__ logprobs, int greedy = 0) {
  const int lane = lane_id(), wave = uni((int)(threadIdx.x / WAVE));
  float* lg = (float*)smem + (size_t)wave * pmlp_lgcap(obs_rows);   // logits of this wave's environment
  if (!live) return 0;
  const int nraw = rows[env];
  const float uu = greedy ? 0.f : u[env];                   // (greedy: u is not read and may be null)
  const int n = pmlp_logits_wave<NB, KS>(lg, obs + (size_t)env * obs_rows * cols, nraw, obs_rows, cols, wp, lane & 31, lane >> 5);
  if (n <= 0) { if (lane == 0) { actions[env] = 0; logprobs[env] = 0.f; } return 0; }
  wave_sync();
  return pmlp_pick(lg, n, env, uu, greedy, actions, logprobs);
}
template <int NB, int KS>
__global__ __launch_bounds__(256, 4) void bbx_pmlp_act_mfma_kernel(const int32_t* __restrict__ obs, const int32_t* __restrict__ rows, int B, int obs_rows,
                                                                   int cols, const float* __restrict__ wp, const float* __restrict__ u,
                                                                   int32_t* __restrict__ actions, float* __restrict__ logprobs, int greedy) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int env = blockIdx.x * ((int)blockDim.x / WAVE) + (int)(threadIdx.x / WAVE);
  pmlp_act_wave<NB, KS>(smem, env, env < B, obs, rows, obs_rows, cols, wp, u, actions, logprobs, greedy);
}
// LDS bytes of pmlp_act_wave for a workgroup of `waves` waves (the logits)
__host__ __device__ constexpr size_t pmlp_lds_bytes(int waves, int obs_rows) { return (size_t)waves * pmlp_lgcap(obs_rows) * sizeof(float); }

// ------------------------------------------------------------------ two and three hidden layers
// The scoring of one 16-row tile by ParallelMultilayerPerceptron(hidden_layers=[h1, h2]) or [h1, hm, h2] (networks.py:562-571;
// operand mapping and weight layout: bbx_pmlp2.hip), shared by the stand-alone kernel (bbx_pmlp2_act_kernel) and the policy
// rollouts inside the step kernels (fast_body POL2, bbx_fast.h; binom_body POL2, bbx_binom.h): one code for all of them, so
// that a logit computed inside a step kernel is bit-identical to the stand-alone kernel's.
// The prepared weights and the padding of the layers (HP = 64 or 128 units, KS = k-steps of four columns): bbx_pmlp_shape.h.

// one hidden layer behind the first: hout = relu(b + A hin) (LAST = false) or the deciding layer's dot over it (LAST = true:
// returns this lane's share of the logit).  Two blocks of 16 units in flight, their A operands requested half a block pair ahead
// (NPART = 2; NPART = NKI: one k-group ahead — 24 registers fewer at 128 units, for the step kernels, whose own state stays live
// around the tile; the MFMAs and their order, hence every result bit, are the same).
template <int NKI, int NKO, bool LAST, int NPART = 2>
__device__ __forceinline__ float pmlp2_hidden(const bbx_f32x4 (&hin)[NKI], bbx_f32x4* hout, const float* A, const float* bl, const float* wl,
                                              int lane, int lg4) {
  constexpr int HS = NKI / NPART;
  float part = 0.f;
  auto pair = [&](int b2i) __attribute__((always_inline)) {
    bbx_f32x4 acc0 = *(const bbx_f32x4*)(bl + 16 * b2i + 4 * lg4), acc1 = *(const bbx_f32x4*)(bl + 16 * b2i + 16 + 4 * lg4);
    const bbx_f32x4* ap = (const bbx_f32x4*)A + (size_t)b2i * NKI * 64 + lane;
#pragma unroll
    for (int hf = 0; hf < NPART; hf++) {
      bbx_f32x4 av0[HS], av1[HS];
#pragma unroll
      for (int q = 0; q < HS; q++) { av0[q] = ap[(hf * HS + q) * 64]; av1[q] = ap[(NKI + hf * HS + q) * 64]; }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int q = 0; q < HS; q++) {
        const bbx_f32x4 hb = hin[hf * HS + q];
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av0[q].x, hb.x, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av1[q].x, hb.x, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av0[q].y, hb.y, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av1[q].y, hb.y, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av0[q].z, hb.z, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av1[q].z, hb.z, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av0[q].w, hb.w, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av1[q].w, hb.w, acc1, 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    acc0.x = acc0.x > 0.f ? acc0.x : 0.f; acc0.y = acc0.y > 0.f ? acc0.y : 0.f; acc0.z = acc0.z > 0.f ? acc0.z : 0.f; acc0.w = acc0.w > 0.f ? acc0.w : 0.f;
    acc1.x = acc1.x > 0.f ? acc1.x : 0.f; acc1.y = acc1.y > 0.f ? acc1.y : 0.f; acc1.z = acc1.z > 0.f ? acc1.z : 0.f; acc1.w = acc1.w > 0.f ? acc1.w : 0.f;
    if constexpr (LAST) {
      const bbx_f32x4 w0 = *(const bbx_f32x4*)(wl + 16 * b2i + 4 * lg4), w1v = *(const bbx_f32x4*)(wl + 16 * b2i + 16 + 4 * lg4);
      part = fmaf(acc0.x, w0.x, part); part = fmaf(acc0.y, w0.y, part); part = fmaf(acc0.z, w0.z, part); part = fmaf(acc0.w, w0.w, part);
      part = fmaf(acc1.x, w1v.x, part); part = fmaf(acc1.y, w1v.y, part); part = fmaf(acc1.z, w1v.z, part); part = fmaf(acc1.w, w1v.w, part);
    } else { hout[b2i] = acc0; hout[b2i + 1] = acc1; }
  };
  if constexpr (LAST) {
#pragma clang loop unroll(disable)
    for (int b2i = 0; b2i < NKO; b2i += 2) pair(b2i);
  } else {
#pragma unroll
    for (int b2i = 0; b2i < NKO; b2i += 2) pair(b2i);
  }
  return part;
}

// The logit of row (lane & 15) of a tile, without the deciding layer's bias, from the lane's B operands xa[s] = x[row][4 s +
// (lane >> 4)] (0 beyond the columns); every lane of the row returns it.  NK1 / NKM / NK2: blocks of 16 units of the first,
// the middle (0: none) and the last hidden layer.  W1p / b1p: the first layer, in memory (L1 hits); aml / bml and a2l / b2l /
// w3l: the permuted matrices, biases and deciding weights of the layers behind it (the caller's LDS copy, or memory).
// NPART: how far ahead the last layer's A operands are requested (pmlp2_hidden).
template <int NK1, int NKM, int NK2, int KS, int NPART = 2>
__device__ __forceinline__ float pmlp2_tile(const float (&xa)[KS], const float* W1p, const float* b1p, const float* aml, const float* bml,
                                            const float* a2l, const float* b2l, const float* w3l, int lane, int lr, int lg4) {
  constexpr int HP1 = 16 * NK1;
  // ---- layer 1: h[blk][v] = relu(b1 + sum_k W1[k][unit] x[row][k]), unit = 16 blk + 4 (lane >> 4) + v
  // (the first-layer weights stay in memory: L1 hits; the base pointer is opaque per tile so that the optimiser does not
  // hoist KS x NK1 loads out of the loops into registers the 128-register budget does not have)
  bbx_f32x4 h[NK1];
#pragma unroll
  for (int j = 0; j < NK1; j++) h[j] = *(const bbx_f32x4*)(b1p + 16 * j + 4 * lg4);
  const float* W1q = W1p + lg4 * HP1 + lr;
  asm volatile("" : "+v"(W1q));
#pragma unroll
  for (int s = 0; s < KS; s++) {
#pragma unroll
    for (int j = 0; j < NK1; j++) h[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(W1q[4 * s * HP1 + 16 * j], xa[s], h[j], 0, 0, 0);
    if (KS > 3 && (s & 1)) __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int j = 0; j < NK1; j++) {
    h[j].x = h[j].x > 0.f ? h[j].x : 0.f; h[j].y = h[j].y > 0.f ? h[j].y : 0.f;
    h[j].z = h[j].z > 0.f ? h[j].z : 0.f; h[j].w = h[j].w > 0.f ? h[j].w : 0.f;
  }
  // ---- the hidden layers behind the first, then the deciding layer's dot
  float part;
  if constexpr (NKM != 0) {
    bbx_f32x4 hm[NKM];
    pmlp2_hidden<NK1, NKM, false>(h, hm, aml, bml, nullptr, lane, lg4);
    part = pmlp2_hidden<NKM, NK2, true>(hm, nullptr, a2l, b2l, w3l, lane, lg4);
  } else part = pmlp2_hidden<NK1, NK2, true, NPART>(h, nullptr, a2l, b2l, w3l, lane, lg4);
  part += __shfl_xor(part, 16, WAVE);                                         // the other lane groups hold the row's other units
  part += __shfl_xor(part, 32, WAVE);
  return part;
}

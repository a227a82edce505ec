// PMLP policy, TWO hidden layers, as a differentiable function of its weights (bbx_pmlp2_logprob, bbx_pmlp2_grad of include/bbx.h):
// the log-probability of a recorded action, the entropy over a state's rows, and the gradient of
//   L = sum_s glogp[s] logprob_s + gent[s] entropy_s
// with respect to W1, b1, W2, b2, w3, b3.  Nothing of size [n][rows][hidden] ever exists in memory: the backward pass recomputes
// both hidden tiles.  The weights are the buffer bbx_pmlp2_prepare leaves (bbx_pmlp_shape.h); the permuted second-layer matrix
// A2 | b2 | w3 is staged in LDS once per workgroup, as in bbx_pmlp2_act_kernel.
//
// Forward (bbx_pmlp2_logprob_kernel): a wave per state; the logits of every 16-row tile come from pmlp2_tile, the maximum, the
// sum and lg[a] - logz from pmlp_softmax_wave (= pmlp_sample's order): for an action bbx_pmlp2_act has just drawn from the same
// block and weights the log-probability is that call's, bit for bit.
//
// Backward (bbx_pmlp2_grad_kernel<..., HEAD> + bbx_pmlp2_grad_reduce_kernel; the text describes the policy's head, the critic's
// differs in the states it skips and in g_r alone): a workgroup of NW = max(HP1, HP2) / 32 waves takes states
// p, p + groups, ... (pmlp2_grad_groups(n) workgroups: bbx_pmlp_shape.h).  Wave w owns units 32 w .. 32 w + 31 of BOTH layers:
// the columns dW1[:, slice], dW2[:, slice] (at most 32 + 64 accumulator registers) and the matching db1, db2, dw3.  Per state:
//   the logits (pmlp2_tile, the tiles dealt to the waves), p_r, H, then g_r = glogp (delta_{r,a} - p_r) - gent p_r (log p_r + H)
//   overwrites the logits in LDS (zero beyond the live rows up to the next multiple of 32);
// per 32-row tile.  The two pre-activations are recomputed with f64 accumulation (v_mfma_f64_16x16x4_f64; four 16x16 tiles per
// wave, lane l register v: row (l >> 4) + 4 v, unit l & 15): the accuracy bound of tests/policy2_grad_cases.py takes the
// activations at their exact values, and an fp32 chain leaves an activation that survives a cancellation with an error of its own
// size.  Everything behind them is v_mfma_f32_32x32x2_f32 with D[row][unit] (lane l, register v: row
// pv = (v & 3) + 8 (v >> 2) + 4 (l >> 5), unit 32 w + (l & 31)), so that a UNIT's rows lie along the registers of lanes l and l + 32:
//   1. z1[:, slice w] = b1 + x W1 (f64)   A: x[row l & 15][k = 4 s + (l >> 4)]   B: W1p[k][unit]   a1 = relu(z1) -> fp32 LDS a1t[row][unit]
//   2. z2[:, slice w] = b2 + a1 W2 (f64)  A: a1t[row l & 15][k = 16 S + 4 (l >> 4) + j], one 16-byte read per four steps
//                                         B: A2[blk2][S][lane][j], the 16-byte read the prepared layout was made for
//      a2 = relu(z2) -> fp32, through the wave's own columns of LDS dz2t[row][unit] into the 32x32 layout;
//      dz2 = g_r w3 [a2 > 0] (register v; overwrites a2 in dz2t), dw3 += g_r a2, db2 += dz2 in-lane over the registers;
//      dW2[32 ib ..][slice w] += a1^T dz2 for every unit block ib of layer 1: register v of dz2 IS the B operand of k-step v (the
//      step's two k are rows pv of the two lane halves), the A operand a1t[row pv][32 ib + (l & 31)]
//   3. dz1[:, slice w] = (dz2 W2^T) [a1 > 0]     A: dz2t[row l & 31][u2]   B: W2[unit 32 w + (l & 31)][u2] out of A2 (pmlp2_a2_index,
//      the inverse of pmlp2_perm; u2 of step 4 G + j in lane half h is 8 G + 4 h + j)
//      db1 += dz1; dW1[32 cb ..][slice w] += x^T dz1 the same way (A operand x[row pv][32 cb + (l & 31)])
// with a barrier behind each of the three.  At the end every wave writes its partial sums to the workgroup's slot of the
// caller's workspace and the second kernel adds the slots of every output in a fixed order: no floating-point atomics, and the
// partition depends on (n, cols, hidden1, hidden2) alone.
// Every barrier is reached by the whole workgroup: the state loop, the row count, the action and the tile loop are the same
// for all its threads, and a state that contributes nothing (the head's takes(): no row, one row, a bad action) is skipped before its
// first barrier.
//
// Indexed form (IDX; bbx_pmlp2_logprob_at, bbx_pmlp2_grad_at): position k of the call is about recorded state index[k] — obs, rows
// and actions are read there, the per-call arrays (logprobs, entropy, glogp, gent) at k.  An index outside [0, n_src): NaN / NaN,
// nothing for the gradients (skipped before its first barrier: the index is the same for the whole workgroup), and no read of the
// recorded arrays at that index.
#pragma once
#include "bbx_pmlp.h"

typedef double bbx_f64x4 __attribute__((ext_vector_type(4)));
constexpr int PMLP2_GRAD_PAD = 4;                                    // floats between the rows of an LDS tile (16-byte rows, spread banks)
__host__ __device__ constexpr int pmlp2_grad_lgcap(int obs_rows) { return ((pmlp_lgcap(obs_rows) + 31) / 32) * 32; }
__host__ __device__ constexpr int pmlp2_logprob_lgcap(int obs_rows) { return ((pmlp_lgcap(obs_rows) + 63) / 64) * 64; }
// LDS bytes: A2 | b2 | w3, then the logits of every wave (forward) or the g_r of the state and the two tiles (backward)
__host__ __device__ constexpr size_t pmlp2_logprob_lds_bytes(int hp1, int hp2, int waves, int obs_rows) {
  return ((size_t)hp1 * hp2 + 2 * hp2 + (size_t)waves * pmlp2_logprob_lgcap(obs_rows)) * sizeof(float);
}
// (exact_a1: a head that keeps the low halves of the first layer's activations too — a third tile, behind the other two)
__host__ __device__ constexpr size_t pmlp2_grad_lds_bytes(int hp1, int hp2, int obs_rows, bool exact_a1 = false) {
  return ((size_t)hp1 * hp2 + 2 * hp2 + pmlp2_grad_lgcap(obs_rows) + (exact_a1 ? 64 : 32) * (hp1 + PMLP2_GRAD_PAD) + 32 * (hp2 + PMLP2_GRAD_PAD)) * sizeof(float);
}
// where W2[k][unit] lies in the permuted A2 [HP2 / 16][S4 = HP1 / 16][64][4] (the inverse of pmlp2_perm, bbx_pmlp2.hip)
__host__ __device__ constexpr int pmlp2_a2_index(int k, int unit, int S4) {
  return ((((unit >> 4) * S4 + (k >> 4)) * 64 + ((k >> 2) & 3) * 16 + (unit & 15)) << 2) + (k & 3);
}

// the logits of rows r0 .. r0 + 15 of one state into lg: the scoring of bbx_pmlp2_act_kernel, operand for operand
template <int HP1, int HP2, int KS>
__device__ __forceinline__ void pmlp2_logits_tile(float* lg, const int32_t* __restrict__ ob, int r0, int n, int obs_rows, int cols, const float* W1p,
                                                  const float* b1p, const float* a2l, const float* b2l, const float* w3l, float b3, int lane) {
  const int lr = lane & 15, lg4 = lane >> 4;
  int r = r0 + lr; r = r < obs_rows ? r : obs_rows - 1;                       // inside the block whatever the row count is
  const int32_t* xr = ob + (size_t)r * cols;
  float xa[KS];
#pragma unroll
  for (int s = 0; s < KS; s++) {
    const int k = 4 * s + lg4;
    const int32_t xi = xr[k < cols ? k : 0];
    xa[s] = k < cols ? (float)xi : 0.f;
  }
  const float part = pmlp2_tile<HP1 / 16, 0, HP2 / 16, KS>(xa, W1p, b1p, nullptr, nullptr, a2l, b2l, w3l, lane, lr, lg4);
  if (lg4 == 0 && r0 + lr < n) lg[r0 + lr] = part + b3;
}

// LOSS: the instantiations of bbx_pmlp2_ppo_grad — lane 0 goes on from logprob_k and H_k to the loss's coefficients and terms
// (pmlp_loss_lane0); logprobs and entropy may then both be null, and H is computed whether entropy is wanted or not.  Without
// LOSS the argument `loss` is not read.
// EPI = PmlpXent (with LOSS): the instantiations of bbx_pmlp2_xent[_grad] — the wave goes on from its scores to the cross-entropy
// against the state's target row (pmlp_xent_wave); `actions` is not read, `logprobs` takes the losses.
template <int HP1, int HP2, int KS, bool IDX = false, bool LOSS = false, class EPI = PmlpLoss>
__global__ __launch_bounds__(512) void bbx_pmlp2_logprob_kernel(const int32_t* __restrict__ obs, const int32_t* __restrict__ rows,
                                                                const int32_t* __restrict__ actions, int B, int obs_rows, int cols,
                                                                const float* __restrict__ wp, float* __restrict__ logprobs,
                                                                float* __restrict__ entropy, int lgcap, const int32_t* __restrict__ index, int n_src,
                                                                EPI loss) {
  constexpr bool XENT = PmlpEpilogue<EPI>::xent;
  static_assert(LOSS || !XENT, "the cross-entropy is an epilogue");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int A2F = HP1 * HP2;
  float* a2 = (float*)smem;
  const float* W1p = wp;
  const float* b1p = wp + 4 * KS * HP1;
  const float* a2g = b1p + HP1;
  for (int i = (int)threadIdx.x; i < (A2F + 2 * HP2) / 4; i += (int)blockDim.x) ((bbx_f32x4*)a2)[i] = ((const bbx_f32x4*)a2g)[i];
  __syncthreads();
  const float* b2l = a2 + A2F;
  const float* w3l = b2l + HP2;
  const float b3 = a2g[A2F + 2 * HP2];
  const int lane = lane_id(), wave = uni((int)(threadIdx.x / WAVE)), nw = (int)blockDim.x / WAVE;
  float* lg = a2 + A2F + 2 * HP2 + (size_t)wave * lgcap;                      // logits of this wave's state
  for (int k = (int)blockIdx.x * nw + wave; k < B; k += (int)gridDim.x * nw) {   // position k of the call: recorded state s
    int s = k;
    if constexpr (IDX) {
      s = uni(index[k]);
      if (s < 0 || s >= n_src) {
        if constexpr (XENT) { if (lane == 0) pmlp_xent_lane0(loss, logprobs, entropy, k, false, false, 0.f, 0.f, 0.f); }
        else if constexpr (LOSS) { if (lane == 0) pmlp_loss_out(loss, logprobs, entropy, k, __builtin_nanf(""), __builtin_nanf("")); }
        else if (lane == 0) { logprobs[k] = __builtin_nanf(""); if (entropy) entropy[k] = __builtin_nanf(""); }
        continue;
      }
    }
    int n = uni(rows[s]);
    int a = 0;
    if constexpr (!XENT) a = uni(actions[s]);
    n = n < obs_rows ? n : obs_rows; n = n < PMLP_MAXROWS ? n : PMLP_MAXROWS;
    if (n <= 0) {
      if constexpr (XENT) { if (lane == 0) pmlp_xent_lane0(loss, logprobs, entropy, k, true, false, 0.f, 0.f, 0.f); }
      else if constexpr (LOSS) { if (lane == 0) pmlp_loss_out(loss, logprobs, entropy, k, 0.f, 0.f); }
      else if (lane == 0) { logprobs[k] = 0.f; if (entropy) entropy[k] = 0.f; }
      continue;
    }
    const int32_t* ob = obs + (size_t)s * obs_rows * cols;
    wave_sync();                                                              // (the previous state's logits have been read)
    for (int r0 = 0; r0 < n; r0 += 16) pmlp2_logits_tile<HP1, HP2, KS>(lg, ob, r0, n, obs_rows, cols, W1p, b1p, a2, b2l, w3l, b3, lane);
    wave_sync();
    const PmlpSoftmax sm = pmlp_softmax_wave(lg, n, lane);
    if constexpr (XENT) {
      pmlp_xent_wave(loss, logprobs, entropy, k, loss.targets + (size_t)s * obs_rows, lg, n, lane, sm);
      continue;
    }
    const bool ok = a >= 0 && a < n;
    if constexpr (LOSS && !XENT) {
      const float H = pmlp_entropy_wave(lg, n, lane, sm);
      if (lane == 0) pmlp_loss_out(loss, logprobs, entropy, k, ok ? lg[a] - sm.logz : __builtin_nanf(""), H);
      continue;
    }
    if (lane == 0) logprobs[k] = ok ? lg[a] - sm.logz : __builtin_nanf("");
    if (entropy) {
      const float H = pmlp_entropy_wave(lg, n, lane, sm);
      if (lane == 0) entropy[k] = H;
    }
  }
}

// The policy's head of the gradient kernel: which states contribute, and the row coefficients g_r that take the place of the scores
// in LDS.  A head (the critic's: Pmlp2ValueHead, bbx_pmlp2_value.h) travels by value as a kernel argument and has
//   state(s)                   what it reads of recorded state s (an index in range), the same in every thread of the workgroup
//   takes(n)                   whether that state, with n live rows, contributes — workgroup-uniform, asked before the first barrier
//   coefs(lg, n, k, lane, db3) called by the whole workgroup with the n > 0 scores of position k complete in lg (a barrier lies behind
//                              them): what it needs of them, ONE barrier, then g_r over the scores, zero up to the next multiple of 32,
//                              every thread its own entries r = threadIdx.x, + blockDim.x, ..., each added to db3
//   exact_a1                   whether stage 2 recomputes z2 from a1 = relu(z1) as a float32 PAIR (hi + lo, good to 2^-48) instead of the one
//                              float32 the tile holds: the critic's sum and mean pools have K_s = 1 in their bound, which takes the
//                              activations at their exact values, and a second-layer unit that a single row holds active with a z2
//                              left by cancellation then shows the 2^-24 of sum_k |a1_k W2_ku| a rounded a1 puts into it (measured:
//                              2646 units of the bound against 64).  The policy's head keeps the single float: its outputs are
//                              what they were, bit for bit
struct Pmlp2PolicyHead {
  static constexpr bool exact_a1 = false;
  const int32_t* actions;
  const float* glogp;
  const float* gent;
  int a;                                                                      // the action of the state in hand
  __device__ __forceinline__ void state(int s) { a = uni(actions[s]); }
  __device__ __forceinline__ bool takes(int n) const { return n > 1 && a >= 0 && a < n; }   // no row, one row (delta - p = 0) or a bad action: nothing
  __device__ __forceinline__ void coefs(float* lg, int n, int k, int lane, float& db3) const {
    const PmlpSoftmax sm = pmlp_softmax_wave(lg, n, lane);                    // (every wave for itself: the same numbers)
    const float H = pmlp_entropy_wave(lg, n, lane, sm);
    const float gl = glogp[k], ge = gent ? gent[k] : 0.f;
    const float rse = 1.f / sm.se;
    const int n32 = (n + 31) & ~31;
    __syncthreads();                                                          // (every wave has read the logits)
    for (int r = (int)threadIdx.x; r < n32; r += (int)blockDim.x) {           // (every thread reads and writes its own entries only)
      const float g = r < n ? pmlp_policy_coef(lg[r], r == a, sm, H, gl, ge, rse) : 0.f;
      lg[r] = g; db3 += g;
    }
  }
};

// The cross-entropy's head (bbx_pmlp2_xent_grad[_at]; the contract above): g_r = c_k (T_k p_r - t_r) (pmlp_xent_coef, bbx_pmlp.h) from
// coef = c | T as the forward kernel's epilogue wrote it, the target row of the recorded state and the recomputed softmax.  One
// live row: T p - t = 0, not taken.  c = 0 (the position is not counted, or weighs nothing) is known by position, which takes()
// is not told: such a state is scored and gets g_r = 0 throughout — its target row is not read and it adds exact zeros
struct Pmlp2XentHead {
  static constexpr bool exact_a1 = false;
  const float* targets;
  const float* coef;
  int n_pos, obs_rows;
  const float* tg;                                                            // the target row of the state in hand
  __device__ __forceinline__ void state(int s) { tg = targets + (size_t)s * obs_rows; }
  __device__ __forceinline__ bool takes(int n) const { return n > 1; }
  __device__ __forceinline__ void coefs(float* lg, int n, int k, int lane, float& db3) const {
    const PmlpSoftmax sm = pmlp_softmax_wave(lg, n, lane);                    // (every wave for itself: the same numbers)
    const float c = coef[k], T = coef[(size_t)n_pos + k];
    const float trse = T * (1.f / sm.se);
    const int n32 = (n + 31) & ~31;
    __syncthreads();                                                          // (every wave has read the logits)
    for (int r = (int)threadIdx.x; r < n32; r += (int)blockDim.x) {           // (every thread reads and writes its own entries only)
      const float g = (r < n && c != 0.f) ? pmlp_xent_coef(lg[r], tg[r], sm, c, trse) : 0.f;
      lg[r] = g; db3 += g;
    }
  }
};

// One kernel for the policy's gradients (HEAD = Pmlp2PolicyHead) and the critic's (Pmlp2ValueHead, bbx_pmlp2_value.h): the staging,
// the state loop, the scores, then — behind the head — the f64 recomputation of both pre-activations, the three MFMA stages, the
// accumulators and the partial layout bbx_pmlp2_grad_reduce_kernel reads.  (The body stays in the kernel itself: moved into a
// device function that two kernels call, it is inlined with other register classes — 32 more AGPRs at 64 units.)
template <int HP1, int HP2, int KS, bool IDX = false, class HEAD = Pmlp2PolicyHead>
__global__ __launch_bounds__(2 * (HP1 > HP2 ? HP1 : HP2)) void bbx_pmlp2_grad_kernel(const int32_t* __restrict__ obs, const int32_t* __restrict__ rows, int B,
                                                                                     int obs_rows, int cols, const float* __restrict__ wp, HEAD head,
                                                                                     int groups, float* __restrict__ ws,
                                                                                     const int32_t* __restrict__ index, int n_src) {
  constexpr int NB1 = HP1 / 32, NB2 = HP2 / 32, NW = NB1 > NB2 ? NB1 : NB2;  // pmlp2_grad_waves
  constexpr int CB = KS == 16 ? 2 : 1;                                        // pmlp2_grad_cb
  constexpr int S1 = HP1 + PMLP2_GRAD_PAD, S2 = HP2 + PMLP2_GRAD_PAD, S4 = HP1 / 16, A2F = HP1 * HP2;
  constexpr Pmlp2GradLayout L = pmlp2_grad_layout(32 * CB, HP1, HP2);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* a2 = (float*)smem;
  const float* W1p = wp;
  const float* b1p = wp + 4 * KS * HP1;
  const float* a2g = b1p + HP1;
  for (int i = (int)threadIdx.x; i < (A2F + 2 * HP2) / 4; i += (int)blockDim.x) ((bbx_f32x4*)a2)[i] = ((const bbx_f32x4*)a2g)[i];
  __syncthreads();
  const float* b2l = a2 + A2F;
  const float* w3l = b2l + HP2;
  const float b3 = a2g[A2F + 2 * HP2];
  float* lg = a2 + A2F + 2 * HP2;                                             // the state's logits, then its g_r
  float* a1t = lg + pmlp2_grad_lgcap(obs_rows);                               // [32][S1] relu(z1) of the tile
  float* dz2t = a1t + 32 * S1;                                                // [32][S2]
  [[maybe_unused]] float* a1lo = dz2t + 32 * S2;                              // [32][S1] relu(z1) - (float)relu(z1) (HEAD::exact_a1 only)
  const int lane = lane_id(), w = uni((int)(threadIdx.x / WAVE));
  const int lr = lane & 31, lk = lane >> 5, l15 = lane & 15, l4 = lane >> 4;
  const bool own1 = w < NB1, own2 = w < NB2;                                  // (wave-uniform: does the wave own a slice of the layer)
  const int u = 32 * w + lr;                                                  // my unit in either layer

  bbx_f32x16 dW2[NB1], dW1[CB];
  float db1a = 0.f, db2a = 0.f, dw3a = 0.f, db3a = 0.f;
#pragma unroll
  for (int v = 0; v < 16; v++) {
#pragma unroll
    for (int ib = 0; ib < NB1; ib++) dW2[ib][v] = 0.f;
#pragma unroll
    for (int cb = 0; cb < CB; cb++) dW1[cb][v] = 0.f;
  }

  for (int k = (int)blockIdx.x; k < B; k += groups) {                        // position k of the call: recorded state s
    int s = k;
    if constexpr (IDX) {
      s = uni(index[k]);
      if (s < 0 || s >= n_src) continue;                                      // nothing, and nothing read there
    }
    int n = uni(rows[s]);
    head.state(s);
    n = n < obs_rows ? n : obs_rows; n = n < PMLP_MAXROWS ? n : PMLP_MAXROWS;
    if (!head.takes(n)) continue;                                          // (the same for the whole workgroup: no barrier is left out)
    const int32_t* ob = obs + (size_t)s * obs_rows * cols;
    // (the previous state's g_r and tiles have been read: the barrier that ends its last tile)
    for (int r0 = 16 * w; r0 < n; r0 += 16 * NW) pmlp2_logits_tile<HP1, HP2, KS>(lg, ob, r0, n, obs_rows, cols, W1p, b1p, a2, b2l, w3l, b3, lane);
    __syncthreads();
    head.coefs(lg, n, k, lane, db3a);
    __syncthreads();
    for (int r0 = 0; r0 < n; r0 += 32) {
      bbx_f32x16 D;
      // ---- 1. a1[:, my slice] of the tile's rows in f64 (rows beyond n count as zero rows: their g_r is 0)
      if (own1) {
        bbx_f64x4 Z[2][2];                                                    // [row half][unit half]
        int32_t xs[2][KS];
        bool in[2];
#pragma unroll
        for (int rt = 0; rt < 2; rt++) {
          in[rt] = r0 + 16 * rt + l15 < n;
          const int32_t* xr = ob + (size_t)(in[rt] ? r0 + 16 * rt + l15 : 0) * cols;
#pragma unroll
          for (int s4 = 0; s4 < KS; s4++) { const int k = 4 * s4 + l4; xs[rt][s4] = xr[k < cols ? k : 0]; }
        }
        // (the weights are the same for every state and tile: the pointer is opaque per tile, so that the optimiser does not
        // hoist the loads out of the loops into registers the accumulators need)
        const float* wq = W1p + l4 * HP1 + 32 * w + l15;
        asm volatile("" : "+v"(wq));
#pragma unroll
        for (int ut = 0; ut < 2; ut++) {
          const double bu = (double)wq[(4 * KS - l4) * HP1 + 16 * ut];        // b1p[32 w + 16 ut + l15]
#pragma unroll
          for (int rt = 0; rt < 2; rt++)
#pragma unroll
            for (int v = 0; v < 4; v++) Z[rt][ut][v] = bu;
        }
#pragma unroll
        for (int s4 = 0; s4 < KS; s4++) {
          const int k = 4 * s4 + l4;
          double xa[2], wb[2];
#pragma unroll
          for (int rt = 0; rt < 2; rt++) xa[rt] = (in[rt] && k < cols) ? (double)xs[rt][s4] : 0.0;
#pragma unroll
          for (int ut = 0; ut < 2; ut++) wb[ut] = (double)wq[4 * s4 * HP1 + 16 * ut];
#pragma unroll
          for (int rt = 0; rt < 2; rt++)
#pragma unroll
            for (int ut = 0; ut < 2; ut++) Z[rt][ut] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[rt], wb[ut], Z[rt][ut], 0, 0, 0);
        }
#pragma unroll
        for (int rt = 0; rt < 2; rt++)
#pragma unroll
          for (int ut = 0; ut < 2; ut++)
#pragma unroll
            for (int v = 0; v < 4; v++) {
              const double z = Z[rt][ut][v];
              const float hi = z > 0.0 ? (float)z : 0.f;
              a1t[(16 * rt + l4 + 4 * v) * S1 + 32 * w + 16 * ut + l15] = hi;
              if constexpr (HEAD::exact_a1) a1lo[(16 * rt + l4 + 4 * v) * S1 + 32 * w + 16 * ut + l15] = z > 0.0 ? (float)(z - (double)hi) : 0.f;
            }
      }
      __syncthreads();
      // ---- 2. a2[:, my slice] in f64, through my columns of the dz2 tile into the 32x32 layout; dz2, dw3, db2, dW2[:, my slice]
      if (own2) {
        const float wu = w3l[u];
        {
          bbx_f64x4 Z[2][2];
#pragma unroll
          for (int ut = 0; ut < 2; ut++) {
            const double bu = (double)b2l[32 * w + 16 * ut + l15];
#pragma unroll
            for (int rt = 0; rt < 2; rt++)
#pragma unroll
              for (int v = 0; v < 4; v++) Z[rt][ut][v] = bu;
          }
          const float* ap = a1t + l15 * S1 + 4 * l4;                          // + 16 rt S1 + 16 S: k = 16 S + 4 l4 + j
          const float* bp = a2 + (size_t)(2 * w * S4 * 64 + lane) * 4;        // + (ut S4 + S) 256: A2[2 w + ut][S][lane][j] as prepared
#pragma unroll 2
          for (int S = 0; S < S4; S++) {
            bbx_f32x4 av[2], bv[2];
            [[maybe_unused]] bbx_f32x4 al[2];
#pragma unroll
            for (int rt = 0; rt < 2; rt++) {
              av[rt] = *(const bbx_f32x4*)(ap + 16 * rt * S1 + 16 * S);
              if constexpr (HEAD::exact_a1) al[rt] = *(const bbx_f32x4*)(ap + (a1lo - a1t) + 16 * rt * S1 + 16 * S);
            }
#pragma unroll
            for (int ut = 0; ut < 2; ut++) bv[ut] = *(const bbx_f32x4*)(bp + (ut * S4 + S) * 256);
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
              for (int rt = 0; rt < 2; rt++)
#pragma unroll
                for (int ut = 0; ut < 2; ut++) {
                  double a = (double)av[rt][j];
                  if constexpr (HEAD::exact_a1) a += (double)al[rt][j];
                  Z[rt][ut] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, (double)bv[ut][j], Z[rt][ut], 0, 0, 0);
                }
          }
#pragma unroll
          for (int rt = 0; rt < 2; rt++)
#pragma unroll
            for (int ut = 0; ut < 2; ut++)
#pragma unroll
              for (int v = 0; v < 4; v++) {
                const double z = Z[rt][ut][v];
                dz2t[(16 * rt + l4 + 4 * v) * S2 + 32 * w + 16 * ut + l15] = z > 0.0 ? (float)z : 0.f;
              }
        }
        wave_sync();                                                          // (my own columns of the tile: written and read by this wave alone)
        float gv[16];
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const bbx_f32x4 g4 = *(const bbx_f32x4*)(lg + r0 + 8 * q + 4 * lk);
          gv[4 * q] = g4.x; gv[4 * q + 1] = g4.y; gv[4 * q + 2] = g4.z; gv[4 * q + 3] = g4.w;
        }
#pragma unroll
        for (int v = 0; v < 16; v++) {
          float* cell = dz2t + ((v & 3) + 8 * (v >> 2) + 4 * lk) * S2 + u;    // (a2 in, dz2 out: this lane's cell both times)
          const float h = *cell;
          dw3a = fmaf(gv[v], h, dw3a);
          const float dz = h > 0.f ? gv[v] * wu : 0.f;
          db2a += dz;
          D[v] = dz;
          *cell = dz;
        }
#pragma unroll
        for (int ib = 0; ib < NB1; ib++)
#pragma unroll
          for (int v = 0; v < 16; v++)
            dW2[ib] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1t[((v & 3) + 8 * (v >> 2) + 4 * lk) * S1 + 32 * ib + lr], D[v], dW2[ib], 0, 0, 0);
      }
      __syncthreads();
      // ---- 3. dz1[:, my slice], db1, dW1[:, my slice]
      if (own1) {
#pragma unroll
        for (int v = 0; v < 16; v++) D[v] = 0.f;
        const float* ap = dz2t + lr * S2 + 4 * lk;                            // u2 = 8 G + 4 lk + j
        const float* bp = a2 + pmlp2_a2_index(u, 0, S4) + 16 * lk;
#pragma unroll
        for (int G = 0; G < HP2 / 8; G++) {
          const bbx_f32x4 av = *(const bbx_f32x4*)(ap + 8 * G);
          const float* bq = bp + (G >> 1) * (S4 * 256) + (G & 1) * 32;
          D = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bq[0], D, 0, 0, 0);
          D = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bq[4], D, 0, 0, 0);
          D = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bq[8], D, 0, 0, 0);
          D = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bq[12], D, 0, 0, 0);
        }
#pragma unroll
        for (int v = 0; v < 16; v++) {
          const float dz = a1t[((v & 3) + 8 * (v >> 2) + 4 * lk) * S1 + u] > 0.f ? D[v] : 0.f;
          db1a += dz;
          D[v] = dz;
        }
#pragma unroll
        for (int v = 0; v < 16; v++) {
          const int r = r0 + (v & 3) + 8 * (v >> 2) + 4 * lk;
          const bool in = r < n;
          const int32_t* xr = ob + (size_t)(in ? r : 0) * cols;
#pragma unroll
          for (int cb = 0; cb < CB; cb++) {
            const int k = 32 * cb + lr;
            const int32_t xi = xr[k < cols ? k : 0];
            const float xt = (in && k < cols) ? (float)xi : 0.f;
            dW1[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(xt, D[v], dW1[cb], 0, 0, 0);
          }
        }
      }
      __syncthreads();                                                        // (the tiles and, behind the last one, the g_r are free)
    }
  }

  // the workgroup's partial sums (pmlp2_grad_layout): dW1 [32 CB][HP1] | db1 [HP1] | dW2 [HP1][HP2] | db2 [HP2] | dw3 [HP2] | db3 [NW]
  float* part = ws + (size_t)blockIdx.x * L.total;
  if (own1) {
#pragma unroll
    for (int cb = 0; cb < CB; cb++)
#pragma unroll
      for (int v = 0; v < 16; v++) part[L.w1 + (32 * cb + (v & 3) + 8 * (v >> 2) + 4 * lk) * HP1 + u] = dW1[cb][v];
    const float tb = db1a + __shfl_xor(db1a, 32, WAVE);                       // the unit's other 16 rows
    if (lk == 0) part[L.b1 + u] = tb;
  }
  if (own2) {
#pragma unroll
    for (int ib = 0; ib < NB1; ib++)
#pragma unroll
      for (int v = 0; v < 16; v++) part[L.w2 + (32 * ib + (v & 3) + 8 * (v >> 2) + 4 * lk) * HP2 + u] = dW2[ib][v];
    const float tb = db2a + __shfl_xor(db2a, 32, WAVE), tw = dw3a + __shfl_xor(dw3a, 32, WAVE);
    if (lk == 0) { part[L.b2 + u] = tb; part[L.w3 + u] = tw; }
  }
  const float t3 = wave_sum_f32(db3a);
  if (lane == WAVE - 1) part[L.b3 + w] = t3;
}

// The second stage: output i of dW1 [cols][h1] | db1 [h1] | dW2 [h1][h2] | db2 [h2] | dw3 [h2] | db3 is the sum of its partials
// over the `groups` workgroup slots — 64 outputs per workgroup, the slots of an output dealt to four threads (slot q, q + 4, ...
// in order; db3: the waves of a slot in order), the four sums added as (s0 + s1) + (s2 + s3).  groups = 0: zeros.
__global__ __launch_bounds__(256) void bbx_pmlp2_grad_reduce_kernel(const float* __restrict__ ws, int groups, int cols, int h1, int h2,
                                                                    float* __restrict__ gw1, float* __restrict__ gb1, float* __restrict__ gw2,
                                                                    float* __restrict__ gb2, float* __restrict__ gw3, float* __restrict__ gb3) {
  __shared__ float part[4][64];
  const int hp1 = pmlp2_hp_for(h1), hp2 = pmlp2_hp_for(h2);
  const Pmlp2GradLayout L = pmlp2_grad_layout(32 * pmlp2_grad_cb(cols), hp1, hp2);
  const int n1 = cols * h1, n2 = n1 + h1, n3 = n2 + h1 * h2, n4 = n3 + h2, n5 = n4 + h2, total = n5 + 1;
  const int j = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + j;
  float* out = nullptr;
  float sum = 0.f;
  if (i < total) {
    int off, cnt = 1;
    if (i < n1) { const int k = i / h1; off = L.w1 + k * hp1 + (i - k * h1); out = gw1 + i; }
    else if (i < n2) { off = L.b1 + (i - n1); out = gb1 + (i - n1); }
    else if (i < n3) { const int t = i - n2, k = t / h2; off = L.w2 + k * hp2 + (t - k * h2); out = gw2 + t; }
    else if (i < n4) { off = L.b2 + (i - n3); out = gb2 + (i - n3); }
    else if (i < n5) { off = L.w3 + (i - n4); out = gw3 + (i - n4); }
    else { off = L.b3; out = gb3; cnt = pmlp2_grad_waves(hp1, hp2); }
    for (int g = q; g < groups; g += 4) {
      const float* src = ws + (size_t)g * L.total + off;
      for (int c = 0; c < cnt; c++) sum += src[c];
    }
  }
  part[q][j] = sum;
  __syncthreads();
  if (q == 0 && out) *out = (part[0][j] + part[1][j]) + (part[2][j] + part[3][j]);
}

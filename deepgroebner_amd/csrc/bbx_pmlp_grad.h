// PMLP policy, one hidden layer, as a differentiable function of its weights (bbx_pmlp_logprob, bbx_pmlp_grad of include/bbx.h):
// the log-probability of a recorded action, the entropy over a state's rows, and the gradient of
//   L = sum_s glogp[s] logprob_s + gent[s] entropy_s
// with respect to W1, b1, w2, b2 — what the reference's update (pg.py _fit_policy_model) needs per recorded state.  Nothing of
// size [n][rows][hidden] ever exists in memory: the backward pass recomputes the hidden tile.
//
// Forward (bbx_pmlp_logprob_kernel): one wave per state; the logits go to the wave's LDS array through pmlp_logits_wave, the row
// loop of pmlp_act_wave (bbx_pmlp.h), then the same max / sum order and the same lg[a] - logz: the log-probability of an action
// bbx_pmlp_act has just sampled from the same block and weights is that call's, bit for bit.  Entropy: with e_r = exp(z_r - max),
// se = sum e_r:   H = log(se) - (sum_r e_r (z_r - max)) / se   (= logZ - sum_r p_r z_r with the maximum taken out of both terms,
// so that large logits do not cancel).
//
// Backward (bbx_pmlp_grad_kernel + bbx_pmlp_grad_reduce_kernel): a wave takes states p, p + waves, ... (pmlp_grad_waves(n) waves
// per unit group: bbx_pmlp_shape.h).  Per state: the logits as above, then p_r, H and
//   g_r = glogp (delta_{r,a} - p_r) - gent p_r (log p_r + H)          (pmlp_policy_coef, bbx_pmlp.h)
// overwrite the logits in LDS (zero beyond the live rows, up to the next multiple of 32).  That is the kernel's own head; what
// follows is PmlpGradWave below, which the critic's gradient kernel (bbx_pmlp_value.h) runs behind a head of its own.  Per 32-row
// tile and unit block the hidden tile is recomputed THE OTHER WAY ROUND, D'[row][unit]: the operands of pmlp_tile swapped —
//   A operand  lane l: x[row r0 + (l & 31)][2s + (l >> 5)]           B operand  lane l: W1[2s + (l >> 5)][unit 32 ub + (l & 31)]
//   D'         lane l, register v: row r0 + (v & 3) + 8 (v >> 2) + 4 (l >> 5), unit 32 ub + (l & 31); starts at b1[unit]
// so a UNIT's 32 rows lie along the registers of lanes l and l + 32: relu, dh = g_r w2[unit] [h > 0], dw2 += g_r relu(h) and
// db1 += dh are in-lane sums over the registers (g_r: four 16-byte LDS reads per lane, a broadcast per lane half), and register v
// of dh is directly the B operand of k-step v of   dW1[k][unit] += sum_rows x[row][k] dh[row][unit]   (the step's two k values
// are the rows of register v in the two lane halves), whose A operand is x[r0 + (v & 3) + 8 (v >> 2) + 4 (l >> 5)][32 cb + (l & 31)]:
// the same permuted row order.  dW1 comes out as lane l, register v: column 32 cb + (v & 3) + 8 (v >> 2) + 4 (l >> 5), unit on the lane.
// dW1, db1, dw2 and db2 stay in registers across all states of the wave; at the end the wave writes its partial sums to the
// caller's workspace, and the second kernel adds the partials of every output in a fixed order: no floating-point atomics,
// and the partition depends on n and the shape alone, so the same inputs give the same bits on any device.
// 8 unit blocks x 2 column blocks x 16 accumulators do not fit in a wave: a wave owns pmlp_grad_ubw unit blocks (at most 64 dW1
// accumulators) and the unit groups are spread ACROSS THE GRID (blockIdx.y); every group computes the logits of its states
// itself (db2 is taken from group 0).
#pragma once
#include "bbx_pmlp.h"

// LDS floats per wave of the gradient kernel: the g_r of a state, padded to whole tiles
__host__ __device__ constexpr int pmlp_grad_lgcap(int obs_rows) { return ((pmlp_lgcap(obs_rows) + 31) / 32) * 32; }
__host__ __device__ constexpr size_t pmlp_grad_lds_bytes(int waves, int obs_rows) { return (size_t)waves * pmlp_grad_lgcap(obs_rows) * sizeof(float); }

// (pmlp_logits_wave: bbx_pmlp.h, the row loop pmlp_act_wave runs; pmlp_softmax_wave / pmlp_entropy_wave / pmlp_policy_coef: beside
// pmlp_sample, whose order they keep)
// LOSS: the instantiations of bbx_pmlp_ppo_grad — lane 0 goes on from logprob_k and H_k to the loss's coefficients and terms
// (pmlp_loss_lane0); logprobs and entropy may then both be null, and H is computed whether entropy is wanted or not.  Without
// LOSS the argument `loss` is not read.
// EPI = PmlpXent (with LOSS): the instantiations of bbx_pmlp_xent[_grad] — the wave goes on from its scores to the cross-entropy against
// the state's target row (pmlp_xent_wave); `actions` is not read, `logprobs` takes the losses.
template <int NB, int KS, bool IDX = false, bool LOSS = false, class EPI = PmlpLoss>
__global__ __launch_bounds__(256, 2) void bbx_pmlp_logprob_kernel(const int32_t* __restrict__ obs, const int32_t* __restrict__ rows,
                                                                  const int32_t* __restrict__ actions, int B, int obs_rows, int cols,
                                                                  const float* __restrict__ wp, float* __restrict__ logprobs, float* __restrict__ entropy,
                                                                  const int32_t* __restrict__ index, int n_src, EPI loss) {
  constexpr bool XENT = PmlpEpilogue<EPI>::xent;
  static_assert(LOSS || !XENT, "the cross-entropy is an epilogue");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = lane_id(), wave = uni((int)(threadIdx.x / WAVE));
  const int k = blockIdx.x * ((int)blockDim.x / WAVE) + wave;         // my position in the call
  if (k >= B) return;
  int s = k;                                                          // the recorded state it is about
  if constexpr (IDX) {
    s = uni(index[k]);
    if (s < 0 || s >= n_src) {
      if constexpr (XENT) { if (lane == 0) pmlp_xent_lane0(loss, logprobs, entropy, k, false, false, 0.f, 0.f, 0.f); }
      else if constexpr (LOSS) { if (lane == 0) pmlp_loss_out(loss, logprobs, entropy, k, __builtin_nanf(""), __builtin_nanf("")); }
      else if (lane == 0) { logprobs[k] = __builtin_nanf(""); if (entropy) entropy[k] = __builtin_nanf(""); }
      return;
    }
  }
  float* lg = (float*)smem + (size_t)wave * pmlp_lgcap(obs_rows);
  const int nraw = rows[s];
  int a = 0;
  if constexpr (!XENT) a = uni(actions[s]);
  const int n = pmlp_logits_wave<NB, KS>(lg, obs + (size_t)s * obs_rows * cols, nraw, obs_rows, cols, wp, lane & 31, lane >> 5);
  if (n <= 0) {
    if constexpr (XENT) { if (lane == 0) pmlp_xent_lane0(loss, logprobs, entropy, k, true, false, 0.f, 0.f, 0.f); }
    else if constexpr (LOSS) { if (lane == 0) pmlp_loss_out(loss, logprobs, entropy, k, 0.f, 0.f); }
    else if (lane == 0) { logprobs[k] = 0.f; if (entropy) entropy[k] = 0.f; }
    return;
  }
  wave_sync();
  const PmlpSoftmax sm = pmlp_softmax_wave(lg, n, lane);
  if constexpr (XENT) {
    pmlp_xent_wave(loss, logprobs, entropy, k, loss.targets + (size_t)s * obs_rows, lg, n, lane, sm);
    return;
  }
  const bool ok = a >= 0 && a < n;
  if constexpr (LOSS && !XENT) {
    const float H = pmlp_entropy_wave(lg, n, lane, sm);
    if (lane == 0) pmlp_loss_out(loss, logprobs, entropy, k, ok ? lg[a] - sm.logz : __builtin_nanf(""), H);
    return;
  }
  if (lane == 0) logprobs[k] = ok ? lg[a] - sm.logz : __builtin_nanf("");
  if (entropy) {
    const float H = pmlp_entropy_wave(lg, n, lane, sm);
    if (lane == 0) entropy[k] = H;
  }
}

// The back half of a gradient kernel, one code for the policy's (bbx_pmlp_grad_kernel) and the critic's (bbx_pmlp_value_grad_kernel,
// bbx_pmlp_value.h): what a wave keeps across its states, and what it does to a state before and after the kernel's own head has
// written the row coefficients g_r over the scores in LDS.  The shape constants are bbx_pmlp_shape.h's at the built-in shape.
template <int NB, int KS>
struct PmlpGradWave {
  static_assert(pmlp_ks_for(2 * KS) == KS && pmlp_nb_for(32 * NB) == NB, "not a built-in shape");
  static constexpr int HP = 32 * NB;
  static constexpr int CB = pmlp_grad_cb(2 * KS), UBW = pmlp_grad_ubw(2 * KS, HP);   // column blocks; unit blocks of a wave
  static constexpr int UW = 32 * UBW, NG = NB / UBW;                                 // units of a wave; unit groups (blockIdx.y)
  static constexpr int PW = pmlp_grad_partial_floats(2 * KS, HP);

  int lr, lk;
  const float* wl;                                                    // my B-operand column: + 2 s HP + 32 u
  bbx_f32x16 dW[UBW][CB];
  float db1a[UBW], dw2a[UBW], db2a;                                   // (db2a: the kernel's head adds the g_r it writes)

  __device__ __forceinline__ void start(const float* __restrict__ wp, int lane) {
    lr = lane & 31; lk = lane >> 5;
    wl = wp + lk * HP + (int)blockIdx.y * UW + lr;
    db2a = 0.f;
#pragma unroll
    for (int u = 0; u < UBW; u++) {
      db1a[u] = 0.f; dw2a[u] = 0.f;
#pragma unroll
      for (int cb = 0; cb < CB; cb++)
#pragma unroll
        for (int v = 0; v < 16; v++) dW[u][cb][v] = 0.f;
    }
  }

  // position k of the call -> the recorded state it is about.  An index out of range: in_src = false, for which the caller takes
  // no row (the kernels skip such a state) — and state 0 in its place for the addresses (the launcher sees to n_src > 0).  A
  // branch around the state here instead costs 20-30 vector registers and, from 33 columns on, spills
  template <bool IDX>
  static __device__ __forceinline__ int state_of(const int32_t* __restrict__ index, int n_src, int k, bool& in_src) {
    int s = k;
    in_src = true;
    if constexpr (IDX) {
      s = uni(index[k]);
      in_src = s >= 0 && s < n_src;
      s = in_src ? s : 0;
    }
    return s;
  }

  // the scores of a state into lg; returns the live row count
  __device__ __forceinline__ int logits(float* lg, const int32_t* __restrict__ ob, int nraw, int obs_rows, int cols, const float* __restrict__ wp) {
    wave_sync();                                                      // (the previous state's g_r have been read)
    // (the weights are the same for every state and tile: their base pointers are opaque per use, so that the optimiser does not
    // hoist hundreds of loads out of the loops into registers the dW1 accumulators need)
    const float* wq = wp;
    asm volatile("" : "+s"(wq));
    return pmlp_logits_wave<NB, KS>(lg, ob, nraw, obs_rows, cols, wq, lr, lk);
  }

  // the n > 0 rows of a state, their g_r in lg (zero up to the next multiple of 32), into the accumulators
  __device__ __forceinline__ void tiles(const float* lg, const int32_t* __restrict__ ob, int n, int cols) {
    for (int r0 = 0; r0 < n; r0 += 32) {
      // the rows of this tile twice: as the k-step operands of the hidden tile (row on the lane), and in the permuted row
      // order of the accumulator registers with the column on the lane (dW1's A operands); rows beyond n count as zero
      float xa[KS];
      {
        const bool in = r0 + lr < n;
        const int32_t* xr = ob + (size_t)(in ? r0 + lr : 0) * cols;
#pragma unroll
        for (int s2 = 0; s2 < KS; s2++) {
          const int k = 2 * s2 + lk;
          const int32_t xi = xr[k < cols ? k : 0];
          xa[s2] = (in && k < cols) ? (float)xi : 0.f;
        }
      }
      float xt[CB][16], gv[16];
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const bbx_f32x4 g4 = *(const bbx_f32x4*)(lg + r0 + 8 * q + 4 * lk);
        gv[4 * q] = g4.x; gv[4 * q + 1] = g4.y; gv[4 * q + 2] = g4.z; gv[4 * q + 3] = g4.w;
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
          xt[cb][v] = (in && k < cols) ? (float)xi : 0.f;
        }
      }
#pragma unroll
      for (int u = 0; u < UBW; u++) {
        const float* wlq = wl + 32 * u;
        asm volatile("" : "+v"(wlq));
        const float bu = wlq[(2 * KS - lk) * HP], wu = wlq[(2 * KS + 1 - lk) * HP];   // b1p / w2p [grp UW + 32 u + lr]
        bbx_f32x16 D;
#pragma unroll
        for (int v = 0; v < 16; v++) D[v] = bu;
#pragma unroll
        for (int s2 = 0; s2 < KS; s2++) D = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[s2], wlq[2 * s2 * HP], D, 0, 0, 0);
        float dw2 = dw2a[u], db1 = db1a[u];
#pragma unroll
        for (int v = 0; v < 16; v++) {
          const float h = D[v];
          const bool pos = h > 0.f;
          dw2 = fmaf(gv[v], pos ? h : 0.f, dw2);
          const float dh = pos ? gv[v] * wu : 0.f;
          db1 += dh;
          D[v] = dh;
        }
        dw2a[u] = dw2; db1a[u] = db1;
#pragma unroll
        for (int cb = 0; cb < CB; cb++)
#pragma unroll
          for (int v = 0; v < 16; v++) dW[u][cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(xt[cb][v], D[v], dW[u][cb], 0, 0, 0);
      }
    }
  }

  // the partial sums of wave p of my unit group, as bbx_pmlp_grad_reduce_kernel reads them: dW1 [32 CB][UW] | db1 [UW] | dw2 [UW] | db2
  __device__ __forceinline__ void store(float* __restrict__ ws, int p, int lane) {
    float* part = ws + ((size_t)p * NG + (int)blockIdx.y) * PW;
#pragma unroll
    for (int u = 0; u < UBW; u++) {
#pragma unroll
      for (int cb = 0; cb < CB; cb++)
#pragma unroll
        for (int v = 0; v < 16; v++) part[(32 * cb + (v & 3) + 8 * (v >> 2) + 4 * lk) * UW + 32 * u + lr] = dW[u][cb][v];
      const float tb = db1a[u] + __shfl_xor(db1a[u], 32, WAVE), tw = dw2a[u] + __shfl_xor(dw2a[u], 32, WAVE);   // the unit's other 16 rows
      if (lk == 0) { part[32 * CB * UW + 32 * u + lr] = tb; part[32 * CB * UW + UW + 32 * u + lr] = tw; }
    }
    const float t2 = wave_sum_f32(db2a);
    if (lane == WAVE - 1) part[32 * CB * UW + 2 * UW] = t2;
  }
};

template <int NB, int KS, bool IDX = false>
__global__ __launch_bounds__(256, 2) void bbx_pmlp_grad_kernel(const int32_t* __restrict__ obs, const int32_t* __restrict__ rows,
                                                               const int32_t* __restrict__ actions, int B, int obs_rows, int cols,
                                                               const float* __restrict__ wp, const float* __restrict__ glogp,
                                                               const float* __restrict__ gent, int nwaves, float* __restrict__ ws,
                                                               const int32_t* __restrict__ index, int n_src) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = lane_id(), wave = uni((int)(threadIdx.x / WAVE));
  const int p = blockIdx.x * ((int)blockDim.x / WAVE) + wave;       // my place among the group's waves
  if (p >= nwaves) return;
  float* lg = (float*)smem + (size_t)wave * pmlp_grad_lgcap(obs_rows);
  PmlpGradWave<NB, KS> G;
  G.start(wp, lane);
  for (int k = p; k < B; k += nwaves) {                               // position k of the call: recorded state s
    bool in_src;
    const int s = G.template state_of<IDX>(index, n_src, k, in_src);
    const int nraw = in_src ? rows[s] : 0;
    const int a = uni(actions[s]);
    const int32_t* ob = obs + (size_t)s * obs_rows * cols;
    const int n = G.logits(lg, ob, nraw, obs_rows, cols, wp);
    if (n <= 1 || a < 0 || a >= n) continue;                         // no row, one row (delta - p = 0) or a bad action: nothing
    wave_sync();
    const PmlpSoftmax sm = pmlp_softmax_wave(lg, n, lane);
    const float H = pmlp_entropy_wave(lg, n, lane, sm);
    const float gl = glogp[k], ge = gent ? gent[k] : 0.f;
    const float rse = 1.f / sm.se;
    const int n32 = (n + 31) & ~31;
    for (int r = lane; r < n32; r += WAVE) {                          // (every lane reads and writes its own entries only)
      const float g = r < n ? pmlp_policy_coef(lg[r], r == a, sm, H, gl, ge, rse) : 0.f;
      lg[r] = g; G.db2a += g;
    }
    wave_sync();
    G.tiles(lg, ob, n, cols);
  }
  G.store(ws, p, lane);
}

// The cross-entropy's gradient kernel (bbx_pmlp_xent_grad[_at]): bbx_pmlp_grad_kernel with the head of
//   L = scale sum_k w_k l_k,  l_k = -sum_r t_r log p_r:    g_r = c_k (T_k p_r - t_r)          (pmlp_xent_coef, bbx_pmlp.h)
// from coef = c | T as the forward kernel's epilogue wrote it (c = 0: the position is not counted, or weighs nothing — skipped,
// and its target row is not read), the target row of the recorded state and the recomputed softmax.  One live row: T p - t = 0,
// skipped.  The partition, the accumulators, the tile loop and the partial layout are PmlpGradWave's.
template <int NB, int KS, bool IDX = false>
__global__ __launch_bounds__(256, 2) void bbx_pmlp_xent_grad_kernel(const int32_t* __restrict__ obs, const int32_t* __restrict__ rows,
                                                                    const float* __restrict__ targets, int B, int obs_rows, int cols,
                                                                    const float* __restrict__ wp, const float* __restrict__ coef, int nwaves,
                                                                    float* __restrict__ ws, const int32_t* __restrict__ index, int n_src) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = lane_id(), wave = uni((int)(threadIdx.x / WAVE));
  const int p = blockIdx.x * ((int)blockDim.x / WAVE) + wave;       // my place among the group's waves
  if (p >= nwaves) return;
  float* lg = (float*)smem + (size_t)wave * pmlp_grad_lgcap(obs_rows);
  PmlpGradWave<NB, KS> G;
  G.start(wp, lane);
  for (int k = p; k < B; k += nwaves) {                               // position k of the call: recorded state s
    bool in_src;
    const int s = G.template state_of<IDX>(index, n_src, k, in_src);
    const int nraw = in_src ? rows[s] : 0;
    const float c = __builtin_bit_cast(float, uni(__builtin_bit_cast(int, coef[k])));
    const float T = coef[(size_t)B + k];
    const int32_t* ob = obs + (size_t)s * obs_rows * cols;
    const int n = G.logits(lg, ob, nraw, obs_rows, cols, wp);
    if (n <= 1 || c == 0.f) continue;                                 // no row, one row (T p - t = 0), not counted or no weight: nothing
    wave_sync();
    const PmlpSoftmax sm = pmlp_softmax_wave(lg, n, lane);
    const float trse = T * (1.f / sm.se);
    const float* tg = targets + (size_t)s * obs_rows;
    const int n32 = (n + 31) & ~31;
    for (int r = lane; r < n32; r += WAVE) {                          // (every lane reads and writes its own entries only)
      const float g = r < n ? pmlp_xent_coef(lg[r], tg[r], sm, c, trse) : 0.f;
      lg[r] = g; G.db2a += g;
    }
    wave_sync();
    G.tiles(lg, ob, n, cols);
  }
  G.store(ws, p, lane);
}

// The second stage: output i of dW1 [cols][hidden] | db1 [hidden] | dw2 [hidden] | db2 is the sum of its nwaves partials —
// 64 outputs per workgroup, the partials of an output dealt to four threads (partial q, q + 4, ... in order), the four sums
// added as (s0 + s1) + (s2 + s3).  nwaves = 0: zeros.
static __global__ __launch_bounds__(256) void bbx_pmlp_grad_reduce_kernel(const float* __restrict__ ws, int nwaves, int cols, int hidden,
                                                                   float* __restrict__ gw1, float* __restrict__ gb1, float* __restrict__ gw2,
                                                                   float* __restrict__ gb2) {
  __shared__ float part[4][64];
  const int cb = pmlp_grad_cb(cols), ubw = pmlp_grad_ubw(cols, hidden), uw = 32 * ubw;
  const int ng = pmlp_nb_for(hidden) / ubw, pw = pmlp_grad_partial_floats(cols, hidden);
  const int total = cols * hidden + 2 * hidden + 1;
  const int j = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + j;
  float* out = nullptr;
  float sum = 0.f;
  if (i < total) {
    int k, unit;                                                      // row of the partial block (column of W1, or 32 cb: db1, + 1: dw2), unit
    if (i < cols * hidden) { k = i / hidden; unit = i - k * hidden; out = gw1 + i; }
    else if (i < cols * hidden + hidden) { k = 32 * cb; unit = i - cols * hidden; out = gb1 + unit; }
    else if (i < total - 1) { k = 32 * cb + 1; unit = i - cols * hidden - hidden; out = gw2 + unit; }
    else { k = 32 * cb + 2; unit = 0; out = gb2; }
    const int grp = unit / uw;
    const float* src = ws + (size_t)grp * pw + (size_t)k * uw + (unit - grp * uw);
    for (int w = q; w < nwaves; w += 4) sum += src[(size_t)w * ng * pw];
  }
  part[q][j] = sum;
  __syncthreads();
  if (q == 0 && out) *out = (part[0][j] + part[1][j]) + (part[2][j] + part[3][j]);
}

// What both statistics kernels (bbx_pmlp_ppo_stats_kernel; bbx_pmlp_value_stats_kernel, bbx_pmlp_value.h) end with: the six sums
// of the workgroup's PMLP_PPO_STAT_THREADS threads into stats[0..5] — the 64 lanes of a wave by a butterfly (every lane ends with
// the same sum), the 16 waves in order by one thread per statistic.
__device__ __forceinline__ void pmlp_stats_sum(double (&acc)[6], double* __restrict__ stats) {
  __shared__ double part[PMLP_PPO_STAT_THREADS / WAVE][6];
#pragma unroll
  for (int i = 0; i < 6; i++) {
#pragma unroll
    for (int m = 1; m < WAVE; m <<= 1) acc[i] += __shfl_xor(acc[i], m, WAVE);
  }
  const int wave = (int)(threadIdx.x / WAVE);
  if ((threadIdx.x & (WAVE - 1)) == 0) {
#pragma unroll
    for (int i = 0; i < 6; i++) part[wave][i] = acc[i];
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    double t = 0.;
    for (int w = 0; w < PMLP_PPO_STAT_THREADS / WAVE; w++) t += part[w][threadIdx.x];
    stats[threadIdx.x] = t;
  }
}

// The statistics of a PPO call (bbx_pmlp_ppo_grad, bbx_pmlp2_ppo_grad) from the tail the loss epilogue wrote: stats[0..5] = counted
// positions, sum u_k, sum H_k, sum (old_k - new_k), positions clipped, positions not counted; the sums in double over the float32
// terms.  ONE workgroup of PMLP_PPO_STAT_THREADS threads: thread t adds positions t, t + threads, ..., then pmlp_stats_sum.  No
// atomics, and a partition that depends on n alone.  n == 0: zeros.
static __global__ __launch_bounds__(PMLP_PPO_STAT_THREADS) void bbx_pmlp_ppo_stats_kernel(const float* __restrict__ tail, int n_, double* __restrict__ stats) {
  const size_t n = (size_t)n_;
  const int32_t* flags = (const int32_t*)tail + 3 * n;
  double acc[6] = {0., 0., 0., 0., 0., 0.};
  for (size_t k = threadIdx.x; k < n; k += PMLP_PPO_STAT_THREADS) {
    const int f = flags[k];
    if (f & PMLP_LOSS_COUNTED) {
      acc[0] += 1.; acc[1] += (double)tail[k]; acc[2] += (double)tail[n + k]; acc[3] += (double)tail[2 * n + k];
      if (f & PMLP_LOSS_CLIPPED) acc[4] += 1.;
    } else acc[5] += 1.;
  }
  pmlp_stats_sum(acc, stats);
}

// The statistics of a cross-entropy call (bbx_pmlp_xent_grad, bbx_pmlp2_xent_grad) from the tail its epilogue wrote: stats[0..5] =
// counted positions, sum w l, sum w T, sum H, sum w, positions not counted; the same workgroup, order and sums.  n == 0: zeros.
static __global__ __launch_bounds__(PMLP_PPO_STAT_THREADS) void bbx_pmlp_xent_stats_kernel(const float* __restrict__ tail, int n_, double* __restrict__ stats) {
  const size_t n = (size_t)n_;
  const int32_t* flags = (const int32_t*)tail + 4 * n;
  double acc[6] = {0., 0., 0., 0., 0., 0.};
  for (size_t k = threadIdx.x; k < n; k += PMLP_PPO_STAT_THREADS) {
    if (flags[k] & PMLP_LOSS_COUNTED) {
      acc[0] += 1.; acc[1] += (double)tail[k]; acc[2] += (double)tail[n + k]; acc[3] += (double)tail[2 * n + k]; acc[4] += (double)tail[3 * n + k];
    } else acc[5] += 1.;
  }
  pmlp_stats_sum(acc, stats);
}

// PMLP critic: a learned value baseline over the observation block the rollout has recorded (bbx_pmlp_value, bbx_pmlp_value_grad,
// bbx_pmlp_value_fit of include/bbx.h).  The model is the one-hidden-layer policy's — W1 [cols][hidden], b1, w2, b2, prepared by
// bbx_pmlp_prepare, the row score z_r = w2 . relu(W1^T x_r + b1) + b2 through pmlp_logits_wave, hence the policy kernels' bits —
// with a POOL over the n live rows of a state in place of the softmax:
//   BBX_POOL_SUM   V = sum_r z_r      lane t adds z_t, z_{t + 64}, ... in row order from 0.f, the lanes by wave_sum_f32      g_r = g
//   BBX_POOL_MEAN  V = that sum / (float)n   (an IEEE division)                                                            g_r = g / (float)n
//   BBX_POOL_LSE   V = pmlp_softmax_wave(...).logz                                               g_r = g (__expf(z_r - mx) (1.f / se))
// g_r: the coefficient of row r in dL/dz for L = sum_k g_k V_k, what the backward half is fed with.  n <= 0: V = 0.0f and no
// gradient (a finished state is worth nothing: what GAE assumes behind a done flag); ONE live row contributes like any other
// count (the policy kernel skips such a state: delta - p = 0 there, not here).
//
// Forward (bbx_pmlp_value_kernel): one wave per position.  FIT: lane 0 goes on to the squared-error epilogue (pmlp_fit_lane0).
// Backward (bbx_pmlp_value_grad_kernel): bbx_pmlp_grad_kernel's structure and partial layout with the pool's coefficients —
// waves stride over positions, unit groups over blockIdx.y, g_r over the scores in LDS, the hidden tile recomputed transposed,
// dW1 / db1 / dw2 / db2 in registers across the wave's states — so that bbx_pmlp_grad_reduce_kernel finishes the job unchanged and
// the workspace is bbx_pmlp_grad_workspace_floats(n, ...).  The back half is written again here (as pmlp_logits_wave was beside
// pmlp_act_wave): the policy's gradient kernel keeps its bits and its register budget.
// Statistics (bbx_pmlp_value_stats_kernel): one workgroup, the summation order of bbx_pmlp_ppo_stats_kernel.
#pragma once
#include "bbx_pmlp_grad.h"

// the squared-error epilogue of the forward kernel's FIT instantiations, called by lane 0 once a wave has V_k: float32, in this
// order, no contraction into fused multiply-adds:   d = V - target   u = d * d   coef = scale * d
// (L = scale 1/2 sum d^2: coef = dL/dV_k).  A NaN value (an index out of range) is not counted: zeros everywhere.
__device__ __forceinline__ void pmlp_fit_lane0(const PmlpFit& F, int k, float V) {
#pragma clang fp contract(off)
  const size_t n = (size_t)F.n;
  float coef = 0.f, u = 0.f, v = 0.f, t = 0.f;
  int flags = 0;
  if (V == V) {
    t = F.targets[k];
    const float d = V - t;
    u = d * d;
    coef = F.scale * d;
    v = V;
    flags = PMLP_LOSS_COUNTED;
  }
  F.coef[k] = coef;
  F.tail[k] = u; F.tail[n + k] = v; F.tail[2 * n + k] = t; ((int*)F.tail)[3 * n + k] = flags;
}
// what lane 0 of the forward kernel ends with: the value in either width (each may be null), then the epilogue
template <bool FIT>
__device__ __forceinline__ void pmlp_value_out(const PmlpFit& F, float* values, double* values64, int k, float V) {
  if (values) values[k] = V;
  if (values64) values64[k] = (double)V;
  if constexpr (FIT) pmlp_fit_lane0(F, k, V);
}

// the n > 0 scores in lg pooled (every lane returns the value)
__device__ __forceinline__ float pmlp_pool_wave(const float* lg, int n, int lane, int pool) {
  if (pool == PMLP_POOL_LSE) return pmlp_softmax_wave(lg, n, lane).logz;
  float acc = 0.f;
  for (int r = lane; r < n; r += WAVE) acc += lg[r];
  const float t = lane63_f32(wave_sum_f32(acc));
  return pool == PMLP_POOL_MEAN ? t / (float)n : t;           // (the correctly rounded division: hipcc's default for float)
}

template <int NB, int KS, bool IDX = false, bool FIT = false>
__global__ __launch_bounds__(256, 2) void bbx_pmlp_value_kernel(const int32_t* __restrict__ obs, const int32_t* __restrict__ rows, int B, int obs_rows,
                                                                int cols, const float* __restrict__ wp, int pool, float* __restrict__ values,
                                                                double* __restrict__ values64, const int32_t* __restrict__ index, int n_src,
                                                                PmlpFit fit) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = lane_id(), wave = uni((int)(threadIdx.x / WAVE));
  const int k = blockIdx.x * ((int)blockDim.x / WAVE) + wave;         // my position in the call
  if (k >= B) return;
  int s = k;                                                          // the recorded state it is about
  if constexpr (IDX) {
    s = uni(index[k]);
    if (s < 0 || s >= n_src) {
      if (lane == 0) pmlp_value_out<FIT>(fit, values, values64, k, __builtin_nanf(""));
      return;
    }
  }
  float* lg = (float*)smem + (size_t)wave * pmlp_lgcap(obs_rows);
  const int nraw = rows[s];
  const int n = pmlp_logits_wave<NB, KS>(lg, obs + (size_t)s * obs_rows * cols, nraw, obs_rows, cols, wp, lane & 31, lane >> 5);
  if (n <= 0) {
    if (lane == 0) pmlp_value_out<FIT>(fit, values, values64, k, 0.f);
    return;
  }
  wave_sync();
  const float V = pmlp_pool_wave(lg, n, lane, pool);
  if (lane == 0) pmlp_value_out<FIT>(fit, values, values64, k, V);
}

template <int NB, int KS, bool IDX = false>
__global__ __launch_bounds__(256, 2) void bbx_pmlp_value_grad_kernel(const int32_t* __restrict__ obs, const int32_t* __restrict__ rows, int B, int obs_rows,
                                                                     int cols, const float* __restrict__ wp, int pool, const float* __restrict__ gvalue,
                                                                     int nwaves, float* __restrict__ ws, const int32_t* __restrict__ index, int n_src) {
  constexpr int HP = 32 * NB;
  constexpr int CB = KS == 32 ? 2 : 1;                               // pmlp_grad_cb
  constexpr int UBW = NB < (CB == 2 ? 2 : 4) ? NB : (CB == 2 ? 2 : 4);   // pmlp_grad_ubw
  constexpr int UW = 32 * UBW, NG = NB / UBW;
  constexpr int PW = UW * (32 * CB + 2) + 4;                         // pmlp_grad_partial_floats
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = lane_id(), wave = uni((int)(threadIdx.x / WAVE));
  const int p = blockIdx.x * ((int)blockDim.x / WAVE) + wave;       // my place among the group's waves
  const int grp = blockIdx.y;                                        // my unit group: unit blocks grp UBW ...
  if (p >= nwaves) return;
  float* lg = (float*)smem + (size_t)wave * pmlp_grad_lgcap(obs_rows);
  const int lr = lane & 31, lk = lane >> 5;
  const float* wl = wp + lk * HP + grp * UW + lr;                    // my B-operand column: + 2 s HP + 32 u

  bbx_f32x16 dW[UBW][CB];
  float db1a[UBW], dw2a[UBW], db2a = 0.f;
#pragma unroll
  for (int u = 0; u < UBW; u++) {
    db1a[u] = 0.f; dw2a[u] = 0.f;
#pragma unroll
    for (int cb = 0; cb < CB; cb++)
#pragma unroll
      for (int v = 0; v < 16; v++) dW[u][cb][v] = 0.f;
  }

  for (int k = p; k < B; k += nwaves) {                               // position k of the call: recorded state s
    int s = k;
    bool in_src = true;
    if constexpr (IDX) {
      // an index out of range: no row, which the test below skips — and state 0 in its place for the addresses (the launcher
      // sees to n_src > 0), as in bbx_pmlp_grad_kernel
      s = uni(index[k]);
      in_src = s >= 0 && s < n_src;
      s = in_src ? s : 0;
    }
    const int nraw = in_src ? rows[s] : 0;
    const int32_t* ob = obs + (size_t)s * obs_rows * cols;
    wave_sync();                                                      // (the previous state's g_r have been read)
    // (the weights are the same for every state and tile: their base pointers are opaque per use, so that the optimiser does not
    // hoist hundreds of loads out of the loops into registers the dW1 accumulators need)
    const float* wq = wp;
    asm volatile("" : "+s"(wq));
    const int n = pmlp_logits_wave<NB, KS>(lg, ob, nraw, obs_rows, cols, wq, lr, lk);
    if (n <= 0) continue;                                             // no row: nothing (its gvalue is not read)
    wave_sync();
    const float g = gvalue[k];
    float mx = 0.f, rse = 0.f;
    if (pool == PMLP_POOL_LSE) { const PmlpSoftmax sm = pmlp_softmax_wave(lg, n, lane); mx = sm.mx; rse = 1.f / sm.se; }
    const float gm = pool == PMLP_POOL_MEAN ? g / (float)n : g;
    const int n32 = (n + 31) & ~31;
    for (int r = lane; r < n32; r += WAVE) {                          // (every lane reads and writes its own entries only)
      float gr = 0.f;
      if (r < n) gr = pool == PMLP_POOL_LSE ? g * (__expf(lg[r] - mx) * rse) : gm;
      lg[r] = gr; db2a += gr;
    }
    wave_sync();
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

  // the wave's partial sums, in bbx_pmlp_grad_kernel's layout: dW1 [32 CB][UW] | db1 [UW] | dw2 [UW] | db2
  float* part = ws + ((size_t)p * NG + grp) * PW;
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

// The statistics of a fit call (bbx_pmlp_value_fit) from the tail the epilogue wrote: stats[0..5] = counted positions, sum d^2,
// sum V, sum target, sum target^2 (the float32 product target * target), positions not counted; the sums in double over the
// float32 terms.  ONE workgroup of PMLP_PPO_STAT_THREADS threads in the order of bbx_pmlp_ppo_stats_kernel: thread t adds
// positions t, t + threads, ...; the lanes of a wave by a butterfly, the waves in order by one thread per statistic.  n == 0: zeros.
__global__ __launch_bounds__(PMLP_PPO_STAT_THREADS) void bbx_pmlp_value_stats_kernel(const float* __restrict__ tail, int n_, double* __restrict__ stats) {
#pragma clang fp contract(off)
  __shared__ double part[PMLP_PPO_STAT_THREADS / WAVE][6];
  const size_t n = (size_t)n_;
  const int32_t* flags = (const int32_t*)tail + 3 * n;
  double acc[6] = {0., 0., 0., 0., 0., 0.};
  for (size_t k = threadIdx.x; k < n; k += PMLP_PPO_STAT_THREADS) {
    if (flags[k] & PMLP_LOSS_COUNTED) {
      const float t = tail[2 * n + k], tt = t * t;
      acc[0] += 1.; acc[1] += (double)tail[k]; acc[2] += (double)tail[n + k]; acc[3] += (double)t; acc[4] += (double)tt;
    } else acc[5] += 1.;
  }
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

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
// Backward (bbx_pmlp_value_grad_kernel): bbx_pmlp_grad_kernel with the pool's coefficients in place of the policy's — the head,
// which writes g_r over the scores in LDS, is this kernel's own; the partition (waves stride over positions, unit groups over
// blockIdx.y), the accumulators, the transposed tile loop and the partial layout are PmlpGradWave (bbx_pmlp_grad.h), one code for
// both, so that bbx_pmlp_grad_reduce_kernel finishes the job and the workspace is bbx_pmlp_grad_workspace_floats(n, ...).
// Statistics (bbx_pmlp_value_stats_kernel): one workgroup, its own accumulation loop, then pmlp_stats_sum (bbx_pmlp_grad.h).
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
    const int32_t* ob = obs + (size_t)s * obs_rows * cols;
    const int n = G.logits(lg, ob, nraw, obs_rows, cols, wp);
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
      lg[r] = gr; G.db2a += gr;
    }
    wave_sync();
    G.tiles(lg, ob, n, cols);
  }
  G.store(ws, p, lane);
}

// The statistics of a fit call (bbx_pmlp_value_fit) from the tail the epilogue wrote: stats[0..5] = counted positions, sum d^2,
// sum V, sum target, sum target^2 (the float32 product target * target), positions not counted; the sums in double over the
// float32 terms.  ONE workgroup of PMLP_PPO_STAT_THREADS threads in the order of bbx_pmlp_ppo_stats_kernel: thread t adds
// positions t, t + threads, ..., then pmlp_stats_sum.  n == 0: zeros.
static __global__ __launch_bounds__(PMLP_PPO_STAT_THREADS) void bbx_pmlp_value_stats_kernel(const float* __restrict__ tail, int n_, double* __restrict__ stats) {
#pragma clang fp contract(off)
  const size_t n = (size_t)n_;
  const int32_t* flags = (const int32_t*)tail + 3 * n;
  double acc[6] = {0., 0., 0., 0., 0., 0.};
  for (size_t k = threadIdx.x; k < n; k += PMLP_PPO_STAT_THREADS) {
    if (flags[k] & PMLP_LOSS_COUNTED) {
      const float t = tail[2 * n + k], tt = t * t;
      acc[0] += 1.; acc[1] += (double)tail[k]; acc[2] += (double)tail[n + k]; acc[3] += (double)t; acc[4] += (double)tt;
    } else acc[5] += 1.;
  }
  pmlp_stats_sum(acc, stats);
}

// PMLP critic, TWO hidden layers (bbx_pmlp2_value, bbx_pmlp2_value_grad, bbx_pmlp2_value_fit of include/bbx.h): the one-layer critic
// of bbx_pmlp_value.h — its pools, its row-count conventions, its squared-error epilogue — over the two-layer policy's weights
// (bbx_pmlp2_prepare) and row scores z_r = w3 . relu(W2^T relu(W1^T x_r + b1) + b2) + b3 through pmlp2_logits_tile, hence the
// two-layer policy kernels' bits.  pmlp_pool_wave, pmlp_value_out and pmlp_fit_lane0 are bbx_pmlp_value.h's own.
//
// Forward (bbx_pmlp2_value_kernel): the frame of bbx_pmlp2_logprob_kernel — A2 | b2 | w3 staged in LDS once per workgroup, a wave
// per position, a grid-stride loop — with the pool in place of softmax and action.  FIT: lane 0 goes on to pmlp_fit_lane0.
// Backward: bbx_pmlp2_grad_kernel (bbx_pmlp2_grad.h) instantiated with the pool's head, Pmlp2ValueHead — the partition
// (pmlp2_grad_groups(n) workgroups), the f64 recomputation, the MFMA stages and the partial layout are the policy's, so that
// bbx_pmlp2_grad_reduce_kernel finishes the job and the workspace is bbx_pmlp2_grad_workspace_floats(n, ...).
// Statistics: bbx_pmlp_value_stats_kernel (bbx_pmlp_value.h, launched from bbx_aux.hip) over the same tail.
#pragma once
#include "bbx_pmlp2_grad.h"
#include "bbx_pmlp_value.h"

template <int HP1, int HP2, int KS, bool IDX = false, bool FIT = false>
__global__ __launch_bounds__(512) void bbx_pmlp2_value_kernel(const int32_t* __restrict__ obs, const int32_t* __restrict__ rows, int B, int obs_rows,
                                                              int cols, const float* __restrict__ wp, int pool, float* __restrict__ values,
                                                              double* __restrict__ values64, int lgcap, const int32_t* __restrict__ index, int n_src,
                                                              PmlpFit fit) {
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
  float* lg = a2 + A2F + 2 * HP2 + (size_t)wave * lgcap;                      // scores of this wave's state
  for (int k = (int)blockIdx.x * nw + wave; k < B; k += (int)gridDim.x * nw) {   // position k of the call: recorded state s
    int s = k;
    if constexpr (IDX) {
      s = uni(index[k]);
      if (s < 0 || s >= n_src) {
        if (lane == 0) pmlp_value_out<FIT>(fit, values, values64, k, __builtin_nanf(""));
        continue;
      }
    }
    int n = uni(rows[s]);
    n = n < obs_rows ? n : obs_rows; n = n < PMLP_MAXROWS ? n : PMLP_MAXROWS;
    if (n <= 0) {
      if (lane == 0) pmlp_value_out<FIT>(fit, values, values64, k, 0.f);
      continue;
    }
    const int32_t* ob = obs + (size_t)s * obs_rows * cols;
    wave_sync();                                                              // (the previous state's scores have been read)
    for (int r0 = 0; r0 < n; r0 += 16) pmlp2_logits_tile<HP1, HP2, KS>(lg, ob, r0, n, obs_rows, cols, W1p, b1p, a2, b2l, w3l, b3, lane);
    wave_sync();
    const float V = pmlp_pool_wave(lg, n, lane, pool);
    if (lane == 0) pmlp_value_out<FIT>(fit, values, values64, k, V);
  }
}

// The critic's head of the gradient kernel (the contract: Pmlp2PolicyHead, bbx_pmlp2_grad.h): every state with a live row
// contributes, ONE row too; g_r = g (sum), g / (float)n (mean), g (__expf(z_r - mx) (1.f / se)) (lse) — bbx_pmlp_value_grad_kernel's
struct Pmlp2ValueHead {
  static constexpr bool exact_a1 = true;                                      // (K_s = 1 for sum and mean: see the contract)
  const float* gvalue;
  int pool;
  __device__ __forceinline__ void state(int) const {}
  __device__ __forceinline__ bool takes(int n) const { return n > 0; }        // (no row: nothing, and its gvalue is not read)
  __device__ __forceinline__ void coefs(float* lg, int n, int k, int lane, float& db3) const {
    const float g = gvalue[k];
    float mx = 0.f, rse = 0.f;
    if (pool == PMLP_POOL_LSE) { const PmlpSoftmax sm = pmlp_softmax_wave(lg, n, lane); mx = sm.mx; rse = 1.f / sm.se; }   // (every wave for itself)
    const float gm = pool == PMLP_POOL_MEAN ? g / (float)n : g;
    const int n32 = (n + 31) & ~31;
    __syncthreads();                                                          // (every wave has read the scores)
    for (int r = (int)threadIdx.x; r < n32; r += (int)blockDim.x) {           // (every thread reads and writes its own entries only)
      float gr = 0.f;
      if (r < n) gr = pool == PMLP_POOL_LSE ? g * (__expf(lg[r] - mx) * rse) : gm;
      lg[r] = gr; db3 += gr;
    }
  }
};

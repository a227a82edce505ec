// What the host API and the launchers of the kernel files share: every bbx_launch_* prototype (defined in bbx_general.hip,
// bbx_binom.hip, bbx_fast.hip, bbx_wide.hip, bbx_aux.hip, bbx_pmlp2.hip, bbx_algebra.hip; called from bbx_api*.cpp, bbx_alg.cpp
// and, the four class launchers, bbx_aux.hip), the argument record of the algebra kernels, and the host-side launch helpers.
// Callers AND definers include it: the names have C linkage, so only a definition that sees its prototype is checked against it.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <mutex>

#include "bbx_common.h"
#include "bbx_pick.h"
#include "bbx_pmlp_shape.h"

struct AlgParams {                    // bbx_alg_kernel (bbx_algebra.hip), filled by bbx_alg.cpp
  char* recs; char* recs2;            // the lists; the lists minimalize / interreduce build
  BbxLayout L;
  int32_t n, op, elim;
  const int32_t* args;                // [n][4] operands: element indices i, j (binary operations), dividend index and number of divisors (reduce)
  int32_t* out;                       // [n][4]: {status (0 = done), reduction steps, -, -}
};

// ---- the step kernels: bbx_launch_step (bbx_aux.hip) picks the class launcher
extern "C" int bbx_launch_step(const BbxParams* p, BbxKernel kind, int envs_per_block, hipStream_t stream);
extern "C" int bbx_launch_general(const BbxParams* p, BbxKernel kind, int blocks, int threads, size_t lds, hipStream_t stream);
extern "C" int bbx_launch_binom(const BbxParams* p, BbxKernel kind, int blocks, int threads, size_t lds, hipStream_t stream);
extern "C" int bbx_launch_fast(const BbxParams* p, int blocks, int threads, int envs_per_block, hipStream_t stream);
extern "C" int bbx_launch_wide(const BbxParams* p, int nw, hipStream_t stream);
// ---- housekeeping (bbx_aux.hip)
extern "C" int bbx_launch_clone(const char* src_recs, char* dst_recs, const BbxLayout* L, const int32_t* src, const int32_t* dst, int n,
                                const uint32_t* seeds, int keep_counters, int seed_std, int ngen, uint8_t* flags, hipStream_t stream);
extern "C" int bbx_launch_value_resort(char* recs, const BbxLayout* L, int n, const uint8_t* flags, hipStream_t stream);
extern "C" int bbx_launch_value_iota(int32_t* idx, int n, hipStream_t stream);
extern "C" int bbx_launch_value_seeds(const int64_t* seeds, uint32_t* states, int n, hipStream_t stream);
extern "C" int bbx_launch_value_collect_device(const char* recs, uint32_t rec_bytes, int n, double* values, uint32_t* word, int only_nan, hipStream_t stream);
extern "C" int bbx_launch_av_offsets(const char* recs, uint32_t rec_bytes, int B, int max_rows, int32_t* out, hipStream_t stream);
extern "C" int bbx_launch_av_expand(const int32_t* off, int B, int first, int n, int32_t* src, int32_t* act, hipStream_t stream);
extern "C" int bbx_launch_av_fill(double* q, double* rewards, uint8_t* dones, size_t cells, uint32_t* word, hipStream_t stream);
extern "C" int bbx_launch_av_collect(const char* recs, uint32_t rec_bytes, int n, const int32_t* src, const int32_t* act, const double* rew,
                                     const uint8_t* done, double gamma, int max_rows, double* q, double* rewards, uint8_t* dones, uint32_t* word,
                                     hipStream_t stream);
extern "C" int bbx_launch_gae(const double* rewards, const double* values, const uint8_t* dones, int T, int B, double gam, double gl,
                              const double* last_values, double* returns, double* advantages, uint8_t* complete, double* lambda_returns,
                              hipStream_t stream);
extern "C" int bbx_launch_episodes(const double* rewards, const uint8_t* dones, int T, int B, double* carry_return, int32_t* carry_len, int32_t* ep_count,
                                   double* ep_return, int32_t* ep_len, hipStream_t stream);
extern "C" int bbx_launch_relayout(const char* src_recs, char* dst_recs, const BbxLayout* Ls, const BbxLayout* Ld, int B, hipStream_t stream);
extern "C" int bbx_launch_ctl(unsigned long long* ctl, unsigned long long value, hipStream_t stream);
extern "C" int bbx_launch_gather_lite(const char* recs, uint32_t rec_bytes, int B, void* out, hipStream_t stream);
extern "C" int bbx_launch_gather_hdr(const char* recs, uint32_t rec_bytes, int B, BbxHdr* out, hipStream_t stream);
extern "C" int bbx_launch_scatter_queue(const uint32_t* stage, int n, uint32_t ring_words, uint32_t* q, int32_t* tail, hipStream_t stream);
extern "C" int bbx_launch_obs_pack(const int32_t* padded, int cap, int cols, const int32_t* rows, int B, int32_t* off, int32_t* packed, hipStream_t stream);
extern "C" int bbx_launch_init(char* recs, uint32_t rec_bytes, int B, const uint32_t* agent_seeds, hipStream_t stream);
extern "C" int bbx_launch_mark_reset(char* recs, uint32_t rec_bytes, int B, const uint8_t* mask, hipStream_t stream);
// ---- polynomial algebra (bbx_algebra.hip)
extern "C" int bbx_launch_alg(const AlgParams* p, hipStream_t stream);
extern "C" int bbx_launch_alg_from_envs(const char* src_recs, const BbxLayout* Ls, const int32_t* idx, int n, char* dst_recs, const BbxLayout* Ld, hipStream_t stream);
// ---- the PMLP policy with one hidden layer (bbx_aux.hip)
extern "C" int bbx_launch_pmlp_prepare(const float* w1, const float* b1, const float* w2, float b2, int cols, int hidden, float* out, hipStream_t stream);
extern "C" int bbx_launch_pmlp_act(const int32_t* obs, const int32_t* rows, int B, int obs_rows, int cols, const float* wp, int hidden, const float* u,
                                   int32_t* actions, float* logprobs, int greedy, hipStream_t stream);   // (greedy: the argmax, u unread)
// the training launchers take the records of bbx_pmlp_shape.h (states, network, gradient outputs) and their head's own arguments
// (loss / fit: null, or the arguments of the forward kernel's epilogue)
extern "C" int bbx_launch_pmlp_logprob(const PmlpStates& s, const PmlpNet& net, const int32_t* actions, float* logprobs, float* entropy, const PmlpLoss* loss,
                                       hipStream_t stream);
extern "C" int bbx_launch_pmlp_ppo_stats(const float* tail, int n, double* stats, hipStream_t stream);
extern "C" int bbx_launch_pmlp_grad(const PmlpStates& s, const PmlpNet& net, const int32_t* actions, const float* glogp, const float* gent, const PmlpGrads& g,
                                    hipStream_t stream);
extern "C" int bbx_launch_pmlp_xent(const PmlpStates& s, const PmlpNet& net, const PmlpXent& x, float* losses, float* entropy, hipStream_t stream);
extern "C" int bbx_launch_pmlp_xent_stats(const float* tail, int n, double* stats, hipStream_t stream);
extern "C" int bbx_launch_pmlp_xent_grad(const PmlpStates& s, const PmlpNet& net, const float* targets, const float* coef, const PmlpGrads& g, hipStream_t stream);
extern "C" int bbx_launch_pmlp_value(const PmlpStates& s, const PmlpNet& net, int pool, float* values, double* values64, const PmlpFit* fit, hipStream_t stream);
extern "C" int bbx_launch_pmlp_value_stats(const float* tail, int n, double* stats, hipStream_t stream);
extern "C" int bbx_launch_pmlp_value_grad(const PmlpStates& s, const PmlpNet& net, int pool, const float* gvalue, const PmlpGrads& g, hipStream_t stream);
// ---- ... with two or three hidden layers (bbx_pmlp2.hip), which size their launch by the device (cus, max_lds: bbx_host::DeviceInfo)
extern "C" int bbx_launch_pmlp2_prepare(const float* w1, const float* b1, const float* wm, const float* bm, const float* w2, const float* b2,
                                        const float* wd, const float* bd, int cols, int h1, int hm, int h2, float* out, hipStream_t stream);
extern "C" int bbx_launch_pmlp2_act(const int32_t* obs, const int32_t* rows, int B, int obs_rows, int cols, const float* wp, int h1, int hm, int h2,
                                    const float* u, int32_t* actions, float* logprobs, int greedy, int cus, int max_lds, hipStream_t stream);   // (hm = 0: no middle layer)
extern "C" int bbx_launch_pmlp2_logprob(const PmlpStates& s, const PmlpNet& net, const int32_t* actions, float* logprobs, float* entropy, const PmlpLoss* loss,
                                        int cus, int max_lds, hipStream_t stream);
extern "C" int bbx_launch_pmlp2_grad(const PmlpStates& s, const PmlpNet& net, const int32_t* actions, const float* glogp, const float* gent, const PmlpGrads& g,
                                     int max_lds, hipStream_t stream);
extern "C" int bbx_launch_pmlp2_xent(const PmlpStates& s, const PmlpNet& net, const PmlpXent& x, float* losses, float* entropy, int cus, int max_lds,
                                     hipStream_t stream);
extern "C" int bbx_launch_pmlp2_xent_grad(const PmlpStates& s, const PmlpNet& net, const float* targets, const float* coef, const PmlpGrads& g, int max_lds,
                                          hipStream_t stream);
extern "C" int bbx_launch_pmlp2_value(const PmlpStates& s, const PmlpNet& net, int pool, float* values, double* values64, const PmlpFit* fit, int cus,
                                      int max_lds, hipStream_t stream);
extern "C" int bbx_launch_pmlp2_value_grad(const PmlpStates& s, const PmlpNet& net, int pool, const float* gvalue, const PmlpGrads& g, int max_lds,
                                           hipStream_t stream);

// ------------------------------------------------------------------ host-side launch helpers (the launchers' own)
static_assert(BBX_PICK_NONE == (int)hipErrorInvalidValue, "bbx_pick refuses an unlisted value with hipErrorInvalidValue");

// launch Kern; the arguments have the kernel's parameter types exactly.  Returns 0: launch errors are hipGetLastError's (bbx_launched)
template <auto Kern, class... A>
static int bbx_launch(dim3 grid, int threads, size_t lds, hipStream_t stream, A... args) {
  void (*const kern)(A...) = Kern;
  void* argv[] = {(void*)&args...};
  (void)hipLaunchKernel((const void*)kern, grid, dim3(threads), argv, lds, stream);
  return 0;
}
// launch Kern with `lds` bytes of dynamic LDS: the one place that raises a kernel's dynamic-LDS limit, which more than 64 KB
// needs.  The call is not free and the attribute belongs to the current device's code object: a high-water mark per device and
// kernel, published once the call has succeeded, and a call only for more than that.  Returns that call's error, or 0.
template <auto Kern, class... A>
static int launch_lds(int blocks, int threads, size_t lds, hipStream_t stream, A... args) {
  void (*const kern)(A...) = Kern;                          // (the arguments have the kernel's parameter types exactly)
  static std::mutex mu; static std::atomic<size_t> mark[64];
  int dev = 0; (void)hipGetDevice(&dev);
  std::atomic<size_t>& m = mark[dev & 63];
  if (m.load(std::memory_order_acquire) < lds) {
    std::lock_guard<std::mutex> g(mu);                      // (of two threads the smaller request must not lower the limit behind the larger)
    if (m.load(std::memory_order_relaxed) < lds) {
      const hipError_t err = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (err != hipSuccess) return (int)err;
      m.store(lds, std::memory_order_release);
    }
  }
  return bbx_launch<Kern>(dim3(blocks), threads, lds, stream, args...);
}
// what a launcher returns: the code of a refused or failed launch helper, otherwise hipGetLastError()
static inline int bbx_launched(int rc) { return rc ? rc : (int)hipGetLastError(); }

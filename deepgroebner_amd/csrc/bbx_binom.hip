// Binomial class of the step kernel (bbx_binom.h): launcher of the HBM-resident, LDS-staged and aux kernels.
#include "bbx_device.h"
#include "bbx_pmlp.h"
#include "bbx_binom.h"

template <int W>
static int launch_binom_w(const BbxParams* p, BbxKernel kind, int blocks, int threads, size_t lds, hipStream_t stream) {
  const bool trace = p->trace != nullptr;
  if (kind == BBX_K_AUX) { hipLaunchKernelGGL(bbx_binom_aux_kernel<W>, dim3(blocks), dim3(threads), lds, stream, *p); return 0; }
  if (kind == BBX_K_STAGED)
    return trace ? launch_lds<bbx_binom_kernel<W, true, true>>(blocks, threads, lds, stream, *p) : launch_lds<bbx_binom_kernel<W, true, false>>(blocks, threads, lds, stream, *p);
  lds = (size_t)(threads / WAVE) * update_lds_bytes<W>();           // Gebauer-Moeller peel scratch, one per wave
  const size_t lds_plain = W == 4 ? (size_t)(threads / WAVE) * BC_BYTES : lds;   // 16-byte monomials: the LDS copy instead (BEnvC)
  if constexpr (W == 2 || W == 4) {
    if (p->policy && p->policy->rollout) {               // a policy rollout: its continuation pass, or the whole of it
      BbxParams q = *p; q.policy = nullptr; q.actions = nullptr; q.rewards = nullptr; q.dones = nullptr; q.rows = nullptr; q.obs_every_step = 0;
      const int cols = 2 * p->nvars * p->k, nb = pmlp_nb_for(p->policy->hidden), ks = pmlp_ks_for(cols);
      const size_t lds_pol = (size_t)(threads / WAVE) * binom_scratch_bytes<W>(q.obs_rows);
      if (p->policy->hidden2 > 0) {                        // two hidden layers
        if (!pmlp2_step_has(W, cols, p->policy->hidden, p->policy->hidden2)) return (int)hipErrorInvalidValue;   // (what bbx_api_policy.cpp admits by)
        const int h1 = pmlp2_hp_for(p->policy->hidden), h2 = pmlp2_hp_for(p->policy->hidden2), k2 = pmlp2_ks_for(cols);
#define BBX_BPOL2(A, C, KSV) hipLaunchKernelGGL((bbx_binom_policy2_kernel<W, A, C, KSV>), dim3(blocks), dim3(threads), lds_pol, stream, q, *p->policy)
#define BBX_BPOL2_H(KSV) do { if (h1 == 64 && h2 == 64) BBX_BPOL2(64, 64, KSV); else if (h1 == 64) BBX_BPOL2(64, 128, KSV); \
                              else if (h2 == 64) BBX_BPOL2(128, 64, KSV); else BBX_BPOL2(128, 128, KSV); } while (0)
        if (k2 == 3) BBX_BPOL2_H(3);
        else if constexpr (W == 4) { if (k2 == 8) BBX_BPOL2_H(8); else return (int)hipErrorInvalidValue; }
        else return (int)hipErrorInvalidValue;
#undef BBX_BPOL2_H
#undef BBX_BPOL2
        return 0;
      }
#define BBX_BPOL(NBV, KSV) hipLaunchKernelGGL((bbx_binom_policy_kernel<W, NBV, KSV>), dim3(blocks), dim3(threads), lds_pol, stream, q, *p->policy)
      if (!pmlp_step_has(W, cols, p->policy->hidden)) return (int)hipErrorInvalidValue;
      if (ks == 6) { if (nb == 2) BBX_BPOL(2, 6); else BBX_BPOL(4, 6); }
      else if (W == 4 && ks == 10) { if (nb == 2) BBX_BPOL(2, 10); else BBX_BPOL(4, 10); }
      else return (int)hipErrorInvalidValue;             // (unreachable behind pmlp_step_has)
#undef BBX_BPOL
      return 0;
    }
  }
  lds = lds_plain;
  if (trace) hipLaunchKernelGGL((bbx_binom_kernel<W, false, true>), dim3(blocks), dim3(threads), lds, stream, *p);
  else hipLaunchKernelGGL((bbx_binom_kernel<W, false, false>), dim3(blocks), dim3(threads), lds, stream, *p);
  return 0;
}
extern "C" int bbx_launch_binom(const BbxParams* p, BbxKernel kind, int blocks, int threads, size_t lds, hipStream_t stream) {
  return p->L.W == 2 ? launch_binom_w<2>(p, kind, blocks, threads, lds, stream)
       : p->L.W == 4 ? launch_binom_w<4>(p, kind, blocks, threads, lds, stream) : launch_binom_w<8>(p, kind, blocks, threads, lds, stream);
}
#ifdef BBX_PROF_BUILD
extern "C" int bbx_bin_prof_read(unsigned long long* out, int reset) {   // diagnostic build only
  hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(bbx_bin_prof_acc), 32 * sizeof(unsigned long long));
  if (e == hipSuccess && reset) { unsigned long long z[32] = {0}; e = hipMemcpyToSymbol(HIP_SYMBOL(bbx_bin_prof_acc), z, sizeof z); }
  return (int)e;
}
#endif

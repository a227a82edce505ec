// Binomial class of the step kernel (bbx_binom.h): launcher of the HBM-resident, LDS-staged and aux kernels.
#include "bbx_device.h"
#include "bbx_launch.h"
#include "bbx_pmlp.h"
#include "bbx_binom.h"

template <int W>
static int launch_binom_w(const BbxParams* p, BbxKernel kind, int blocks, int threads, size_t lds, hipStream_t stream) {
  const bool trace = p->trace != nullptr;
  return bbx_pick_bool(p->episode_limit != 0, [&](auto LIM) {   // (an episode step limit set: the LIM instantiations, bbx_binom.h)
  if (kind == BBX_K_AUX) return bbx_launch<bbx_binom_aux_kernel<W>>(dim3(blocks), threads, lds, stream, *p);
  if (kind == BBX_K_STAGED)
    return bbx_pick_bool(trace, [&](auto TRACE) { return launch_lds<bbx_binom_kernel<W, true, TRACE(), LIM()>>(blocks, threads, lds, stream, *p); });
  if constexpr (W == 2 || W == 4) {
    if (p->policy && p->policy->rollout) {               // a policy rollout: its continuation pass, or the whole of it
      BbxParams q = *p; q.policy = nullptr; q.actions = nullptr; q.rewards = nullptr; q.dones = nullptr; q.rows = nullptr; q.obs_every_step = 0;
      const BbxPolicy& pol = *p->policy;
      const int cols = 2 * p->nvars * p->k;
      const size_t lds_pol = (size_t)(threads / WAVE) * binom_scratch_bytes<W>(q.obs_rows);
      if (pol.hidden2 > 0) {                               // two hidden layers: 3 k-steps, or 8 with 16-byte monomials
        if (!pmlp2_step_has(W, cols, pol.hidden, pol.hidden2)) return (int)hipErrorInvalidValue;   // (what bbx_api_policy.cpp admits by)
        return bbx_pick<3, 8>(pmlp2_ks_for(cols), [&](auto KS) { return bbx_pick<64, 128>(pmlp2_hp_for(pol.hidden), [&](auto H1) {
          return bbx_pick<64, 128>(pmlp2_hp_for(pol.hidden2), [&](auto H2) {
            if constexpr (KS() == 8 && W != 4) return (int)hipErrorInvalidValue;
            else return bbx_launch<bbx_binom_policy2_kernel<W, H1(), H2(), KS(), LIM()>>(dim3(blocks), threads, lds_pol, stream, q, pol);
          }); }); });
      }
      if (!pmlp_step_has(W, cols, pol.hidden)) return (int)hipErrorInvalidValue;
      return bbx_pick<6, 10>(pmlp_ks_for(cols), [&](auto KS) { return bbx_pick<2, 4>(pmlp_nb_for(pol.hidden), [&](auto NB) {   // 6 k-steps, or 10 with 16-byte monomials
        if constexpr (KS() == 10 && W != 4) return (int)hipErrorInvalidValue;
        else return bbx_launch<bbx_binom_policy_kernel<W, NB(), KS(), LIM()>>(dim3(blocks), threads, lds_pol, stream, q, pol);
      }); });
    }
  }
  // Gebauer-Moeller peel scratch, one per wave; 16-byte monomials: the LDS copy instead (BEnvC)
  const size_t peel = (size_t)(threads / WAVE) * (W == 4 ? BC_BYTES : update_lds_bytes<W>());
  return bbx_pick_bool(trace, [&](auto TRACE) { return bbx_launch<bbx_binom_kernel<W, false, TRACE(), LIM()>>(dim3(blocks), threads, peel, stream, *p); });
  });
}
extern "C" int bbx_launch_binom(const BbxParams* p, BbxKernel kind, int blocks, int threads, size_t lds, hipStream_t stream) {
  return bbx_pick<2, 4, 8>((int)p->L.W, [&](auto W) { return launch_binom_w<W()>(p, kind, blocks, threads, lds, stream); });
}
#ifdef BBX_PROF_BUILD
extern "C" int bbx_bin_prof_read(unsigned long long* out, int reset) {   // diagnostic build only
  hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(bbx_bin_prof_acc), 32 * sizeof(unsigned long long));
  if (e == hipSuccess && reset) { unsigned long long z[32] = {0}; e = hipMemcpyToSymbol(HIP_SYMBOL(bbx_bin_prof_acc), z, sizeof z); }
  return (int)e;
}
#endif

// Hand-tuned register/LDS-resident kernel of the headline class (bbx_fast.h): launcher.
#include "bbx_device.h"
#include "bbx_launch.h"
#include "bbx_pmlp.h"
#include "bbx_binom.h"
#include "bbx_fast.h"

#ifdef BBX_PROF_BUILD
static unsigned long long bbx_fast_prof_acc[8];           // diagnostic build only: phase cycle sums over the launches since the last read
extern "C" int bbx_fast_prof_read(unsigned long long* out, int reset) {
  for (int i = 0; i < 8; i++) { out[i] = bbx_fast_prof_acc[i]; if (reset) bbx_fast_prof_acc[i] = 0; }
  return 0;
}
#endif

// kind 3: the hand-tuned LDS/register-resident kernel (bbx_fast.h) for W == 2 binomial, GM, sorted reducers
extern "C" int bbx_launch_fast(const BbxParams* p, int blocks, int threads, int envs_per_block, hipStream_t stream) {
  BbxFastParams f{};
  f.recs = p->recs; f.qwords = p->q.words; f.qtail = p->q.tail; f.inv_table = p->inv_table;
  f.actions = p->actions; f.rewards = p->rewards; f.dones = p->dones; f.rows = p->rows; f.obs = p->obs; f.trace = p->trace;
  f.rec_bytes = p->L.rec_bytes; f.hbmG = p->L.maxG;
  f.q_env_stride = p->q.env_stride; f.q_slot_words = p->q.slot_words; f.q_nslots = p->q.nslots; f.q_fixed = p->q.fixed;
  f.B = p->B; f.nsteps = p->nsteps; f.obs_rows = p->obs_rows; f.trace_stride = p->trace_stride; f.k = p->k; f.nvars = p->nvars;
  f.lim_G = p->fast_G; f.lim_P = p->fast_P;
  f.agent = p->agent; f.auto_reset = p->auto_reset; f.set_budget = p->set_budget; f.pass = p->pass;
  f.obs_every_step = p->obs_every_step; f.obs_fill = p->obs_fill; f.rewards_mode = p->rewards_mode;
  f.lite = p->lite; f.done_seq = p->done_seq;
  f.gen = p->gen;
  f.sort_input = p->sort_input;
  f.ctl = p->ctl; f.sess_target = p->sess_target; f.ctl_stats = p->ctl_stats; f.slice_ticks = p->slice_ticks; f.mbox = p->mbox;
  f.gamma = p->gamma; f.values = p->values;
  f.episode_limit = p->episode_limit;
  // (four workgroups of four waves per CU, one wave per SIMD each: 4 x 4 x 9472 = 151,552 of the CU's 163,840 bytes; a layout that
  // no longer fits would lose the fourth workgroup without a word)
  static_assert(4 * 4 * FLay<FNBK_WIDE>::BYTES == 151552 && 4 * 4 * FLay<FNBK_WIDE>::BYTES <= 163840, "fast class: 16 environments per CU");
  const size_t lds = (size_t)envs_per_block * FLay<FNBK_WIDE>::BYTES, lds_pol = (size_t)envs_per_block * FLay<FNBK_POL>::BYTES;
#ifdef BBX_PROF_BUILD
  static unsigned long long* d_prof = nullptr;
  if (getenv("BBX_PROF") && !p->trace) {          // diagnostic: per-phase cycle sums, printed here and summed for bbx_fast_prof_read()
    if (!d_prof) (void)hipMalloc((void**)&d_prof, (size_t)p->B * 8 * sizeof(unsigned long long));
    f.prof = d_prof;
    bbx_launch<bbx_fast_prof_kernel>(dim3(blocks), threads, lds, stream, f);
    (void)hipStreamSynchronize(stream);
    std::vector<unsigned long long> h((size_t)p->B * 8);
    (void)hipMemcpy(h.data(), d_prof, h.size() * 8, hipMemcpyDeviceToHost);
    double s[8] = {0}; for (int e = 0; e < p->B; e++) for (int i = 0; i < 8; i++) s[i] += (double)h[(size_t)e * 8 + i];
    double tot = 0; for (int i = 0; i < 8; i++) { tot += s[i]; bbx_fast_prof_acc[i] += (unsigned long long)s[i]; }
    fprintf(stderr, "[bbx prof] nsteps=%d ticks/step/env:", p->nsteps);
    for (int i = 0; i < 8; i++) fprintf(stderr, " p%d=%.0f(%.0f%%)", i, s[i] / p->B / (p->nsteps ? p->nsteps : 1), 100.0 * s[i] / tot);
    fprintf(stderr, "\n");
    return 0;
  }
#endif
  if (p->policy) {                                         // policy + step in one launch
    BbxFastPolicyParams q; q.f = f; q.pol = *p->policy;
    const int cols = 2 * f.k * f.nvars;                    // (the shapes built in: the predicates bbx_api_policy.cpp admits a call by)
    if (!(!q.pol.rollout ? pmlp_fused_step_has(cols, q.pol.hidden) : q.pol.hidden2 > 0 ? pmlp2_step_has(2, cols, q.pol.hidden, q.pol.hidden2)
                                                                                       : pmlp_step_has(2, cols, q.pol.hidden))) return (int)hipErrorInvalidValue;
    q.f.agent = BBX_AGENT_EXTERNAL; q.f.actions = q.pol.actions;
    if (q.pol.rollout) {                                   // nsteps steps, the policy inside the step loop (3 variables, k = 2)
      q.f.actions = nullptr; q.f.rewards = nullptr; q.f.dones = nullptr; q.f.rows = q.pol.post_obs ? q.pol.rows_t : nullptr; q.f.obs_every_step = 0; q.f.auto_reset = 1;
      if (q.pol.hidden2 > 0) {                             // two hidden layers: envs_per_block = BBX_POL2_WAVES (plan_launch)
        const int h1 = pmlp2_hp_for(q.pol.hidden), h2 = pmlp2_hp_for(q.pol.hidden2);
        // per wave its state and the logits of up to 256 rows (5.5 KB), per workgroup the layers behind the first (65 KB at 128 x 128):
        // 16 waves = 153 KB of the CU's 160
        static_assert((size_t)BBX_POL2_WAVES * (FLay<FNBK_POL>::BYTES + 4 * FLay<FNBK_POL>::P) + ((size_t)128 * 128 + 2 * 128 + 4) * sizeof(float) == 156688,
                      "policy2<128,128>: the workgroup's LDS (the CU holds 163,840 bytes)");
        const size_t rl2 = (size_t)envs_per_block * (FLay<FNBK_POL>::BYTES + 4 * FLay<FNBK_POL>::P) + ((size_t)h1 * h2 + 2 * h2 + 4) * sizeof(float);
        return bbx_pick<64, 128>(h1, [&](auto H1) { return bbx_pick<64, 128>(h2, [&](auto H2) {
          return bbx_pick_bool(q.f.episode_limit != 0, [&](auto LIM) {
            return launch_lds<bbx_fast_policy2_rollout_kernel<H1(), H2(), LIM()>>(blocks, threads, rl2, stream, q); }); }); });
      }
      const size_t rl = (size_t)envs_per_block * (FLay<FNBK_POL>::BYTES + 4 * FLay<FNBK_POL>::P) + ((size_t)(2 * 6 + 2) * 32 * pmlp_nb_for(q.pol.hidden) + 4) * sizeof(float);
      const int nb = pmlp_nb_for(q.pol.hidden);
      if (p->ctl)                                          // per-step calls served by a persistent session
        return bbx_pick<2, 4>(nb, [&](auto NB) { return bbx_launch<bbx_fast_policy_session_kernel<NB()>>(dim3(blocks), threads, rl, stream, q); });
      return bbx_pick<2, 4>(nb, [&](auto NB) { return bbx_launch<bbx_fast_policy_rollout_kernel<NB()>>(dim3(blocks), threads, rl, stream, q); });
    }
    const size_t pl = pmlp_lds_bytes(envs_per_block, f.obs_rows), ll = pl > lds_pol ? pl : lds_pol;
    return bbx_pick<3, 6>(pmlp_ks_for(cols), [&](auto KS) { return bbx_pick<2, 4>(pmlp_nb_for(q.pol.hidden), [&](auto NB) {
      return bbx_launch<bbx_fast_policy_kernel<NB(), KS()>>(dim3(blocks), threads, ll, stream, q); }); });
  }
  if (p->value_mode) return bbx_launch<bbx_fast_value_kernel>(dim3(blocks), threads, lds, stream, f);   // (lean, untraced: bbx_api.cpp)
  // the headline shape: what bbx_fast_headline[_persistent]_kernel is specialised for
  // (bbx_common.h; with an episode step limit set it is the general lean kernel that runs: the headline kernels know none)
  const bool headline = bbx_headline_shape(*p);
  if (p->ctl) {                                            // the kernel of a persistent session (bbx_api.cpp admits lean, untraced launches only)
    if (headline) return bbx_launch<bbx_fast_headline_persistent_kernel>(dim3(blocks), threads, lds, stream, f);
    return bbx_launch<bbx_fast_persistent_kernel>(dim3(blocks), threads, lds, stream, f);
  }
  if (p->trace) return bbx_launch<bbx_fast_kernel<true, true>>(dim3(blocks), threads, lds, stream, f);
  if (p->accounting) return bbx_launch<bbx_fast_kernel<false, true>>(dim3(blocks), threads, lds, stream, f);
  if (headline) return bbx_launch<bbx_fast_headline_kernel>(dim3(blocks), threads, lds, stream, f);
  return bbx_launch<bbx_fast_kernel<false, false>>(dim3(blocks), threads, lds, stream, f);
}

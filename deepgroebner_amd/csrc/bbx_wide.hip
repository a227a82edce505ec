// Wide class (one workgroup per environment, bbx_wide.h): launcher.  nw = waves per environment.
#include "bbx_device.h"
#include "bbx_launch.h"
#include "bbx_wide.h"

extern "C" int bbx_launch_wide(const BbxParams* p, int nw, hipStream_t stream) {
    BbxParams q = *p;                                      // LDS capacities of the workgroup (terms): forced by the caller or
    const int W_ = (int)q.L.W;                             // as large as the residency aimed at allows
    // lean variants: random and external agents let h grow long — reducer tails collect in an LDS accumulator and h is
    // rewritten only when it is full (LAZY); the ordering strategies keep h short — plain eager merges without the
    // accumulator's bookkeeping
    const bool strategy = q.agent == BBX_AGENT_DEGREE || q.agent == BBX_AGENT_FIRST || q.agent == BBX_AGENT_NORMAL || q.agent == BBX_AGENT_SUGAR ||
                          q.agent == BBX_AGENT_LAST || q.agent == BBX_AGENT_CODEGREE || q.agent == BBX_AGENT_STRANGE || q.agent == BBX_AGENT_SPICE;
    bool lazy = !q.accounting && !strategy;
    if (W_ == 8) lazy = false;                             // (32-byte monomials have no sort key: the accumulator holds keys)
    const bool acct = q.accounting != 0;
    bool one_per_cu = false;
    if (q.wide_hc > 0) {                                   // forced capacities (tests, experiments): as asked, as far as 160 KB go
      q.wide_hc = (q.wide_hc + 7) & ~7;
      while (q.wide_hc > 8 && wide_lds_bytes(W_, q.wide_hc, q.wide_hc, q.wide_hc, lazy ? q.wide_hc : 0) > 160u * 1024u) q.wide_hc -= 8;
      q.wide_fc = q.wide_hc; q.wide_rc = q.wide_hc; q.wide_sc = lazy ? q.wide_hc : 0;
    }
    else {
      const int ncu = q.wide_ncu > 0 ? q.wide_ncu : 256;   // (plan_launch: the device's CUs; unknown: as many as the largest part has)
      // one workgroup per CU while the batch fits that way (160 KB each), otherwise two per CU (80 KB each)
      const bool one = q.B <= ncu || q.wide_tail == 2;     // (the tail kernel: the workgroups with work left fit one per CU)
      one_per_cu = one;
      const size_t budget = one ? 160u * 1024u : 80u * 1024u;
      // (without the accumulator's two buffers the reducer table can hold twice as many reducers)
      q.wide_fc = one ? 1024 : 512; q.wide_rc = one ? (lazy ? 1024 : 2048) : (lazy ? 704 : 1024); q.wide_sc = lazy ? (one ? 1536 : 1024) : 0;
      const size_t fixed = wide_lds_bytes(W_, 0, q.wide_fc, q.wide_rc, q.wide_sc);
      q.wide_hc = (int)((budget - fixed) / 20) & ~63;       // a term in LDS: 8-byte sort key + u16 coefficient, two buffers
      while (wide_lds_bytes(W_, q.wide_hc, q.wide_fc, q.wide_rc, q.wide_sc) > budget) q.wide_hc -= 64;
    }
    const size_t wl = wide_lds_bytes(W_, q.wide_hc, q.wide_fc, q.wide_rc, q.wide_sc);
    const bool tr = q.trace != nullptr;
    const int threads = nw * WAVE;
    // (an episode step limit set: the LIM instantiations, bbx_wide.h; off: the kernels as they were before the limit existed)
    int rc = bbx_pick_bool(q.episode_limit != 0, [&](auto LIM) {
    int rc;
    if (W_ == 8)                                           // one variant: tier 3 throughout
      rc = bbx_pick_bool(tr, [&](auto TR) { return launch_lds<bbx_wide_kernel<8, TR(), false, LIM()>>(q.B, threads, wl, stream, q); });
    else if (!tr && one_per_cu)                            // lazy, or eager with or without accounting (lazy never counts)
      rc = bbx_pick<2, 4>(W_, [&](auto W) { return bbx_pick_bool(lazy, [&](auto LAZY) { return bbx_pick_bool(acct, [&](auto ACCT) {
        if constexpr (LAZY() && ACCT()) return (int)hipErrorInvalidValue;
        else return launch_lds<bbx_wide_kernel_1cu<W(), LAZY(), ACCT(), LIM()>>(q.B, threads, wl, stream, q);
      }); }); });
    else if (!tr && !lazy && !acct)
      rc = bbx_pick<2, 4>(W_, [&](auto W) { return launch_lds<bbx_wide_eager_kernel<W(), LIM()>>(q.B, threads, wl, stream, q); });
    else
      rc = bbx_pick<2, 4>(W_, [&](auto W) { return bbx_pick_bool(tr, [&](auto TR) { return bbx_pick_bool(lazy, [&](auto LAZY) {
        return launch_lds<bbx_wide_kernel<W(), TR(), LAZY(), LIM()>>(q.B, threads, wl, stream, q); }); }); });
    return rc;
    });
    return bbx_launched(rc);
}
#ifdef BBX_PROF_BUILD
extern "C" int bbx_wide_prof_read(unsigned long long* out, int reset) {   // diagnostic build only
  hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(bbx_wide_prof_acc), 32 * sizeof(unsigned long long));
  if (e == hipSuccess && reset) { unsigned long long z[32] = {0}; e = hipMemcpyToSymbol(HIP_SYMBOL(bbx_wide_prof_acc), z, sizeof z); }
  return (int)e;
}
#endif

// General class of the step kernel: term arena + scratch polynomials in HBM/L2, merge-path tiles through per-wave LDS
// (non-binomial random ideals, 8-variable fixed ideals, big batches of fixed ideals).  One wavefront per environment.
// Reference semantics: buchberger.cpp:18-99, 299-329, 354-408; polynomials.cpp:41-202.
#include "bbx_device.h"
#include "bbx_launch.h"

// ------------------------------------------------------------------ the step kernel
// LIM: the instantiation that knows the episode step limit, launched when one is set; without it the limit is the constant 0
template <int W, bool STAGED, bool TRACE, bool PROF = false, bool LIM = false>
__device__ __forceinline__ void step_body(const BbxParams& p, char* smem, unsigned long long* prof_out = nullptr) {
  const int lane = lane_id();
  unsigned long long ps[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // diagnostic build: cycles per phase
  unsigned long long pl = PROF ? __builtin_amdgcn_s_memtime() : 0;
#define GSTAMP(slot) do { if (PROF) { unsigned long long t_ = __builtin_amdgcn_s_memtime(); ps[slot] += t_ - pl; pl = t_; } } while (0)
  const int wave_in_block = uni((int)(threadIdx.x / WAVE));   // provably wave-uniform: record addresses live in SGPRs
  const int env = (int)(blockIdx.x * (blockDim.x / WAVE) + wave_in_block);
  if (env >= p.B) return;                       // whole wave exits together
  char* grec = p.recs + (size_t)env * p.L.rec_bytes;
  BbxHdr* ghdr = (BbxHdr*)grec;
  const BbxLayout& L = STAGED ? p.LL : p.L;      // the layout this kernel works in

  StepState s = hdr_load(ghdr);                 // the protocol around the algebra: bbx_device.h
  step_budget(s, p);
  if (p.pass == 1 && !bbx_pass_has_work(s.status, s.need_reset, s.budget, s.nP)) return;  // nothing left to do here

  // What the algebra's functions take by reference lives in locals of its own from here to the exit: a struct of which one
  // member's address goes into a call that is not inlined (32-byte monomials) would stay in memory as a whole.
  int nG = s.nG, nP = s.nP, arena_used = s.arena_used, status = s.status, q_head = s.q_head;
  uint32_t gen_state = s.gen_state;

  Env<W> ge = env_view<W>(grec, p.L);
  // In the staged instantiation the working view is ALWAYS the LDS copy (never a select between an LDS and
  // a global pointer), so that every access below compiles to ds_read/ds_write instead of flat_*.
  Env<W> e = STAGED ? env_view<W>(smem + (size_t)wave_in_block * L.rec_bytes, L) : ge;
  bool staged_in = false;
  if (STAGED) {
    if (status == BBX_ST_OK && !(!s.need_reset && nP == 0)) {   // (an idle environment is not staged: bbx_fast.h, idle0)
      if (nG > (int)L.maxG || nP > (int)L.maxP || arena_used > (int)L.arena) status = BBX_ST_SPILL;
      else {
        stage_copy<W>(e, ge, nG, nP, arena_used);
        staged_in = true;
        wave_sync();
      }
    }
  }
  const bool tracing = TRACE && p.trace != nullptr;   // hashing code exists only in the TRACE instantiations
  // per-wave LDS tile scratch of the merge-path merge (HBM-resident class only; the launcher provides it)
  char* mlds = (!STAGED && smem != nullptr) ? smem + (size_t)wave_in_block * merge_lds_bytes<W>() : nullptr;

  // scratch polynomials
  const int maxT = (int)L.maxT;
  Mono<W>* hm0 = e.hm;            uint16_t* hc0 = e.hc;
  Mono<W>* hm1 = e.hm + maxT;     uint16_t* hc1 = e.hc + maxT;
  Mono<W>* rm = e.hm + 2 * maxT;  uint16_t* rc = e.hc + 2 * maxT;
  Mono<W>* tm = e.hm + 3 * maxT;  uint16_t* tc = e.hc + 3 * maxT;   // 2*maxT staging

  for (;;) {
    if (status != BBX_ST_OK) break;
    s.rng_mark = s.std_rng;                       // the selection engine's state before the step in progress
    if (s.need_reset) {                           // also serves a reset left pending by the last step
      if (!wave_reset<W>(e, p, L, env, nG, nP, arena_used, q_head, &status, gen_state)) {
        // the reset restarts from the same queued ideal: in the LDS class a capacity miss is only a spill
        if (STAGED && (status == BBX_ST_G_FULL || status == BBX_ST_P_FULL || status == BBX_ST_ARENA_FULL)) {
          status = BBX_ST_SPILL; nG = 0; nP = 0; arena_used = 0;
        }
        break;
      }
      s.need_reset = 0; s.episode_steps = 0;
    }
    if (s.budget <= 0) break;
    if (nP == 0) break;                         // finished episode and no auto-reset: nothing to do
    // headroom for the worst case of this step, checked BEFORE anything is modified so that a miss leaves a
    // consistent state: one new basis element of <= maxT terms and at most |G| new pairs
    if (nG + 1 > (int)L.maxG || nP - 1 + nG > (int)L.maxP || arena_used + maxT > (int)L.arena) {
      status = STAGED ? BBX_ST_SPILL : (nG + 1 > (int)L.maxG ? BBX_ST_G_FULL : (nP - 1 + nG > (int)L.maxP ? BBX_ST_P_FULL : BBX_ST_ARENA_FULL));
      break;
    }

    // ---- choose the pair ------------------------------------------------------------------
    int action;
    if (!table_agent_action(p, env, s.agent_seed, s.t_agent, nP, s.std_rng, action))
      action = select_pair<W>(e, nP, p.agent, [&](int g) { return (int)e.psug[g]; });
    action = uni(action);
    if (action < 0 || action >= nP) { status = BBX_ST_BAD_ACTION; break; }
    const uint32_t pr = (uint32_t)uni((int)e.pairs[action]);
    const int gi = pr & 0xffffu, gj = pr >> 16;
    // (the pair leaves P — buchberger.cpp:319 — only once the reduction is through: S-polynomial and reduction work in
    // scratch, so a polynomial that outgrows max_poly_terms leaves the record exactly as the step found it and the step
    // is taken again after the host has enlarged the scratch: bbx_common.h, bbx_st_capacity)
    long long sb = 0;                            // algorithmic bytes of this step

    // ---- S-polynomial  buchberger.cpp:18-21 -----------------------------------------------------
    int hn, hoff = 0, hsug;
    Mono<W>* hm = hm0; uint16_t* hc = hc0;
    {
      const Mono<W> lmi = e.lm[gi], lmj = e.lm[gj];
      const Mono<W> gamma = m_lcm(lmi, lmj);
      const int offi = uni((int)e.poff[gi]), offj = uni((int)e.poff[gj]);
      PView<W> A, Bv;
      A.m = e.am + offi + 1; A.c = e.ac + offi + 1; A.n = uni((int)e.plen[gi]) - 1;
      A.shift = m_div(gamma, lmi); A.scale = (uint32_t)uni((int)e.pinv[gi]);
      Bv.m = e.am + offj + 1; Bv.c = e.ac + offj + 1; Bv.n = uni((int)e.plen[gj]) - 1;
      Bv.shift = m_div(gamma, lmj); Bv.scale = negmod((uint32_t)uni((int)e.pinv[gj]));
      int si = uni((int)e.psug[gi]) + (int)m_deg(A.shift), sj = uni((int)e.psug[gj]) + (int)m_deg(Bv.shift);
      hsug = uni(si > sj ? si : sj);
      if (hsug > 65535) { status = BBX_ST_DEG_OVERFLOW; break; }
      if (!STAGED && p.spill_terms && A.n + Bv.n > p.spill_terms) { status = BBX_ST_SPILL; break; }   // long polynomials: a workgroup's job
      if (A.n + Bv.n > 2 * maxT) { status = BBX_ST_POLY_TOO_LONG; break; }
      GSTAMP(0);                                   // 0: loop top, agent, pair removal
      const bool big = mlds && A.n > 0 && Bv.n > 0 && A.n + Bv.n > 64;
      hn = big ? wave_merge_tiled<W>(A, Bv, mlds, hm, hc, maxT) : wave_merge<W>(A, Bv, tm, tc, hm, hc, maxT);
      if (hn < 0) { status = BBX_ST_POLY_TOO_LONG; break; }
      GSTAMP(1);                                   // 1: S-polynomial merge
      sb += 12LL * (A.n + Bv.n + 2 + hn);          // both inputs read, S-polynomial written
    }

    // ---- reduce  buchberger.cpp:24-49 -----------------------------------------------------------
    int nsteps_red = 0, rn = 0, rsug = 0;
    bool overflow = false;
    while (hn - hoff > 0) {
      const Mono<W> lmh = hm[hoff];
      int found = -1;
      for (int base = 0; base < nG; base += WAVE) {   // first reducer (in G_ order) whose LM divides LM(h)
        int k = base + lane;
        bool d = k < nG && m_divides(e.slm[k], lmh);
        uint64_t mask = ballot64(d);
        if (mask) { found = base + __builtin_ctzll(mask); break; }
      }
      GSTAMP(2);                                  // 2: divisor scans
      if (found >= 0) {                         // h <- h - (LT h / LT f) f     (34-36)
        const int g = uni((int)e.sidx[found]);
        const uint32_t c = mulmod((uint32_t)uni((int)hc[hoff]), (uint32_t)uni((int)e.pinv[g]));
        const int offg = uni((int)e.poff[g]);
        PView<W> A, Bv;
        A.m = hm + hoff + 1; A.c = hc + hoff + 1; A.n = hn - hoff - 1; A.shift = m_zero<W>(); A.scale = 1;
        Bv.m = e.am + offg + 1; Bv.c = e.ac + offg + 1; Bv.n = uni((int)e.plen[g]) - 1;
        Bv.shift = m_div(lmh, e.lm[g]); Bv.scale = negmod(c);
        int fs = uni((int)e.psug[g]) + (int)m_deg(Bv.shift);
        hsug = uni(fs > hsug ? fs : hsug);
        if (hsug > 65535) { status = BBX_ST_DEG_OVERFLOW; overflow = true; break; }
        if (!STAGED && p.spill_terms && A.n + Bv.n > p.spill_terms) { status = BBX_ST_SPILL; overflow = true; break; }
        if (A.n + Bv.n > 2 * maxT) { status = BBX_ST_POLY_TOO_LONG; overflow = true; break; }
        Mono<W>* nm = (hm == hm0) ? hm1 : hm0; uint16_t* nc = (hc == hc0) ? hc1 : hc0;
        GSTAMP(3);                                // 3: reducer fetch / setup
        const bool big = mlds && A.n > 0 && Bv.n > 0 && A.n + Bv.n > 64;
        const int nn = big ? wave_merge_tiled<W>(A, Bv, mlds, nm, nc, maxT) : wave_merge<W>(A, Bv, tm, tc, nm, nc, maxT, PROF ? &ps[6] : nullptr);
        if (nn < 0) { status = BBX_ST_POLY_TOO_LONG; overflow = true; break; }
        GSTAMP(4);                                // 4: reduction merges (6/7: their pass 1 / pass 2)
        sb += 8LL * (found + 1) + 12LL * (Bv.n + 1) + 12LL * (A.n + 1 + nn);
        hm = nm; hc = nc; hn = nn; hoff = 0;
        nsteps_red++;
        if (nsteps_red > (1 << 24)) { status = BBX_ST_RUNAWAY; overflow = true; break; }
      } else {                                  // r <- r + LT h ; h <- h - LT h   (41-44)
        if (rn >= maxT) { status = BBX_ST_POLY_TOO_LONG; overflow = true; break; }
        sb += 8LL * nG + 12LL * (2 * (hn - hoff) - 1);
        if (lane == 0) { rm[rn] = lmh; rc[rn] = hc[hoff]; }
        int d = uni((int)m_deg(lmh));
        rsug = d > rsug ? d : rsug;
        rn++; hoff++;
        GSTAMP(5);                                // 5: tail moves
      }
    }
    if (overflow) break;
    wave_sync();
    rsug = rsug > hsug ? rsug : hsug;            // sugar of r + h (48), h's sugar survives its terms
    if (rn > 65535) { status = BBX_ST_POLY_LIMIT; break; }   // plen[] is 16 bits

    // ---- P.erase(remove(action))  buchberger.cpp:319 — stable; from here on the step cannot fail for capacity -------
    for (int base = action; base < nP - 1; base += WAVE) {
      int k = base + lane;
      uint32_t v = 0;
      if (k < nP - 1) v = e.pairs[k + 1];
      wave_sync();
      if (k < nP - 1) e.pairs[k] = v;
      wave_sync();
    }
    nP -= 1;

    // ---- basis / pair-set update  buchberger.cpp:321-327 ---------------------------------------
    const int nG_before = nG, nP_before = nP;
    if (rn != 0) {
      if (!wave_add_poly<W>(e, L, nG, nP, arena_used, rm, rc, rn, rsug, p.elim, p.sort_reducers, &status)) break;
      sb += 12LL * rn + 8LL * nG_before + 8LL * (nP_before + nP);
    } else s.zero_red++;
    sb += 4LL * nP * 2 * p.nvars * p.k;             // the observation matrix of the new state
    s.alg_bytes += sb;
    const double reward = step_reward(p.rewards_mode, nsteps_red);
    const int limit = LIM ? p.episode_limit : 0;
    const int end = step_end(s, limit, nP);
    const bool done = end != 0;                   // (the pair set is empty, or the episode step limit cuts it)

    // ---- the observation a policy would consume after this step ---------------------------------
    if (p.obs_every_step && p.obs) { wave_obs<W>(e, p, env, nP, true, false); s.obs_trunc |= nP > p.obs_rows ? 1 : 0; }
    // ---- parity trace (tests): hashes of the post-step observation / pair set / new element ---
    if (TRACE && tracing) {
      uint64_t oh = wave_obs<W, true>(e, p, env, nP, false, true);
      uint64_t ph = wave_pairs_hash<W, Env<W>>(e, nP);
      uint64_t nh = nG > nG_before ? wave_poly_hash<W>(e, nG - 1) : 0;
      if (lane == 0) trace_put(p, env, s.rollout_pos, action, nP, nG, done, reward, oh, ph, nh);
    }
    step_account(s, p, ghdr, reward, nsteps_red, end, limit);
  }

  if (PROF && prof_out && lane == 0) for (int i = 0; i < 10; i++) prof_out[(size_t)env * 10 + i] = ps[i];
  // ---- observation of the state the caller sees next ------------------------------------------
  if (p.obs && status == BBX_ST_OK) { wave_obs<W>(e, p, env, nP, true, false); s.obs_trunc |= nP > p.obs_rows ? 1 : 0; }

  if (STAGED && staged_in) {
    wave_sync();
    stage_copy<W>(ge, e, nG, nP, arena_used);
  }
  s.nG = nG; s.nP = nP; s.arena_used = arena_used; s.status = status; s.q_head = q_head; s.gen_state = gen_state;
  // the engine rewinds when the step did not happen (the draw comes before the merges that can miss max_poly_terms or hand the
  // step to the wide class); an environment that must continue in the follow-up pass reports nothing yet
  if (lane == 0) hdr_store(ghdr, p, env, s, bbx_st_capacity(s.status) || s.status == BBX_ST_SPILL, s.status == BBX_ST_SPILL);
}

template <int W, bool STAGED, bool TRACE, bool LIM = false>
__global__ __launch_bounds__(256) void bbx_step_kernel(BbxParams p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  step_body<W, STAGED, TRACE, false, LIM>(p, smem);
}
// the same body under its own name for launches that only reset / refresh observations (nsteps == 0), so that
// profiles of bbx_step_kernel contain step launches only
template <int W>
__global__ __launch_bounds__(256) void bbx_aux_kernel(BbxParams p) {
  step_body<W, false, false>(p, nullptr);
}
#ifdef BBX_PROF_BUILD
// diagnostic build with s_memtime stamps (BBX_PROF=1), never used for reported numbers
template <int W>
__global__ __launch_bounds__(256) void bbx_step_prof_kernel(BbxParams p, unsigned long long* prof) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  step_body<W, false, false, true>(p, smem, prof);
}

#endif

template <int W>
static int launch_general_w(const BbxParams* p, BbxKernel kind, int blocks, int threads, size_t lds, hipStream_t stream) {
  const bool trace = p->trace != nullptr, lim = p->episode_limit != 0;   // (lim: the LIM instantiations)
  if (kind == BBX_K_AUX) return bbx_launch<bbx_aux_kernel<W>>(dim3(blocks), threads, lds, stream, *p);
  if (kind == BBX_K_STAGED)
    return bbx_pick_bool(trace, [&](auto TRACE) { return bbx_pick_bool(lim, [&](auto LIM) { return launch_lds<bbx_step_kernel<W, true, TRACE(), LIM()>>(blocks, threads, lds, stream, *p); }); });
#ifdef BBX_PROF_BUILD   // diagnostic build only (-DBBX_PROF_BUILD): per-phase s_memtime sums, never in the product library
  if (!trace && getenv("BBX_PROF")) {
    static unsigned long long* d_prof = nullptr;
    if (!d_prof) (void)hipMalloc((void**)&d_prof, (size_t)p->B * 10 * sizeof(unsigned long long));
    lds = (size_t)(threads / WAVE) * merge_lds_bytes<W>();
    (void)launch_lds<bbx_step_prof_kernel<W>>(blocks, threads, lds, stream, *p, d_prof);
    (void)hipStreamSynchronize(stream);
    std::vector<unsigned long long> h((size_t)p->B * 10);
    (void)hipMemcpy(h.data(), d_prof, h.size() * 8, hipMemcpyDeviceToHost);
    double s[10] = {0}, tot = 0;
    for (int e = 0; e < p->B; e++) for (int i = 0; i < 10; i++) s[i] += (double)h[(size_t)e * 10 + i];
    for (int i = 0; i < 6; i++) tot += s[i];
    fprintf(stderr, "[bbx prof general] nsteps=%d kcycles/env:", p->nsteps);
    for (int i = 0; i < 10; i++) fprintf(stderr, " p%d=%.0f(%.0f%%)", i, s[i] / p->B / 1e3, 100.0 * s[i] / tot);
    fprintf(stderr, "\n");
    return 0;
  }
#endif
  lds = (size_t)(threads / WAVE) * merge_lds_bytes<W>();          // merge-path tile scratch, one per wave
  return bbx_pick_bool(trace, [&](auto TRACE) { return bbx_pick_bool(lim, [&](auto LIM) { return launch_lds<bbx_step_kernel<W, false, TRACE(), LIM()>>(blocks, threads, lds, stream, *p); }); });
}
extern "C" int bbx_launch_general(const BbxParams* p, BbxKernel kind, int blocks, int threads, size_t lds, hipStream_t stream) {
  return bbx_pick<2, 4, 8>((int)p->L.W, [&](auto W) { return launch_general_w<W()>(p, kind, blocks, threads, lds, stream); });
}

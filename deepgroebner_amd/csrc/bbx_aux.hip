// Housekeeping kernels of libbbx (initialisation, queue refill, ragged observations, clones, value() and action-value
// bookkeeping, record growth, header gathers), the stand-alone PMLP policy launchers and the launcher that picks a kernel class
// (bbx_launch_step).  Every launcher here and the four class launchers it calls are declared in bbx_launch.h.
#include "bbx_device.h"
#include "bbx_launch.h"
#include "bbx_pmlp.h"
#include "bbx_pmlp_grad.h"
#include "bbx_pmlp_value.h"
#include "bbx_binom.h"

// ------------------------------------------------------------------ housekeeping kernels
// zero the headers and set the per-environment agent seeds
__global__ void bbx_init_kernel(char* recs, uint32_t rec_bytes, int B, const uint32_t* agent_seeds) {
  int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= B) return;
  BbxHdr* h = (BbxHdr*)(recs + (size_t)env * rec_bytes);
  BbxHdr z = {};
  z.agent_seed = agent_seeds ? agent_seeds[env] : (uint32_t)env;
  z.std_rng = 1u;                               // std::default_random_engine's default seed
  *h = z;
}
// request a reset (mask == null: every environment); clears a sticky error so the slot can be reused
__global__ void bbx_mark_reset_kernel(char* recs, uint32_t rec_bytes, int B, const uint8_t* mask) {
  int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= B) return;
  if (mask && !mask[env]) return;
  BbxHdr* h = (BbxHdr*)(recs + (size_t)env * rec_bytes);
  h->need_reset = 1; h->status = BBX_ST_OK; h->nP = 0; h->nG = 0; h->arena_used = 0; h->done_last = 0;
}
// refill of the ideal queue: the host stages the rings of the environments it topped up ([n ids][n tails][n rings]) and
// uploads them with one copy; this kernel moves every ring to its place (one workgroup per ring)
__global__ void bbx_scatter_queue_kernel(const uint32_t* stage, int n, uint32_t ring_words, uint32_t* q, int32_t* tail) {
  const int i = blockIdx.x;
  if (i >= n) return;
  const int env = (int)stage[i];
  const uint32_t* src = stage + 2 * (size_t)n + (size_t)i * ring_words;
  uint32_t* dst = q + (size_t)env * ring_words;
  for (uint32_t w = threadIdx.x; w < ring_words; w += blockDim.x) dst[w] = src[w];
  if (threadIdx.x == 0) tail[env] = (int32_t)stage[n + i];
}
extern "C" int bbx_launch_scatter_queue(const uint32_t* stage, int n, uint32_t ring_words, uint32_t* q, int32_t* tail, hipStream_t stream) {
  return bbx_launched(bbx_launch<bbx_scatter_queue_kernel>(dim3(n), 256, 0, stream, stage, n, ring_words, q, tail));
}
// ragged observation: the rows of every environment back to back (what a list of per-environment matrices needs),
// packed on the device from the padded block a step launch leaves behind.  Kernel 1: off[e] = sum of min(rows, cap)
// over the environments before e (one workgroup); kernel 2: one workgroup per environment copies its rows.
__global__ __launch_bounds__(1024) void bbx_obs_offsets_kernel(const int32_t* rows, int B, int cap, int32_t* off) {
  __shared__ int part[1024];
  const int t = threadIdx.x, per = (B + 1023) / 1024;
  int s = 0;
  for (int i = 0; i < per; i++) { const int e = t * per + i; if (e < B) { const int r = rows[e]; s += r < cap ? r : cap; } }
  part[t] = s;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {                     // inclusive scan (Hillis-Steele)
    const int v = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int base = t ? part[t - 1] : 0;
  for (int i = 0; i < per; i++) {
    const int e = t * per + i;
    if (e < B) { off[e] = base; const int r = rows[e]; base += r < cap ? r : cap; }
  }
  if (t == 1023) off[B] = part[1023];
}
__global__ void bbx_obs_pack_kernel(const int32_t* padded, int cap, int cols, const int32_t* off, int B, int32_t* packed) {
  const int e = blockIdx.x;
  if (e >= B) return;
  const int n = (off[e + 1] - off[e]) * cols;
  const int32_t* src = padded + (size_t)e * cap * cols;
  int32_t* dst = packed + (size_t)off[e] * cols;
  for (int i = threadIdx.x; i < n; i += blockDim.x) dst[i] = src[i];
}
extern "C" int bbx_launch_obs_pack(const int32_t* padded, int cap, int cols, const int32_t* rows, int B, int32_t* off, int32_t* packed, hipStream_t stream) {
  bbx_launch<bbx_obs_offsets_kernel>(dim3(1), 1024, 0, stream, rows, B, cap, off);
  return bbx_launched(bbx_launch<bbx_obs_pack_kernel>(dim3(B), 64, 0, stream, padded, cap, cols, (const int32_t*)off, B, packed));
}
extern "C" int bbx_launch_init(char* recs, uint32_t rec_bytes, int B, const uint32_t* agent_seeds, hipStream_t stream) {
  return bbx_launched(bbx_launch<bbx_init_kernel>(dim3((B + 255) / 256), 256, 0, stream, recs, rec_bytes, B, agent_seeds));
}
extern "C" int bbx_launch_mark_reset(char* recs, uint32_t rec_bytes, int B, const uint8_t* mask, hipStream_t stream) {
  return bbx_launched(bbx_launch<bbx_mark_reset_kernel>(dim3((B + 255) / 256), 256, 0, stream, recs, rec_bytes, B, mask));
}

// value(): clone environment src[k] of one record array into slot k of another (live prefixes only), optionally
// re-seeding the built-in random agent of the clone
// seed_std != 0: the seeds are states of the std::default_random_engine behind the seeded Random selection (BbxHdr.std_rng)
// instead of seeds of the counter-hash agent.  flags (or null): per clone, bit 0 = the source is in an error state, bit 1 =
// two of its first ngen basis elements (the ideal's generators) have the same lead monomial (value(): buchberger() sorts
// its reducers with std::sort, whose order of equal elements the host reproduces — bbx_api.cpp).
template <int W>
__global__ void bbx_clone_kernel(const char* src_recs, char* dst_recs, BbxLayout L, const int32_t* src, const int32_t* dst, int n,
                                 const uint32_t* seeds, int keep_counters, int seed_std, int ngen, uint8_t* flags) {
  const int k = blockIdx.x * (blockDim.x / WAVE) + (int)(threadIdx.x / WAVE);
  if (k >= n) return;
  char* s = const_cast<char*>(src_recs) + (size_t)src[k] * L.rec_bytes;
  char* d = dst_recs + (size_t)(dst ? dst[k] : k) * L.rec_bytes;
  BbxHdr h = *(const BbxHdr*)s;
  if (L.kind == 1) bstage_copy<W>(benv_view<W>(d, L), benv_view<W>(s, L), h.nG, h.nP);
  else stage_copy<W>(env_view<W>(d, L), env_view<W>(s, L), h.nG, h.nP, h.arena_used);
  if (flags) {
    const Mono<W>* lm = (const Mono<W>*)(s + L.off_lm);
    const int ng = h.nG < ngen ? h.nG : ngen;
    bool tie = false;
    for (int i = lane_id(); i < ng; i += WAVE) {
      const Mono<W> mi = lm[i];
      for (int j = i + 1; j < ng; j++) tie = tie || m_eq(mi, lm[j]);
    }
    const bool any = ballot64(tie) != 0;
    if (lane_id() == 0) flags[k] = (uint8_t)((h.status != BBX_ST_OK ? 1 : 0) | (any ? 2 : 0));
  }
  if (lane_id() == 0) {
    if (!keep_counters) { h.need_reset = 0; h.budget = 0; h.rollout_pos = 0; h.t = 0; }
    if (seeds) { if (seed_std) h.std_rng = seeds[k]; else h.agent_seed = seeds[k]; }
    *(BbxHdr*)d = h;
  }
}
extern "C" int bbx_launch_clone(const char* src_recs, char* dst_recs, const BbxLayout* L, const int32_t* src, const int32_t* dst, int n,
                                const uint32_t* seeds, int keep_counters, int seed_std, int ngen, uint8_t* flags, hipStream_t stream) {
  return bbx_launched(bbx_pick<2, 4, 8>((int)L->W, [&](auto W) {
    return bbx_launch<bbx_clone_kernel<W()>>(dim3((n + 3) / 4), 256, 0, stream, src_recs, dst_recs, *L, src, dst, n, seeds, keep_counters, seed_std, ngen, flags);
  }));
}
// ---- value(): the reducer order buchberger() starts from ---------------------------------------------------------------
// buchberger() re-sorts its reducers with std::sort (buchberger.cpp:157-158: G_ = F in basis order, sorted by lead
// monomial).  The environment keeps its own reducer order by upper_bound insertion, which is the STABLE order; the two
// differ only when lead monomials tie — possible among the ideal's generators only — AND the basis has more than 16
// elements, where libstdc++'s std::sort stops being an insertion sort: introsort (median-of-three quicksort with a depth
// limit of 2 log2 n and a heapsort fallback, segments of <= 16 left to a final insertion sort; bits/stl_algo.h
// __introsort_loop / __final_insertion_sort, GCC 11: ss_std_sort in bbx_device.h).  For the clones that need it one lane
// reproduces that sort on an index array, the wave then rebuilds the reducer-order arrays.
template <int W>
__global__ void bbx_value_resort_kernel(char* recs, BbxLayout L, int n, const uint8_t* flags) {
  const int k = blockIdx.x * (blockDim.x / WAVE) + (int)(threadIdx.x / WAVE);
  if (k >= n || !(flags[k] & 2)) return;
  char* rec = recs + (size_t)k * L.rec_bytes;
  const BbxHdr* h = (const BbxHdr*)rec;
  const int nG = h->nG, lane = lane_id();
  if (nG <= 16) return;                                    // std::sort is its (stable) insertion sort there: the environment's order
  const Mono<W>* lm = (const Mono<W>*)(rec + L.off_lm);
  uint16_t* ord = (uint16_t*)(rec + L.off_lcm);            // (the update's scratch: idle between steps)
  if (lane == 0) {
    for (int i = 0; i < nG; i++) ord[i] = (uint16_t)i;
    SortCtx<W> c{lm, ord};
    ss_std_sort<W>(c, nG);
  }
  wave_sync();
  Mono<W>* slm = (Mono<W>*)(rec + L.off_slm);
  if (L.kind == 1) {
    const Mono<W>* tm = (const Mono<W>*)(rec + L.off_tm);
    Mono<W>* stm = (Mono<W>*)(rec + L.off_stm);
    const uint2* gi = (const uint2*)(rec + L.off_ginfo);
    uint2* si = (uint2*)(rec + L.off_sinfo);
    for (int r = lane; r < nG; r += WAVE) {
      const int g = ord[r];
      const uint2 gg = gi[g];
      const uint32_t tc = gg.x >> 16, inv = gg.y & 0xffffu, sug = gg.y >> 16;
      slm[r] = lm[g]; stm[r] = tm[g];
      si[r] = make_uint2(tc | (negmod(mulmod(tc, inv)) << 16), sug | ((uint32_t)g << 16));   // .x = tc | (-tc / lc) << 16 (bin_add_poly)
    }
  } else {
    uint16_t* sidx = (uint16_t*)(rec + L.off_sidx);
    for (int r = lane; r < nG; r += WAVE) { const int g = ord[r]; slm[r] = lm[g]; sidx[r] = (uint16_t)g; }
  }
}
extern "C" int bbx_launch_value_resort(char* recs, const BbxLayout* L, int n, const uint8_t* flags, hipStream_t stream) {
  return bbx_launched(bbx_pick<2, 4, 8>((int)L->W, [&](auto W) {
    return bbx_launch<bbx_value_resort_kernel<W()>>(dim3((n + 3) / 4), 256, 0, stream, recs, *L, n, flags);
  }));
}

// A clone that did not run to the end (pairs left, or a status other than OK), folded into the word pair the host reads at its next wait:
// word[0] |= 1 << status if it waits for room (bbx_st_capacity), bit 31 otherwise; word[1] = 1 + the largest `index` so reported
__device__ inline void bbx_unfinished_fold(uint32_t* word, int st, uint32_t index) {
  atomicOr(&word[0], bbx_st_capacity(st) ? 1u << st : 1u << 31);
  atomicMax(&word[1], index + 1u);
}

// ---- bbx_values_device: the asynchronous form (bbx_api_value.cpp) -------------------------------------------------------
// slot k of a clone array <- environment k (the identity source indices of the clone kernel)
__global__ void bbx_value_iota_kernel(int32_t* idx, int n) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) idx[k] = k;
}
extern "C" int bbx_launch_value_iota(int32_t* idx, int n, hipStream_t stream) {
  return bbx_launched(bbx_launch<bbx_value_iota_kernel>(dim3((n + 255) / 256), 256, 0, stream, idx, n));
}
// "random": seed -> engine state of std::default_random_engine::seed(s), minstd_state_of_seed of bbx_api_value.cpp on the
// device (the int seed converts to the unsigned result type first; x = s mod 2^31 - 1, and 0 becomes 1)
__global__ void bbx_value_seeds_kernel(const int64_t* seeds, uint32_t* states, int n) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const uint32_t x = (uint32_t)((uint64_t)seeds[k] % 2147483647ull);
  states[k] = x ? x : 1u;
}
extern "C" int bbx_launch_value_seeds(const int64_t* seeds, uint32_t* states, int n, hipStream_t stream) {
  return bbx_launched(bbx_launch<bbx_value_seeds_kernel>(dim3((n + 255) / 256), 256, 0, stream, seeds, states, n));
}
// per clone (the synchronous calls use it too): its discounted return into values[k], NaN where the rollout did not run to the
// end and the clone's index folded into the call's word pair.
// only_nan != 0 (the carry-over of waiting clones after the records were enlarged): entries that already hold a value stay.
__global__ void bbx_value_collect_device_kernel(const char* recs, uint32_t rec_bytes, int n, double* values, uint32_t* word, int only_nan) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  if (only_nan && values[k] == values[k]) return;
  const BbxHdr* h = (const BbxHdr*)(recs + (size_t)k * rec_bytes);
  const int st = h->status;
  const bool finished = st == BBX_ST_OK && h->nP == 0;
  values[k] = finished ? h->vret : __builtin_nan("");
  if (!finished) bbx_unfinished_fold(word, st, (uint32_t)k);
}
extern "C" int bbx_launch_value_collect_device(const char* recs, uint32_t rec_bytes, int n, double* values, uint32_t* word, int only_nan, hipStream_t stream) {
  return bbx_launched(bbx_launch<bbx_value_collect_device_kernel>(dim3((n + 255) / 256), 256, 0, stream, recs, rec_bytes, n, values, word, only_nan));
}

// ---- bbx_action_values: one clone per (environment, pair), a forced first step, then value() (bbx_api_value.cpp) ----------
// The flat list of clones: environment e contributes its actions 0 .. count[e] - 1, count[e] = min(nP, max_rows) — 0 for an
// environment without pairs or one that awaits its reset.  Kernel 1 (one workgroup, the scan of bbx_obs_offsets_kernel, from
// the record headers): out[0 .. B] = the exclusive scan of the counts; out[B + 1], out[B + 2] = 1 + the first environment in
// an error state and its status (0: none); out[B + 3 + e] = the FULL pair count of environment e.  All the host reads of the states.
__global__ __launch_bounds__(1024) void bbx_av_offsets_kernel(const char* recs, uint32_t rec_bytes, int B, int max_rows, int32_t* out) {
  __shared__ int part[1024];
  __shared__ int bad;
  const int t = threadIdx.x, per = (B + 1023) / 1024;
  if (t == 0) bad = B;
  __syncthreads();
  int s = 0;
  for (int i = 0; i < per; i++) {
    const int e = t * per + i;
    if (e >= B) break;
    const BbxHdr* h = (const BbxHdr*)(recs + (size_t)e * rec_bytes);
    const int full = h->need_reset ? 0 : h->nP;
    out[B + 3 + e] = full;
    s += full < max_rows ? full : max_rows;
    if (h->status != BBX_ST_OK) atomicMin(&bad, e);
  }
  part[t] = s;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {                     // inclusive scan (Hillis-Steele)
    const int v = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int base = t ? part[t - 1] : 0;
  for (int i = 0; i < per; i++) {
    const int e = t * per + i;
    if (e < B) { out[e] = base; const int full = out[B + 3 + e]; base += full < max_rows ? full : max_rows; }   // (this thread's own store)
  }
  if (t == 1023) out[B] = part[1023];
  if (t == 0) {
    out[B + 1] = bad < B ? bad + 1 : 0;
    out[B + 2] = bad < B ? ((const BbxHdr*)(recs + (size_t)bad * rec_bytes))->status : 0;
  }
}
// Kernel 2: positions [first, first + n) of the flat list -> src[k] = the environment, act[k] = its action.  The environment
// is the last one whose offset is <= the position (empty environments share their successor's offset and are passed over);
// the caller keeps first + n <= off[B].
__global__ void bbx_av_expand_kernel(const int32_t* off, int B, int first, int n, int32_t* src, int32_t* act) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const int flat = first + k;
  int lo = 0, hi = B;                                       // off[lo] <= flat < off[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= flat) lo = mid; else hi = mid;
  }
  src[k] = lo; act[k] = flat - off[lo];
}
// the [B][max_rows] staging blocks before the passes: NaN / NaN / 0 padding, the status word pair cleared
__global__ void bbx_av_fill_kernel(double* q, double* rewards, uint8_t* dones, size_t cells, uint32_t* word) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 2) word[i] = 0u;
  if (i >= cells) return;
  q[i] = __builtin_nan(""); rewards[i] = __builtin_nan(""); dones[i] = 0;
}
// Kernel 3, after the forced step and the rollouts of a pass: clone k writes Q = r + gamma * value at [src[k]][act[k]] — in
// double, one rounded product and one rounded sum (contraction off, as in bbx_gae_kernel: what the host forms from
// bbx_step's reward and bbx_values' value) —, the step's reward and done flag beside it.  A clone that did not run to the end
// leaves its cells as they are and is folded into the call's word pair under its environment's index.
__global__ void bbx_av_collect_kernel(const char* recs, uint32_t rec_bytes, int n, const int32_t* src, const int32_t* act, const double* rew,
                                      const uint8_t* done, double gamma, int max_rows, double* q, double* rewards, uint8_t* dones, uint32_t* word) {
#pragma clang fp contract(off)
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const BbxHdr* h = (const BbxHdr*)(recs + (size_t)k * rec_bytes);
  const int st = h->status;
  if (!(st == BBX_ST_OK && h->nP == 0)) { bbx_unfinished_fold(word, st, (uint32_t)src[k]); return; }
  const size_t at = (size_t)src[k] * max_rows + act[k];
  const double r = rew[k];
  const double tail = gamma * h->vret;
  q[at] = r + tail; rewards[at] = r; dones[at] = done[k];
}
extern "C" int bbx_launch_av_offsets(const char* recs, uint32_t rec_bytes, int B, int max_rows, int32_t* out, hipStream_t stream) {
  return bbx_launched(bbx_launch<bbx_av_offsets_kernel>(dim3(1), 1024, 0, stream, recs, rec_bytes, B, max_rows, out));
}
extern "C" int bbx_launch_av_expand(const int32_t* off, int B, int first, int n, int32_t* src, int32_t* act, hipStream_t stream) {
  return bbx_launched(bbx_launch<bbx_av_expand_kernel>(dim3((n + 255) / 256), 256, 0, stream, off, B, first, n, src, act));
}
extern "C" int bbx_launch_av_fill(double* q, double* rewards, uint8_t* dones, size_t cells, uint32_t* word, hipStream_t stream) {
  const size_t m = cells > 2 ? cells : 2;
  return bbx_launched(bbx_launch<bbx_av_fill_kernel>(dim3((unsigned)((m + 255) / 256)), 256, 0, stream, q, rewards, dones, cells, word));
}
extern "C" int bbx_launch_av_collect(const char* recs, uint32_t rec_bytes, int n, const int32_t* src, const int32_t* act, const double* rew,
                                     const uint8_t* done, double gamma, int max_rows, double* q, double* rewards, uint8_t* dones, uint32_t* word,
                                     hipStream_t stream) {
  return bbx_launched(bbx_launch<bbx_av_collect_kernel>(dim3((n + 255) / 256), 256, 0, stream, recs, rec_bytes, n, src, act, rew, done, gamma, max_rows, q, rewards,
                                                        dones, word));
}

// ---- GAE over a [T][B] trajectory block (DeviceTrajectoryBuffer.finish(), pg.py:20-76 per trajectory) -------------------
// One thread per environment, reverse scan over t; consecutive threads read consecutive elements of every row.  The
// arithmetic is the torch loop's, operation for operation: every product is rounded before it is added (no fused
// multiply-add: contraction is off in the kernel body), gl = gam * lam was formed once in double by the caller.
// last_values (or NULL): the value of the state behind step T - 1 of every environment, where the scan starts instead of at
// zero (truncated-horizon GAE: an episode cut by the end of the block is bootstrapped, and every step counts as complete); a
// done flag clears the carries before anything reads them, so the entry of an environment whose last step ended its episode
// is never used.  LAM: lambda_returns[i] = adv + v, the TD(lambda) value target, one rounded sum.
template <bool LAM>
__global__ void bbx_gae_kernel(const double* __restrict__ rewards, const double* __restrict__ values, const uint8_t* __restrict__ dones,
                               int T, int B, double gam, double gl, const double* __restrict__ last_values, double* __restrict__ returns,
                               double* __restrict__ advantages, uint8_t* __restrict__ complete, double* __restrict__ lambda_returns) {
#pragma clang fp contract(off)                              // (the default contracts a * b + c into one rounding; __dmul_rn / __dadd_rn are
                                                            // inline * and + that carry the default with them, so plain operators under this)
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= B) return;
  double nret = 0.0, nadv = 0.0, nval = 0.0;
  uint8_t comp = 0;
  if (last_values) { nret = nval = last_values[e]; comp = 1; }
#pragma unroll 8                                            // (the loads of a row do not depend on the row above: issued ahead of the chain)
  for (int t = T - 1; t >= 0; t--) {
    const size_t i = (size_t)t * B + e;
    if (dones[i]) { nret = 0.0; nadv = 0.0; nval = 0.0; comp = 1; }   // step t ends its episode: nothing follows it
    const double r = rewards[i], v = values[i];
    const double ret = r + gam * nret;
    const double adv = ((r - v) + gam * nval) + gl * nadv;
    returns[i] = ret; advantages[i] = adv; complete[i] = comp;
    if (LAM) lambda_returns[i] = adv + v;
    nret = ret; nadv = adv; nval = v;
  }
}
extern "C" int bbx_launch_gae(const double* rewards, const double* values, const uint8_t* dones, int T, int B, double gam, double gl,
                              const double* last_values, double* returns, double* advantages, uint8_t* complete, double* lambda_returns,
                              hipStream_t stream) {
  return bbx_launched(bbx_pick_bool(lambda_returns != nullptr, [&](auto LAM) {
    return bbx_launch<bbx_gae_kernel<LAM()>>(dim3((B + 63) / 64), 64, 0, stream, rewards, values, dones, T, B, gam, gl, last_values, returns, advantages, complete,
                                             lambda_returns);
  }));
}

// ---- per-episode returns and lengths from the [T][B] rewards and dones of a rollout (run_episodes, pg.py: one return and one
// length per episode) -----------------------------------------------------------------------------------------------------
// One thread per environment, forward scan over t: a plain double add per step, in step order (what the CPU loop of
// rollout.episode_returns does).  The step that ends an episode carries its return and its length, every other step zeros;
// what an unfinished episode has gathered goes back to the carries, so that a long evaluation is a chain of chunks.
__global__ void bbx_episodes_kernel(const double* __restrict__ rewards, const uint8_t* __restrict__ dones, int T, int B,
                                    double* __restrict__ carry_return, int32_t* __restrict__ carry_len, int32_t* __restrict__ ep_count,
                                    double* __restrict__ ep_return, int32_t* __restrict__ ep_len) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= B) return;
  double acc = carry_return ? carry_return[e] : 0.0;
  int len = carry_len ? carry_len[e] : 0;
  int count = 0;
#pragma unroll 8                                            // (the loads of a row do not depend on the row above: issued ahead of the chain)
  for (int t = 0; t < T; t++) {
    const size_t i = (size_t)t * B + e;
    acc += rewards[i]; len += 1;
    const bool d = dones[i] != 0;
    ep_return[i] = d ? acc : 0.0; ep_len[i] = d ? len : 0;
    if (d) { count++; acc = 0.0; len = 0; }
  }
  if (carry_return) carry_return[e] = acc;
  if (carry_len) carry_len[e] = len;
  if (ep_count) ep_count[e] += count;
}
extern "C" int bbx_launch_episodes(const double* rewards, const uint8_t* dones, int T, int B, double* carry_return, int32_t* carry_len, int32_t* ep_count,
                                   double* ep_return, int32_t* ep_len, hipStream_t stream) {
  return bbx_launched(bbx_launch<bbx_episodes_kernel>(dim3((B + 63) / 64), 64, 0, stream, rewards, dones, T, B, carry_return, carry_len, ep_count, ep_return, ep_len));
}

// enlarged records (bbx_api.cpp grow_records): every environment's live state moves from its record in the old layout to
// its record in the new one; an environment that was waiting for room (bbx_st_capacity) is released
template <int W>
__global__ void bbx_relayout_kernel(const char* src_recs, char* dst_recs, BbxLayout Ls, BbxLayout Ld, int B) {
  const int k = blockIdx.x * (blockDim.x / WAVE) + (int)(threadIdx.x / WAVE);
  if (k >= B) return;
  char* s = const_cast<char*>(src_recs) + (size_t)k * Ls.rec_bytes;
  char* d = dst_recs + (size_t)k * Ld.rec_bytes;
  BbxHdr h = *(const BbxHdr*)s;
  if (Ls.kind == 1) bstage_copy<W>(benv_view<W>(d, Ld), benv_view<W>(s, Ls), h.nG, h.nP);
  else stage_copy<W>(env_view<W>(d, Ld), env_view<W>(s, Ls), h.nG, h.nP, h.arena_used);
  if (lane_id() == 0) {
    if (bbx_st_capacity(h.status)) h.status = BBX_ST_OK;
    *(BbxHdr*)d = h;
  }
}
extern "C" int bbx_launch_relayout(const char* src_recs, char* dst_recs, const BbxLayout* Ls, const BbxLayout* Ld, int B, hipStream_t stream) {
  return bbx_launched(bbx_pick<2, 4, 8>((int)Ls->W, [&](auto W) {
    return bbx_launch<bbx_relayout_kernel<W()>>(dim3((B + 3) / 4), 256, 0, stream, src_recs, dst_recs, *Ls, *Ld, B);
  }));
}

// persistent sessions: the host's hand on the control word (one relaxed agent-scope atomic store: what the waves' polls observe)
__global__ void bbx_ctl_kernel(unsigned long long* ctl, unsigned long long value) {
  if (threadIdx.x == 0 && blockIdx.x == 0) __hip_atomic_store(ctl, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
extern "C" int bbx_launch_ctl(unsigned long long* ctl, unsigned long long value, hipStream_t stream) {
  return bbx_launched(bbx_launch<bbx_ctl_kernel>(dim3(1), 64, 0, stream, ctl, value));
}

// compact copy of every header so the host reads them with one contiguous transfer
__global__ void bbx_gather_hdr_kernel(const char* recs, uint32_t rec_bytes, int B, BbxHdr* out) {
  int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= B) return;
  out[env] = *(const BbxHdr*)(recs + (size_t)env * rec_bytes);
}
// the four header words the host polls after every launch
__global__ void bbx_gather_lite_kernel(const char* recs, uint32_t rec_bytes, int B, int4* out) {
  int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= B) return;
  const BbxHdr* h = (const BbxHdr*)(recs + (size_t)env * rec_bytes);
  out[env] = make_int4(bbx_lite_word0(h->status, 0, 0), h->q_head, h->budget, h->nP);
}
extern "C" int bbx_launch_gather_lite(const char* recs, uint32_t rec_bytes, int B, void* out, hipStream_t stream) {
  return bbx_launched(bbx_launch<bbx_gather_lite_kernel>(dim3((B + 255) / 256), 256, 0, stream, recs, rec_bytes, B, (int4*)out));
}
extern "C" int bbx_launch_gather_hdr(const char* recs, uint32_t rec_bytes, int B, BbxHdr* out, hipStream_t stream) {
  return bbx_launched(bbx_launch<bbx_gather_hdr_kernel>(dim3((B + 255) / 256), 256, 0, stream, recs, rec_bytes, B, out));
}

// prepared weights of the PMLP policy kernels (layout: bbx_pmlp.h)
__global__ void bbx_pmlp_prepare_kernel(const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2, float b2,
                                        int cols, int hidden, float* __restrict__ out) {
  const int HP = 32 * pmlp_nb_for(hidden), K2 = 2 * pmlp_ks_for(cols);
  const int total = (K2 + 2) * HP + 4;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int k = i / HP, h = i - k * HP;
    float v = 0.f;
    if (k < K2) v = (k < cols && h < hidden) ? w1[(size_t)k * hidden + h] : 0.f;
    else if (k == K2) v = h < hidden ? b1[h] : 0.f;
    else if (k == K2 + 1) v = h < hidden ? w2[h] : 0.f;
    else v = h == 0 ? b2 : 0.f;
    out[i] = v;
  }
}
extern "C" int bbx_launch_pmlp_prepare(const float* w1, const float* b1, const float* w2, float b2, int cols, int hidden, float* out, hipStream_t stream) {
  return bbx_launched(bbx_launch<bbx_pmlp_prepare_kernel>(dim3(16), 256, 0, stream, w1, b1, w2, b2, cols, hidden, out));
}
// the (NB, KS) table of the one-layer kernels: f(NB, KS) of the network's unit blocks and the columns' k-steps
template <class F>
static int pmlp_pick_shape(int hidden, int cols, F&& f) {
  return bbx_pick<1, 2, 4, 8>(pmlp_nb_for(hidden), [&](auto NB) { return bbx_pick<3, 6, 10, 16, 32>(pmlp_ks_for(cols), [&](auto KS) { return f(NB, KS); }); });
}
extern "C" int bbx_launch_pmlp_act(const int32_t* obs, const int32_t* rows, int B, int obs_rows, int cols, const float* wp, int hidden, const float* u,
                                   int32_t* actions, float* logprobs, int greedy, hipStream_t stream) {
  const int waves = 4;
  return bbx_launched(pmlp_pick_shape(hidden, cols, [&](auto NB, auto KS) {
    return bbx_launch<bbx_pmlp_act_mfma_kernel<NB(), KS()>>(dim3((B + waves - 1) / waves), waves * WAVE, pmlp_lds_bytes(waves, obs_rows), stream, obs, rows, B, obs_rows,
                                                            cols, wp, u, actions, logprobs, greedy);
  }));
}
// log-probability / entropy of recorded actions, the weight gradients (bbx_pmlp_grad.h) and the critic (bbx_pmlp_value.h), all over
// the same (NB, KS) table, and each for s.index null or not (non-null: the indexed instantiations, position k is about recorded
// state index[k] of n_src); the forward kernels also with or without their epilogue (loss / fit).
// (the launchers take the records of bbx_pmlp_shape.h)
extern "C" int bbx_launch_pmlp_logprob(const PmlpStates& s, const PmlpNet& net, const int32_t* actions, float* logprobs, float* entropy, const PmlpLoss* loss,
                                       hipStream_t stream) {
  if (s.n <= 0) return 0;
  const int waves = 4;
  const PmlpLoss ls = loss ? *loss : PmlpLoss{};
  return bbx_launched(pmlp_pick_shape(net.h1, s.cols, [&](auto NB, auto KS) { return bbx_pick_bool(s.index != nullptr, [&](auto IDX) {
    return bbx_pick_bool(loss != nullptr, [&](auto LOSS) {
      return bbx_launch<bbx_pmlp_logprob_kernel<NB(), KS(), IDX(), LOSS()>>(dim3((s.n + waves - 1) / waves), waves * WAVE, pmlp_lds_bytes(waves, s.obs_rows), stream, s.obs,
                                                                            s.rows, actions, s.n, s.obs_rows, s.cols, net.prepared, logprobs, entropy, s.index, s.n_src, ls);
    }); }); }));
}
// the statistics of a PPO call, one or two hidden layers, from the tail its forward kernel wrote (n == 0: zeros)
extern "C" int bbx_launch_pmlp_ppo_stats(const float* tail, int n, double* stats, hipStream_t stream) {
  return bbx_launched(bbx_launch<bbx_pmlp_ppo_stats_kernel>(dim3(1), PMLP_PPO_STAT_THREADS, 0, stream, tail, n, stats));
}
// how the policy's and the critic's gradient kernels are launched: nw waves per unit group (0: no launch, the second kernel writes
// zeros), ng unit groups
struct PmlpGradLaunch {
  static constexpr int waves = 4;
  int nw, ng;
  dim3 grid;
  size_t lds;
  // (indexed with no recorded state at all: every index is out of range, nothing contributes, and the kernel, which reads state 0
  // in place of an index out of range, is not launched)
  PmlpGradLaunch(const PmlpStates& s, int hidden)
      : nw(s.n > 0 && !(s.index && s.n_src == 0) ? pmlp_grad_waves(s.n) : 0), ng(pmlp_nb_for(hidden) / pmlp_grad_ubw(s.cols, hidden)),
        grid((nw + waves - 1) / waves, ng), lds(pmlp_grad_lds_bytes(waves, s.obs_rows)) {}
};
// the second kernel of either, unless launching the first (rc) has failed: the nw partial sums of every output added in order
static int pmlp_grad_reduce(int rc, const PmlpGrads& g, int nw, int cols, int hidden, hipStream_t stream) {
  if (rc) return rc;
  if ((rc = (int)hipGetLastError())) return rc;
  return bbx_launched(bbx_launch<bbx_pmlp_grad_reduce_kernel>(dim3((cols * hidden + 2 * hidden + 1 + 63) / 64), 256, 0, stream, (const float*)g.workspace, nw, cols,
                                                               hidden, g.gw1, g.gb1, g.gw2, g.gb2));
}
extern "C" int bbx_launch_pmlp_grad(const PmlpStates& s, const PmlpNet& net, const int32_t* actions, const float* glogp, const float* gent, const PmlpGrads& g,
                                    hipStream_t stream) {
  const PmlpGradLaunch L(s, net.h1);
  int rc = 0;
  if (L.nw > 0) rc = pmlp_pick_shape(net.h1, s.cols, [&](auto NB, auto KS) { return bbx_pick_bool(s.index != nullptr, [&](auto IDX) {
    return bbx_launch<bbx_pmlp_grad_kernel<NB(), KS(), IDX()>>(L.grid, L.waves * WAVE, L.lds, stream, s.obs, s.rows, actions, s.n, s.obs_rows, s.cols, net.prepared, glogp,
                                                               gent, L.nw, g.workspace, s.index, s.n_src);
  }); });
  return pmlp_grad_reduce(rc, g, L.nw, s.cols, net.h1, stream);
}
// cross-entropy against target rows: the forward kernel with the cross-entropy epilogue (x.coef null: losses and entropy alone),
// the statistics of a call, one or two hidden layers, from the tail it wrote (n == 0: zeros), and the gradient kernel on coef = c | T
extern "C" int bbx_launch_pmlp_xent(const PmlpStates& s, const PmlpNet& net, const PmlpXent& x, float* losses, float* entropy, hipStream_t stream) {
  if (s.n <= 0) return 0;
  const int waves = 4;
  return bbx_launched(pmlp_pick_shape(net.h1, s.cols, [&](auto NB, auto KS) { return bbx_pick_bool(s.index != nullptr, [&](auto IDX) {
    return bbx_launch<bbx_pmlp_logprob_kernel<NB(), KS(), IDX(), true, PmlpXent>>(dim3((s.n + waves - 1) / waves), waves * WAVE, pmlp_lds_bytes(waves, s.obs_rows), stream,
                                                                                  s.obs, s.rows, (const int32_t*)nullptr, s.n, s.obs_rows, s.cols, net.prepared, losses,
                                                                                  entropy, s.index, s.n_src, x);
  }); }));
}
extern "C" int bbx_launch_pmlp_xent_stats(const float* tail, int n, double* stats, hipStream_t stream) {
  return bbx_launched(bbx_launch<bbx_pmlp_xent_stats_kernel>(dim3(1), PMLP_PPO_STAT_THREADS, 0, stream, tail, n, stats));
}
extern "C" int bbx_launch_pmlp_xent_grad(const PmlpStates& s, const PmlpNet& net, const float* targets, const float* coef, const PmlpGrads& g, hipStream_t stream) {
  const PmlpGradLaunch L(s, net.h1);
  int rc = 0;
  if (L.nw > 0) rc = pmlp_pick_shape(net.h1, s.cols, [&](auto NB, auto KS) { return bbx_pick_bool(s.index != nullptr, [&](auto IDX) {
    return bbx_launch<bbx_pmlp_xent_grad_kernel<NB(), KS(), IDX()>>(L.grid, L.waves * WAVE, L.lds, stream, s.obs, s.rows, targets, s.n, s.obs_rows, s.cols, net.prepared,
                                                                    coef, L.nw, g.workspace, s.index, s.n_src);
  }); });
  return pmlp_grad_reduce(rc, g, L.nw, s.cols, net.h1, stream);
}
// the critic: values of n positions (fit != null: with the squared-error epilogue)
extern "C" int bbx_launch_pmlp_value(const PmlpStates& s, const PmlpNet& net, int pool, float* values, double* values64, const PmlpFit* fit, hipStream_t stream) {
  if (s.n <= 0) return 0;
  const int waves = 4;
  const PmlpFit ft = fit ? *fit : PmlpFit{};
  return bbx_launched(pmlp_pick_shape(net.h1, s.cols, [&](auto NB, auto KS) { return bbx_pick_bool(s.index != nullptr, [&](auto IDX) {
    return bbx_pick_bool(fit != nullptr, [&](auto FIT) {
      return bbx_launch<bbx_pmlp_value_kernel<NB(), KS(), IDX(), FIT()>>(dim3((s.n + waves - 1) / waves), waves * WAVE, pmlp_lds_bytes(waves, s.obs_rows), stream, s.obs,
                                                                         s.rows, s.n, s.obs_rows, s.cols, net.prepared, pool, values, values64, s.index, s.n_src, ft);
    }); }); }));
}
// the statistics of a fit call from the tail its forward kernel wrote (n == 0: zeros)
extern "C" int bbx_launch_pmlp_value_stats(const float* tail, int n, double* stats, hipStream_t stream) {
  return bbx_launched(bbx_launch<bbx_pmlp_value_stats_kernel>(dim3(1), PMLP_PPO_STAT_THREADS, 0, stream, tail, n, stats));
}
// the critic's weight gradients
extern "C" int bbx_launch_pmlp_value_grad(const PmlpStates& s, const PmlpNet& net, int pool, const float* gvalue, const PmlpGrads& g, hipStream_t stream) {
  const PmlpGradLaunch L(s, net.h1);
  int rc = 0;
  if (L.nw > 0) rc = pmlp_pick_shape(net.h1, s.cols, [&](auto NB, auto KS) { return bbx_pick_bool(s.index != nullptr, [&](auto IDX) {
    return bbx_launch<bbx_pmlp_value_grad_kernel<NB(), KS(), IDX()>>(L.grid, L.waves * WAVE, L.lds, stream, s.obs, s.rows, s.n, s.obs_rows, s.cols, net.prepared, pool,
                                                                     gvalue, L.nw, g.workspace, s.index, s.n_src);
  }); });
  return pmlp_grad_reduce(rc, g, L.nw, s.cols, net.h1, stream);
}


// ------------------------------------------------------------------ host-callable launcher
// (BBX_K_WIDE: envs_per_block is the number of waves per environment)
extern "C" int bbx_launch_step(const BbxParams* p, BbxKernel kind, int envs_per_block, hipStream_t stream) {
  const int threads = envs_per_block * WAVE;
  const int blocks = (p->B + envs_per_block - 1) / envs_per_block;
  if (kind == BBX_K_FAST) return bbx_launched(bbx_launch_fast(p, blocks, threads, envs_per_block, stream));
  if (kind == BBX_K_WIDE) {
    if (p->L.W != 2 && p->L.W != 4 && p->L.W != 8) return (int)hipErrorInvalidValue;
    return bbx_launch_wide(p, envs_per_block, stream);
  }
  const size_t lds = kind == BBX_K_STAGED ? (size_t)envs_per_block * p->LL.rec_bytes : 0;
  return bbx_launched(p->L.kind == 1 ? bbx_launch_binom(p, kind, blocks, threads, lds, stream) : bbx_launch_general(p, kind, blocks, threads, lds, stream));
}

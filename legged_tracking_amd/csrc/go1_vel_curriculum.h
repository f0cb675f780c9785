// go1_vel_curriculum.h -- the curriculum launch of the velocity step: RngD (the f64 draws), CArgs, CkShared, the
// prologue / phase / commit sections of a resample, hist_shift, go1_vel_curriculum_kernel and go1_vel_list_kernel.
// Restates _resample_commands (legged_robot_velocity_tracking.py:728-842) with RewardThresholdCurriculum.update,
// and Curriculum.sample (go1_gym/envs/base/curriculum.py), and HistoryWrapper.step's shift (history_wrapper.py:22).
// A part of go1_velocity.hip, included after go1_vel_step.h.
#pragma once
#ifndef GO1_VELOCITY_HIP
#error "include this part from go1_velocity.hip: its parts are not self-contained"
#endif
#pragma clang fp contract(off)  // pinned bit for bit to the oracle

// =====================================================================
//        command curriculum (_resample_commands) + history shift
// =====================================================================
// ---------------------------------------------------------------- f64 draws (curriculum RandomState)
struct RngD {
  const double* U;  // parity mode (n_envs, GO1_VEL_D_PER_ENV) or nullptr
  uint64_t seed, step;
  int e, gid;
  __device__ double operator()(int slot) const {
    if (U) return U[(size_t)e * GO1_VEL_D_PER_ENV + slot];
    // numpy's random_sample from two 32-bit words: (a >> 5, b >> 6) -> 53 bits
    uint32_t c[4] = {(uint32_t)gid, 0x40000000u | ((uint32_t)slot >> 1), (uint32_t)step, (uint32_t)(step >> 32)};
    philox4x32(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const uint32_t a = c[2 * (slot & 1)] >> 5, b = c[2 * (slot & 1) + 1] >> 6;
    return ((double)a * 67108864.0 + (double)b) * (1.0 / 9007199254740992.0);
  }
};

#define CK_THREADS 1024
#ifdef GO1_VEL_STAMPS  // diagnostic build only (tools/vel_stamps.py): per section of block 0, cycle sums
// [phase B / A][section] and the number of phases that ran with selected envs
__device__ unsigned long long g_vstamps[2][16];
#define VSTAMP(ph, k, t0)                                                            \
  do {                                                                              \
    if (threadIdx.x == 0 && blockIdx.x == 0) {                                      \
      const unsigned long long t_ = __builtin_amdgcn_s_memtime();                    \
      atomicAdd(&g_vstamps[ph][k], t_ - t0);                                        \
      t0 = t_;                                                                      \
    }                                                                               \
  } while (0)
#else
#define VSTAMP(ph, k, t0)
#endif
#define CK_PRE 1024  // list records prefetched into LDS per phase (one per thread); the rest read from memory
static_assert(CK_PRE <= CK_THREADS, "the prologue fills one prefetched record per thread (S.rec[ph][tid], tid < CK_THREADS)");
// the curriculum's record of a selected env: (env, command category, command bin, success of every task over the
// episode's command sums) -- written by the step kernel (or go1_vel_list_kernel) before the launch
typedef int4 CkRec;
struct CArgs {
  // the prologue's inputs lead (a launch that preloads the first kernel-argument dwords into registers has them
  // without a load)
  int n_envs, nb, R;    // nb, R: v->n_bins, v->resample_interval (no load of the config block in the prologue)
  int doA;              // A kind below: the next step's interval resample
  const uint8_t* maskB; // B kind below: reset_idx's envs
  const int32_t* episode_length;  // st.episode_length
  double* cdf;          // (GO1_VEL_N_CATEGORIES, n_bins): numpy's normalised cdf of each curriculum
  int32_t* cdf_ok;      // [GO1_VEL_N_CATEGORIES]: cdf current for the weights
  const CkRec* list;    // the selection lists: B at [0, n_envs), A at [n_envs, 2 n_envs)
  const unsigned long long* cnt;  // their lengths: B low word, A high word
  go1_vel_state st;
  const double* grid;   // (GO1_VEL_N_KEYS, n_bins)
  const int32_t* adj_ptr;  // neighbourhood table (CSR): cells adjacent to bin b are adj_idx[adj_ptr[b] ..]
  const int32_t* adj_idx;
  int env_id_offset;
  int nblk;             // curriculum workgroups (blocks 0 .. nblk - 1; the rest shift the history)
  int* done;            // their completion count (zero between launches)
  uint64_t seed;
  // B kind: the envs of maskB (reset_idx's resample)
  const float* UB;
  const double* UDB;
  uint64_t stepB;
  // A kind: envs with (episode_length + 1) % resample_interval == 0 (the next step's interval resample)
  const float* UA;
  const double* UDA;
  uint64_t stepA;
  // with B: extras["time_outs"] = time_out if some env was selected (:251-252), and the obs / obs_history
  // command columns of the resampled envs
  const uint8_t* time_out;
  uint8_t* extras_time_outs;
  float* obs;
  float* hist_out;
  const float* hist_in;
  int64_t ld_in, ld_out;  // row strides (floats)
  int hist_w;
  int hist_aligned;  // hist_w and both strides % 4 == 0, both buffers 16-byte aligned: 16-byte chunks
  uint32_t delay;    // test knob (GO1_VEL_CK_DELAY, 0 in use): workgroups 1.. wait this many s_memtime ticks before
                     // their success counts, so workgroup 0 samples (writes the command state) first
};

// numpy's pairwise summation (np.add.reduce of a contiguous f64 array), PW_BLOCKSIZE 128
template <int D>
__device__ double np_pairwise_sum(const double* a, int n) {
  if (D == 0 || n <= 128) {
    if (n < 8) {
      double r = 0.0;
      for (int i = 0; i < n; ++i) r += a[i];
      return r;
    }
    double r[8];
    for (int j = 0; j < 8; ++j) r[j] = a[j];
    int i = 8;
    for (; i < n - (n % 8); i += 8)
      for (int j = 0; j < 8; ++j) r[j] += a[i + j];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i];
    return res;
  }
  int n2 = n / 2;
  n2 -= n2 % 8;
  return np_pairwise_sum<(D > 0 ? D - 1 : 0)>(a, n2) + np_pairwise_sum<(D > 0 ? D - 1 : 0)>(a + n2, n - n2);
}

__device__ __forceinline__ float remainder1(float a) { return remainder_f(a, 1.0f); }

// LDS of a curriculum workgroup (one allocation for the launch)
struct CkShared {
  int hist[GO1_VEL_N_CATEGORIES * GO1_VEL_MAX_BINS];  // success count per (category, bin)
  double p[GO1_VEL_N_CATEGORIES * GO1_VEL_MAX_BINS];  // per category: the cdf the sampling searches
  double w[GO1_VEL_N_CATEGORIES * GO1_VEL_MAX_BINS];  // the curriculum weights (committed by the last workgroup)
  int list[GO1_VEL_N_CATEGORIES * GO1_VEL_MAX_BINS];  // distinct (category, bin) success pairs
  int inc[GO1_VEL_N_CATEGORIES * GO1_VEL_MAX_BINS];   // +0.2 steps per weight cell
  CkRec rec[2][CK_PRE];                               // the first CK_PRE records of the B and the A list
  int cnt[4];                                         // |list B|, |list A|, |pairs|, last-workgroup flag
  int dirty[GO1_VEL_N_CATEGORIES];                    // weights changed in this phase
  int pvalid[GO1_VEL_N_CATEGORIES];                   // p holds the cdf of the current weights
  int rec_[GO1_VEL_N_CATEGORIES];                     // p recomputed in this launch (the cache to commit)
  int wchg;                                           // some weight changed in this launch
  int wloaded;                                        // w holds the weights (loaded on first need)
};

// Workgroup barrier for LDS hand-offs: every exchange between the curriculum's sections goes through LDS, and
// __syncthreads also waits out every global access in flight -- the sampling's command / observation stores
// and the rebinding's writes, ~2 k cycles at each phase end for nothing (nothing in the launch reads them back).
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// the weights into LDS, once per launch, when a phase first needs them (called by the whole workgroup)
__device__ void ensure_weights(VCfg* v, const CArgs& K, CkShared& S) {
  if (S.wloaded) return;
  const int nb = K.nb;
  for (int i = threadIdx.x; i < GO1_VEL_N_CATEGORIES * nb; i += CK_THREADS) {
    const int c = i / nb;
    S.w[(size_t)c * GO1_VEL_MAX_BINS + (i - c * nb)] = K.st.curriculum_weights[i];
  }
  lds_barrier();
  if (threadIdx.x == 0) S.wloaded = 1;
  lds_barrier();
}

// The curriculum runs on K.nblk workgroups.  Everything _resample_commands computes for the batch as a whole --
// the selections, the success counts, the weight update and the cdf -- is computed by every workgroup from the
// same inputs (identical results, no cross-workgroup hand-off); the per-env work (the draws, the commands, the
// observation patch) is split: the env at position i of a phase's ascending list belongs to workgroup
// i % nblk.  The last workgroup to finish commits the weights and the cdf cache.  An env selected by both
// phases is written by phase A only (its phase-B commands reach this step's observation; the state the
// reference's second resample overwrites is never written twice by two workgroups), and phase A's success
// check for it recomputes the category and bin phase B drew (a pure function of its draws and phase B's cdf).
__device__ __forceinline__ bool selectedB(const CArgs& K, int e) { return K.maskB && K.maskB[e] != 0; }
__device__ __forceinline__ bool selectedA(const CArgs& K, int e, int R) {
  return K.doA && (K.st.episode_length[e] + 1) % R == 0;
}

// The launch is latency-bound: a handful of envs per phase behind a chain of barrier-separated sections, and
// a barrier waits out every memory access in flight.  So each section issues all the memory reads it can at
// once: the prologue loads the list lengths, the first CK_PRE records of both lists (at clamped positions,
// before their lengths are known) and the cached cdfs in one round trip; a phase then costs the success counts
// (LDS only), the weight update (when some env succeeded), the cdf of changed weights, and the sampling
// (commands and grid cells together).
// The prologue's inputs come as the launch's leading scalar arguments (the same values as the CArgs fields):
// with kernel-argument preloading they arrive in registers with the wave.
__device__ __forceinline__ void resample_prologue(VCfg* v, const CArgs& K, CkShared& S, int pn, int pnb,
                                                  const unsigned long long* pcnt, const CkRec* plist,
                                                  const double* pcdf, const int32_t* pcdf_ok) {
  const int tid = threadIdx.x, n = pn, nb = pnb;
#ifdef GO1_VEL_STAMPS
  unsigned long long t0 = __builtin_amdgcn_s_memtime();
#endif
  const int lane = tid & 63, wv = tid >> 6;
  const unsigned long long cc = *pcnt;
  const CkRec rB = plist[min(tid, n - 1)], rA = plist[(size_t)n + min(tid, n - 1)];
  for (int i = tid; i < GO1_VEL_N_CATEGORIES * nb; i += CK_THREADS) S.hist[i] = 0;
  if (tid < GO1_VEL_N_CATEGORIES) { S.dirty[tid] = 0; S.rec_[tid] = 0; }
  if (tid == 0) { S.wchg = 0; S.wloaded = 0; S.cnt[2] = 0; S.cnt[3] = 0; }
  // the cached cdfs (wave c), whether or not a phase will need them
  double t[GO1_VEL_MAX_BINS / 64];
  int ok = 0;
  if (wv < GO1_VEL_N_CATEGORIES) {  // the weights are loaded only when a phase needs them (ensure_weights)
    const int c = wv & 3;
    const double* g = pcdf + (size_t)c * nb;
    ok = pcdf_ok[c];
    // unconditional loads (index clamped): a load under a condition makes hipcc wait for it right away
#pragma unroll
    for (int i = 0; i < GO1_VEL_MAX_BINS / 64; ++i) t[i] = g[min(lane + 64 * i, nb - 1)];
  }
  const int nB = (int)(uint32_t)cc, nA = (int)(uint32_t)(cc >> 32);
  if (tid == 0) { S.cnt[0] = nB; S.cnt[1] = nA; }
  if (tid < nB) S.rec[0][tid] = rB;
  if (tid < nA) S.rec[1][tid] = rA;
  if (wv < GO1_VEL_N_CATEGORIES) {
    const int c = wv & 3;
    double* dst = S.p + (size_t)c * GO1_VEL_MAX_BINS;
#pragma unroll
    for (int i = 0; i < GO1_VEL_MAX_BINS / 64; ++i)
      if (lane + 64 * i < nb) dst[lane + 64 * i] = t[i];
    if (lane == 0) S.pvalid[c] = ok;
  }
  lds_barrier();
  VSTAMP(0, 10, t0);
}

// record i of a phase's list (ph 0: B, 1: A)
__device__ __forceinline__ CkRec ck_rec(const CArgs& K, const CkShared& S, int ph, int i) {
  return i < CK_PRE ? S.rec[ph][i] : K.list[(size_t)ph * K.n_envs + i];
}

// searchsorted(cdf, u, side='right') clipped to the last bin (numpy's choice)
__device__ __forceinline__ int cdf_search(const double* cdf, int nb, double u) {
  int lo = 0, hi = nb;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (cdf[mid] <= u) lo = mid + 1; else hi = mid;
  }
  return min(lo, nb - 1);
}

// the category draw of a resample: category c when 0.25 c <= u < 0.25 (c + 1) (as f32), -1 otherwise
__device__ __forceinline__ int draw_category(float uc) {
  int cat = -1;
  for (int c = 0; c < GO1_VEL_N_CATEGORIES; ++c)
    if ((float)(0.25 * c) <= uc && uc < (float)(0.25 * (c + 1))) cat = c;
  return cat;
}

// One resample (_resample_commands :728-842) of kind B (mask) or A (interval), by the whole workgroup.
__device__ void resample_phase(VCfg* v, const CArgs& K, bool kindB, CkShared& S) {
  const int tid = threadIdx.x, n = K.n_envs, nb = K.nb, R = K.R;
  const int blk = blockIdx.x, nblk = K.nblk;
  const go1_vel_state& st = K.st;
  const float* U = kindB ? K.UB : K.UA;
  const double* UD = kindB ? K.UDB : K.UDA;
  const uint64_t step = kindB ? K.stepB : K.stepA;
  const int ucat = kindB ? GO1_VEL_U_CAT_B : GO1_VEL_U_CAT_A;
  const int dch = kindB ? GO1_VEL_D_CHOICE_B : GO1_VEL_D_CHOICE_A;
  const int NC = v->n_terms + GO1_VEL_SUM_EXTRA;
  const int ph = kindB ? 0 : 1;
#ifdef GO1_VEL_STAMPS
  unsigned long long t0 = __builtin_amdgcn_s_memtime();
#endif
  const int count = S.cnt[ph];
  VSTAMP(ph, 0, t0);
  if (count == 0) return;  // len(env_ids) == 0 (:730): nothing, not even the time-out rebinding
  VSTAMP(ph, 15, t0);
  if (K.delay && blk > 0) {  // test knob only (tests/test_gpu_velocity.py)
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    while (__builtin_amdgcn_s_memtime() - t1 < (unsigned long long)K.delay) __builtin_amdgcn_s_sleep(16);
  }
  // ---- RewardThresholdCurriculum.update per old category (:736-757, curriculum.py:135-154): success
  // counts per (category, bin), and the list of the (category, bin) pairs that have any.  The inputs come
  // from the records (the state at the end of the step), never from the command state the sampling rewrites.
  for (int i = tid; i < count; i += CK_THREADS) {
    if (v->n_task == 0) break;
    const CkRec r = ck_rec(K, S, ph, i);
    const int e = r.x;
    int cat = r.y, b = r.z;
    bool ok = r.w != 0;
    if (!kindB && selectedB(K, e)) {
      // phase B resampled this env: its sums are zero and its category / bin are phase B's draws, recomputed
      // here from phase B's uniforms and cdf (S.p still holds it: phase A's cdf comes after these counts)
      const Rng rng = {K.UB, K.seed, K.stepB, e, e + K.env_id_offset, GO1_VEL_U_PER_ENV};
      const RngD rngd = {K.UDB, K.seed, K.stepB, e, e + K.env_id_offset};
      const int cb = draw_category(rng(GO1_VEL_U_CAT_B));
      if (cb >= 0) {
        cat = cb;
        b = cdf_search(S.p + (size_t)cat * GO1_VEL_MAX_BINS, nb, rngd(GO1_VEL_D_CHOICE_B));
      }
      ok = true;
      for (int k = 0; k < v->n_task; ++k) ok = ok && (0.0f / v->curriculum_ep_len > v->task_threshold[k]);
    }
    if (cat < 0 || cat >= GO1_VEL_N_CATEGORIES) continue;
    if (ok && b >= 0 && b < nb) {
      if (atomicAdd(&S.hist[cat * nb + b], 1) == 0) {
        const int slot = atomicAdd(&S.cnt[2], 1);
        S.list[slot] = cat * nb + b;  // at most GO1_VEL_N_CATEGORIES * nb distinct pairs
      }
    }
  }
  if (kindB && K.extras_time_outs)  // this workgroup's share of the rebinding
    for (int e = blk * CK_THREADS + tid; e < n; e += nblk * CK_THREADS) K.extras_time_outs[e] = K.time_out[e];
  lds_barrier();
  VSTAMP(ph, 1, t0);
  const int n_list = S.cnt[2];
  // weights: cell j of category c gets +0.2 (clipped) once if it was a success bin and once per success
  // env whose bin's neighbourhood holds it -- a sequence of identical clip(w + 0.2, 0, 1) steps, so the
  // count decides the result whatever the order.  Neighbourhoods come from the handle's table
  // (get_local_bins, curriculum.py:123-133, evaluated on the host in the same f64 comparisons).
  if (n_list > 0) {
    ensure_weights(v, K, S);
    for (int i = tid; i < GO1_VEL_N_CATEGORIES * nb; i += CK_THREADS) S.inc[i] = 0;
    lds_barrier();
    for (int l = tid; l < n_list; l += CK_THREADS) {
      const int cb = S.list[l], cat = cb / nb, b = cb % nb, h = S.hist[cb];
      atomicAdd(&S.inc[cb], 1);  // weights[bin_inds[is_success]] += 0.2 (once per distinct bin)
      const int q0 = K.adj_ptr[b], q1 = K.adj_ptr[b + 1];
      for (int q = q0; q < q1; q += 8) {  // eight neighbour indices in flight at a time
        int j[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) j[u] = q + u < q1 ? K.adj_idx[q + u] : -1;
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (j[u] >= 0) atomicAdd(&S.inc[cat * nb + j[u]], h);
      }
    }
    lds_barrier();
    for (int i = tid; i < GO1_VEL_N_CATEGORIES * nb; i += CK_THREADS) {
      const int k = S.inc[i];
      if (k > 0) {
        const int c = i / nb;
        double w = S.w[(size_t)c * GO1_VEL_MAX_BINS + (i - c * nb)];
        for (int t = 0; t < k; ++t) w = fmin(fmax(w + 0.2, 0.0), 1.0);
        S.w[(size_t)c * GO1_VEL_MAX_BINS + (i - c * nb)] = w;
        S.dirty[c] = 1;
        S.wchg = 1;
      }
    }
    lds_barrier();
  }
  VSTAMP(ph, 2, t0);
  // ---- numpy rng.choice(p = w / w.sum()): cdf = cumsum(p) / cdf[-1], wave c for category c, in LDS
  // (S.p), recomputed where the weights changed (or no cdf is cached)
  if (!S.pvalid[0] || !S.pvalid[1] || !S.pvalid[2] || !S.pvalid[3]) ensure_weights(v, K, S);  // uniform
  {
    const int wv = tid >> 6, ln = tid & 63;
    if (wv < GO1_VEL_N_CATEGORIES && (S.dirty[wv] || !S.pvalid[wv])) {
      double* p = S.p + (size_t)wv * GO1_VEL_MAX_BINS;
      const double* w = S.w + (size_t)wv * GO1_VEL_MAX_BINS;
      for (int j = ln; j < nb; j += 64) p[j] = w[j];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      double s = 0.0;
      if (ln == 0) s = np_pairwise_sum<4>(p, nb);
      s = __shfl(s, 0);
      for (int j = ln; j < nb; j += 64) p[j] = p[j] / s;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      if (ln == 0) {  // numpy's sequential cumsum: the adds are a dependent chain, the LDS reads of a
                      // batch are issued ahead of it (in place, one read-write per element, it would wait
                      // out the LDS latency at every element)
        double acc = 0.0;
        for (int j0 = 0; j0 < nb; j0 += 32) {
          double u[32];
#pragma unroll
          for (int i = 0; i < 32; ++i) u[i] = j0 + i < nb ? p[j0 + i] : 0.0;
#pragma unroll
          for (int i = 0; i < 32; ++i) { acc += u[i]; u[i] = acc; }
#pragma unroll
          for (int i = 0; i < 32; ++i)
            if (j0 + i < nb) p[j0 + i] = u[i];
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const double last = p[nb - 1];
      for (int j = ln; j < nb; j += 64) p[j] = p[j] / last;
      if (ln == 0) {
        S.pvalid[wv] = 1;
        S.rec_[wv] = 1;
        S.dirty[wv] = 0;
      }
#ifdef GO1_VEL_STAMPS
      if (ln == 0 && blk == 0) atomicAdd(&g_vstamps[kindB ? 0 : 1][14], 1ull);
#endif
    }
  }
  lds_barrier();
  VSTAMP(ph, 3, t0);
  // ---- new category, cell and command per env (:759-842), this workgroup's envs (list positions
  // blk, blk + nblk, ...; env ids e % nblk == blk beyond the list capacity), 16 lanes per env: lane k < 15
  // draws and finishes command k (the gait rules and binary phases act per command; only the small-command
  // rule pairs commands 0 and 1), lane 15 draws the choice and searches the cdf.  One Philox evaluation per
  // lane instead of ~30 in sequence on one thread; the env's old commands are loaded before the search, so
  // they and the grid cells share one memory round trip.
  {
    const int sub = tid & 15, grp = tid >> 4;
    const int n_own = count > blk ? (count - blk + nblk - 1) / nblk : 0;
    for (int i0 = 0; i0 < n_own; i0 += CK_THREADS / 16) {
      const int i = i0 + grp;
      if (i >= n_own) continue;  // uniform over the env's 16 lanes
      const int e = ck_rec(K, S, ph, blk + i * nblk).x;
      // an env phase A resamples again: phase A writes its state, phase B only its observed commands
      const bool state_out = !(kindB && selectedA(K, e, R));
      const Rng rng = {U, K.seed, step, e, e + K.env_id_offset, GO1_VEL_U_PER_ENV};
      const RngD rngd = {UD, K.seed, step, e, e + K.env_id_offset};
      const int subc = min(sub, GO1_VEL_NUM_COMMANDS - 1);  // clamped: unconditional loads
      // the old command (kept when the category draw fails) is read first and not touched before the draws and
      // the cdf search are done
      const float cmd_old = st.commands[(size_t)e * GO1_VEL_NUM_COMMANDS + subc];
      const double half = v->bin_sizes[subc] / 2.0;
      const int cat = draw_category(rng(ucat));
      float cmd = 0.0f;
      if (cat >= 0) {
        const double u = rngd(sub < GO1_VEL_NUM_COMMANDS ? dch + 1 + sub : dch);
        VSTAMP(ph, 5, t0);
        int idx = 0;
        if (sub == 15) {
          idx = cdf_search(S.p + (size_t)cat * GO1_VEL_MAX_BINS, nb, u);
          if (state_out) {
            st.command_bins[e] = idx;
            st.command_categories[e] = cat;
          }
        }
        idx = __shfl(idx, 15, 16);
        VSTAMP(ph, 6, t0);
        const double cen = K.grid[(size_t)subc * nb + idx];
        if (sub < GO1_VEL_NUM_COMMANDS) {
          const double l = cen + half, h = cen - half;
          cmd = (float)(l + (h - l) * u);
          if (v->gaitwise_curricula && sub >= 5 && sub < 8) {
            if (cat == CAT_PRONK) cmd = remainder1(cmd / 2.0f - 0.25f);
            else if (sub - 5 == cat - 1) cmd = cmd / 2.0f + 0.25f;  // trot: 5, pace: 6, bound: 7
            else cmd = 0.0f;
          }
        }
      } else {
        cmd = sub < GO1_VEL_NUM_COMMANDS ? cmd_old : 0.0f;
      }
      if (v->binary_phases && sub >= 5 && sub < 8) cmd = remainder1(rintf(2.0f * cmd) / 2.0f);
      {
        const float c0 = __shfl(cmd, 0, 16), c1 = __shfl(cmd, 1, 16);
        const float keep = norm2_f(c0, c1) > 0.2f ? 1.0f : 0.0f;
        if (sub < 2) cmd = cmd * keep;
      }
      if (state_out) {
        if (sub < GO1_VEL_NUM_COMMANDS) st.commands[(size_t)e * GO1_VEL_NUM_COMMANDS + sub] = cmd;
        for (int k = sub; k < NC; k += 16) st.command_sums[(size_t)e * NC + k] = 0.0f;
      }
      if (kindB && K.obs && sub < GO1_VEL_NUM_COMMANDS) {  // this step's observation of the resampled commands (:339)
        const float clip = v->clip_obs;
        float val = cmd * v->cmd_scale[sub];
        if (v->add_noise) val = val + (2.0f * rng(GO1_VEL_U_NOISE + 3 + sub) - 1.0f) * v->noise_vec[3 + sub];
        val = clampf(val, -clip, clip);
        K.obs[(size_t)e * GO1_VEL_NUM_OBS + 3 + sub] = val;
        if (K.hist_out) K.hist_out[(size_t)e * K.ld_out + K.hist_w - GO1_VEL_NUM_OBS + 3 + sub] = val;
      }
    }
  }
  VSTAMP(ph, 7, t0);
  // ready for the next phase: success counts and the pair list cleared
  for (int i = tid; i < GO1_VEL_N_CATEGORIES * nb; i += CK_THREADS) S.hist[i] = 0;
  if (tid == 0) S.cnt[2] = 0;
  lds_barrier();
  VSTAMP(ph, 4, t0);
}

// The last curriculum workgroup to finish writes the weights and the recomputed cdfs (every workgroup holds
// the same values; all of them have read the old ones by then).  Release: every workgroup's reads and writes
// precede its ticket; acquire: the last one sees every other workgroup done before it writes.
__device__ void resample_commit(VCfg* v, const CArgs& K, CkShared& S) {
  const int tid = threadIdx.x, nb = K.nb;
  lds_barrier();
  // every workgroup takes the same decisions: with no weight changed and no cdf recomputed there is nothing
  // to commit, and none of them takes a ticket
  if (!S.wchg && !S.rec_[0] && !S.rec_[1] && !S.rec_[2] && !S.rec_[3]) return;
  __syncthreads();  // (a commit: every thread's global accesses precede the ticket's release)
#ifdef GO1_VEL_STAMPS
  unsigned long long t0 = __builtin_amdgcn_s_memtime();
#endif
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    const int old = __hip_atomic_fetch_add(K.done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    S.cnt[3] = old == K.nblk - 1;
    if (S.cnt[3]) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  }
  __syncthreads();
  if (!S.cnt[3]) return;
  for (int i = tid; i < GO1_VEL_N_CATEGORIES * nb; i += CK_THREADS) {
    const int c = i / nb, j = i - c * nb;
    if (S.rec_[c]) {  // a category whose weights changed had its cdf recomputed
      K.st.curriculum_weights[i] = S.w[(size_t)c * GO1_VEL_MAX_BINS + j];
      K.cdf[i] = S.p[(size_t)c * GO1_VEL_MAX_BINS + j];
    }
  }
  if (tid < GO1_VEL_N_CATEGORIES && S.rec_[tid]) K.cdf_ok[tid] = 1;
  if (tid == 0) *K.done = 0;  // the next launch's count (stream order)
  VSTAMP(0, 11, t0);
}

// HistoryWrapper.step's shift (history_wrapper.py:22): new[:, :W - 70] = old[:, 70:], by workgroups 1.. of
// the curriculum launch (g0: the thread's index among them, G: their thread count).  A pure HBM stream of
// 2 x 33 MB at 4096 envs x 30 observations.  Measured alternative, not kept: the shift as its own kernel on
// a side stream beside the step kernel -- it overlapped (27 us under the 47 us step kernel), but the two
// cross-stream hand-offs per step left ~11 us of idle GPU between steps: 70.6 against 69.1 us per step.
__device__ void hist_shift(const CArgs& K, size_t g0, size_t G) {
  if (!K.hist_in || !K.hist_out) return;
  const int W = K.hist_w, D = W - GO1_VEL_NUM_OBS;
  const size_t Li = (size_t)K.ld_in, Lo = (size_t)K.ld_out;
  if (K.hist_aligned) {
    // 16-byte chunks: rows are 16-byte aligned (W % 4 == 0), the source starts 70 = 4 x 17 + 2 floats in,
    // so dest chunk i = (z, w) of aligned source chunk 17 + i and (x, y) of chunk 18 + i, which the next
    // lane holds (lane 63 loads it).  Chunks per row padded to a multiple of 64 keep a wave in one row;
    // four chunks per thread are loaded before any is stored (HBM latency x bandwidth needs them in flight).
    // D = W - 70 is 2 mod 4: the last chunk of a row is half (its other half is the new obs row).
    const int Cn = (D + 3) / 4, Cp = (Cn + 63) & ~63;
    const size_t total = (size_t)K.n_envs * Cp;
    const bool last_lane = (threadIdx.x & 63) == 63;
    for (size_t t0 = g0; t0 < total; t0 += 4 * G) {
      float4 own[4];
      size_t ev[4];
      int iv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const size_t t = t0 + u * G;
        ev[u] = t / Cp;
        iv[u] = (int)(t % Cp);
        own[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (t < total && iv[u] < Cn) own[u] = reinterpret_cast<const float4*>(K.hist_in + ev[u] * Li)[17 + iv[u]];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const size_t t = t0 + u * G;  // t < total is uniform over the wave (total, G, t0 - lane: multiples of 64)
        if (t >= total) break;
        float nx = __shfl_down(own[u].x, 1), ny = __shfl_down(own[u].y, 1);
        const int i = iv[u];
        if (last_lane && i + 1 < Cn) {
          const float4 o2 = reinterpret_cast<const float4*>(K.hist_in + ev[u] * Li)[18 + i];
          nx = o2.x;
          ny = o2.y;
        }
        if (i < Cn) {
          float* dst = K.hist_out + ev[u] * Lo + 4 * i;
          if (4 * i + 4 <= D) *reinterpret_cast<float4*>(dst) = make_float4(own[u].z, own[u].w, nx, ny);
          else *reinterpret_cast<float2*>(dst) = make_float2(own[u].z, own[u].w);
        }
      }
    }
    return;
  }
  // any other width / alignment: f32 pairs (rows are 8-byte aligned: 70 x 4 B is not a multiple of 16)
  const int W2 = D / 2;
  const size_t total = (size_t)K.n_envs * W2;
  for (size_t i = g0; i < total; i += G) {
    const size_t e = i / W2, k = i % W2;
    const float2 val = *(const float2*)(K.hist_in + e * Li + GO1_VEL_NUM_OBS + 2 * k);
    *(float2*)(K.hist_out + e * Lo + 2 * k) = val;
  }
}

__global__ __launch_bounds__(CK_THREADS) void go1_vel_curriculum_kernel(const go1_vel_config* __restrict__ v_gen,
                                                                        int pn, int pnb,
                                                                        const unsigned long long* pcnt,
                                                                        const CkRec* plist, const double* pcdf,
                                                                        const int32_t* pcdf_ok, CArgs K) {
  VCfg* __restrict__ v = (VCfg*)v_gen;
  if ((int)blockIdx.x >= K.nblk) {
    hist_shift(K, (size_t)(blockIdx.x - K.nblk) * CK_THREADS + threadIdx.x, (size_t)(gridDim.x - K.nblk) * CK_THREADS);
    return;
  }
  __shared__ CkShared S;
  resample_prologue(v, K, S, pn, pnb, pcnt, plist, pcdf, pcdf_ok);
  if (K.maskB) resample_phase(v, K, true, S);
  if (K.doA) resample_phase(v, K, false, S);
  resample_commit(v, K, S);
}

// The selection lists of an explicit resample (go1_vel_resample: reset_idx's mask, or the interval envs) in
// ascending env order, one workgroup: thread t takes a contiguous run of envs, a block-wide scan places the
// runs.  The records carry the state the curriculum's success counts read.
__global__ __launch_bounds__(CK_THREADS) void go1_vel_list_kernel(const go1_vel_config* __restrict__ v_gen, CArgs K,
                                                                  CkRec* list, unsigned long long* cnt) {
  VCfg* __restrict__ v = (VCfg*)v_gen;
  __shared__ int wsum[2][CK_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, n = K.n_envs, R = K.R;
  const int NC = v->n_terms + GO1_VEL_SUM_EXTRA;
  const int per = (n + CK_THREADS - 1) / CK_THREADS, eb = tid * per;
  int cb = 0, ca = 0;
  for (int k = 0; k < per; ++k) {
    const int e = eb + k;
    if (e < n) {
      cb += selectedB(K, e) ? 1 : 0;
      ca += selectedA(K, e, R) ? 1 : 0;
    }
  }
  int ib = cb, ia = ca;  // inclusive scans over the wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int ub = __shfl_up(ib, o), ua = __shfl_up(ia, o);
    ib += lane >= o ? ub : 0;
    ia += lane >= o ? ua : 0;
  }
  if (lane == 63) { wsum[0][wv] = ib; wsum[1][wv] = ia; }
  __syncthreads();
  int ob = ib - cb, oa = ia - ca, totb = 0, tota = 0;
  for (int w = 0; w < CK_THREADS / 64; ++w) {
    ob += w < wv ? wsum[0][w] : 0;
    oa += w < wv ? wsum[1][w] : 0;
    totb += wsum[0][w];
    tota += wsum[1][w];
  }
  for (int k = 0; k < per; ++k) {
    const int e = eb + k;
    if (e >= n) break;
    const bool sb = selectedB(K, e), sa = selectedA(K, e, R);
    if (!sb && !sa) continue;
    bool ok = true;
    for (int t = 0; t < v->n_task; ++t)
      ok = ok && (K.st.command_sums[(size_t)e * NC + v->task_slot[t]] / v->curriculum_ep_len > v->task_threshold[t]);
    const CkRec r = make_int4(e, K.st.command_categories[e], K.st.command_bins[e], ok ? 1 : 0);
    if (sb) list[ob++] = r;
    if (sa) list[(size_t)n + oa++] = r;
  }
  if (tid == 0) *cnt = (unsigned long long)(uint32_t)totb | ((unsigned long long)(uint32_t)tota << 32);
}

// policy_split.h -- the per-net workgroups of the policy: SPLIT_D2, SplitLds, lds_barrier, split_body and its two
// kernels, policy_kernel_split (GO1_POLICY_FULL's second launch shape; GO1_POLICY_STUDENT with its actor workgroups
// only) and policy_kernel_split_teacher (GO1_POLICY_TEACHER), with SPLIT_ET_* (envs per workgroup).  The same nets
// as policy_full.h, K order and partial sums included.  A part of rollout.hip, included inside its anonymous
// namespace after policy_full.h (policy_fallback, PSTAMP).
#pragma once
#ifndef GO1_ROLLOUT_HIP
#error "include this part from rollout.hip: its parts are not self-contained"
#endif

// ---------------------------------------------------------------- per-net workgroups
// policy_kernel streams all 2.8 MB of split weights through every CU (each workgroup serves 16 envs
// with all three nets), the L2 -> CU floor of that decomposition.  Here a workgroup runs ONE net for
// 32 envs as two 16-env B tiles that share every weight fragment: the first ceil(n / 32)
// workgroups run the adaptation module + actor (1.6 MB), the others the critic (1.2 MB), so a CU
// streams at most 1.6 MB for twice the envs.  K order, tile split and partial-sum order are those
// of policy_kernel, so the outputs are identical.
// weight groups (32 K values) in flight per wave: the 512-wide first layers run two ahead (split_body's
// load0 / load1 register sets), the 256-wide second layers SPLIT_D2 ahead (in 16-deep groups, (4, 8),
// (6, 12), (8, 12) and (8, 16) for the two were all within 1 %)
constexpr int SPLIT_D2 = 6;

// LDS of policy_kernel_split: three env tiles of inputs and of 512-wide outputs.  Aliases (each used only
// after a barrier that ends the previous use): the 256-wide L2 outputs live in the input planes (dead once
// L1 has run); the adaptation module's L2 outputs in rows 256-383 of h1 (its L1 outputs hold rows 0-255)
// and its K-split partials in rows 384-511; the output layer's partials in the input planes.
struct SplitLds {
  Act<PIN> xin[3];
  Act<512> h1[3];
};
typedef float Scr[4][16][16];  // the output layer's K-split partials of one env tile

// Workgroup barrier over LDS only: waits for this wave's LDS operations, not for its global loads, so
// weight fragments requested ahead of a barrier stay in flight across it (__syncthreads' release fence
// waits for every memory operation).  policy_kernel_split never reads global memory it writes.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// TEACHER (with !CRITIC; GO1_POLICY_TEACHER): the actor on [history, privileged obs].  No adaptation layer runs;
// the privileged inputs are staged as the critic's are and every L1 group runs in the chunk pass.
template <int ET, bool CRITIC, bool TEACHER = false>
__device__ __forceinline__ void split_body(const go1_policy_args& P, SplitLds& S, int e0, int ne, int* s_ovf) {
  static_assert(!(CRITIC && TEACHER), "the teacher mode is the actor's");
  constexpr bool ADAPT = !CRITIC && !TEACHER;  // the adaptation module runs in front of the net
  constexpr bool PRIV = CRITIC || TEACHER;     // the net's last inputs are the privileged observations
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int q = lane >> 4, c = lane & 15;
  const int NP = P.num_priv;
  ActV vx[ET][1], v1[ET][1], v2[ET][1];
#pragma unroll
  for (int et = 0; et < ET; ++et) {
    vx[et][0] = S.xin[et].v();
    v1[et][0] = S.h1[et].v();
    v2[et][0] = S.xin[et].v();  // L2 outputs over the dead inputs
  }
  // Every layer's first weight fragments are requested before the barrier that ends the previous phase
  // (they depend on nothing the workgroup computes), so a layer starts with its weights landed instead
  // of one L2 round trip after the barrier.
  const PolicyLayer* Ls = P.layers;
  const PolicyLayer* LN = Ls + (CRITIC ? 7 : 3);
  // First layers, K-streamed in chunks of CG groups (PIN inputs) through the input planes: the adaptation
  // module's L1 over the history (GA groups), the actor's / critic's L1 over [history, latent | priv] (GL
  // groups).  The actor's groups from gl = H / 32 on hold latent inputs: they run after the adaptation
  // module, from the last chunk's planes (the host guarantees they lie in it).  One chunk when the inputs
  // fit PIN (the README configuration); the velocity task's 30-deep history (2,100) takes eight.
  const int H = P.hist_dim, KIN = H + NP;
  const int GA = (H + 31) / 32, GL = (KIN + 31) / 32, gl = H / 32;
  constexpr int CG = PIN / 32;
  const int nch = (GL + CG - 1) / CG, g_last = CG * (nch - 1);
  const int g_pass = PRIV ? GL : gl;  // L1 groups of the chunk pass
  // the f32 staging copy (h1 is free until the L1 epilogue); one chunk: the workgroup's rows are one
  // contiguous block of ne x H floats, copied with coalesced loads from one base pointer (all of the
  // thread's in flight) before the accumulators are live
  float* flat = reinterpret_cast<float*>(&S.h1[0]);
  const int fs = nch == 1 ? H : PIN;
  // L1 weight fragments, two groups ahead (two register sets, the group loop unrolled by two)
  f8_t wA0, wL00, wL01, wA1, wL10, wL11;
  auto load0 = [&](int g) {
    if constexpr (ADAPT) wA0 = reinterpret_cast<const f8_t*>(Ls[0].w)[((size_t)wave * GA + g) * 64 + lane];
    wL00 = reinterpret_cast<const f8_t*>(LN[0].w)[((size_t)wave * GL + g) * 64 + lane];
    wL01 = reinterpret_cast<const f8_t*>(LN[0].w)[((size_t)(wave + PW) * GL + g) * 64 + lane];
  };
  auto load1 = [&](int g) {
    if constexpr (ADAPT) wA1 = reinterpret_cast<const f8_t*>(Ls[0].w)[((size_t)wave * GA + g) * 64 + lane];
    wL10 = reinterpret_cast<const f8_t*>(LN[0].w)[((size_t)wave * GL + g) * 64 + lane];
    wL11 = reinterpret_cast<const f8_t*>(LN[0].w)[((size_t)(wave + PW) * GL + g) * 64 + lane];
  };
  // the first chunk's first two groups are requested before the inputs: they depend on nothing the workgroup
  // computes, so the weight stream starts under the input loads' latency instead of after the staging
  {
    const int gb0 = PRIV ? min(CG, GL) : min(gl, min(CG, GL));
    if (0 < gb0) load0(0);
    if (1 < gb0) load1(1);
    __builtin_amdgcn_sched_barrier(0);
  }
  if (nch == 1) {
    constexpr int NI = (ET * 16 * PIN + 64 * PW - 1) / (64 * PW);
    const int64_t LD = P.hist_ld;
    const float* src = P.obs_history + (size_t)e0 * LD;
    const int total = ne * H;
    float v[NI];
    // unconditional loads at clamped indices: a load under a condition is waited for right after it is
    // issued (one HBM round trip per load instead of one for all)
    if (LD == H) {
#pragma unroll
      for (int i = 0; i < NI; ++i) v[i] = src[min(tid + i * 64 * PW, total - 1)];
    } else {  // rows of a wider buffer (row-strided window)
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int j = min(tid + i * 64 * PW, total - 1), r = j / H;
        v[i] = src[(size_t)r * LD + (j - r * H)];
      }
    }
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int j = tid + i * 64 * PW;
      if (j < total) flat[j] = v[i];
    }
    PSTAMP(9);
  }
  // the critic's privileged inputs into LDS behind the f32 copy (one clamped load per thread; the split
  // passes read them from there)
  float* pflat = flat + ET * 16 * PIN;
  static_assert(ET * 16 * (PIN + 8) * sizeof(float) <= sizeof(SplitLds::h1), "f32 staging exceeds h1");
  if constexpr (PRIV) {
    const int t = min(tid, ET * 16 * NP - 1), e = t / NP;
    const float x = P.privileged_obs[(size_t)(e0 + min(e, ne - 1)) * NP + (t - e * NP)];
    if (tid < ET * 16 * NP) pflat[tid] = x;
    if constexpr (TEACHER) {  // policy_info["latents"] = privileged_info: the rows are one contiguous block
      if (P.latent && tid < ne * NP) P.latent[(size_t)e0 * NP + tid] = x;
    }
  }
  f4_t accA[ET], accL[ET][2];
  {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const f4_t b = *reinterpret_cast<const f4_t*>(LN[0].b + 16 * (wave + i * PW) + 4 * q);
#pragma unroll
      for (int et = 0; et < ET; ++et) accL[et][i] = b;
    }
    if constexpr (ADAPT) {
      const f4_t b = *reinterpret_cast<const f4_t*>(Ls[0].b + 16 * wave + 4 * q);
#pragma unroll
      for (int et = 0; et < ET; ++et) accA[et] = b;
    }
  }
  for (int ch = 0; ch < nch; ++ch) {
    const int g0 = CG * ch, k0 = 32 * g0;
    // inputs of the chunk, in two passes through LDS: coalesced loads of each env's window (all of the
    // thread's in flight) into a flat f32 copy; then each lane splits eight consecutive features of one
    // env into one 16-byte record per plane, the lanes of a wave filling consecutive records
    // (element-wise split stores hit the same LDS banks 8-16 times over)
    // the f32 copy holds the history part of the chunk: rows of fs floats (one chunk: copied above)
    if (nch > 1) {
      // thread -> (env, column phase): TPE threads per env row, one row pointer per thread (per-element
      // addresses would be hoisted out of the chunk loop and spill)
      constexpr int TPE = (64 * PW) / (ET * 16), NI = (PIN + TPE - 1) / TPE;
      const int e = tid / TPE, kk = tid - e * TPE;
      const bool live = e < ET * 16;
      const bool row = live && e < ne;
      const float* src = P.obs_history + (size_t)(e0 + (row ? e : 0)) * P.hist_ld;
      float v[NI];
#pragma unroll
      for (int i = 0; i < NI; ++i) {  // unconditional loads (index clamped), then the mask
        const int kc = kk + TPE * i, k = k0 + kc;
        const float x = src[min(k, H - 1)];
        v[i] = (row && kc < PIN && k < H) ? x : 0.0f;
      }
      if (live) {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
          const int kc = kk + TPE * i;
          if (kc < PIN) flat[e * PIN + kc] = v[i];
        }
      }
    }
    lds_barrier();
    if (ch == 0) PSTAMP(10);
    {
      constexpr int NC = PIN / 8, NTASK = ET * 16 * NC;
      for (int t = tid; t < NTASK; t += 64 * PW) {
        const int c = t & 15, rest = t >> 4, kc = rest % NC, et = rest / NC, e = 16 * et + c;
        h8_t hi8, lo8;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          const int kl = 8 * kc + r, k = k0 + kl;
          float x = 0.0f;
          if (e < ne) {
            if (k < H) x = flat[e * fs + kl];
            else if (PRIV && k < KIN) x = pflat[e * NP + (k - H)];
          }
          ovf_check(x, s_ovf);
          hi8[r] = (_Float16)x;
          lo8[r] = (_Float16)(x - (float)hi8[r]);
        }
        S.xin[et].hi[kc][c] = hi8;
        S.xin[et].lo[kc][c] = lo8;
      }
    }
    lds_barrier();
    if (ch == 0) PSTAMP(1);
    // the chunk's groups (uniform runtime bounds, no predicated MFMAs): [g0, gb) feed the adaptation
    // module (actor) and L1; the next group's fragments are requested before this group's MFMAs
    {
      const int g1 = min(g0 + CG, GL), gb = PRIV ? g1 : min(gl, g1);
      auto group = [&](int gi, const f8_t& a, const f8_t& l0, const f8_t& l1) {
#pragma unroll
        for (int et = 0; et < ET; ++et) {
          const h8_t xh = S.xin[et].hi[4 * gi + q][c], xl = S.xin[et].lo[4 * gi + q][c];
          if constexpr (ADAPT) accA[et] = mfma3(a, xh, xl, accA[et]);
          accL[et][0] = mfma3(l0, xh, xl, accL[et][0]);
          accL[et][1] = mfma3(l1, xh, xl, accL[et][1]);
        }
      };
      if (ch > 0) {  // the first chunk's were requested before the staging
        if (g0 < gb) load0(g0);
        if (g0 + 1 < gb) load1(g0 + 1);
      }
      for (int g = g0; g < gb; g += 2) {
        group(g - g0, wA0, wL00, wL01);
        if (g + 2 < gb) load0(g + 2);
        if (g + 1 < gb) {
          group(g + 1 - g0, wA1, wL10, wL11);
          if (g + 3 < gb) load1(g + 3);
        }
      }
      if constexpr (ADAPT) {  // the history's last, partial group (adaptation module only; the actor's
        if (GA > gl && gl >= g0 && gl < g1) {  // L1 takes it with the latent)
          const f8_t a = reinterpret_cast<const f8_t*>(Ls[0].w)[((size_t)wave * GA + gl) * 64 + lane];
#pragma unroll
          for (int et = 0; et < ET; ++et)
            accA[et] = mfma3(a, S.xin[et].hi[4 * (gl - g0) + q][c], S.xin[et].lo[4 * (gl - g0) + q][c], accA[et]);
        }
      }
    }
    if (ch + 1 < nch) lds_barrier();  // the next chunk's staging overwrites the planes and the copy
  }
  // no barrier: the copy in h1 was last read before the last chunk's MFMAs (every wave has passed that
  // barrier), so each wave stores its first-layer outputs as soon as its own MFMAs are done, overlapping the
  // other waves' MFMAs (a barrier here made every wave run its ELUs at the same time)
  if constexpr (ADAPT) {
    // adaptation module epilogue: ELU, split into h1 rows 0-255
#pragma unroll
    for (int et = 0; et < ET; ++et) {
      f4_t v = accA[et];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = elu(v[r]);
      act_store4(v1[et][0], 4 * wave + q, c, v, s_ovf);
    }
    // K-split partials of the adaptation module: 16 x 16 blocks in rows 384-511 of h1 (block t < 4 in
    // the hi plane, t >= 4 in the lo plane), free until the actor's L1 epilogue
    auto blk = [&](int et, int t) -> float(*)[16] {
      return reinterpret_cast<float(*)[16]>(t < 4 ? &S.h1[et].hi[384 / 8][0] : &S.h1[et].lo[384 / 8][0]) + 16 * (t & 3);
    };
    ActV va2[ET];  // adaptation L2 outputs: rows 256-383 of h1
#pragma unroll
    for (int et = 0; et < ET; ++et) va2[et] = ActV{&S.h1[et].hi[256 / 8][0], &S.h1[et].lo[256 / 8][0]};
    f8_t pa2[4];
    partial_load<4>(Ls[1], 8, wave & 7, 4 * (wave >> 3), lane, pa2);
    lds_barrier();
    PSTAMP(2);
    f8_t pa3[1];
    if (wave < 4) partial_load<1>(Ls[2], 4, 0, wave, lane, pa3);
    {  // 256 -> 128: waves w and w + 8 take the two K halves of tile w & 7
      const int t = wave & 7, half = wave >> 3;
      ActV src[ET];
#pragma unroll
      for (int et = 0; et < ET; ++et) src[et] = v1[et][0];
      f4_t acc[ET];
      tile_partial_e<4, ET>(Ls[1], 8, t, 4 * half, src, lane, acc, pa2);
      if (half) {
#pragma unroll
        for (int et = 0; et < ET; ++et)
#pragma unroll
          for (int r = 0; r < 4; ++r) blk(et, t)[4 * q + r][c] = acc[et][r];
      }
      lds_barrier();
      if (!half) {
        const f4_t b = *reinterpret_cast<const f4_t*>(Ls[1].b + 16 * t + 4 * q);
#pragma unroll
        for (int et = 0; et < ET; ++et) {
          f4_t v;
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = elu((b[r] + acc[et][r]) + blk(et, t)[4 * q + r][c]);
          act_store4(va2[et], 4 * t + q, c, v, s_ovf);
        }
      }
    }
    lds_barrier();
    PSTAMP(3);
    {  // 128 -> num_priv (the latent): one K group per wave (4 waves), partials summed by waves 0 .. ET-1
      if (wave < 4) {
        f4_t acc[ET];
        tile_partial_e<1, ET>(Ls[2], 4, 0, wave, va2, lane, acc, pa3);
#pragma unroll
        for (int et = 0; et < ET; ++et)
#pragma unroll
          for (int r = 0; r < 4; ++r) blk(et, wave)[4 * q + r][c] = acc[et][r];
      }
      lds_barrier();
      if (wave < ET && q < 2) {
        const int et = wave, e = 16 * et + c;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int f = 4 * q + r;
          if (f < NP) {
            float l = Ls[2].b[f];
#pragma unroll
            for (int w = 0; w < 4; ++w) l += blk(et, w)[f][c];
            act_store1(S.xin[et].v(), H + f - 32 * g_last, c, l, s_ovf);  // the last chunk's planes
            if (e < ne && P.latent) P.latent[(size_t)(e0 + e) * NP + f] = l;
          }
        }
      }
    }
    lds_barrier();
    PSTAMP(4);
    // the actor's L1 groups that hold the latent
    for (int g = gl; g < GL; ++g) {
      const int gi = g - g_last;
      f8_t w[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) w[i] = reinterpret_cast<const f8_t*>(LN[0].w)[((size_t)(wave + i * PW) * GL + g) * 64 + lane];
#pragma unroll
      for (int et = 0; et < ET; ++et) {
        const h8_t xh = S.xin[et].hi[4 * gi + q][c], xl = S.xin[et].lo[4 * gi + q][c];
#pragma unroll
        for (int i = 0; i < 2; ++i) accL[et][i] = mfma3(w[i], xh, xl, accL[et][i]);
      }
    }
  } else {
    PSTAMP(2);
    PSTAMP(3);
    PSTAMP(4);
  }
  // actor (Ls 3-6) or critic (Ls 7-10), layer by layer; L1 epilogue: ELU, split into h1
#pragma unroll
  for (int et = 0; et < ET; ++et)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      f4_t v = accL[et][i];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = elu(v[r]);
      act_store4(v1[et][0], 4 * (wave + i * PW) + q, c, v, s_ovf);
    }
  f8_t pl2[SPLIT_D2][1][1];
  policy_prefetch<1, 1, 512 / 32, SPLIT_D2>(LN + 1, wave, PW, lane, pl2);
  lds_barrier();
  PSTAMP(5);
  policy_tiles_e<1, 1, ET, 512 / 32, SPLIT_D2, true>(LN + 1, v1, wave, PW, v2, true, lane, s_ovf, pl2);  // 256
  f8_t pl3[4][1][1];
  if (wave < 8) policy_prefetch<1, 1, 256 / 32, 4>(LN + 2, wave, 8, lane, pl3);
  lds_barrier();
  PSTAMP(6);
  f8_t pl4[1];
  if (wave < 4) partial_load<1>(LN[3], 4, 0, wave, lane, pl4);
  if (wave < 8) policy_tiles_e<1, 1, ET, 256 / 32, 4, true>(LN + 2, v2, wave, 8, v1, true, lane, s_ovf, pl3);  // 128 -> h1
  lds_barrier();
  PSTAMP(7);
  // 128 -> num_actions / 1: one K group per wave, partials through LDS (the inputs' planes, dead now)
  Scr* scr = reinterpret_cast<Scr*>(&S.xin[0]);  // [et], over the dead input planes
  if (wave < 4) {
    ActV src[ET];
#pragma unroll
    for (int et = 0; et < ET; ++et) src[et] = v1[et][0];
    f4_t part[ET];
    tile_partial_e<1, ET>(LN[3], 4, 0, wave, src, lane, part, pl4);
#pragma unroll
    for (int et = 0; et < ET; ++et)
#pragma unroll
      for (int r = 0; r < 4; ++r) scr[et][wave][4 * q + r][c] = part[et][r];
  }
  lds_barrier();
  if (wave < ET) {
    const int et = wave, e = 16 * et + c;
    f4_t acc = *reinterpret_cast<const f4_t*>(LN[3].b + 4 * q);
#pragma unroll
    for (int w = 0; w < 4; ++w)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] += scr[et][w][4 * q + r][c];
    if constexpr (!CRITIC) {
      if (P.actions) {
        float lp = 0.0f;
        f4_t a4, s4;
        float z4[4];
        normal4((uint32_t)(e0 + e + P.env_id_offset), q, P.rng_step, P.rng_seed, z4);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int f = 4 * q + r;
          const bool real = f < P.num_actions;
          const float sd = real ? P.std[f] : 1.0f;
          const float z = z4[r];
          a4[r] = acc[r] + sd * z;
          s4[r] = sd;
          if (real) lp += -0.5f * z * z - __logf(sd) - 0.91893853320467274f;  // log sqrt(2 pi)
        }
        auto x = __builtin_amdgcn_permlane16_swap(__float_as_uint(lp), __float_as_uint(lp), false, false);
        lp = __uint_as_float(x[0]) + __uint_as_float(x[1]);
        auto y = __builtin_amdgcn_permlane32_swap(__float_as_uint(lp), __float_as_uint(lp), false, false);
        lp = __uint_as_float(y[0]) + __uint_as_float(y[1]);
        if (e < ne) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int f = 4 * q + r;
            if (f < P.num_actions) {
              P.actions[(size_t)(e0 + e) * P.num_actions + f] = a4[r];
              P.action_sigma[(size_t)(e0 + e) * P.num_actions + f] = s4[r];
            }
          }
          if (q == 0) P.log_prob[e0 + e] = lp;
        }
      }
      if (e < ne) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int f = 4 * q + r;
          if (f < P.num_actions) P.action_mean[(size_t)(e0 + e) * P.num_actions + f] = acc[r];
        }
      }
    } else if (e < ne && q == 0) {
      P.value[e0 + e] = acc[0];
    }
  }
  PSTAMP(8);
  __syncthreads();
  if (*s_ovf) {
    if constexpr (TEACHER) policy_fallback_actor<true>(P, e0, ne, reinterpret_cast<float*>(&S.h1[0]));
    else policy_fallback(P, e0, ne, !CRITIC, CRITIC, reinterpret_cast<float*>(&S.h1[0]));
  }
}

// envs per workgroup: actor workgroups (adaptation module + actor, 1.6 MB of split weights) take SPLIT_ET_A
// env tiles, critic workgroups (1.2 MB) SPLIT_ET_C, so the two kinds take about as long (4096 envs: actor
// 65.8 k / critic 58.5 k cycles; with 3 + 3 tiles the actor workgroups grew to 84 k: 39 against 32.5 us)
constexpr int SPLIT_ET_A = 2, SPLIT_ET_C = 3;
constexpr int SE_A = 16 * SPLIT_ET_A, SE_C = 16 * SPLIT_ET_C;

// GO1_POLICY_STUDENT is this kernel launched with its actor workgroups only.
__global__ __launch_bounds__(64 * PW) void policy_kernel_split(go1_policy_args P) {
  __shared__ SplitLds S;
  __shared__ int s_ovf;
  PSTAMP(0);
  if (threadIdx.x == 0) s_ovf = 0;
  const int na = (P.n_envs + SE_A - 1) / SE_A;
  if ((int)blockIdx.x < na) {
    const int e0 = blockIdx.x * SE_A;
    split_body<SPLIT_ET_A, false>(P, S, e0, min(SE_A, P.n_envs - e0), &s_ovf);
  } else {
    const int e0 = (blockIdx.x - na) * SE_C;
    split_body<SPLIT_ET_C, true>(P, S, e0, min(SE_C, P.n_envs - e0), &s_ovf);
  }
}

// GO1_POLICY_TEACHER: ceil(n / SE_A) workgroups of the actor on [history, privileged obs] (a kernel of its own:
// policy_kernel_split's code is what it was without the modes)
__global__ __launch_bounds__(64 * PW) void policy_kernel_split_teacher(go1_policy_args P) {
  __shared__ SplitLds S;
  __shared__ int s_ovf;
  PSTAMP(0);
  if (threadIdx.x == 0) s_ovf = 0;
  const int e0 = blockIdx.x * SE_A;
  split_body<SPLIT_ET_A, false, true>(P, S, e0, min(SE_A, P.n_envs - e0), &s_ovf);
}

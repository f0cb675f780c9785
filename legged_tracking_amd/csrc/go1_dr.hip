// go1_dr.hip -- the after-start domain randomiser of include/go1_dr.h: one launch per env step, after the step kernel.
//
// One lane per env, 256-lane workgroups.  A lane loads reset[e] and episode_length[e] and leaves unless its env is
// due; with rand_interval and push_interval in the hundreds that is almost every lane, so almost every wave ends after
// those two loads.  A due lane evaluates one Philox block per kind of work it has (rigid props, push), with the step
// kernels' generator (go1_lanes.h), and writes its few values with plain stores.  u * range + lo is a multiply and an
// add (contraction off, as in the step kernels), and the privileged observation uses their clampf.  The error message
// and the launch check are go1_host.h's, shared with the other add-on libraries.
#include "../../include/go1_dr.h"
#include "go1_device.h"
#include "go1_host.h"

namespace {

constexpr int THREADS = 256;

struct Params {
  go1_dr_config c;
  go1_dr_state s;
  go1_dr_args a;
};

// the four uniforms of block blk of local env e: the injected row, or Philox (counter layout: go1_dr.h)
__device__ __forceinline__ void dr_quad(const go1_dr_config& c, const float* uniforms, uint64_t step, int e, int blk,
                                        float* u) {
  if (uniforms) {
#pragma unroll
    for (int k = 0; k < 4; ++k) u[k] = uniforms[(size_t)e * GO1_DR_U + 4 * blk + k];
    return;
  }
  uint32_t ctr[4] = {(uint32_t)(c.env_id_offset + e), (uint32_t)GO1_DR_TAG + (uint32_t)blk, (uint32_t)step,
                     (uint32_t)(step >> 32)};
  philox4x32(ctr, (uint32_t)c.rng_seed, (uint32_t)(c.rng_seed >> 32));
#pragma unroll
  for (int k = 0; k < 4; ++k) u[k] = (float)(ctr[k] >> 8) * (1.0f / 16777216.0f);
}

// _randomize_rigid_body_props (:710-732) for env e from block 0; dbg: the env's row of dbg_uniforms or nullptr
__device__ __forceinline__ void redraw_rigids(const go1_dr_config& c, const go1_dr_state& s, int e, const float* u,
                                              float* dbg) {
  if (c.randomize_payload) {
    if (s.payloads) s.payloads[e] = u[GO1_DR_U_PAYLOAD] * c.payload_range + c.payload_lo;
    if (dbg) dbg[GO1_DR_U_PAYLOAD] = u[GO1_DR_U_PAYLOAD];
  }
  if (c.randomize_friction) {
    s.friction[e] = u[GO1_DR_U_FRICTION] * c.friction_range + c.friction_lo;
    if (dbg) dbg[GO1_DR_U_FRICTION] = u[GO1_DR_U_FRICTION];
  }
  if (c.randomize_restitution) {
    s.restitution[e] = u[GO1_DR_U_RESTITUTION] * c.restitution_range + c.restitution_lo;
    if (dbg) dbg[GO1_DR_U_RESTITUTION] = u[GO1_DR_U_RESTITUTION];
  }
}

__global__ __launch_bounds__(THREADS) void go1_dr_step_kernel(const Params p) {
  const go1_dr_config& c = p.c;
  const go1_dr_state& s = p.s;
  const go1_dr_args& a = p.a;
  const int e = blockIdx.x * THREADS + threadIdx.x;
  if (e >= c.n_envs) return;
  const bool r = a.reset[e] != 0;
  const int ep = a.episode_length[e];
  const bool rigids = c.rigids_after_start && (r || ep % c.rand_interval == 0);
  const bool push = c.push_robots && !r && ep % c.push_interval == 0;
  if (!rigids && !push) return;

  float* dbg = a.dbg_uniforms ? a.dbg_uniforms + (size_t)e * GO1_DR_U : nullptr;
  if (rigids) {
    float u[4];
    dr_quad(c, a.uniforms, a.rng_step, e, 0, u);
    redraw_rigids(c, s, e, u, dbg);
    if (a.priv && (c.randomize_friction || c.randomize_restitution)) {
      // compute_observations runs after both call sites: the step kernels' expression on the new planes
      float* pv = a.priv + (size_t)e * a.priv_stride;
      pv[0] = clampf((s.friction[e] - c.priv_friction_shift) * c.priv_friction_scale, -c.clip_obs, c.clip_obs);
      pv[1] = clampf((s.restitution[e] - c.priv_rest_shift) * c.priv_rest_scale, -c.clip_obs, c.clip_obs);
    }
  }
  if (push) {  // _push_robots (:1074-1084)
    float u[4];
    dr_quad(c, a.uniforms, a.rng_step, e, 1, u);
    s.root[(size_t)e * 13 + 7] = c.push_range * u[GO1_DR_U_PUSH_X - 4] + c.push_lo;
    s.root[(size_t)e * 13 + 8] = c.push_range * u[GO1_DR_U_PUSH_Y - 4] + c.push_lo;
    if (dbg) {
      dbg[GO1_DR_U_PUSH_X] = u[GO1_DR_U_PUSH_X - 4];
      dbg[GO1_DR_U_PUSH_Y] = u[GO1_DR_U_PUSH_Y - 4];
    }
  }
}

// reset_idx (:233-235) for explicit ids; `uniforms` rows are indexed by env, as in go1_dr_step
__global__ __launch_bounds__(THREADS) void go1_dr_reset_kernel(const go1_dr_config c, const go1_dr_state s,
                                                               const int32_t* ids, int n_ids, uint64_t rng_step,
                                                               const float* uniforms) {
  const int i = blockIdx.x * THREADS + threadIdx.x;
  if (i >= n_ids) return;
  const int e = ids[i];
  if (e < 0 || e >= c.n_envs) return;
  float u[4];
  dr_quad(c, uniforms, rng_step, e, 0, u);
  redraw_rigids(c, s, e, u, nullptr);
}

int check_cfg(const char* fn, const go1_dr_config* c, const go1_dr_state* s) {
  if (c->n_envs < 1) return fail("%s: n_envs must be >= 1", fn);
  if (c->env_id_offset < 0) return fail("%s: env_id_offset must be >= 0", fn);
  if (c->rand_interval < 1) return fail("%s: rand_interval must be >= 1", fn);
  if (c->push_interval < 1) return fail("%s: push_interval must be >= 1", fn);
  if (!(c->payload_range >= 0.0f) || !(c->friction_range >= 0.0f) || !(c->restitution_range >= 0.0f) ||
      !(c->push_range >= 0.0f))
    return fail("%s: every range must be >= 0", fn);
  if (!s->root || !s->friction || !s->restitution) return fail("%s: state: root, friction and restitution must be set", fn);
  return 0;
}

}  // namespace

extern "C" {

int go1_dr_abi_version(void) { return GO1_DR_ABI_VERSION; }

void go1_dr_abi_sizes(int64_t out[4]) {
  out[0] = sizeof(go1_dr_config);
  out[1] = sizeof(go1_dr_state);
  out[2] = sizeof(go1_dr_args);
  out[3] = GO1_DR_U;
}

GO1_LAST_ERROR(go1_dr)

int go1_dr_step(const go1_dr_config* c, const go1_dr_state* s, const go1_dr_args* a, void* stream) {
  const char* fn = "go1_dr_step";
  if (!c || !s || !a) return fail("%s: null cfg, state or args", fn);
  if (check_cfg(fn, c, s)) return -1;
  if (!a->reset || !a->episode_length) return fail("%s: args: reset and episode_length must be set", fn);
  if (a->priv && a->priv_stride < 2) return fail("%s: priv_stride must be >= 2 (friction, restitution)", fn);
  if (!c->rigids_after_start && !c->push_robots) return 0;  // nothing to do: no launch
  Params p;
  p.c = *c;
  p.s = *s;
  p.a = *a;
  const unsigned blocks = ((unsigned)c->n_envs + THREADS - 1) / THREADS;
  hipLaunchKernelGGL(go1_dr_step_kernel, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, p);
  return launched(fn);
}

int go1_dr_reset(const go1_dr_config* c, const go1_dr_state* s, const int32_t* ids, int32_t n_ids, uint64_t rng_step,
                 const float* uniforms, void* stream) {
  const char* fn = "go1_dr_reset";
  if (!c || !s) return fail("%s: null cfg or state", fn);
  if (check_cfg(fn, c, s)) return -1;
  if (n_ids < 0) return fail("%s: n_ids must be >= 0", fn);
  if (n_ids > 0 && !ids) return fail("%s: ids must be set", fn);
  if (n_ids == 0 || !c->rigids_after_start) return 0;
  const unsigned blocks = ((unsigned)n_ids + THREADS - 1) / THREADS;
  hipLaunchKernelGGL(go1_dr_reset_kernel, dim3(blocks), dim3(THREADS), 0, (hipStream_t)stream, *c, *s, ids, (int)n_ids,
                     rng_step, uniforms);
  return launched(fn);
}

}  // extern "C"

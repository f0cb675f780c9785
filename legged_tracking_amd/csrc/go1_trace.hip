// go1_trace.hip -- the episode tracer of include/go1_trace.h: one launch per env step.
//
// A workgroup of 256 lanes owns ENVS = 32 consecutive envs.  The common path is a coalesced copy: the workgroup's
// 32 x 26 output words of ring[push % depth] are contiguous, lane t owns words t, t + 256, ... (at most WORDS = 4),
// each read with one load from the root / dof_pos / wp_index plane (runs of 13, 12 and 1 words): 104 B in and
// 104 B out per env.  All of a lane's loads are issued at the top, together with the one reset byte per env, so the
// kernel waits for memory once; a single barrier tells the workgroup whether any of its envs ended, and the stores
// follow.  Only when one did does the episode path run in between: the env's lane does the bookkeeping and claims
// the capture slot, and the whole workgroup walks the kept rows x 26 words (and the trajectory) of each ended env,
// four loads in flight per lane, so a burst in which every env ends (the first time-out of an evaluation) is
// copied at full width.  The barrier behind the episode path orders its ring reads before the stores that
// overwrite ring[push % depth] for the same envs.  The error message and the launch check are go1_host.h's, shared
// with the other add-on libraries.
#include "../../include/go1_trace.h"
#include "go1_host.h"

namespace {

constexpr int THREADS = 256;
constexpr int ENVS = 32;
constexpr int ROW = GO1_TRACE_ROW;
constexpr int WORDS = (ENVS * ROW + THREADS - 1) / THREADS;  // ring words per lane and push

struct Params {
  go1_trace_args a;
  uint32_t cur;  // push % depth; an ended env's oldest kept row sits at ring slot (cur + depth - kept) % depth
};

__global__ __launch_bounds__(THREADS) void go1_trace_push_kernel(const Params p) {
  const go1_trace_args& a = p.a;
  const int t = threadIdx.x;
  const int e0 = blockIdx.x * ENVS;
  const int n = a.n_envs;
  const int nb = min(ENVS, n - e0);
  const uint32_t depth = (uint32_t)a.depth;
  uint32_t* __restrict__ ring = reinterpret_cast<uint32_t*>(a.ring);

  __shared__ int s_slot[ENVS];   // -2: the env did not end, -1: ended without a capture, >= 0: capture slot
  __shared__ uint32_t s_kept[ENVS];

  // this step's row words: every load is issued before anything waits
  const uint32_t* __restrict__ root = reinterpret_cast<const uint32_t*>(a.root);
  const uint32_t* __restrict__ dof = reinterpret_cast<const uint32_t*>(a.dof_pos);
  const uint32_t* __restrict__ wpi = reinterpret_cast<const uint32_t*>(a.wp_index);
  // (a lane past the workgroup's last word copies that last word once more: the same value to the same address,
  // which keeps the loads and the stores free of branches and of the waits the compiler puts behind them)
  const int last = nb * ROW - 1;
  uint32_t v[WORDS];
#pragma unroll
  for (int k = 0; k < WORDS; ++k) {
    const int w = min(t + k * THREADS, last);
    const int i = w / ROW, c = w - i * ROW;
    const size_t e = (size_t)(e0 + i);
    const uint32_t* src = c < 13 ? root + e * 13 + c : c < 25 ? dof + e * 12 + (c - 13) : wpi ? wpi + e : root;
    const uint32_t x = *src;
    v[k] = (c < 25 || wpi) ? x : 0u;
  }
  int ended = 0;
  if (t < nb) ended = a.reset[e0 + t] != 0;
  if (__syncthreads_or(ended)) {
    if (t < ENVS) {
      int slot = -2;
      uint32_t kept = 0;
      if (ended) {
        const int e = e0 + t;
        const uint64_t len = a.push - a.ep_start[e];
        kept = len < (uint64_t)depth ? (uint32_t)len : depth;
        const int ord = a.ep_ordinal[e];
        const int cause = a.time_out[e] ? GO1_TRACE_TIMEOUT : GO1_TRACE_TERMINATED;
        slot = -1;
        if ((cause & a.want) && (!a.eligible || a.eligible[e])) {
          const uint32_t k = atomicAdd(&a.cap_count[0], 1u);
          if (k < (uint32_t)a.capacity) {
            slot = (int)k;
            int32_t* m = a.cap_meta + (size_t)k * GO1_TRACE_META;
            m[GO1_TM_ENV] = e;
            m[GO1_TM_ORDINAL] = ord;
            m[GO1_TM_END_PUSH] = (int32_t)(uint32_t)a.push;
            m[GO1_TM_KEPT] = (int32_t)kept;
            m[GO1_TM_LENGTH] = len > (uint64_t)INT32_MAX ? INT32_MAX : (int32_t)len;
            m[GO1_TM_CAUSE] = cause;
            m[GO1_TM_SPARE0] = 0;
            m[GO1_TM_SPARE1] = 0;
          } else {
            atomicAdd(&a.cap_count[1], 1u);
          }
        }
        a.ep_ordinal[e] = ord + 1;
        a.ep_start[e] = a.push;
      }
      s_slot[t] = slot;
      s_kept[t] = kept;
    }
    __syncthreads();
    const uint32_t tw = a.wp_trajectory ? 6u * (uint32_t)a.wp_length : 0u;
    const uint32_t* __restrict__ traj = reinterpret_cast<const uint32_t*>(a.wp_trajectory);
    uint32_t* __restrict__ traj_start = reinterpret_cast<uint32_t*>(a.traj_start);
    uint32_t* __restrict__ cap_traj = reinterpret_cast<uint32_t*>(a.cap_traj);
    uint32_t* __restrict__ cap_rows = reinterpret_cast<uint32_t*>(a.cap_rows);
    for (int i = 0; i < nb; ++i) {
      const int slot = s_slot[i];  // uniform over the workgroup
      if (slot == -2) continue;
      const size_t e = (size_t)(e0 + i);
      for (uint32_t w = t; w < tw; w += THREADS) {  // the ended episode's trajectory out, the new one's in
        const uint32_t old = traj_start[e * tw + w];
        if (slot >= 0) cap_traj[(size_t)slot * tw + w] = old;
        traj_start[e * tw + w] = traj[e * tw + w];
      }
      if (slot < 0) continue;
      const uint32_t kept = s_kept[i];
      const uint32_t first = p.cur + depth - kept;  // ring slot of the oldest kept row, before the wrap
      uint32_t* dst = cap_rows + (size_t)slot * depth * ROW;
      const uint32_t total = kept * ROW;
      for (uint32_t w0 = t; w0 < total; w0 += 4 * THREADS) {
        uint32_t x[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint32_t w = w0 + k * THREADS;
          const uint32_t r = w / ROW, c = w - r * ROW;
          uint32_t sr = first + r;
          sr = sr >= depth ? sr - depth : sr;
          x[k] = w < total ? ring[((size_t)sr * n + e) * ROW + c] : 0u;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint32_t w = w0 + k * THREADS;
          if (w < total) dst[w] = x[k];
        }
      }
    }
    __syncthreads();  // the ring reads above come before the write of ring[cur] below
  }

  uint32_t* out = ring + ((size_t)p.cur * n + e0) * ROW;
#pragma unroll
  for (int k = 0; k < WORDS; ++k) out[min(t + k * THREADS, last)] = v[k];
}

}  // namespace

extern "C" {

int go1_trace_abi_version(void) { return GO1_TRACE_ABI_VERSION; }

void go1_trace_abi_sizes(int64_t out[3]) {
  out[0] = sizeof(go1_trace_args);
  out[1] = GO1_TRACE_ROW;
  out[2] = GO1_TRACE_META;
}

GO1_LAST_ERROR(go1_trace)

int go1_trace_push(const go1_trace_args* a, void* stream) {
  if (!a) return fail("go1_trace_push: null args");
  if (!a->root || !a->dof_pos || !a->reset || !a->time_out)
    return fail("go1_trace_push: root, dof_pos, reset and time_out must be set");
  if (!a->ring || !a->ep_start || !a->ep_ordinal || !a->cap_rows || !a->cap_meta || !a->cap_count)
    return fail("go1_trace_push: ring, ep_start, ep_ordinal, cap_rows, cap_meta and cap_count must be set");
  if (a->n_envs < 1 || a->depth < 1 || a->capacity < 1) return fail("go1_trace_push: n_envs, depth and capacity must be >= 1");
  if ((uint64_t)a->depth * (uint64_t)ROW > 0x7fffffffull) return fail("go1_trace_push: depth too large");
  if (a->want & ~(GO1_TRACE_TERMINATED | GO1_TRACE_TIMEOUT)) return fail("go1_trace_push: unknown want bits");
  if (a->wp_trajectory && (a->wp_length < 1 || !a->traj_start || !a->cap_traj))
    return fail("go1_trace_push: wp_trajectory needs wp_length >= 1, traj_start and cap_traj");
  Params p;
  p.a = *a;
  p.cur = (uint32_t)(a->push % (uint64_t)a->depth);
  const unsigned grid = ((unsigned)a->n_envs + ENVS - 1) / ENVS;
  hipLaunchKernelGGL(go1_trace_push_kernel, dim3(grid), dim3(THREADS), 0, (hipStream_t)stream, p);
  return launched("go1_trace_push");
}

}  // extern "C"

/*
 * go1_trace.h -- C ABI of the MI355X episode tracer ("flight recorder"): one small launch after each env step
 * that keeps the last `depth` poses of every env in a device ring and, when an env's episode ends for a wanted
 * cause, copies that episode out of the ring into a capture buffer -- before the host could know of the reset,
 * and without a host synchronisation.  A captured episode's rows are the (T, 13) / (T, 12) pose planes that
 * go1_render (go1_render.h) draws as T "envs" in one launch.
 *
 * Conventions as go1_render.h: caller-owned device buffers, asynchronous on the caller's stream, no allocation,
 * 0 or -1 with go1_trace_last_error(), one host thread per call site.
 *
 * Row (GO1_TRACE_ROW = 26 32-bit words): root[13] | dof_pos[12] | the bits of wp_index (0 when wp_index is NULL).
 * Every copy is a bit copy of 32-bit words: NaN payloads, infinities and -0.0 come through unchanged.
 *
 * go1_trace_push with push = s, for env e, in this order:
 *   1. reset[e] != 0: the episode that began at ep_start[e] has ended.  Its rows are pushes
 *      max(ep_start[e], s - depth) .. s - 1 (kept = min(s - ep_start[e], depth) of them), its full length is
 *      s - ep_start[e], its cause GO1_TRACE_TIMEOUT when time_out[e] != 0, else GO1_TRACE_TERMINATED.
 *      If (cause & want) and (eligible == NULL or eligible[e] != 0), slot = atomic add of 1 on cap_count[0].
 *        slot < capacity: cap_rows[slot, 0 .. kept - 1] = the rows, oldest first; cap_traj[slot] = traj_start[e];
 *                         cap_meta[slot] = {e, ep_ordinal[e], (int32) s, kept, min(full length, INT32_MAX), cause, 0, 0}
 *        else:            cap_count[1] += 1, nothing is copied.
 *      cap_count[0] keeps counting past capacity: the claimed slots are min(cap_count[0], capacity).
 *      Then ep_ordinal[e] += 1, ep_start[e] = s, traj_start[e] = wp_trajectory[e].
 *   2. ring[s % depth, e] = this step's row.
 * Step 1 reads ring slot (s - depth) % depth == s % depth before step 2 overwrites it.  Only env e's own column
 * is involved, and an env belongs to one workgroup, so a workgroup barrier between the two steps is the whole
 * ordering.  The slot order within one push is the order of the atomics; which candidates one overflowing push
 * drops is unspecified, their number (cap_count[1]) is exact.  The caller passes consecutive `push` values and
 * zeroes ep_start, ep_ordinal and cap_count before push 0.
 */
#ifndef GO1_TRACE_H
#define GO1_TRACE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GO1_TRACE_ABI_VERSION 1
#define GO1_TRACE_ROW 26  /* words of a row */
#define GO1_TRACE_META 8  /* int32 words of a capture's meta record */

/* cause bits (go1_trace_args.want, cap_meta[5]) */
#define GO1_TRACE_TERMINATED 1 /* reset && !time_out */
#define GO1_TRACE_TIMEOUT 2    /* reset && time_out */

/* cap_meta words */
enum go1_trace_meta {
  GO1_TM_ENV = 0, GO1_TM_ORDINAL, GO1_TM_END_PUSH, GO1_TM_KEPT, GO1_TM_LENGTH, GO1_TM_CAUSE, GO1_TM_SPARE0, GO1_TM_SPARE1
};

typedef struct go1_trace_args {
  /* this step's inputs */
  const float* root;          /* (n_envs, 13) state plane */
  const float* dof_pos;       /* (n_envs, 12) state plane */
  const int32_t* wp_index;    /* (n_envs) or NULL */
  const float* wp_trajectory; /* (n_envs, 6 wp_length) state plane or NULL */
  const uint8_t* reset;       /* (n_envs) this step's reset output */
  const uint8_t* time_out;    /* (n_envs) this step's time_out output */
  const uint8_t* eligible;    /* (n_envs) or NULL: every env */
  /* tracer-owned state */
  float* ring;                /* (depth, n_envs, 26) words, time-major */
  uint64_t* ep_start;         /* (n_envs) push at which the env's current episode began */
  int32_t* ep_ordinal;        /* (n_envs) episodes the env has ended so far */
  float* traj_start;          /* (n_envs, 6 wp_length) the current episode's trajectory; NULL with wp_trajectory */
  /* capture outputs */
  float* cap_rows;            /* (capacity, depth, 26) words */
  float* cap_traj;            /* (capacity, 6 wp_length); NULL with wp_trajectory */
  int32_t* cap_meta;          /* (capacity, 8) */
  uint32_t* cap_count;        /* (2) slots claimed (counts past capacity), candidates dropped */
  int32_t n_envs, depth, capacity, wp_length;
  int32_t want;               /* GO1_TRACE_* bits */
  int32_t pad;
  uint64_t push;              /* consecutive per call, from 0 */
} go1_trace_args;

int go1_trace_abi_version(void);
/* sizeof go1_trace_args, GO1_TRACE_ROW, GO1_TRACE_META */
void go1_trace_abi_sizes(int64_t out[3]);
const char* go1_trace_last_error(void);
int go1_trace_push(const go1_trace_args* args, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GO1_TRACE_H */

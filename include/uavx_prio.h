/* uavx_prio.h — C ABI of libuavx_prio.so: proportional prioritized experience replay (Schaul et al.) on the zero-copy ring
 * of DeviceReplay (replay.py), for MI355X (gfx950).  A per-transition priority table, a hierarchy of partial sums over it,
 * a sampler that draws a transition with probability p / total and gathers its row, and the feedback of TD errors into
 * the table.
 *
 * Priorities are INTEGERS: uint32 in Q16.16 (65 536 stands for 1.0; 0 means "cannot be drawn"), and every sum over them is
 * a uint64.  Sums are exact and do not depend on their order, so the drawn entry is a pure function of the table and the
 * uniforms: a flat cumulative sum over the table restates the search bit for bit, whatever hierarchy the kernels use.
 * The table holds at most UAVX_PRIO_MAX_ENTRIES = 2^26 entries, so that total < 2^58.
 *
 * The ring is uavx_replay.h's uavx_replay_ring (the same fields; flags packed into done, or the three flag arrays).
 * State owned by the caller, all of it device memory:
 *   table [slots][envs][learners] uint32; flat index f = (slot·envs + e)·learners + i
 *   sums  uavx_prio_state_bytes(entries) bytes, 16-byte aligned: the partial sums, fan-out 64.  Level 1 holds the sums of 64
 *         consecutive entries, level 2 of 64 level-1 nodes (4 096 entries), levels 3 and 4 likewise (at the limit 2^20,
 *         2^14, 256 and 4 nodes), then per level-2 node its smallest positive entry and its number of positive entries.
 *   rec   uavx_prio_record: total; p_min, the smallest positive entry (0 without one); p_max, the running maximum (the
 *         caller starts it at UAVX_PRIO_ONE); seen, the steps that have been given a priority; valid, the entries > 0.
 *
 * With c = max(1, count), T = slots − 1, lo = max(0, c − T): slot s belongs to step k if k = lo + ((s − lo) mod slots) < c.
 *
 * uavx_prio_refresh, every entry (s, e, i):
 *   s belongs to no step of the window (the head slot c % slots is such a slot)     -> 0
 *   skip(s, e) is set (a re-initialisation row, or one DeviceReplay.reset took out) -> 0
 *   k >= max(seen, lo): a step written since the last refresh                        -> p_max
 *   otherwise                                                                        unchanged
 * then every partial sum, total, p_min and valid are rebuilt from the table, and seen = c.  Two launches, no atomics.
 *
 * uavx_prio_sample, row j of u [rows] f32:
 *   t = stratified ? ((double)j + (double)u_j) / (double)rows : (double)u_j; a t that is NaN or negative counts as 0
 *   target = min(total − 1, (uint64)floor(t · (double)total)); a t at or past 1, +inf included, gives total − 1
 *   f = the smallest flat index whose inclusive cumulative sum exceeds target; (s, e, i) from f, k the step of slot s
 *   state = obs[s, e, i], action = act[..], reward = rew[..], next_state = obs[(s + 1) % slots, e, i],
 *   mask = 1 − (float)(done[s, e, i] & 1), truncated / ended = the flags at (s, e) as 0 / 1 bytes,
 *   key = k·(envs·learners) + e·learners + i,
 *   weight = (float)pow((double)p_min / (double)table[f], (double)beta): (N·P_f)^−beta over its maximum; 0 if table[f] is 0
 *   total == 0: key = −1, weight = 0, and the gathers read (slot (c − 1) % slots, env 0, agent 0).
 *   One launch, 16 lanes per row: at most five steps of 64 children each.  Every index is clamped into its level, so
 *   no bit pattern of u, and no table that disagrees with its sums, leads to a read outside the ring or the state.
 *
 * uavx_prio_update, row j of key [rows] int64, q [towers][rows] f32, y [rows] f32 with a stride (NULL: q is |delta| itself,
 * towers = 1):
 *   delta = max_t |q_t − y| in float32 (a NaN in any tower makes delta NaN)
 *   p = 1 if delta is NaN and 2^32 − 1 if it is +inf, for every alpha, alpha = 0 included; otherwise
 *   p = min(2^32 − 1, max(1, floor(pow((double)delta + eps, alpha)·65536 + 0.5))), where
 *       alpha == 1 takes (double)delta + eps itself and alpha == 0 takes 1 in place of the pow
 *   a row is ignored if key < 0, or if its step k = key / (envs·learners) is < lo or >= c when the kernel runs
 *   an entry addressed several times ends at the MAXIMUM of its rows' p whatever the execution order: a first launch stores
 *   0 to every addressed entry, a second applies an unsigned atomic max; p_max is raised the same way.
 *   The sums are not touched: the next refresh rebuilds them.  The order of calls is refresh, sample, ..., update.
 *
 * Conventions (as uavx_replay.h; the status codes are uavx_actor.h's values)
 *   - every pointer but `ring` is a DEVICE pointer on the current device; outputs are contiguous.
 *   - work is enqueued on `stream` (hipStream_t as void*, NULL = the null stream); nothing synchronises and nothing is
 *     allocated: every call can be captured into a graph.  count_dev (device int64, 8-byte aligned) replaces count when
 *     set; beta_dev (device float) replaces beta when set.
 *   - every argument is checked before any GPU call and a refused call enqueues nothing; rows = 0 enqueues nothing.
 *   - index arithmetic is 64-bit; no workgroup waits on another.
 */
#ifndef UAVX_PRIO_H
#define UAVX_PRIO_H
#include <stdint.h>
#include "uavx_replay.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UAVX_PRIO_VERSION 1
#define UAVX_PRIO_ONE 65536
#define UAVX_PRIO_MAX_ENTRIES 67108864
#define UAVX_PRIO_MAX_ROWS 1048576
#define UAVX_PRIO_MAX_TOWERS 2

typedef struct uavx_prio_record {
    uint64_t total;
    uint32_t p_min;
    uint32_t p_max;
    int64_t seen;
    uint64_t valid;
} uavx_prio_record;

typedef struct uavx_prio_state {
    const uavx_replay_ring *ring;
    int64_t count;            /* steps written so far (>= 1), read when count_dev is NULL */
    const int64_t *count_dev; /* device int64, read by the kernels in its place (a value < 1 is taken as 1) */
    uint32_t *table;          /* [slots][envs][learners], 4-byte aligned */
    void *sums;               /* uavx_prio_state_bytes(slots·envs·learners) bytes, 16-byte aligned */
    int64_t sums_bytes;
    uavx_prio_record *rec;    /* 8-byte aligned */
} uavx_prio_state;

typedef struct uavx_prio_sample_args {
    const float *u;           /* [rows] */
    int64_t rows;             /* 0..UAVX_PRIO_MAX_ROWS */
    int32_t stratified;       /* 0 or 1 */
    float beta;               /* [0, 1], read when beta_dev is NULL */
    const float *beta_dev;
    float *state;             /* [rows, 10], 8-byte aligned */
    float *action;            /* [rows, 2], 8-byte aligned */
    float *reward;            /* [rows] */
    float *next_state;        /* [rows, 10], 8-byte aligned */
    float *mask;              /* [rows] */
    uint8_t *truncated;       /* [rows], both NULL or both set */
    uint8_t *ended;
    int64_t *key;             /* [rows], 8-byte aligned */
    float *weight;            /* [rows] */
} uavx_prio_sample_args;

int uavx_prio_version(void);

/* bytes of the partial sums over `entries` entries (1..UAVX_PRIO_MAX_ENTRIES), a multiple of 16. */
int uavx_prio_state_bytes(int64_t entries, int64_t *bytes);

int uavx_prio_refresh(const uavx_prio_state *state, void *stream);

int uavx_prio_sample(const uavx_prio_state *state, const uavx_prio_sample_args *args, void *stream);

/* key [rows] int64; q [towers][rows] f32; y: f32 with a stride of y_stride elements, or NULL (then towers must be 1 and q is
 * |delta|); alpha in [0, 1]; eps > 0. */
int uavx_prio_update(const uavx_prio_state *state, const int64_t *key, const float *q, int32_t towers, const float *y,
                     int64_t y_stride, int64_t rows, double alpha, double eps, void *stream);

#ifdef __cplusplus
}
#endif
#endif

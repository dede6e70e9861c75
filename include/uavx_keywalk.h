/* uavx_keywalk.h — C ABI of libuavx_keywalk.so: the n-step walk of uavx_nstep.h started from KEYS, on the zero-copy ring
 * of DeviceReplay (replay.py; uavx_replay.h describes it) for MI355X (gfx950).  A prioritized sample (uavx_prio.h) returns,
 * per row, the key of the transition it drew and that transition's one-step reward, next_state and mask; this call reads
 * each row's key and OVERWRITES reward, next_state and mask (and the flags) with the n-step values of the walk that starts
 * at that transition.  Prioritized n-step replay is therefore uavx_prio_refresh + uavx_prio_sample, unchanged, and then this
 * ONE launch.
 *
 * With c = max(1, count), T = slots − 1, lo = max(0, c − T) as in uavx_replay.h, and per = envs·learners:
 *   1. key.  A key q >= 0 names step k = q / per, env e = (q mod per) / learners, agent i = q mod learners: what
 *      uavx_prio_sample wrote, k·per + e·learners + i.  e and i are in range by construction.
 *   2. a row is IGNORED when q < 0, k < lo or k >= c: the rule uavx_prio_update has for stale keys.  For an ignored row
 *      nothing is loaded from the ring and nothing is written but length = 0 (when length is given): reward, next_state,
 *      mask and the flags keep what they held.  A prioritized sample with total == 0 (every key −1) so keeps the one-step
 *      kernel's outputs.  k is compared with the window BEFORE any address is formed: no bit pattern of a key leads to an
 *      access outside the ring.
 *   3. walk, from the start row (k, e, i), exactly step 3 of uavx_nstep.h.  R = −0 and g = 1 in float64 (−0 + x is x for
 *      every x: one step returns its reward bit for bit, a reward of −0 included).  For j = 0, 1, … at step k + j,
 *      slot (k + j) % slots:
 *        R += g·(double)rew[slot, e, i]                       (one float64 multiply, one float64 add)
 *      and the walk ENDS after this step when any of
 *        j == n_step − 1;   done[slot, e, i] & 1;   ended(slot, e);   k + j + 1 >= c  (the ring's head);
 *        skip((k + j + 1) % slots, e)  (the next row is a re-initialisation row, or one DeviceReplay.reset took out);
 *      otherwise g *= gamma (float64) and the walk goes on.  len = j + 1, and g = gamma^(len − 1) as that chain of products.
 *      The START row's own skip flag is not looked at: a prioritized draw never returns such a row (its priority is 0), and
 *      a hand-made key is walked like any other.
 *   4. reward = (float)R, next_state = obs[(k + len) % slots, e, i], mask = (float)((1 − (done_last & 1))·g),
 *      truncated / ended = the flags at the LAST row walked, as 0 / 1 bytes, length = len.
 *
 * n_step = 1 writes −0 + 1·(double)r and (1 − d)·1, which round back to r and to 1 − (float)d: the bits uavx_prio_sample
 * wrote.  Through the unchanged TD target y = r + (mask·γ)·(…) with γ = gamma: y = R + gamma^len·(1 − done_last)·(…).
 *
 * Conventions: those of uavx_prio.h (device pointers but `args` and `ring`, outputs contiguous, next_state 8-byte aligned
 * like ring->obs, key 8-byte aligned, the floats 4-byte aligned; enqueued on `stream`, nothing allocated, nothing
 * synchronised, capturable; count_dev, a device int64, replaces count when set and a value < 1 is taken as 1).  Every
 * argument is checked before any GPU call and a refused call enqueues nothing; rows = 0 enqueues nothing and looks at no
 * buffer, but the ring, the count, n_step and gamma are checked all the same.  A ring is refused when envs·learners
 * exceeds 2^31 − 1 or when its observation array would pass 2^63 bytes: every index the kernel forms fits its type.
 * No atomics, no reductions, no LDS, no workgroup waits on another: the same inputs give the same bits.  The status codes
 * are uavx_actor.h's.
 */
#ifndef UAVX_KEYWALK_H
#define UAVX_KEYWALK_H
#include <stdint.h>
#include "uavx_replay.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UAVX_KEYWALK_VERSION 1
#define UAVX_KEYWALK_MAX_STEP 8
#define UAVX_KEYWALK_MAX_ROWS 1048576

typedef struct uavx_keywalk_args {
    const uavx_replay_ring *ring;   /* as uavx_prio_state.ring: packed flags (skip, trunc, ended all NULL) or all three arrays */
    int64_t count;                  /* steps written so far (>= 1), read when count_dev is NULL */
    const int64_t *count_dev;       /* device int64, 8-byte aligned, read by the kernel in its place (< 1 is taken as 1) */
    const int64_t *key;             /* [rows], 8-byte aligned: as uavx_prio_sample wrote them */
    int64_t rows;                   /* 0..UAVX_KEYWALK_MAX_ROWS */
    int32_t n_step;                 /* 1..UAVX_KEYWALK_MAX_STEP */
    double gamma;                   /* finite, in [0, 1] */
    float *reward;                  /* [rows] */
    float *next_state;              /* [rows, 10], 8-byte aligned */
    float *mask;                    /* [rows] */
    uint8_t *length;                /* [rows] steps summed, 1..n_step, 0 for an ignored row; may be NULL */
    uint8_t *truncated;             /* [rows] flags of the LAST row walked; both NULL or both set */
    uint8_t *ended;
} uavx_keywalk_args;

int uavx_keywalk_version(void);

int uavx_keywalk(const uavx_keywalk_args *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif

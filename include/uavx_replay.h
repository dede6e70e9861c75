/* uavx_replay.h — C ABI of the replay sampler in libuavx_actor.so: DeviceReplay.sample (replay.py) from the zero-copy ring
 * to the learner's batch on MI355X (gfx950), in ONE kernel launch up to UAVX_REPLAY_SINGLE_ROWS rows and TWO above.
 *
 * The ring (time-major, slot k % slots holds what step k produced; replay.py):
 *   obs [slots, envs, agents, 10] f32, act [slots, envs, agents, 2] f32, rew [slots, envs, agents] f32,
 *   done [slots, envs, agents] u8, and skip / trunc / ended [slots, envs] u8 -- or, all three NULL, those flags in bits
 *   1 / 3 / 2 of done[slot, env, 0] (UAVX_FLAGS_IN_DONE).  T = slots − 1 steps are kept; agents [0, learners) are sampled.
 *
 * With c = max(1, count), lo = max(0, c − T), span = c − lo, and u [2][3][rows] f32 (first draw, redraw):
 *   1. per draw d and row j:  k = lo + min(trunc(u[d][0][j]·(float)span), span − 1),
 *                             e = min(trunc(u[d][1][j]·(float)envs), envs − 1),
 *                             i = min(trunc(u[d][2][j]·(float)learners), learners − 1)
 *      one float32 multiply, truncated toward zero.  A product that is negative or NaN gives 0, one at or past the range
 *      (+inf too) gives its top: whatever bits u holds, every index stays inside the ring.
 *   2. row j takes draw 1 if skip(k0 % slots, e0) is set, draw 0 otherwise; valid_j = !skip(k % slots, e) of that draw.
 *   3. src_j = the largest valid p <= j; without one the smallest valid p > j; without one rows − 1.  Row j uses the
 *      (k, e, i) of row src_j.
 *   4. state = obs[k % slots, e, i], action = act[..], reward = rew[..], next_state = obs[(k + 1) % slots, e, i],
 *      mask = 1 − (float)(done[k % slots, e, i] & 1), truncated / ended = the flags at (k % slots, e), as 0 / 1 bytes.
 *
 * Conventions (as uavx_optim.h; the status codes are uavx_actor.h's)
 *   - every pointer but `ring` is a DEVICE pointer on the current device; outputs are contiguous ([rows, 10], [rows, 2],
 *     [rows]), state, action and next_state 8-byte aligned like ring->obs and ring->act, the other floats 4-byte aligned.
 *   - work is enqueued on `stream` (hipStream_t as void*, NULL = the null stream); nothing synchronises and nothing is
 *     allocated: the call can be captured into a graph.  With count_dev the window (lo, span, slot rotation) is derived
 *     in the kernel from *count_dev, so a replay samples what the ring holds at that time.
 *   - arguments are checked before any GPU call and a rejected call enqueues nothing; rows = 0 enqueues nothing either
 *     (u, the outputs and the workspace are then not looked at).
 *   - no atomics, no reductions, no workgroup waits on another: the same inputs give bitwise-identical outputs, and
 *     only the boundary between the two launches orders the two phases of a large batch.
 */
#ifndef UAVX_REPLAY_H
#define UAVX_REPLAY_H
#include <stdint.h>
#include "uavx_actor.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UAVX_REPLAY_VERSION 1
#define UAVX_REPLAY_MAX_ROWS 1048576
#define UAVX_REPLAY_SINGLE_ROWS 1024

typedef struct uavx_replay_ring {
    const float *obs;
    const float *act;
    const float *rew;
    const uint8_t *done;
    const uint8_t *skip;      /* skip, trunc, ended: all NULL = packed into done (bits 1, 3, 2 of agent 0's byte) */
    const uint8_t *trunc;
    const uint8_t *ended;
    int64_t slots;            /* T + 1, 2..2^31 − 1 */
    int64_t envs;             /* 1..2^31 − 1 */
    int64_t agents;           /* 1..2^31 − 1 */
    int64_t learners;         /* 1..agents */
} uavx_replay_ring;

int uavx_replay_version(void);

/* bytes of workspace a call with `rows` rows needs: 0 up to UAVX_REPLAY_SINGLE_ROWS. */
int uavx_replay_workspace_bytes(int64_t rows, int64_t *bytes);

/* count: steps written so far (>= 1), read when count_dev is NULL.  count_dev: device int64, 8-byte aligned, read by the
 *   kernel in its place (a value < 1 is taken as 1).
 * u: [2][3][rows] f32.  rows: 0..UAVX_REPLAY_MAX_ROWS.
 * truncated, ended: [rows] u8, both NULL or both set.
 * workspace: device memory of at least uavx_replay_workspace_bytes(rows), 16-byte aligned; may be NULL when that is 0. */
int uavx_replay_sample(const uavx_replay_ring *ring, int64_t count, const int64_t *count_dev, const float *u, int64_t rows,
                       float *state, float *action, float *reward, float *next_state, float *mask, uint8_t *truncated,
                       uint8_t *ended, void *workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif

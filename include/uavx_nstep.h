/* uavx_nstep.h — C ABI of the n-step replay sampler in libuavx_actor.so: a draw from the zero-copy ring of replay.py
 * (uavx_replay.h describes it) turned into one row of an n-step batch on MI355X (gfx950) — the discounted return of up to
 * n_step steps, the observation that many steps on and the discount the bootstrap still carries — with the start row drawn
 * uniformly or, per row, with a weight that grows linearly with recency.  ONE kernel launch up to UAVX_NSTEP_SINGLE_ROWS
 * rows and TWO above, like uavx_replay_sample, whose draw, redraw and fallback rules it keeps: the same kernels serve
 * both, and uavx_replay_sample is this call with n_step = 1, gamma = 1, recency = 0, u_cols = 3 and no length.
 *
 * With c = max(1, count), T = slots − 1, lo = max(0, c − T), span = c − lo as in uavx_replay.h, idx(u, n) its
 * min(trunc(u·(float)n), n − 1) with the same out-of-range rule (a product that is negative or NaN gives 0, one at or past
 * the range, +inf too, gives n − 1), and u [2][u_cols][rows] f32 (first draw, redraw):
 *   1. draw.  Per draw d and row j:  ka = idx(u[d][0][j], span),  e = idx(u[d][1][j], envs),  i = idx(u[d][2][j], learners).
 *      u_cols == 5:  kb = idx(u[d][3][j], span);  the row is RECENT when u[d][4][j] < recency (a NaN compares false);
 *                    k = lo + (recent ? max(ka, kb) : ka).
 *      u_cols == 3:  k = lo + ka.
 *      max(ka, kb) of two uniform indices has P(k − lo < m) = (m/span)², the cumulative sum of weights proportional to
 *      m + ½: the "unbalanced" draw of the reference's older DDPG buffer (weight 0.25 + 0.5·m on the m-th oldest entry)
 *      per step index, without a table, a sort or a square root.
 *   2. redraw and fallback: steps 2 and 3 of uavx_replay.h, unchanged, on the START row (k, e, i): row j takes draw 1 if
 *      skip(k0 % slots, e0) is set, draw 0 otherwise; valid_j = !skip(k % slots, e) of that draw; src_j = the largest valid
 *      p <= j, without one the smallest valid p > j, without one rows − 1; row j uses the (k, e, i) of row src_j.
 *   3. walk.  R = −0 and g = 1 in float64 (−0 + x is x for every x: one step returns its reward bit for bit, a reward
 *      of −0 included).  For j = 0, 1, … at step k + j, slot (k + j) % slots:
 *        R += g·(double)rew[slot, e, i]                       (one float64 multiply, one float64 add)
 *      and the walk ENDS after this step when any of
 *        j == n_step − 1;   done[slot, e, i] & 1;   ended(slot, e);   k + j + 1 >= c  (the ring's head);
 *        skip((k + j + 1) % slots, e)  (the next row is a re-initialisation row, or one DeviceReplay.reset took out);
 *      otherwise g *= gamma (float64) and the walk goes on.  len = j + 1, and g = gamma^(len − 1) as that chain of products.
 *   4. state = obs[k % slots, e, i], action = act[..] of the start row, reward = (float)R,
 *      next_state = obs[(k + len) % slots, e, i], mask = (float)((1 − (done_last & 1))·g), length = len,
 *      truncated / ended = the flags at the LAST row walked, as 0 / 1 bytes.
 *
 * Hence, through the unchanged TD target y = r + (mask·γ)·(…) of uavx_critic_target with γ = gamma:
 * y = R + gamma^len·(1 − done_last)·(…).
 *   - n_step = 1, recency = 0, u_cols = 3 is uavx_replay_sample, bit for bit.
 *   - an agent parked with done = 1 yields len = 1 and mask = 0.
 *   - an episode cut by the step cap in the middle of the walk ends the walk there (ended) with mask > 0: the target
 *     bootstraps from the terminal observation that the next step's auto-reset leaves in slot k + len.
 *
 * Differences from the reference's buffer.py get_batch(unbalance = 0.8), on purpose: its coin is flipped once per batch,
 * here once per row (the same per-row marginal); draws are with replacement, as DeviceReplay.sample's are; the weight is
 * per STEP index, so all envs·learners transitions of one step weigh the same.
 *
 * Conventions: those of uavx_replay.h (device pointers but `args` and `ring`, outputs contiguous, state / action /
 * next_state 8-byte aligned, enqueued on `stream`, nothing allocated, nothing synchronised, capturable; with count_dev the
 * window is derived in the kernel).  Every argument is checked before any GPU call and a refused call enqueues nothing;
 * rows = 0 enqueues nothing and looks at no buffer.  No atomics, no reductions, no workgroup waits on another: the same
 * inputs give the same bits.  The status codes are uavx_actor.h's.
 */
#ifndef UAVX_NSTEP_H
#define UAVX_NSTEP_H
#include <stdint.h>
#include "uavx_actor.h"
#include "uavx_replay.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UAVX_NSTEP_VERSION 1
#define UAVX_NSTEP_MAX 8
#define UAVX_NSTEP_MAX_ROWS 1048576
#define UAVX_NSTEP_SINGLE_ROWS 1024

int uavx_nstep_version(void);

/* bytes of workspace a call with `rows` rows needs: 0 up to UAVX_NSTEP_SINGLE_ROWS. */
int uavx_nstep_workspace_bytes(int64_t rows, int64_t *bytes);

typedef struct uavx_nstep_args {
    const uavx_replay_ring *ring;   /* as uavx_replay_sample takes it, packed flags or arrays */
    int64_t count;                  /* steps written so far (>= 1), read when count_dev is NULL */
    const int64_t *count_dev;       /* device int64, 8-byte aligned, read by the kernel in its place (< 1 is taken as 1) */
    const float *u;                 /* [2][u_cols][rows] f32 */
    int32_t u_cols;                 /* 3 (recency == 0 only) or 5 */
    int32_t n_step;                 /* 1..UAVX_NSTEP_MAX */
    double gamma;                   /* (0, 1] */
    float recency;                  /* [0, 1]: the probability that a row is drawn recency-weighted */
    int64_t rows;                   /* 0..UAVX_NSTEP_MAX_ROWS */
    float *state;                   /* [rows, 10] */
    float *action;                  /* [rows, 2] */
    float *reward;                  /* [rows] */
    float *next_state;              /* [rows, 10] */
    float *mask;                    /* [rows] */
    uint8_t *length;                /* [rows] steps summed, 1..n_step; may be NULL */
    uint8_t *truncated;             /* [rows] flags of the LAST row walked; both NULL or both set */
    uint8_t *ended;
    void *workspace;                /* at least uavx_nstep_workspace_bytes(rows), 16-byte aligned; may be NULL when 0 */
    int64_t workspace_bytes;
} uavx_nstep_args;

int uavx_nstep_sample(const uavx_nstep_args *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif

/* uavx_norm.h — C ABI of libuavx_norm.so: running statistics of the observations and of the discounted returns over the
 * device ring of a DeviceReplay, and the two element-wise calls that apply them, on MI355X (gfx950).  DESIGN.md §30;
 * tests/norm_ref.py restates the definition below in numpy.
 *
 * Ring (uavx_norm_ring; the layout of replay.DeviceReplay, time-major, the fields of uavx_gae_ring)
 *   L = slots = T + 1 slots.  rew [L,E,N] float32 and done [L,E,N] uint8, bit 0 of a done byte = this agent is done.
 *   skip [L,E] and ended [L,E] uint8 (non-zero = set): "the env was re-initialised instead of stepped, the row is not a
 *   transition" and "the env's episode ended AT this transition".  Both NULL: the packed ring, skip(s,e) is bit 1 and
 *   ended(s,e) bit 2 of done[s,e,0].  obs [L,E,N,F] float32 is an argument of its own: obs[k mod L] is the observation step k
 *   started from.  Step k lives in slot k mod L.
 *
 * Samples
 *   A row (k, e, i) is a SAMPLE iff  i < learners  ∧  ¬skip(k,e)  ∧  ¬parked(k,e,i),  where
 *     parked(k,e,i) = k >= 1 ∧ (done[k−1,e,i] & 1) ∧ ¬skip(k−1,e) ∧ ¬ended(k−1,e):
 *   the agent was done before the step, in an env that went on.  (The done bit of row k−1 counts whether or not that row
 *   was itself parked.)  A fold covers the steps k = first, ..., count − 1 with 0 <= first and 1 <= count − first <= T, so
 *   that the row first − 1 that parked looks back at is still in the ring.
 *
 * Record (uavx_norm_record; DEVICE memory, 8-byte aligned, persists between calls, all zero at the start)
 *   n_obs, mean[f], M2[f] for the F observation features (1 <= F <= UAVX_NORM_MAX_FEATURES; entries f >= F are not
 *   touched); n_ret, mean_ret, M2_ret for the returns.  The variance is M2 / (double)n, the population variance; with n = 0
 *   the mean reads as 0 and the variance as 1.
 *
 * Batch statistics (both folds; float64, two passes, in an order the launch geometry alone fixes -- no atomics, no workgroup
 * waits on another)
 *   column sum      column q = e·N + i belongs to thread q mod 256 of workgroup q / 256 (UAVX_NORM_BLOCK columns per
 *                   workgroup; threads past the last column and of columns i >= learners hold +0).  A thread starts from +0
 *                   and adds the samples of its column in the order of the walk, k UPWARDS from first.
 *   workgroup sum   over each wavefront of 64 lanes a halving tree: x[l] += x[l+32], then +16, +8, +4, +2, +1 (lane 0
 *                   holds the sum); then the four wavefront sums w0 + w1 + w2 + w3, left to right -> partial[workgroup].
 *   total           ONE workgroup's worth of threads: thread t starts from +0 and adds partial[t], partial[t + 256], ...
 *                   in index order, then the same workgroup sum.
 *   n_b is the number of samples (summed in int64), S the total of the samples x, mean_b = S / (double)n_b.  The second pass
 *   sums (x − mean_b)·(x − mean_b) -- subtraction, product and addition are three roundings -- in exactly the same order:
 *   M2_b.  With fold_obs each feature f is summed on its own, F accumulators per thread, all with the one n_b.
 *
 * Merge (Chan's update; a = the record, b = the batch; every line is the roundings it shows, in this order)
 *   n_b = 0: the record's bits are left alone.  Otherwise
 *     n    = n_a + n_b                          (int64)
 *     δ    = mean_b − mean_a
 *     w    = (double)n_b / (double)n
 *     mean = mean_a + δ·w                       (product, then sum)
 *     M2   = (M2_a + M2_b) + (δ·δ)·((double)n_a·w)   (t1 = M2_a + M2_b; t2 = δ·δ; t3 = (double)n_a·w; t4 = t2·t3; t1 + t4)
 *
 * uavx_norm_fold_obs       the samples of feature f are (double)obs[k mod L, e, i, f] over the sample rows of the fold.
 *
 * uavx_norm_fold_returns   a FORWARD walk per column (e, i < learners) with a float64 carry C[e,i] in the caller's device
 *   array carry [E,N], +0 at the start of a run and updated by the call (entries i >= learners are neither read nor
 *   written).  For k = first upwards:
 *     skip(k,e) or parked(k,e,i):   C = +0, no sample.
 *     otherwise:                    R = (double)rew[k mod L,e,i] + γ·C  (product, then sum);  R is a sample;
 *                                   C = ((done[k mod L,e,i] & 1) ∨ ended(k,e)) ? +0 : R   (a select: a NaN does not pass an
 *                                   episode end).
 *   The second pass walks again from the carry the call found and forms R anew; R is never stored.
 *
 * uavx_norm_apply_obs      element-wise over rows × F, any rows >= 0:  with mean_f = n_obs > 0 ? mean[f] : 0 and
 *   var_f = n_obs > 0 ? M2[f] / (double)n_obs : 1,
 *     z = ((double)x − mean_f) / sqrt(var_f + eps)   (difference, sum, square root, quotient: four roundings)
 *     y = (float)z;  out = y > c ? c : (y < −c ? −c : y)  with c = (float)clip: comparisons, so a NaN stays a NaN.
 * uavx_norm_scale_rewards  element-wise over count >= 0 elements: var = n_ret > 0 ? M2_ret / (double)n_ret : 1,
 *     y = (float)((double)r / sqrt(var + eps)), clamped as above.  The mean is not subtracted.
 *   Both read the record from device memory when the kernel runs: a captured graph follows the statistics.  out may be in
 *   exactly, or may not overlap it at all.
 *
 * Launches: a fold is THREE (first pass, second pass, one workgroup that totals and merges), an apply call ONE.
 *
 * Conventions (uavx_gae.h's; the status codes are uavx_actor.h's)
 *   - every pointer but the ring struct itself is DEVICE memory on the current device; float32 arrays are 4-byte aligned,
 *     record, carry and workspace 8-byte aligned.
 *   - work is enqueued on `stream` (hipStream_t as void*, NULL = the null stream); nothing synchronises, nothing is allocated.
 *   - every argument is checked before the first launch: a rejected call enqueues nothing.
 *   - first, count, γ, eps and clip are read when the call is made.  The payload and sign of a NaN are not part of the
 *     contract; where a NaN is, is.
 */
#ifndef UAVX_NORM_H
#define UAVX_NORM_H
#include <stdint.h>
#include "uavx_actor.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UAVX_NORM_VERSION 1
#define UAVX_NORM_BLOCK 256
#define UAVX_NORM_MAX_FEATURES 16

typedef struct uavx_norm_ring {
    const float *rew;         /* fold_obs does not look at it */
    const uint8_t *done;
    const uint8_t *skip;      /* skip and ended: both NULL = packed into done (bits 1 and 2 of agent 0's byte) */
    const uint8_t *ended;
    int64_t slots;            /* T + 1, 2..2^31 − 1 */
    int64_t envs;             /* >= 1 */
    int64_t agents;           /* >= 1; envs · agents <= 2^31 − 1 */
    int64_t learners;         /* 1..agents */
} uavx_norm_ring;

/* the running statistics; device memory, 8-byte aligned, 288 bytes */
typedef struct uavx_norm_record {
    int64_t n_obs;
    double mean[UAVX_NORM_MAX_FEATURES];
    double M2[UAVX_NORM_MAX_FEATURES];
    int64_t n_ret;
    double mean_ret;
    double M2_ret;
} uavx_norm_record;

int uavx_norm_version(void);

/* *bytes = 8 · (2·features + 1) · ceil(envs · agents / UAVX_NORM_BLOCK): the per-workgroup partials of a fold_obs of
 * `features` features (two float64 per feature and one int64 per workgroup).  fold_returns needs what features = 1 gives.
 * Reads envs and agents only. */
int uavx_norm_workspace_bytes(const uavx_norm_ring *ring, int64_t features, int64_t *bytes);

/* obs: [slots, envs, agents, features].  The workspace is overwritten. */
int uavx_norm_fold_obs(const uavx_norm_ring *ring, const float *obs, int64_t features, int64_t first, int64_t count,
                       uavx_norm_record *record, void *workspace, int64_t workspace_bytes, void *stream);

/* gamma: in [0, 1].  carry: [envs, agents] float64.  The workspace is overwritten. */
int uavx_norm_fold_returns(const uavx_norm_ring *ring, int64_t first, int64_t count, double gamma, double *carry,
                           uavx_norm_record *record, void *workspace, int64_t workspace_bytes, void *stream);

/* in, out: [rows, features].  eps: finite, >= 0.  clip: finite, > 0. */
int uavx_norm_apply_obs(const uavx_norm_record *record, const float *in, float *out, int64_t rows, int64_t features,
                        double eps, double clip, void *stream);

/* in, out: count elements. */
int uavx_norm_scale_rewards(const uavx_norm_record *record, const float *in, float *out, int64_t count, double eps,
                            double clip, void *stream);

#ifdef __cplusplus
}
#endif
#endif

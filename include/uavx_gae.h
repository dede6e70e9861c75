/* uavx_gae.h — C ABI of libuavx_gae.so: GAE(λ) advantages and returns over the device ring of a DeviceReplay, and their
 * normalisation, on MI355X (gfx950).  DESIGN.md §28; tests/gae_ref.py restates the definition below in numpy.
 *
 * Ring (uavx_gae_ring; the layout of replay.DeviceReplay, time-major)
 *   L = slots = T + 1 slots.  rew [L,E,N] float32 and done [L,E,N] uint8, bit 0 of a done byte = this agent is done.
 *   skip [L,E] and ended [L,E] uint8 (non-zero = set): "the env was re-initialised instead of stepped, the row is not a
 *   transition" and "the env's episode ended AT this transition".  Both NULL: the packed ring, skip(s,e) is bit 1 and
 *   ended(s,e) bit 2 of done[s,e,0].  values [L,E,N] float32: the caller's V(s) of the observation of EVERY slot (slot
 *   count mod L, the state the next step starts from, included).
 *
 * Window
 *   c = count >= 1 steps written so far; 1 <= steps <= min(c, T).  The window is the steps k = c−1, c−2, ..., c−steps;
 *   step k lives in slot s = k mod L and its successor state in slot s1 = (k+1) mod L.
 *
 * Definition.  For every column (e, i) with i < learners, walk k DOWNWARDS from c−1 with a float64 carry A⁺ = 0:
 *   1. skip(k,e):   adv = +0, ret = +0, valid = 0; A⁺ = 0; next k.
 *   2. d = done[s,e,i] & 1;  b = d ? +0 : γ·(double)V[s1]  (a select: a value that is not bootstrapped from is never
 *      multiplied, so its NaN does not leak);  δ = ((double)r + b) − (double)V[s].
 *   3. stop = d ∨ ended(k,e) ∨ (k+1 >= c) ∨ skip(k+1,e);  A = stop ? δ : δ + (γλ)·A⁺  (a select again).  γλ is one
 *      float64 product formed on the host.  Every operation is one float64 rounding (no contraction).
 *   4. adv = (float)A; ret = (float)(A + (double)V[s]); valid = 1; A⁺ = A.
 *   This is the n-step walk's rule for where a walk ends and when it bootstraps (uavx_nstep.h), λ-weighted:
 *   an agent's own done ends it without a bootstrap; the end of the env's episode (a time-limit cut included) for an agent
 *   that is not itself done ends it WITH the bootstrap from V[s1], the successor observation the step launch stored before
 *   it re-initialised the env.  "truncated" is therefore not an input.
 *   Columns with i >= learners get adv = +0, ret = +0, valid = 0 in the window's rows.  Rows outside the window are not
 *   written, in any output.  The payload and sign of a NaN are not part of the contract; where a NaN is, is.
 *
 * Normalisation (adv_norm != NULL)
 *   Over the entries with valid = 1, on the float32-ROUNDED adv (the statistics are a function of the adv tensor alone):
 *   n = their count, mean = Σa / n (0 when n = 0), std = sqrt(Σ(a − mean)² / (n − 1)) (0 when n < 2),
 *   adv_norm = (float)(((double)a − mean) / (std + 1e-8)) on valid entries and +0 elsewhere in the window.
 *   Two passes, float64, in an order the launch geometry alone fixes -- no atomics, no workgroup waits on another:
 *     column sum      column q = e·N + i belongs to thread q mod 256 of workgroup q / 256 (UAVX_GAE_BLOCK columns per
 *                     workgroup; threads past the last column hold +0).  A thread starts from +0 and adds (double)a of its
 *                     column's valid entries in the order of the walk, k downwards.
 *     workgroup sum   over each wavefront of 64 lanes a halving tree: x[l] += x[l+32], then +16, +8, +4, +2, +1 (lane 0
 *                     holds the sum); then the four wavefront sums w0 + w1 + w2 + w3, left to right -> partial[workgroup].
 *     total           ONE workgroup's worth of threads: thread t starts from +0 and adds partial[t], partial[t + 256], ...
 *                     in index order, then the same workgroup sum.  (Every workgroup of the next launch forms this total
 *                     itself, in this order, so all of them hold the same bits.)
 *   The second pass sums ((double)a − mean)·((double)a − mean) -- subtraction, product and addition are three roundings --
 *   in exactly the same order.  n is summed in int64.  stats receives n, mean and std.
 *
 * Launches: the walk (which also leaves the first pass's per-workgroup sums); with adv_norm two more, the second pass and
 * the normalisation.  ONE launch without adv_norm, THREE with it.
 *
 * Conventions (the status codes are uavx_actor.h's)
 *   - every pointer but the ring struct itself is DEVICE memory on the current device; float32 arrays are 4-byte aligned,
 *     stats and workspace 8-byte aligned; the outputs overlap neither each other nor the inputs.
 *   - work is enqueued on `stream` (hipStream_t as void*, NULL = the null stream); nothing synchronises, nothing is allocated.
 *   - every argument is checked before the first launch: a rejected call enqueues nothing.
 *   - count, steps, γ and λ are read when the call is made.
 */
#ifndef UAVX_GAE_H
#define UAVX_GAE_H
#include <stdint.h>
#include "uavx_actor.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UAVX_GAE_VERSION 1
#define UAVX_GAE_BLOCK 256

typedef struct uavx_gae_ring {
    const float *rew;
    const uint8_t *done;
    const uint8_t *skip;      /* skip and ended: both NULL = packed into done (bits 1 and 2 of agent 0's byte) */
    const uint8_t *ended;
    int64_t slots;            /* T + 1, 2..2^31 − 1 */
    int64_t envs;             /* >= 1 */
    int64_t agents;           /* >= 1; envs · agents <= 2^31 − 1 */
    int64_t learners;         /* 1..agents */
} uavx_gae_ring;

/* what the last normalised call measured; device memory, 8-byte aligned */
typedef struct uavx_gae_stats {
    int64_t n;                /* entries with valid = 1 in the window */
    double mean;
    double std;
} uavx_gae_stats;

int uavx_gae_version(void);

/* *bytes = 24 · ceil(envs · agents / UAVX_GAE_BLOCK): the workspace a call with adv_norm needs (two float64 and one int64
 * per workgroup).  Reads envs and agents only. */
int uavx_gae_workspace_bytes(const uavx_gae_ring *ring, int64_t *bytes);

/* values, adv, ret, valid, adv_norm: [slots, envs, agents].  gamma, lambda: in [0, 1].
 * adv_norm: NULL = no normalisation (stats and workspace are then not looked at); otherwise stats must be given and
 * workspace hold workspace_bytes >= uavx_gae_workspace_bytes bytes; the workspace is overwritten. */
int uavx_gae_compute(const uavx_gae_ring *ring, const float *values, int64_t count, int64_t steps, double gamma,
                     double lambda, float *adv, float *ret, uint8_t *valid, float *adv_norm, uavx_gae_stats *stats,
                     void *workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif

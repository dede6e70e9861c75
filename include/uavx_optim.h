/* uavx_optim.h — C ABI of the optimiser step in libuavx_actor.so: torch.optim.Adam (AMSGrad optional) over a table of
 * float32 tensors and the learners' soft target update on MI355X (gfx950), as multi-tensor element-wise launches.
 *
 * One uavx_optim_adam call updates up to UAVX_OPTIM_MAX_TENSORS tensors that share their hyper-parameters and ONE step
 * count (a param group of torch.optim.Adam with weight_decay = 0, maximize = False).  With t' = *step + 1:
 *   prologue (one thread)   *step = t';  scalars[0] = (float)(lr / (1 − β1^t'));  scalars[1] = (float)sqrt(1 − β2^t')
 *                           (float64 arithmetic, rounded once, as torch's Python-float path)
 *   per element, separate float32 operations (no contraction; IEEE divide and square root)
 *     m ← m + (g − m)·(1 − β1)
 *     v ← v·β2 + (g·g)·(1 − β2)
 *     AMSGrad: vmax ← max(vmax, v), and vmax takes the place of v below
 *     p ← p − scalars[0]·(m / (sqrt(v) / scalars[1] + eps))
 *     with a target: θ' ← θ'·(1 − τ) + p·τ       (the new p; 1 − τ formed in float64 and rounded to float32)
 * uavx_optim_soft_update is the last line alone, θ' ← θ'·(1 − τ) + θ·τ (sac.py / ddpg.py soft_update, td3.py:152-156).
 *
 * Conventions (as uavx_critic_grad.h; the status codes are uavx_actor.h's)
 *   - the tables (params, grads, ..., numel) are HOST arrays of n entries, copied into the kernel arguments by the call;
 *     their entries are DEVICE pointers on the current device to contiguous float32 data of numel[i] elements, at least
 *     4-byte aligned.  Tensors whose pointers are all 16-byte aligned move 16 bytes per access, the others 4; the results
 *     do not depend on which.  Tensors of one call must not overlap.
 *   - work is enqueued on `stream` (hipStream_t as void*, NULL = the null stream); nothing synchronises and nothing is
 *     allocated: the calls can be captured into a graph, and a replay advances *step like a call does.
 *   - uavx_optim_adam is TWO kernel launches (prologue, update), uavx_optim_soft_update ONE; arguments are checked before
 *     any GPU call and a rejected call enqueues nothing.
 *   - no atomics and no reductions: the same inputs give bitwise-identical results.
 *   - lr, the betas, eps and tau are read when the call is made (a captured graph keeps the values of its capture).
 */
#ifndef UAVX_OPTIM_H
#define UAVX_OPTIM_H
#include <stdint.h>
#include "uavx_actor.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UAVX_OPTIM_VERSION 1
#define UAVX_OPTIM_MAX_TENSORS 16

int uavx_optim_version(void);

/* n: 1..UAVX_OPTIM_MAX_TENSORS.  params, grads, exp_avg, exp_avg_sq: n device pointers each, none NULL; params, exp_avg and
 *   exp_avg_sq are updated in place, grads are read.
 * max_exp_avg_sq: NULL = no AMSGrad; otherwise n pointers, none NULL, updated in place.
 * targets: NULL = no soft update; otherwise n pointers, a NULL entry leaves that tensor without one.
 * numel: n element counts, each 1..2^31 − 1.
 * lr >= 0, 0 <= beta1, beta2 < 1, eps >= 0, all finite; tau in [0, 1] (read only with targets).
 * step: device int64, 8-byte aligned, >= 0: the number of steps taken so far; read and advanced by the prologue.
 * scalars: device float[2], 8-byte aligned, written by the prologue and read by the update. */
int uavx_optim_adam(int n, float *const *params, const float *const *grads, float *const *exp_avg, float *const *exp_avg_sq,
                    float *const *max_exp_avg_sq, float *const *targets, const int64_t *numel, double lr, double beta1,
                    double beta2, double eps, double tau, int64_t *step, float *scalars, void *stream);

/* targets[i] ← targets[i]·(1 − tau) + sources[i]·tau over n tensors (1..UAVX_OPTIM_MAX_TENSORS; no NULL entry), tau in
 * [0, 1], numel as above. */
int uavx_optim_soft_update(int n, float *const *targets, const float *const *sources, const int64_t *numel, double tau,
                           void *stream);

#ifdef __cplusplus
}
#endif
#endif

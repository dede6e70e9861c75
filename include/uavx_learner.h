/* uavx_learner.h — C ABI of the learners' update tail in libuavx_actor.so: SAC's temperature (alpha) step and the loss
 * record of every learner on MI355X (gfx950), one launch of one wavefront with one working lane.
 *
 * The tail closes one update of a SAC / TD3 / DDPG learner (sac.py:80-98, td3.py:100-156, ddpg.py:50-85).  It reads the
 * device scalars the other units leave (the critic losses of uavx_critic_grad, the actor loss and mean log_pi of
 * uavx_policy_grad_backward), so that an update returns nothing to the host and a captured graph holds all of it.
 *
 * SAC with automatic entropy tuning (log_alpha != NULL), with h = *log_pi_mean + target_entropy (one float32 add):
 *   alpha_loss = −(log_alpha·h)                  (sac.py:82; the mean over the rows is already in *log_pi_mean)
 *   g = −h, t' = *step + 1, *step = t'
 *   step_size = (float)(lr / (1 − β1^t')),  bc2 = (float)sqrt(1 − β2^t')        (float64 arithmetic, rounded once)
 *   m ← m + (g − m)·(1 − β1);  v ← v·β2 + (g·g)·(1 − β2)                        (separate float32 operations)
 *   log_alpha ← log_alpha − step_size·(m / (sqrt(v) / bc2 + eps))               (uavx_optim.h's arithmetic, one element)
 *   *alpha ← (float)exp((double)log_alpha)                                       (float64 exp, rounded once)
 * Every learner, with u = *updates:
 *   log[u mod capacity][0..7] = critic_loss_1, critic_loss_2 (0 for DDPG or a NULL losses_in[1]), actor_loss (0 when
 *                               actor_updated == 0 or losses_in[2] is NULL), alpha_loss (0 without log_alpha),
 *                               *alpha after the step (0 when alpha is NULL), actor_updated, 0, 0
 *   *updates = u + 1
 *
 * Conventions (as uavx_optim.h; the status codes are uavx_actor.h's)
 *   - losses_in is a HOST array of three DEVICE pointers; every other pointer is a device pointer on the current device.
 *   - work is enqueued on `stream` (hipStream_t as void*, NULL = the null stream); nothing synchronises and nothing is
 *     allocated.  Both counts live on the device: the call can be captured into a graph and a replay advances them.
 *   - ONE kernel launch; arguments are checked before any GPU call and a rejected call enqueues nothing.
 *   - no atomics and no reductions: the same inputs give bitwise-identical results.
 *   - lr, the betas, eps and target_entropy are read when the call is made (a captured graph keeps its capture's values).
 */
#ifndef UAVX_LEARNER_H
#define UAVX_LEARNER_H
#include <stdint.h>
#include "uavx_actor.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UAVX_LEARNER_VERSION 1
#define UAVX_LEARNER_LOG_COLUMNS 8

int uavx_learner_version(void);

/* kind: UAVX_ACTOR_SAC / _TD3 / _DDPG.
 * losses_in: three device float pointers, each 4-byte aligned: [0] critic loss 1 (not NULL), [1] critic loss 2 (NULL = 0;
 *   not read for DDPG), [2] actor loss (NULL = 0; not read when actor_updated == 0).
 * log_alpha: NULL = no alpha step (TD3, DDPG, SAC with a fixed alpha).  Otherwise kind must be SAC and log_pi_mean,
 *   exp_avg, exp_avg_sq (device float, one element each), step (device int64, 8-byte aligned, >= 0) and alpha must not be
 *   NULL; target_entropy finite, lr >= 0, 0 <= beta1, beta2 < 1, eps >= 0, all finite.
 * alpha: device float, read and written with log_alpha, only read without it; NULL (allowed without log_alpha) records 0.
 * log: device float [capacity][8], 4-byte aligned; capacity >= 1.
 * updates: device int64, 8-byte aligned, >= 0: the number of updates recorded so far; read and advanced.
 * actor_updated: 0 or 1. */
int uavx_learner_tail(int kind, const float *const *losses_in, const float *log_pi_mean, float target_entropy,
                      float *log_alpha, float *exp_avg, float *exp_avg_sq, int64_t *step, double lr, double beta1,
                      double beta2, double eps, float *alpha, float *log, int64_t capacity, int64_t *updates,
                      int actor_updated, void *stream);

#ifdef __cplusplus
}
#endif
#endif

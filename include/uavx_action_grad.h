/* uavx_action_grad.h — C ABI of the critic action-gradient in libuavx_actor.so: the critic half of the learners' actor
 * update on MI355X (gfx950), f32.
 *
 * In the actor loss (SAC sac.py:70-75, TD3 td3.py:144, DDPG ddpg.py:77-78) the critic is only a differentiable function
 * of the action a = π(s).  One call computes, for the critic a uavx_critic handle describes (include/uavx_critic.h) and
 * the module's LIVE parameters passed at run time, per selected tower t and row:
 *   q_t      = the tower's forward on x = [state, action]                      one float
 *   ∂q_t/∂a  = the Jacobian of that scalar with respect to the two actions     two floats
 *     z1 = W1·x + b1, h1 = act(z1);  z2 = W2·h1 + b2;  q = w3·act(z2) + b3
 *     δ2 = w3 ⊙ act′(z2);  δ1 = (W2ᵀ·δ2) ⊙ act′(z1);  ∂q/∂a_j = Σ_u δ1[u]·W1[u][10 + j]
 * relu′(0) = 0 and leaky′(0) = 0.01, as torch's threshold_backward / leaky_relu_backward.  No weight gradient and no
 * gradient with respect to the state is produced.
 *
 * The handle only supplies the dimensions: its packed snapshot (uavx_critic_pack) is neither read nor changed.
 *
 * Conventions (as uavx_critic.h; the status codes and uavx_critic_strerror are that header's)
 *   - buffer arguments are DEVICE pointers on the handle's device; work is enqueued on `stream` (hipStream_t as void*,
 *     NULL = the null stream); nothing synchronises, nothing is allocated and there is no workspace: the call can be
 *     captured into a graph.
 *   - ONE kernel launch per call, one variant for every row count; arguments are checked before any GPU call and a
 *     rejected call enqueues nothing.
 *   - no atomics: every sum runs in a fixed order and a row's results do not depend on the other rows, so the same
 *     inputs give bitwise-identical outputs whatever the batch around them and whatever the tower mask.
 */
#ifndef UAVX_ACTION_GRAD_H
#define UAVX_ACTION_GRAD_H
#include <stdint.h>
#include "uavx_critic.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UAVX_ACTION_GRAD_VERSION 1
#define UAVX_ACTION_GRAD_MAX_ROWS 262144

int uavx_action_grad_version(void);

/* h: an f32 handle (bf16: UAVX_CRITIC_ERR_UNSUPPORTED).
 * towers_mask: bit t selects tower t (1: TD3's Q1 and DDPG; 3: SAC; 2: the second tower alone).  0, or a bit for a tower
 *   the handle does not have, is UAVX_CRITIC_ERR_INVALID_ARG.  An unselected tower costs no work and its output slots
 *   are not written.
 * params: W1, b1, W2, b2, W3, b3 of the first tower, then W4..b6 of the second (DDPG: input, fc1, fc2, then six NULLs),
 *   as uavx_critic_grad takes them: contiguous float32 in torch layout, read when the kernel runs.  The six pointers of
 *   every selected tower must not be NULL.
 * state: [rows][s_stride] (first 10 read); action: [rows][a_stride] (first 2 read).  Nothing past row rows−1 is read.
 *   rows in 1..UAVX_ACTION_GRAD_MAX_ROWS, s_stride >= 10, a_stride >= 2.
 * q: [T][rows] with T the handle's tower count, tower t at q + t·rows; may be NULL.
 * dqda: [T][rows][2], tower t at dqda + t·rows·2; must not be NULL.
 * Nothing outside the selected towers' `rows` entries is written. */
int uavx_action_grad(const uavx_critic *h, int towers_mask, const float *const *params, const float *state, int64_t rows,
                     int64_t s_stride, const float *action, int64_t a_stride, float *q, float *dqda, void *stream);

#ifdef __cplusplus
}
#endif
#endif

/* uavx_critic_grad.h — C ABI of the critic-loss gradient in libuavx_actor.so: the backward of the learners' critic update
 * on MI355X (gfx950), f32.
 *
 * One call computes, for the critic a uavx_critic handle describes (include/uavx_critic.h: SAC TwinQ, TD3 TD3TwinQ, DDPG
 * DDPGCritic) and the module's LIVE parameters passed at run time:
 *   q_t   = the tower's forward on [state, action]                          (t = 1, 2; DDPG: one tower)
 *   MSE   L_t = mean_b (q_t − y)²,  the gradient is that of L_1 + L_2      (sac.py:61-68, td3.py:129-138)
 *   L1    L_t = mean_b |q_t − y|,   dL/dq = sign(q − y) / B, sign(0) = 0   (ddpg.py:68 nn.L1Loss()(y, q))
 * and writes every parameter's gradient (torch layout: W [out][in], b [out]) OVER the destination — what
 * zero_grad(); loss.backward() leaves in .grad — and the loss value of each tower.  relu′(0) = 0 and leaky′(0) = 0.01, as
 * torch's threshold_backward / leaky_relu_backward.  The optimiser step stays the caller's.
 *
 * The handle only supplies the dimensions: its packed snapshot (uavx_critic_pack) is neither read nor changed.
 *
 * Conventions (as uavx_critic.h; the status codes and uavx_critic_strerror are that header's)
 *   - buffer arguments are DEVICE pointers on the handle's device; work is enqueued on `stream` (hipStream_t as void*,
 *     NULL = the null stream); nothing synchronises and nothing is allocated: the call can be captured into a graph.
 *   - THREE kernel launches per call (row pass, weight pass, combine); arguments are checked before any GPU call and a
 *     rejected call enqueues nothing.
 *   - no atomics: every sum over rows runs in a fixed order, so the same inputs give bitwise-identical gradients and losses.
 *   - the caller's workspace holds every per-row and split-K intermediate; uavx_critic_grad_workspace_bytes sizes it.
 *
 * Workspace (bytes; each region starts on a 256-byte boundary; T towers, B16 = rows rounded up to 16, N1 = 16·ceil(h1/16),
 * N2 = 16·ceil(h2/16), LP = 13·h1 + 2·h2 + 2 rounded up to 4, S split-K slices):
 *   h1 activations  T·B16·N1·4      layer-2 pre-activations, then δ2  T·B16·N2·4
 *   per-16-row partials of W1, b1, b2, W3, b3, loss (f64)  T·(B16/16)·LP·8
 *   W2 split-K partials  S·T·h2·h1·4      small-gradient split-K partials  S·T·LP·8
 */
#ifndef UAVX_CRITIC_GRAD_H
#define UAVX_CRITIC_GRAD_H
#include <stdint.h>
#include "uavx_critic.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UAVX_CRITIC_GRAD_VERSION 1
#define UAVX_CRITIC_GRAD_MAX_ROWS 262144

typedef enum { UAVX_CRITIC_GRAD_MSE = 0, UAVX_CRITIC_GRAD_L1 = 1 } uavx_critic_grad_loss;

int uavx_critic_grad_version(void);

/* Bytes of workspace uavx_critic_grad needs for `rows` rows (1..UAVX_CRITIC_GRAD_MAX_ROWS) on handle h, in *bytes.
 * f32 handles only (bf16: UAVX_CRITIC_ERR_UNSUPPORTED). */
int uavx_critic_grad_workspace_bytes(const uavx_critic *h, int64_t rows, int64_t *bytes);

/* loss: UAVX_CRITIC_GRAD_MSE or UAVX_CRITIC_GRAD_L1, for any kind.
 * params: W1, b1, W2, b2, W3, b3 of the first tower, then W4..b6 of the second (DDPG: input, fc1, fc2, then six NULLs);
 *   contiguous float32 in torch layout, read when the kernels run.
 * state: [rows][s_stride] (first 10 read); action: [rows][a_stride] (first 2 read); y: y[i * y_stride].  Nothing past
 *   row rows−1 is read.  rows in 1..UAVX_CRITIC_GRAD_MAX_ROWS.
 * grads: the twelve (DDPG: six, then NULLs) destinations in the layout of params, overwritten.
 * loss_out: one float per tower.  workspace: 16-byte aligned, at least uavx_critic_grad_workspace_bytes(h, rows). */
int uavx_critic_grad(const uavx_critic *h, int loss, const float *const *params, const float *state, int64_t rows,
                     int64_t s_stride, const float *action, int64_t a_stride, const float *y, int64_t y_stride,
                     float *const *grads, float *loss_out, void *workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif

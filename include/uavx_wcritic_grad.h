/* uavx_wcritic_grad.h — C ABI of the WEIGHTED critic-loss gradient in libuavx_actor.so: the critic-loss gradient of
 * include/uavx_critic_grad.h with a per-row importance-sampling weight (prioritized replay, beta > 0) and the live
 * critic's q(s, a) as an output, on MI355X (gfx950), f32.  DESIGN.md §24.
 *
 * One call computes, for a critic of the given kind and widths and the module's LIVE parameters passed at run time:
 *   q_t   = the tower's forward on [state, action]                          (t = 1, 2; DDPG: one tower)
 *   MSE   L_t = (1/B) sum_b w_b (q_t − y)²,  dL/dq = w (q − y) 2 / B
 *   L1    L_t = (1/B) sum_b w_b |q_t − y|,   dL/dq = w sign(q − y) / B, sign(0) = sign(NaN) = 0
 * and writes every parameter's gradient of L_1 + L_2 (torch layout: W [out][in], b [out]) OVER the destination, the loss
 * value of each tower and, on request, q_t of every row.  With weight == NULL, or every weight exactly 1.0f, every gradient
 * and loss equals uavx_critic_grad's bit for bit: the summation orders are the same.  A row of weight 0 contributes exact
 * zeros, like a padded row.  Weights are not validated on the device (a NaN propagates): the caller keeps them finite, >= 0.
 *
 * The call takes no uavx_critic handle: kind, h1, h2 and towers are arguments.
 *
 * Conventions (as uavx_critic_grad.h)
 *   - buffer arguments are DEVICE pointers on the current device; work is enqueued on `stream` (hipStream_t as void*,
 *     NULL = the null stream); nothing synchronises and nothing is allocated: the call can be captured into a graph.
 *   - THREE kernel launches per call (weighted row pass, weight pass, combine); arguments are checked before any GPU call
 *     and a rejected call enqueues nothing.
 *   - no atomics: every sum over rows runs in a fixed order, so the same inputs give bitwise-identical results.
 *   - the caller's workspace holds every per-row and split-K intermediate; uavx_wcritic_grad_workspace_bytes sizes it.
 *     Its layout and the split-K rule are uavx_critic_grad.h's: for equal kind, widths and rows the two
 *     calls need the same number of bytes.
 */
#ifndef UAVX_WCRITIC_GRAD_H
#define UAVX_WCRITIC_GRAD_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UAVX_WCRITIC_GRAD_VERSION 1
#define UAVX_WCRITIC_GRAD_MAX_ROWS 262144

/* status codes (the values of include/uavx_critic.h) */
#define UAVX_WCRITIC_OK 0
#define UAVX_WCRITIC_ERR_INVALID_ARG (-1)
#define UAVX_WCRITIC_ERR_HIP (-2)
#define UAVX_WCRITIC_ERR_UNSUPPORTED (-3)

/* kind: the learner (the values of uavx_actor_kind): SAC and TD3 are relu towers with h1 in 241..256, DDPG a leaky-relu
 * tower with h1 in 385..400; loss: the values of uavx_critic_grad_loss */
typedef enum { UAVX_WCRITIC_SAC = 0, UAVX_WCRITIC_TD3 = 1, UAVX_WCRITIC_DDPG = 2 } uavx_wcritic_kind;
typedef enum { UAVX_WCRITIC_MSE = 0, UAVX_WCRITIC_L1 = 1 } uavx_wcritic_loss;

int uavx_wcritic_grad_version(void);

/* Bytes of workspace uavx_wcritic_grad needs for `rows` rows (1..UAVX_WCRITIC_GRAD_MAX_ROWS), in *bytes (0 on an error).
 * h1 outside the kind's range: UAVX_WCRITIC_ERR_UNSUPPORTED; h2 >= 1; towers 1 or 2. */
int uavx_wcritic_grad_workspace_bytes(int kind, int h1, int h2, int towers, int64_t rows, int64_t *bytes);

/* params: W1, b1, W2, b2, W3, b3 of the first tower, then of the second (towers == 1: six entries are read); contiguous
 *   float32 in torch layout, read when the kernels run.
 * state: [rows][s_stride] (first 10 read); action: [rows][a_stride] (first 2 read); y: y[i * y_stride].
 * weight: weight[i * w_stride], or NULL for a weight of 1 on every row (w_stride is then not looked at).  Nothing past
 *   row rows−1 is read.
 * grads: the destinations in the layout of params, overwritten.  loss_out: one float per tower.
 * q_out: [towers][rows] receiving q_t(s, a), the f64-summed forward rounded once, or NULL.
 * workspace: 16-byte aligned, at least uavx_wcritic_grad_workspace_bytes(kind, h1, h2, towers, rows). */
int uavx_wcritic_grad(int kind, int h1, int h2, int towers, int loss, const float *const *params, const float *state,
                      int64_t rows, int64_t s_stride, const float *action, int64_t a_stride, const float *y,
                      int64_t y_stride, const float *weight, int64_t w_stride, float *const *grads, float *loss_out,
                      float *q_out, void *workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif

/* uavx_policy_grad.h — C ABI of the actor's own forward and backward of the learners' actor update in libuavx_actor.so,
 * on MI355X (gfx950), f32: the half of the actor-loss block that include/uavx_action_grad.h leaves out.
 *
 * The actor losses (SAC model.py:88-99 and sac.py:70-78, TD3 td3.py:144, DDPG ddpg.py:77-79) are
 *   SAC   L = mean_b(α·logπ − min(Q1, Q2)(s, π(s)))      TD3   L = −mean_b Q1(s, π(s))      DDPG  L = −mean_b Q(s, π(s))
 * and the critic is only a function of the action a = π(s).  The block is cut at that seam:
 *   uavx_policy_grad_forward    a (and SAC's logπ) from the actor's LIVE parameters; the activations stay in the workspace
 *   uavx_action_grad            q_t(s, a) and J_t = ∂q_t/∂a (include/uavx_action_grad.h, unchanged)
 *   uavx_policy_grad_backward   every actor parameter's gradient, L and SAC's mean_b logπ, from q and J as plain inputs
 *
 * Hidden layers: z1 = W1·s + b1, h1 = act(z1); z2 = W2·h1 + b2, h2 = act(z2); act = relu (SAC, TD3) or leaky relu 0.01
 * (DDPG); act′(0) = 0 for relu and 0.01 for leaky relu, as torch.
 * Head, TD3 / DDPG (O = 2):  y = tanh(W3·h2 + b3);  δ3 = −J ⊙ (1 − y²) / B.
 * Head, SAC (O = 4: W3 = mean_linear, W3b = log_std_linear):
 *   μ = W3·h2 + b3;  r = W3b·h2 + b3b;  ℓ = clamp(r, −20, 2);  σ = exp ℓ;  x = μ + σε;  y = tanh x
 *   logπ = Σ_j [−ε_j²/2 − ℓ_j − ½·log 2π − log(1 − y_j² + 1e-6)]
 *   w = 1 where q1 < q2, 0 where q1 > q2, ½ where q1 == q2 (torch.minimum's backward);  J = w·J1 + (1 − w)·J2
 *   g_x = [α·2y(1 − y²)/(1 − y² + 1e-6) − J ⊙ (1 − y²)] / B;  δμ = g_x;  δℓ = (−α/B + g_x·σε)·[−20 ≤ r ≤ 2]
 *   (the clamp passes its gradient at equality, as torch's);  δ3 = [δμ, δℓ].
 * Backward: δ2 = (W3ᵀδ3) ⊙ act′(z2);  δ1 = (W2ᵀδ2) ⊙ act′(z1);  dW3 = Σ_b δ3·h2ᵀ, db3 = Σ_b δ3;  dW2 = Σ_b δ2·h1ᵀ,
 *   db2 = Σ_b δ2;  dW1 = Σ_b δ1·sᵀ, db1 = Σ_b δ1.
 *
 * Conventions (the status codes and uavx_actor_strerror are include/uavx_actor.h's)
 *   - no handle: no snapshot is read.  The dimensions are passed as kind, hidden1, hidden2: kind UAVX_ACTOR_SAC / _TD3 /
 *     _DDPG, hidden1 241..256 (SAC, TD3) or 385..400 (DDPG), hidden2 1..4096; anything else is UAVX_ACTOR_ERR_UNSUPPORTED,
 *     as uavx_actor_create answers.
 *   - buffer arguments are DEVICE pointers; work is enqueued on `stream` (hipStream_t as void*, NULL = the null stream);
 *     nothing synchronises and nothing is allocated: both calls can be captured into a graph.
 *   - arguments are checked before any GPU call and a rejected call enqueues nothing.
 *   - no atomics: every sum runs in a fixed order, so the same inputs give bitwise-identical outputs.
 *   - params / grads: W1, b1, W2, b2, W3, b3, W3b, b3b, contiguous float32 in torch layout (W [out][in]).  SAC: W3, b3 are
 *     mean_linear's and W3b, b3b log_std_linear's; TD3 / DDPG: the last two are not read and may be NULL.
 *   - the caller must not change `state`, the parameters or the workspace between forward and backward.
 *
 * Workspace: uavx_policy_grad_workspace_bytes(kind, h1, h2, rows), at least 16-byte aligned, the sum of six regions each
 * rounded up to 256 bytes, with B16 = rows rounded up to 16, N1 = hidden1 rounded up to 16, N2 = hidden2 rounded up to
 * 16, O = 4 (SAC) or 2, LP = 11·hidden1 + (1 + O)·hidden2 + O + 2 rounded up to 4, and S the split-K slice count:
 *   h1              B16 · N1 · 4
 *   z2, then δ2     B16 · N2 · 4
 *   head records    B16 · 8 · 4
 *   block partials  (B16 / 16) · LP · 8
 *   dW2 slices      S · hidden2 · hidden1 · 4
 *   small slices    S · LP · 8
 *   tiles = ceil(hidden2 / 64) · ceil(hidden1 / 64);  S0 = clamp(8192 / tiles, 1, ceil(B16 / 64));
 *   KC = ceil(B16 / S0) rounded up to 16;  S = ceil(B16 / KC).
 */
#ifndef UAVX_POLICY_GRAD_H
#define UAVX_POLICY_GRAD_H
#include <stdint.h>
#include "uavx_actor.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UAVX_POLICY_GRAD_VERSION 1
#define UAVX_POLICY_GRAD_MAX_ROWS 262144

int uavx_policy_grad_version(void);

/* *bytes = the workspace both calls need for `rows` rows (rows in 1..UAVX_POLICY_GRAD_MAX_ROWS); 0 on an error. */
int uavx_policy_grad_workspace_bytes(int kind, int hidden1, int hidden2, int64_t rows, int64_t *bytes);

/* Launch 1.  params: 8 pointers (see above).  state: [rows][s_stride], first 10 read, s_stride >= 10; nothing past row
 * rows−1 is read.  eps: SAC [rows][2] contiguous, must not be NULL; TD3 / DDPG: not read, NULL.
 * action: [rows][2] contiguous, must not be NULL.  log_pi: SAC [rows], must not be NULL; TD3 / DDPG: not written.
 * Nothing outside `rows` entries of action / log_pi and the workspace is written. */
int uavx_policy_grad_forward(int kind, int hidden1, int hidden2, const float *const *params, const float *state,
                             int64_t rows, int64_t s_stride, const float *eps, float *action, float *log_pi,
                             void *workspace, int64_t workspace_bytes, void *stream);

/* Launches 3 to 5, after uavx_policy_grad_forward on the same kind, sizes, params, state, rows and workspace.
 * q: [T][rows], tower t at q + t·q_tower_stride; dqda: [T][rows][2], tower t at dqda + t·q_tower_stride·2 (the layout of
 *   uavx_action_grad with q_tower_stride = rows); SAC reads two towers, TD3 and DDPG the first; q_tower_stride >= rows.
 * alpha (SAC): read from alpha_dev (one device float, read when the kernel runs) when that is not NULL, else the value.
 * grads: 8 destinations in the order and layout of params (TD3 / DDPG: the last two not written), overwritten.
 * loss_out: one float, L.  log_pi_mean_out: SAC one float, mean_b logπ, must not be NULL; TD3 / DDPG: not written. */
int uavx_policy_grad_backward(int kind, int hidden1, int hidden2, const float *const *params, const float *state,
                              int64_t rows, int64_t s_stride, const float *q, const float *dqda, int64_t q_tower_stride,
                              float alpha, const float *alpha_dev, float *const *grads, float *loss_out,
                              float *log_pi_mean_out, void *workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif

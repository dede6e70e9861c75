/* uavx_ppo.h — C ABI of libuavx_ppo.so: what PPO does between its networks' GEMMs, on MI355X (gfx950).  The sampling head
 * turns a policy's (μ, log σ) and a noise draw into the pre-squash sample, its action and its log density; the loss head
 * turns a minibatch's (μ, log σ, V) into the clipped-surrogate losses and their gradient with respect to those three
 * outputs.  DESIGN.md §29; tests/ppo_heads_ref.py restates everything below in torch on the CPU.
 *
 * All arithmetic is float32 unless it says float64; every operation written below is ONE rounding (the library is built
 * with -ffp-contract=off), brackets give the order.  expf, log1pf and tanhf are the device library's.
 *
 * Log density (one device function, shared by both heads).  For a row with μ[2], ℓ[2] = log σ and pre-squash sample u[2],
 * per action dimension d:
 *     z      = (u − μ) · expf(−ℓ)
 *     gauss  = (((−0.5·z)·z) − ℓ) − 0.5·log 2π
 *     sp     = max(x, 0) + log1pf(expf(−|x|))  at x = −2·u                       softplus(−2u)
 *     squash = 2 · ((log 2 − u) − sp)                                            log(1 − tanh²u)
 *     t_d    = gauss − squash
 *   log π = t_0 + t_1.  The constants are the float32 roundings of 0.5·log 2π and log 2.
 *
 * uavx_ppo_sample: ONE launch, one thread per row.  Per action dimension
 *     σ = expf(ℓ);   u = μ + (σ·ε)   (two roundings);   a = tanhf(u)
 *   u_out = u, action_out = a, logp_out = log π(μ, ℓ, u) of the u that was stored.  The three outputs are independent
 *   pointers (a slot of a ring each, say).
 *
 * uavx_ppo_loss: TWO launches.  Row b of the minibatch reads row j = idx[b] (idx NULL: j = b) of the five flat arrays.
 *   lo = (float)(1 − clip), hi = (float)(1 + clip), both formed in float64 on the host.
 *     log π  from (μ_b, ℓ_b, u_j) as above
 *     r      = expf(log π − logp_old_j)                                          -> ratio[b]
 *     s1     = r · adv_j;   s2 = clamp(r, lo, hi) · adv_j;   surr = s1 < s2 ? s1 : s2
 *     q      = 0.5 · ((v_b − ret_j) · (v_b − ret_j))
 *   Sums over the minibatch in float64, of the exact products (double)w_j·(double)x of float32 values:
 *     W = Σ w,  S = Σ w·surr,  Q = Σ w·q,  P = Σ w·log π.   A weight of 0 MULTIPLIES, it does not select: a row with w = 0
 *     and a non-finite term poisons the sum, as it does in torch.
 *     D = max(1, W);  policy_loss = −S / D;  value_loss = Q / D;  entropy = −P / D   (float64, then rounded to float32)
 *   scalars[4] = (policy_loss, value_loss, entropy, W).
 *   The order of each sum is fixed by the launch geometry alone -- no atomics, no workgroup waits on another:
 *     thread order    row b belongs to thread b mod 256 of workgroup b / 256 (UAVX_PPO_BLOCK rows per workgroup; threads
 *                     past the last row hold +0).
 *     workgroup sum   over each wavefront of 64 lanes a halving tree: x[l] += x[l+32], then +16, +8, +4, +2, +1 (lane 0
 *                     holds the sum); then the four wavefront sums w0 + w1 + w2 + w3, left to right -> partial[workgroup].
 *     total           thread t starts from +0 and adds partial[t], partial[t + 256], ... in index order, then the same
 *                     workgroup sum.  Every workgroup of the second launch forms W this way itself, so all of them hold
 *                     the same bits; workgroup 0 also forms S, Q and P and writes scalars.
 *   Gradient of policy_loss + vf_coef·value_loss − ent_coef·entropy with respect to mean, log_std and v (second launch):
 *     k      = (float)((double)w_j / D)
 *     pass   = (lo <= r <= hi) ∨ (s1 < s2)
 *     g_lp   = k · (ent_coef − (pass ? adv_j·r : 0))
 *     g_mean_d    = (g_lp · z_d) · expf(−ℓ_d)
 *     g_log_std_d = g_lp · ((z_d·z_d) − 1)
 *     g_v         = (k · vf_coef) · (v_b − ret_j)
 *   `pass` is what torch's derivatives of minimum(s1, s2) and clamp(r, lo, hi) give together, tie and edge rules included:
 *   minimum sends the whole gradient to the smaller argument and half to each on a tie; clamp passes it for lo <= r <= hi,
 *   edges included.  Inside the band s1 = s2 and the two halves add up to one; outside it the clamp's path is dead, so the
 *   gradient passes only where s1 is the strictly smaller; s1 = s2 outside the band needs adv = 0, and then the term is 0
 *   either way.
 *   ratio[b], g_mean[b], g_log_std[b] and g_v[b] depend on the row's own inputs and on D only: they are bit-identical
 *   wherever the row sits in the minibatch and whatever B is.
 *
 * Conventions (the status codes are uavx_actor.h's)
 *   - every pointer is DEVICE memory on the current device.  [.,2] float32 arrays and idx are 8-byte aligned, the other
 *     float32 arrays 4-byte, the workspace 8-byte.  Outputs overlap neither each other nor the inputs.
 *   - work is enqueued on `stream` (hipStream_t as void*, NULL = the null stream); nothing synchronises, nothing is allocated.
 *   - every argument is checked before the first launch: a rejected call enqueues nothing.  What the device cannot check is
 *     the caller's responsibility: non-finite inputs (they propagate) and idx values outside [0, R) (they are read as they are).
 *   - rows, B, R: 1..2^31 − 1; without idx B <= R.  clip: finite and > 0.  vf_coef, ent_coef: finite and >= 0.
 */
#ifndef UAVX_PPO_H
#define UAVX_PPO_H
#include <stdint.h>
#include "uavx_actor.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UAVX_PPO_VERSION 1
#define UAVX_PPO_BLOCK 256

int uavx_ppo_version(void);

/* mean, log_std, eps, u_out, action_out: [rows, 2]; logp_out: [rows]. */
int uavx_ppo_sample(const float *mean, const float *log_std, const float *eps, int64_t rows, float *u_out, float *logp_out,
                    float *action_out, void *stream);

/* *bytes = 32 · ceil(B / UAVX_PPO_BLOCK): four float64 partials per workgroup. */
int uavx_ppo_loss_workspace_bytes(int64_t B, int64_t *bytes);

/* mean, log_std, g_mean, g_log_std: [B, 2]; v, ratio, g_v: [B]; idx: [B] int64 or NULL; u: [R, 2]; logp_old, adv, ret,
 * weight: [R]; scalars: [4].  The workspace holds workspace_bytes >= uavx_ppo_loss_workspace_bytes bytes and is overwritten. */
int uavx_ppo_loss(const float *mean, const float *log_std, const float *v, const int64_t *idx, int64_t B, const float *u,
                  const float *logp_old, const float *adv, const float *ret, const float *weight, int64_t R, double clip,
                  double vf_coef, double ent_coef, float *ratio, float *scalars, float *g_mean, float *g_log_std, float *g_v,
                  void *workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif

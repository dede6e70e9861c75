/* uavx_critic.h — C ABI of the critic half of libuavx_actor.so: fused no-grad critic forwards and TD targets of the
 * reference's learners on MI355X (gfx950).
 *
 * Two entry points, each ONE kernel launch:
 *   uavx_critic_q       Q of given (state, action) rows (the critic module's forward).
 *   uavx_critic_target  the whole no-grad block that opens the learners' update, with the next action kept on the chip:
 *     SAC   a', logπ = policy.sample(s')           y = r + (mask·γ)·(min(Q1', Q2')(s', a') − α·logπ)   (sac.py:56-60)
 *     TD3   a' = clamp(actor(s') + clamp(σ·ε, −c, c), −1, 1)   y = r + (mask·γ)·min(Q1', Q2')(s', a')   (td3.py:114-127)
 *     DDPG  a' = actor(s')                         y = r + (γ·mask)·Q'(s', a')                          (ddpg.py:62)
 * The critic layouts are those of policy.py:
 *   UAVX_CRITIC_SAC   TwinQ       relu, relu, linear; two towers (Q1 = linear1..3, Q2 = linear4..6)
 *   UAVX_CRITIC_TD3   TD3TwinQ    the same architecture (Q1 = l1..l3, Q2 = l4..l6)
 *   UAVX_CRITIC_DDPG  DDPGCritic  leaky_relu(0.01), leaky_relu(0.01), linear; one tower
 * on the input [state (10), action (2)].
 *
 * Conventions (as uavx_actor.h)
 *   - every function returns 0 (UAVX_CRITIC_OK) or a negative status; uavx_critic_strerror() names it.
 *   - buffer arguments are DEVICE pointers owned by the caller on the device the handle was created on; work is enqueued on
 *     `stream` (a hipStream_t passed as void*, NULL = the null stream) and nothing synchronises.
 *   - pack, q and target are each ONE kernel launch on `stream` and allocate nothing: all can be captured into a graph.
 *   - arguments are checked before any GPU call; a rejected call enqueues nothing.
 *   - no atomics: the same inputs give bitwise-identical outputs, and a row's outputs depend on that row alone.
 *   - a handle is not thread-safe.
 */
#ifndef UAVX_CRITIC_H
#define UAVX_CRITIC_H
#include <stdint.h>
#include "uavx_actor.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UAVX_CRITIC_VERSION 1

/* Batches of fewer rows than this run the small-batch variant (a workgroup of waves shares each 16-row block and sums its
 * partial outputs through LDS); larger ones the actor's tile (each wave carries its rows through every layer).  The two sum
 * the layer-2 contributions in different orders: see uavx_critic_set_split_rows. */
#define UAVX_CRITIC_SPLIT_ROWS 16384

typedef enum {
    UAVX_CRITIC_OK = 0,
    UAVX_CRITIC_ERR_INVALID_ARG = -1,
    UAVX_CRITIC_ERR_HIP = -2,          /* a HIP runtime call failed */
    UAVX_CRITIC_ERR_UNSUPPORTED = -3,  /* dimensions this build has no kernel for (see uavx_critic_create) */
    UAVX_CRITIC_ERR_NOT_PACKED = -4    /* q / target before the first pack of the critic or of the actor */
} uavx_critic_status;

typedef enum { UAVX_CRITIC_SAC = 0, UAVX_CRITIC_TD3 = 1, UAVX_CRITIC_DDPG = 2 } uavx_critic_kind;
typedef enum { UAVX_CRITIC_F32 = 0, UAVX_CRITIC_BF16 = 1 } uavx_critic_precision;

typedef struct uavx_critic uavx_critic;

int uavx_critic_version(void);
const char *uavx_critic_strerror(int status);

/* obs_dim 10 and act_dim 2; hidden1 in 241..256 for SAC / TD3 and 385..400 for DDPG (the actor's compiled register tiles),
 * hidden2 in 1..4096, for both precisions.  Allocates the packed weight buffer on the current device.  *out stays NULL on
 * failure. */
int uavx_critic_create(int kind, int precision, int obs_dim, int hidden1, int hidden2, int act_dim, uavx_critic **out);
int uavx_critic_destroy(uavx_critic *h);

/* Row threshold of the small-batch variant for this handle (default UAVX_CRITIC_SPLIT_ROWS; 0 = never, INT64_MAX = always).
 * Within one variant a row's result does not depend on the batch size; across the switch the results agree to f32
 * rounding, not bitwise. */
int uavx_critic_set_split_rows(uavx_critic *h, int64_t rows);

/* Copies the weights, in torch layout (W: [out][in] row-major float32, b: [out]), into the handle's packed buffer (MFMA
 * operand order, zero padded, rounded to bf16 with round-to-nearest-even for UAVX_CRITIC_BF16).  W1..b3 are the first tower
 * (DDPG: input, fc1, fc2), W4..b6 the second (NULL for DDPG).  The packed copy is a snapshot: pack again after the weights
 * change. */
int uavx_critic_pack(uavx_critic *h, const float *W1, const float *b1, const float *W2, const float *b2, const float *W3,
                     const float *b3, const float *W4, const float *b4, const float *W5, const float *b5, const float *W6,
                     const float *b6, void *stream);

/* state: [rows][state_stride] (first 10 read), action: [rows][action_stride] (first 2 read), out: [rows][out_stride] with
 * Q1, Q2 in columns 0, 1 (SAC / TD3) or Q in column 0 (DDPG).  rows >= 0 (0 enqueues nothing). */
int uavx_critic_q(uavx_critic *h, const float *state, int64_t rows, int64_t state_stride, const float *action,
                  int64_t action_stride, float *out, int64_t out_stride, void *stream);

/* The TD target of the learner `h` belongs to, with `actor` (same kind and precision) giving the next action.
 * next_state: [rows][state_stride]; reward, mask: one float per row at reward[i * reward_stride], mask[i * mask_stride];
 * eps: [rows][2] contiguous standard normals (SAC: the rsample noise; TD3: the smoothing noise before noise_std and clip;
 * unused by DDPG); alpha: a DEVICE float (SAC only; read at run time so graph replays see updates); noise_std, noise_clip:
 * TD3's policy_noise and noise_clip; out: y at out[i * out_stride]; aux (optional, NULL = none): [rows][aux_stride >= 4]
 * a'0, a'1, logπ (0 for TD3 / DDPG), min Q (DDPG: Q). */
int uavx_critic_target(uavx_critic *h, const uavx_actor *actor, const float *next_state, int64_t rows, int64_t state_stride,
                       const float *reward, int64_t reward_stride, const float *mask, int64_t mask_stride, const float *eps,
                       const float *alpha, float gamma, float noise_std, float noise_clip, float *out, int64_t out_stride,
                       float *aux, int64_t aux_stride, void *stream);

#ifdef __cplusplus
}
#endif
#endif

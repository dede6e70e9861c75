/* uavx_actor.h — C ABI of libuavx_actor.so: fused inference of the reference's actor networks on MI355X (gfx950).
 *
 * One launch computes a whole actor forward (3 linear layers, activations and the action epilogue) for every row of a
 * batch of observations; the hidden activations never leave the chip.  The three layouts are those of policy.py:
 *   UAVX_ACTOR_SAC   GaussianPolicy  relu, relu, two heads (mean; log_std clamped to [-20, 2])
 *   UAVX_ACTOR_TD3   TD3Actor        relu, relu, tanh
 *   UAVX_ACTOR_DDPG  DDPGActor       leaky_relu(0.01), leaky_relu(0.01), tanh
 *
 * Conventions (as uavx.h)
 *   - every function returns 0 (UAVX_ACTOR_OK) or a negative status; uavx_actor_strerror() names it.
 *   - buffer arguments are DEVICE pointers owned by the caller on the device the handle was created on; work is enqueued on
 *     `stream` (a hipStream_t passed as void*, NULL = the null stream) and nothing synchronises.
 *   - pack and forward are each ONE kernel launch on `stream` and allocate nothing: both can be captured into a graph.
 *   - arguments are checked before any GPU call; a rejected call enqueues nothing.
 *   - a handle is not thread-safe.
 */
#ifndef UAVX_ACTOR_H
#define UAVX_ACTOR_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UAVX_ACTOR_VERSION 1

typedef enum {
    UAVX_ACTOR_OK = 0,
    UAVX_ACTOR_ERR_INVALID_ARG = -1,
    UAVX_ACTOR_ERR_HIP = -2,          /* a HIP runtime call failed */
    UAVX_ACTOR_ERR_UNSUPPORTED = -3,  /* dimensions this build has no kernel for (see uavx_actor_create) */
    UAVX_ACTOR_ERR_NOT_PACKED = -4    /* forward before the first pack */
} uavx_actor_status;

typedef enum { UAVX_ACTOR_SAC = 0, UAVX_ACTOR_TD3 = 1, UAVX_ACTOR_DDPG = 2 } uavx_actor_kind;
typedef enum { UAVX_ACTOR_F32 = 0, UAVX_ACTOR_BF16 = 1 } uavx_actor_precision;

/* Epilogue of uavx_actor_forward.  y = pre-tanh output (SAC: mean), ls = SAC's clamped log_std.
 *   RAW            out[:, 0:2] = y; SAC also out[:, 2:4] = ls (4 columns)       (verification)
 *   DETERMINISTIC  out = tanh(y)
 *   SAC_SAMPLE     out = tanh(y + exp(ls) * eps)                                   (SAC only)
 *   ADD_CLAMP      out = clamp(tanh(y) + scale * eps, -1, 1)                       (TD3 exploration, DDPG noise)  */
typedef enum {
    UAVX_ACTOR_RAW = 0,
    UAVX_ACTOR_DETERMINISTIC = 1,
    UAVX_ACTOR_SAC_SAMPLE = 2,
    UAVX_ACTOR_ADD_CLAMP = 3
} uavx_actor_mode;

typedef struct uavx_actor uavx_actor;

int uavx_actor_version(void);
const char *uavx_actor_strerror(int status);

/* obs_dim 10 and act_dim 2 (the environment's); hidden1 in 241..256 for SAC / TD3 and 385..400 for DDPG (the reference's
 * 256 and 400, whose register tiles this build compiles), hidden2 in 1..4096, for both precisions.  Allocates the packed
 * weight buffer on the current device. */
int uavx_actor_create(int kind, int precision, int obs_dim, int hidden1, int hidden2, int act_dim, uavx_actor **out);
int uavx_actor_destroy(uavx_actor *h);

/* Copies the weights, in torch layout (W: [out][in] row-major float32, b: [out]), into the handle's packed buffer (MFMA
 * operand order, zero padded, rounded to bf16 with round-to-nearest-even for UAVX_ACTOR_BF16).  W3 / b3 are the output
 * layer (SAC: mean_linear); W3b / b3b SAC's log_std_linear, NULL for the other kinds.  The packed copy is a snapshot: pack
 * again after the weights change. */
int uavx_actor_pack(uavx_actor *h, const float *W1, const float *b1, const float *W2, const float *b2, const float *W3,
                    const float *b3, const float *W3b, const float *b3b, void *stream);

/* obs: [rows][obs_stride] float32, the first 10 of each row read; out: [rows][out_stride] float32, 2 columns written (4 for
 * SAC in RAW mode); eps: [rows][2] float32 contiguous, read by SAC_SAMPLE and ADD_CLAMP (NULL otherwise allowed).
 * rows >= 0 (0 enqueues nothing).  Deterministic: the same inputs give bitwise-identical outputs. */
int uavx_actor_forward(uavx_actor *h, const float *obs, int64_t rows, int64_t obs_stride, const float *eps, float scale,
                       int mode, float *out, int64_t out_stride, void *stream);

#ifdef __cplusplus
}
#endif
#endif

/* uavx_clip.h — C ABI of libuavx_clip.so: the Adam step of uavx_optim.h behind a clip of the GLOBAL gradient norm, as
 * torch.nn.utils.clip_grad_norm_(all_params, max_norm) followed by torch.optim.Adam.step(), on MI355X (gfx950).
 * DESIGN.md §26.
 *
 * One uavx_clip_step call takes every param group of one optimiser (uavx_clip_group: the arguments of uavx_optim_adam) and
 * clips by ONE norm over all gradients of all groups:
 *
 *   sum of squares   S = Σ (double)g·(double)g over every element of every gradient.  Each product of two float32 values
 *                    is exact in float64; the sum is accumulated in float64 in an order the launch geometry alone fixes:
 *                    every gradient is cut into blocks of UAVX_CLIP_BLOCK elements (each tensor starts a block of its own,
 *                    the blocks of group 0 first), a block is summed by one workgroup of 256 threads -- each thread its
 *                    four elements, a shuffle tree over each wavefront, the four wavefronts through LDS in order -- into
 *                    partials[block], and one workgroup sums the partials: thread t takes partials t, t + 256, ... in
 *                    index order, then the same tree.  No floating-point atomics, no workgroup waits on another, no
 *                    counter of finished blocks: kernel boundaries are the only ordering, and the same inputs give the
 *                    same bits.
 *   record           norm = (float)sqrt(S);  coef = min(1.0f, max_norm / (norm + 1e-6f)) in float32, a NaN passing through
 *                    (torch's clamp(max_norm / (total_norm + 1e-6), max=1.0) with error_if_nonfinite=False): one +inf
 *                    gradient gives coef 0, one NaN a NaN coef.  max_norm is read from a float32 DEVICE slot when the
 *                    kernel runs, so a captured step follows a write into the slot.  rec->norm and rec->coef are written,
 *                    and rec->clipped is advanced by one when coef < 1.
 *   step             g' = g·coef, one float32 rounding, then exactly uavx_optim_adam's element arithmetic on g' (m, v,
 *                    AMSGrad's vmax with NaN propagation, p − step_size·(m / (sqrtf(d)/bc2_sqrt + eps)), separate float32
 *                    operations, no contraction) and, with targets, the soft update from the new p in the same launch.
 *                    Each group's step count is advanced on the device by its prologue, as uavx_optim_adam's.
 *                    The gradients themselves are NOT rewritten (that would be one more pass over them): multiply by
 *                    rec->coef to get the clipped gradient.
 *
 * Launches: one sum-of-squares launch per group, then per group a prologue and the update.  The first group's prologue is
 * the one-workgroup launch that also sums the partials and writes the record; the later groups' prologues are one thread.
 * One group: THREE launches.
 *
 * Conventions (uavx_optim.h's; the status codes are uavx_actor.h's)
 *   - the group array and its tables are HOST memory, copied into the kernel arguments by the call; table entries are
 *     DEVICE pointers on the current device to contiguous float32 data of numel[i] elements, at least 4-byte aligned.
 *     Tensors whose pointers are all 16-byte aligned move 16 bytes per access, the others 4.  Tensors must not overlap.
 *   - work is enqueued on `stream` (hipStream_t as void*, NULL = the null stream); nothing synchronises and nothing is
 *     allocated: the call can be captured into a graph, and a replay advances the step counts like a call does.
 *   - every argument of every group is checked before the first launch: a rejected call enqueues nothing.
 *   - lr, the betas, eps and tau are read when the call is made (a captured graph keeps the values of its capture);
 *     max_norm is read on the device.
 */
#ifndef UAVX_CLIP_H
#define UAVX_CLIP_H
#include <stdint.h>
#include "uavx_actor.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UAVX_CLIP_VERSION 1
#define UAVX_CLIP_MAX_TENSORS 16
#define UAVX_CLIP_MAX_GROUPS 16
#define UAVX_CLIP_BLOCK 1024

/* what the last step measured; device memory, 8-byte aligned */
typedef struct uavx_clip_record {
    float norm;        /* (float)sqrt(S) */
    float coef;        /* what every gradient element was multiplied by */
    int64_t clipped;   /* number of steps with coef < 1 so far */
} uavx_clip_record;

/* One param group: the arguments of uavx_optim_adam (uavx_optim.h), with the same ranges.
 * n: 1..UAVX_CLIP_MAX_TENSORS.  params, grads, exp_avg, exp_avg_sq: n device pointers each, none NULL.
 * max_exp_avg_sq: NULL = no AMSGrad; otherwise n pointers, none NULL.
 * targets: NULL = no soft update; otherwise n pointers, a NULL entry leaves that tensor without one.
 * numel: n element counts, each 1..2^31 − 1.
 * lr >= 0, 0 <= beta1, beta2 < 1, eps >= 0, all finite; tau in [0, 1] (read only with targets).
 * step: device int64, 8-byte aligned; scalars: device float[2], 8-byte aligned (written by the prologue). */
typedef struct uavx_clip_group {
    int32_t n;
    float *const *params;
    const float *const *grads;
    float *const *exp_avg;
    float *const *exp_avg_sq;
    float *const *max_exp_avg_sq;
    float *const *targets;
    const int64_t *numel;
    double lr;
    double beta1;
    double beta2;
    double eps;
    double tau;
    int64_t *step;
    float *scalars;
} uavx_clip_group;

int uavx_clip_version(void);

/* *bytes = 8 · (number of UAVX_CLIP_BLOCK-element blocks over every tensor of every group): the size of `partials`.
 * Reads n and numel of each group only.  groups: 1..UAVX_CLIP_MAX_GROUPS. */
int uavx_clip_workspace_bytes(int groups, const uavx_clip_group *g, int64_t *bytes);

/* partials: device float64 workspace of partials_bytes >= uavx_clip_workspace_bytes bytes, 8-byte aligned; overwritten.
 * max_norm: device float32 slot, 8-byte aligned, read by the first prologue (finite and > 0 is the caller's to keep).
 * rec: device record, 8-byte aligned. */
int uavx_clip_step(int groups, const uavx_clip_group *g, double *partials, int64_t partials_bytes, const float *max_norm,
                   uavx_clip_record *rec, void *stream);

#ifdef __cplusplus
}
#endif
#endif

/* uavx_explore.h — C ABI of the exploration launch in libuavx_actor.so: the trainers' action noise on MI355X (gfx950),
 * one launch behind uavx_actor_forward in UAVX_ACTOR_RAW mode, one thread per row.  DESIGN.md §20.
 *
 * A row is one acting agent.  It owns 16 bytes of state, {double x; uint32 n; uint32 reserved}: x is the value of its
 * Ornstein-Uhlenbeck process (ou.py), n the number of calls the row has seen (it wraps modulo 2^32 and is never reset).
 * Both live on the device, so a replayed graph advances them with no race and no atomics.
 *
 * Random words are Philox4x32-10 with key (seed low word, seed high word) and counter (g low 32 bits, g high 32 bits, n,
 * stream), g = row_offset + row the 64-bit GLOBAL row: a batch cut into shards draws what the whole batch draws.
 *   stream 0, words w0..w3:  u1 = (w0 + 1)·2^-32, u2 = w1·2^-32, r = sqrt(−2·log(u1)),
 *                            n0 = r·cos(6.283185307179586·u2), n1 = r·sin(6.283185307179586·u2)     (all float64)
 *                            uniform action i = (float)(−1 + 2·(w_{2+i}·2^-32))
 *   stream 1, word 0:        ub = w0·2^-32
 * `normals` (float64 [rows][2]) replaces (n0, n1) when given; `normals_out` always receives the pair that was used.
 *
 * Per row, in this order:
 *   1. the state is loaded;
 *   2. with reset_flags: if (reset_flags[(row / rows_per_env)·reset_stride] & reset_mask) x = ou_x_initial;
 *   3. random = (n < warmup_steps) || (p > 0 && ub < (double)p), p = *random_prob_dev when given, else random_prob;
 *   4. random: out = the uniform action and x is not advanced.  Otherwise, by kind (y = the raw row):
 *        SAC   out_i = tanhf(mean_i + expf(log_std_i)·(float)n_i)               (UAVX_ACTOR_SAC_SAMPLE's operations)
 *        TD3   out_i = clamp(tanhf(y_i) + noise_std·(float)n_i, −1, 1)          (UAVX_ACTOR_ADD_CLAMP's operations)
 *        DDPG  x = (x + (ou_theta·(ou_mean − x))·ou_dt) + s·n0 in float64, s = ou_sigma·sqrt(ou_dt) formed once on the
 *              host; out_i = (float)clip((double)tanhf(y_i) + x, −1, 1), the same x for both components (ddpg.py:44)
 *   5. n += 1 and the state is stored.
 *
 * Conventions (as uavx_learner.h; the status codes and kinds are uavx_actor.h's)
 *   - every pointer is a device pointer on the current device; work is enqueued on `stream` (hipStream_t as void*, NULL =
 *     the null stream); nothing synchronises and nothing is allocated: the call can be captured into a graph.
 *   - ONE kernel launch; arguments are checked before any GPU call and a rejected call enqueues nothing.
 *   - no atomics and no reductions: the same inputs give bitwise-identical results.
 *   - every by-value field is read when the call is made (a captured graph keeps its capture's values); what has to
 *     change under a graph lives behind a pointer (the state, random_prob_dev, reset_flags).
 */
#ifndef UAVX_EXPLORE_H
#define UAVX_EXPLORE_H
#include <stdint.h>
#include "uavx_actor.h"

#ifdef __cplusplus
extern "C" {
#endif

#define UAVX_EXPLORE_VERSION 1
#define UAVX_EXPLORE_MAX_ROWS 16777216 /* 2^24 */
#define UAVX_EXPLORE_STATE_BYTES 16

typedef struct uavx_explore_args {
    int32_t kind;                 /* UAVX_ACTOR_SAC / _TD3 / _DDPG */
    int32_t rows_per_env;         /* read with reset_flags only: >= 1 and a divisor of rows */
    int64_t rows;                 /* 1 .. UAVX_EXPLORE_MAX_ROWS */
    int64_t row_offset;           /* >= 0: global row of row 0 */
    uint64_t seed;
    const float *raw;             /* SAC [rows][raw_stride] 4 columns read, 16-byte aligned, raw_stride % 4 == 0;
                                     TD3 / DDPG 2 columns read, 8-byte aligned, raw_stride % 2 == 0 */
    int64_t raw_stride;           /* in floats, >= the columns read */
    float *out;                   /* [rows][out_stride], 2 columns written, 8-byte aligned, out_stride % 2 == 0, >= 2 */
    int64_t out_stride;
    void *state;                  /* [rows] of 16 bytes, 16-byte aligned; read and written */
    const double *normals;        /* NULL or [rows][2], 16-byte aligned */
    double *normals_out;          /* NULL or [rows][2], 16-byte aligned */
    const uint8_t *reset_flags;   /* NULL = no resets */
    int64_t reset_stride;         /* bytes from one env's flag byte to the next, >= 1 */
    int32_t reset_mask;           /* the bits tested, 1 .. 255 */
    int32_t reserved;             /* 0 */
    int64_t warmup_steps;         /* >= 0: rows with n below it act at random */
    const float *random_prob_dev; /* NULL = random_prob below; else one device float in [0, 1], 4-byte aligned */
    float random_prob;            /* in [0, 1] */
    float noise_std;              /* TD3: >= 0, finite */
    double ou_sigma, ou_theta, ou_dt, ou_mean, ou_x_initial; /* sigma, dt >= 0; all finite */
} uavx_explore_args;

int uavx_explore_version(void);

int uavx_explore_act(const uavx_explore_args *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif

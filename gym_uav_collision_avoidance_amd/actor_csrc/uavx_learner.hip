// The learners' update tail (include/uavx_learner.h): SAC's temperature step and the loss record.  DESIGN.md §19.
//
//   tail   one wavefront, lane 0 works: the Adam step of the one-element log_alpha (uavx_optim.hip's arithmetic, the
//          prologue's two scalars formed in place), alpha = exp(log_alpha) into the slot the target and the actor-loss
//          kernels read by pointer, then one 8-float row of the loss ring and the update count.  Every count it advances
//          lives on the device, so a captured graph takes a new step and a new row on every replay.
//
// The unit is built with -ffp-contract=off: every float32 operation below is one rounding; `/` and sqrtf are hipcc's
// correctly rounded defaults; pow, sqrt and exp on doubles are float64 and their results are rounded to float32 once.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/uavx_learner.h"

namespace uavx_learner_k {

constexpr int COLS = UAVX_LEARNER_LOG_COLUMNS;

struct Args {
    const float *loss[3];        // critic 1, critic 2 (NULL: 0), actor (NULL: 0)
    const float *log_pi_mean;
    float *log_alpha;            // NULL: no alpha step
    float *m, *v;
    int64_t *step;
    float *alpha;                // NULL: 0 is recorded
    float *log;
    int64_t *updates;
    int64_t capacity;
    double lr, beta1, beta2;
    float target_entropy, w1, beta2f, w2, eps;     // w1 = 1 − β1, w2 = 1 − β2
    float actor_updated;
};

__global__ __launch_bounds__(64) void tail(const Args a) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float alpha_loss = 0.f, alpha = a.alpha ? *a.alpha : 0.f;
    if (a.log_alpha) {
        const float h = *a.log_pi_mean + a.target_entropy;
        float la = *a.log_alpha, m = *a.m, v = *a.v;
        alpha_loss = -(la * h);
        const float g = -h;
        const int64_t t = *a.step + 1;
        *a.step = t;
        const float step_size = (float)(a.lr / (1.0 - pow(a.beta1, (double)t)));
        const float bc2_sqrt = (float)sqrt(1.0 - pow(a.beta2, (double)t));
        m = m + (g - m) * a.w1;
        v = v * a.beta2f + (g * g) * a.w2;
        la = la - step_size * (m / (sqrtf(v) / bc2_sqrt + a.eps));
        alpha = (float)exp((double)la);
        *a.m = m;
        *a.v = v;
        *a.log_alpha = la;
        *a.alpha = alpha;
    }
    const int64_t u = *a.updates;
    float *row = a.log + (u % a.capacity) * COLS;
    row[0] = *a.loss[0];
    row[1] = a.loss[1] ? *a.loss[1] : 0.f;
    row[2] = a.loss[2] ? *a.loss[2] : 0.f;
    row[3] = alpha_loss;
    row[4] = alpha;
    row[5] = a.actor_updated;
    row[6] = 0.f;
    row[7] = 0.f;
    *a.updates = u + 1;
}

static bool aligned(const void *p, uintptr_t n) { return ((uintptr_t)p & (n - 1)) == 0; }

}  // namespace uavx_learner_k

using namespace uavx_learner_k;

extern "C" {

int uavx_learner_version(void) { return UAVX_LEARNER_VERSION; }

int uavx_learner_tail(int kind, const float *const *losses_in, const float *log_pi_mean, float target_entropy,
                      float *log_alpha, float *exp_avg, float *exp_avg_sq, int64_t *step, double lr, double beta1,
                      double beta2, double eps, float *alpha, float *log, int64_t capacity, int64_t *updates,
                      int actor_updated, void *stream) {
    if (kind != UAVX_ACTOR_SAC && kind != UAVX_ACTOR_TD3 && kind != UAVX_ACTOR_DDPG) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (!losses_in || !losses_in[0] || !log || !updates || capacity < 1 || capacity > INT64_MAX / COLS)
        return UAVX_ACTOR_ERR_INVALID_ARG;
    if (actor_updated != 0 && actor_updated != 1) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (!aligned(log, 4) || !aligned(updates, 8) || !aligned(alpha, 4)) return UAVX_ACTOR_ERR_INVALID_ARG;
    for (int i = 0; i < 3; ++i)
        if (!aligned(losses_in[i], 4)) return UAVX_ACTOR_ERR_INVALID_ARG;
    Args a{};
    a.loss[0] = losses_in[0];
    a.loss[1] = kind == UAVX_ACTOR_DDPG ? nullptr : losses_in[1];
    a.loss[2] = actor_updated ? losses_in[2] : nullptr;
    if (log_alpha) {
        if (kind != UAVX_ACTOR_SAC || !log_pi_mean || !exp_avg || !exp_avg_sq || !step || !alpha)
            return UAVX_ACTOR_ERR_INVALID_ARG;
        if (!aligned(log_pi_mean, 4) || !aligned(log_alpha, 4) || !aligned(exp_avg, 4) || !aligned(exp_avg_sq, 4)
            || !aligned(step, 8))
            return UAVX_ACTOR_ERR_INVALID_ARG;
        if (!isfinite(target_entropy) || !(lr >= 0.0) || !isfinite(lr) || !(eps >= 0.0) || !isfinite(eps))
            return UAVX_ACTOR_ERR_INVALID_ARG;
        if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return UAVX_ACTOR_ERR_INVALID_ARG;
        a.log_pi_mean = log_pi_mean;
        a.log_alpha = log_alpha;
        a.m = exp_avg;
        a.v = exp_avg_sq;
        a.step = step;
        a.lr = lr;
        a.beta1 = beta1;
        a.beta2 = beta2;
        a.target_entropy = target_entropy;
        a.w1 = (float)(1.0 - beta1);
        a.beta2f = (float)beta2;
        a.w2 = (float)(1.0 - beta2);
        a.eps = (float)eps;
    }
    a.alpha = alpha;
    a.log = log;
    a.updates = updates;
    a.capacity = capacity;
    a.actor_updated = (float)actor_updated;
    hipLaunchKernelGGL(tail, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? UAVX_ACTOR_OK : UAVX_ACTOR_ERR_HIP;
}

}  // extern "C"

// Adam step and soft target update (include/uavx_optim.h) as multi-tensor element-wise kernels.  DESIGN.md §15.
//
//   1. adam_prologue  one thread: advances the device step count and writes the two scalars of the step (bias-corrected
//                     step size, sqrt of the second bias correction), float64 arithmetic rounded once to float32.  The
//                     update kernel is ordered behind it by the stream, so a captured graph advances on every replay.
//   2. update<ADAM>   a flat space of 1024-element blocks over every tensor of the by-value table.  A block finds its tensor
//                     by a scalar search over the first-block numbers, then each thread takes one float4 of every array
//                     (16-byte aligned tensors) or four strided floats (the others, and the last < 4 elements of a tensor).
//                     ADAM = false is the soft update alone: `p` is then the read-only source.
//
// The unit is built with -ffp-contract=off: every operation below is one float32 rounding, `/` and sqrtf are hipcc's
// correctly rounded defaults, so the vector and scalar paths give the same bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/uavx_optim.h"

namespace uavx_optim_k {

constexpr int WG = 256, VEC = 4, BLOCK_ELEMS = WG * VEC, MAXT = UAVX_OPTIM_MAX_TENSORS;

struct Table {
    float *p[MAXT];          // parameters (ADAM = false: the sources, only read)
    const float *g[MAXT];
    float *m[MAXT];
    float *v[MAXT];
    float *vmax[MAXT];       // all NULL without AMSGrad
    float *target[MAXT];     // NULL: no soft update of this tensor
    int32_t numel[MAXT];
    int32_t first[MAXT];     // number of the first block of each tensor
    uint32_t vec;            // bit i: every pointer of tensor i is 16-byte aligned
    int32_t n;
    float w1, beta2, w2, eps;     // w1 = 1 − β1, w2 = 1 − β2
    float tau, one_minus_tau;
    const float *scalars;    // step size, sqrt(1 − β2^t): written by adam_prologue
};

__global__ void adam_prologue(int64_t *step, float *scalars, double lr, double beta1, double beta2) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int64_t t = *step + 1;
    *step = t;
    scalars[0] = (float)(lr / (1.0 - pow(beta1, (double)t)));
    scalars[1] = (float)sqrt(1.0 - pow(beta2, (double)t));
}

struct Hyper {
    float w1, beta2, w2, eps, step_size, bc2_sqrt, tau, one_minus_tau;
};

// one element; the arrays' values travel in registers so that both access widths share this code
template <bool ADAM>
__device__ inline void element(const Hyper &h, bool amsgrad, bool soft, float &p, float g, float &m, float &v, float &vmax,
                               float &tgt) {
    if constexpr (ADAM) {
        m = m + (g - m) * h.w1;
        v = v * h.beta2 + (g * g) * h.w2;
        float d = v;
        if (amsgrad) {
            vmax = (v > vmax || v != v) ? v : vmax;     // torch.maximum: a NaN propagates
            d = vmax;
        }
        p = p - h.step_size * (m / (sqrtf(d) / h.bc2_sqrt + h.eps));
    }
    if (soft) tgt = tgt * h.one_minus_tau + p * h.tau;
}

template <bool ADAM>
__global__ __launch_bounds__(WG) void update(const Table t) {
    // block -> tensor: the last tensor whose first block is not past this one (uniform, scalar registers)
    const int32_t blk = (int32_t)blockIdx.x;
    int j = 0;
    for (int i = 1; i < MAXT; ++i)
        if (i < t.n && t.first[i] <= blk) j = i;
    const int32_t n = t.numel[j];
    float *__restrict__ P = t.p[j];
    const float *__restrict__ G = t.g[j];
    float *__restrict__ M = t.m[j];
    float *__restrict__ V = t.v[j];
    float *__restrict__ X = t.vmax[j];
    float *__restrict__ T = t.target[j];
    const bool amsgrad = ADAM && X != nullptr, soft = T != nullptr;
    Hyper h{t.w1, t.beta2, t.w2, t.eps, 0.f, 1.f, t.tau, t.one_minus_tau};
    if constexpr (ADAM) {
        h.step_size = t.scalars[0];
        h.bc2_sqrt = t.scalars[1];
    }
    const int64_t base = (int64_t)(blk - t.first[j]) * BLOCK_ELEMS;     // < 2^31: numel fits int32
    const int64_t i0 = base + (int64_t)threadIdx.x * VEC;
    if (((t.vec >> j) & 1u) && i0 + VEC <= n) {
        float4 p = *(const float4 *)(P + i0), g{}, m{}, v{}, x{}, y{};
        if constexpr (ADAM) {
            g = *(const float4 *)(G + i0);
            m = *(const float4 *)(M + i0);
            v = *(const float4 *)(V + i0);
            if (amsgrad) x = *(const float4 *)(X + i0);
        }
        if (soft) y = *(const float4 *)(T + i0);
        element<ADAM>(h, amsgrad, soft, p.x, g.x, m.x, v.x, x.x, y.x);
        element<ADAM>(h, amsgrad, soft, p.y, g.y, m.y, v.y, x.y, y.y);
        element<ADAM>(h, amsgrad, soft, p.z, g.z, m.z, v.z, x.z, y.z);
        element<ADAM>(h, amsgrad, soft, p.w, g.w, m.w, v.w, x.w, y.w);
        if constexpr (ADAM) {
            *(float4 *)(P + i0) = p;
            *(float4 *)(M + i0) = m;
            *(float4 *)(V + i0) = v;
            if (amsgrad) *(float4 *)(X + i0) = x;
        }
        if (soft) *(float4 *)(T + i0) = y;
        return;
    }
    // scalar path: an unaligned tensor takes its block's elements with a stride of WG (coalesced 4-byte accesses); in an
    // aligned tensor only the thread that holds the last < 4 elements arrives here with anything to do
    const bool strided = !((t.vec >> j) & 1u);
    for (int k = 0; k < VEC; ++k) {
        const int64_t i = strided ? base + (int64_t)k * WG + threadIdx.x : i0 + k;
        if (i >= n) break;
        float p = P[i], g = 0.f, m = 0.f, v = 0.f, x = 0.f, y = 0.f;
        if constexpr (ADAM) {
            g = G[i];
            m = M[i];
            v = V[i];
            if (amsgrad) x = X[i];
        }
        if (soft) y = T[i];
        element<ADAM>(h, amsgrad, soft, p, g, m, v, x, y);
        if constexpr (ADAM) {
            P[i] = p;
            M[i] = m;
            V[i] = v;
            if (amsgrad) X[i] = x;
        }
        if (soft) T[i] = y;
    }
}

static bool aligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// Fills the pointer-independent part of the table; false on a bad count.  Every tensor starts a block of its own.
static bool plan(Table &t, int n, const int64_t *numel, int64_t &blocks) {
    if (n < 1 || n > MAXT || !numel) return false;
    t.n = n;
    blocks = 0;
    for (int i = 0; i < n; ++i) {
        if (numel[i] < 1 || numel[i] > INT32_MAX) return false;
        t.numel[i] = (int32_t)numel[i];
        t.first[i] = (int32_t)blocks;
        blocks += (numel[i] + BLOCK_ELEMS - 1) / BLOCK_ELEMS;     // <= 16 · 2^21
    }
    return true;
}

static bool unit(double x) { return x >= 0.0 && x <= 1.0; }     // false for NaN

}  // namespace uavx_optim_k

using namespace uavx_optim_k;

extern "C" {

int uavx_optim_version(void) { return UAVX_OPTIM_VERSION; }

int uavx_optim_adam(int n, float *const *params, const float *const *grads, float *const *exp_avg, float *const *exp_avg_sq,
                    float *const *max_exp_avg_sq, float *const *targets, const int64_t *numel, double lr, double beta1,
                    double beta2, double eps, double tau, int64_t *step, float *scalars, void *stream) {
    Table t{};
    int64_t blocks = 0;
    if (!params || !grads || !exp_avg || !exp_avg_sq || !plan(t, n, numel, blocks)) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (!step || !scalars || !aligned(step, 8) || !aligned(scalars, 8)) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (!(lr >= 0.0) || !isfinite(lr) || !(eps >= 0.0) || !isfinite(eps)) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (targets && !unit(tau)) return UAVX_ACTOR_ERR_INVALID_ARG;
    for (int i = 0; i < n; ++i) {
        const void *ps[6] = {params[i], grads[i], exp_avg[i], exp_avg_sq[i], max_exp_avg_sq ? max_exp_avg_sq[i] : nullptr,
                             targets ? targets[i] : nullptr};
        if (!ps[0] || !ps[1] || !ps[2] || !ps[3] || (max_exp_avg_sq && !ps[4])) return UAVX_ACTOR_ERR_INVALID_ARG;
        bool v16 = true;
        for (const void *q : ps) {
            if (!aligned(q, 4)) return UAVX_ACTOR_ERR_INVALID_ARG;
            v16 = v16 && aligned(q, 16);
        }
        t.p[i] = params[i];
        t.g[i] = grads[i];
        t.m[i] = exp_avg[i];
        t.v[i] = exp_avg_sq[i];
        t.vmax[i] = (float *)ps[4];
        t.target[i] = (float *)ps[5];
        t.vec |= (uint32_t)v16 << i;
    }
    t.w1 = (float)(1.0 - beta1);
    t.beta2 = (float)beta2;
    t.w2 = (float)(1.0 - beta2);
    t.eps = (float)eps;
    t.tau = (float)tau;
    t.one_minus_tau = (float)(1.0 - tau);
    t.scalars = scalars;
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(adam_prologue, dim3(1), dim3(64), 0, st, step, scalars, lr, beta1, beta2);
    if (hipGetLastError() != hipSuccess) return UAVX_ACTOR_ERR_HIP;
    hipLaunchKernelGGL(update<true>, dim3((unsigned)blocks), dim3(WG), 0, st, t);
    return hipGetLastError() == hipSuccess ? UAVX_ACTOR_OK : UAVX_ACTOR_ERR_HIP;
}

int uavx_optim_soft_update(int n, float *const *targets, const float *const *sources, const int64_t *numel, double tau,
                           void *stream) {
    Table t{};
    int64_t blocks = 0;
    if (!targets || !sources || !plan(t, n, numel, blocks) || !unit(tau)) return UAVX_ACTOR_ERR_INVALID_ARG;
    for (int i = 0; i < n; ++i) {
        if (!targets[i] || !sources[i] || !aligned(targets[i], 4) || !aligned(sources[i], 4))
            return UAVX_ACTOR_ERR_INVALID_ARG;
        t.p[i] = (float *)sources[i];     // update<false> only reads it
        t.target[i] = targets[i];
        t.vec |= (uint32_t)(aligned(targets[i], 16) && aligned(sources[i], 16)) << i;
    }
    t.tau = (float)tau;
    t.one_minus_tau = (float)(1.0 - tau);
    hipLaunchKernelGGL(update<false>, dim3((unsigned)blocks), dim3(WG), 0, (hipStream_t)stream, t);
    return hipGetLastError() == hipSuccess ? UAVX_ACTOR_OK : UAVX_ACTOR_ERR_HIP;
}

}  // extern "C"

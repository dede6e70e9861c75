// The Adam step behind a clip of the global gradient norm (include/uavx_clip.h) as three kinds of launch.
//
//   1. sumsq          the flat space of 1024-element blocks of update<> over one group's gradients.  A block finds its
//                     tensor by the same scalar search, each thread squares its four elements in float64 (one float4 of a
//                     16-byte aligned tensor, four strided floats otherwise and in the last < 4 elements), a shuffle tree
//                     sums each wavefront, the four wavefronts meet in LDS and thread 0 adds them in order into
//                     partials[block].
//   2. finish         ONE workgroup: thread t adds partials t, t + 256, ... in index order, the same tree, and thread 0
//                     writes norm, coef and the clipped count and is the Adam prologue of the first group (step count and
//                     the step's two scalars, as uavx_optim.hip's adam_prologue).  Later groups take adam_prologue alone.
//   3. update         uavx_optim.hip's update<true> with one more multiply: g·coef, coef read from the record.
//
// The Adam arithmetic below (element, the prologue's two scalars, the block-to-tensor table) restates uavx_optim.hip, whose
// library stays as it is; tests/test_gpu_clip.py holds the two to the same bits.  Built with -ffp-contract=off: every
// operation is one rounding, `/` and sqrtf are hipcc's correctly rounded defaults.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/uavx_clip.h"
#include "../common_csrc/uavx_block_reduce.hpp"
#include "../common_csrc/uavx_entry.hpp"

namespace uavx_clip_k {

using namespace uavx_common;

constexpr int WG = 256, VEC = 4, BLOCK_ELEMS = WG * VEC, MAXT = UAVX_CLIP_MAX_TENSORS, WAVES = WG / WAVE;
static_assert(BLOCK_ELEMS == UAVX_CLIP_BLOCK, "the header states the block size");

struct Table {
    float *p[MAXT];
    const float *g[MAXT];
    float *m[MAXT];
    float *v[MAXT];
    float *vmax[MAXT];       // all NULL without AMSGrad
    float *target[MAXT];     // NULL: no soft update of this tensor
    int32_t numel[MAXT];
    int32_t first[MAXT];     // number of the first block of each tensor within its group
    uint32_t vec;            // bit i: every pointer of tensor i is 16-byte aligned
    int32_t n;
    float w1, beta2, w2, eps;     // w1 = 1 − β1, w2 = 1 − β2
    float tau, one_minus_tau;
    const float *scalars;    // step size, sqrt(1 − β2^t): written by the prologue
    const uavx_clip_record *rec;
};

struct NormTable {
    const float *g[MAXT];
    int32_t numel[MAXT];
    int32_t first[MAXT];
    uint32_t vec;            // bit i: the gradient of tensor i is 16-byte aligned
    int32_t n;
    double *partials;        // this group's part of the workspace
};

__global__ __launch_bounds__(WG) void sumsq(const NormTable t) {
    __shared__ double part[WAVES];
    const int32_t blk = (int32_t)blockIdx.x;
    int j = 0;
    for (int i = 1; i < MAXT; ++i)
        if (i < t.n && t.first[i] <= blk) j = i;
    const int32_t n = t.numel[j];
    const float *__restrict__ G = t.g[j];
    const int64_t base = (int64_t)(blk - t.first[j]) * BLOCK_ELEMS;
    const int64_t i0 = base + (int64_t)threadIdx.x * VEC;
    const bool vec = (t.vec >> j) & 1u;
    double s = 0.0;
    if (vec && i0 + VEC <= n) {
        const float4 g = *(const float4 *)(G + i0);
        s = (double)g.x * (double)g.x;
        s += (double)g.y * (double)g.y;
        s += (double)g.z * (double)g.z;
        s += (double)g.w * (double)g.w;
    } else {
        for (int k = 0; k < VEC; ++k) {
            const int64_t i = vec ? i0 + k : base + (int64_t)k * WG + threadIdx.x;
            if (i >= n) break;
            const double g = (double)G[i];
            s += g * g;
        }
    }
    const double r = block_sum<WG>(s, part);
    if (threadIdx.x == 0) t.partials[blk] = r;
}

__device__ inline void prologue(int64_t *step, float *scalars, double lr, double beta1, double beta2) {
    const int64_t t = *step + 1;
    *step = t;
    scalars[0] = (float)(lr / (1.0 - pow(beta1, (double)t)));
    scalars[1] = (float)sqrt(1.0 - pow(beta2, (double)t));
}

__global__ __launch_bounds__(WG) void finish(const double *__restrict__ partials, int64_t count,
                                             const float *__restrict__ max_norm, uavx_clip_record *rec, int64_t *step,
                                             float *scalars, double lr, double beta1, double beta2) {
    __shared__ double part[WAVES];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < count; i += WG) s += partials[i];     // total<WG> with a 64-bit count
    const double S = block_sum<WG>(s, part);
    if (threadIdx.x != 0) return;
    const float norm = (float)sqrt(S);
    const float c = *max_norm / (norm + 1e-6f);
    const float coef = c > 1.0f ? 1.0f : c;     // a NaN stays a NaN
    rec->norm = norm;
    rec->coef = coef;
    if (coef < 1.0f) rec->clipped = rec->clipped + 1;
    prologue(step, scalars, lr, beta1, beta2);
}

__global__ void adam_prologue(int64_t *step, float *scalars, double lr, double beta1, double beta2) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    prologue(step, scalars, lr, beta1, beta2);
}

struct Hyper {
    float w1, beta2, w2, eps, step_size, bc2_sqrt, tau, one_minus_tau;
};

// one element of uavx_optim.hip's update<true>; g arrives clipped
__device__ inline void element(const Hyper &h, bool amsgrad, bool soft, float &p, float g, float &m, float &v, float &vmax,
                               float &tgt) {
    m = m + (g - m) * h.w1;
    v = v * h.beta2 + (g * g) * h.w2;
    float d = v;
    if (amsgrad) {
        vmax = (v > vmax || v != v) ? v : vmax;     // torch.maximum: a NaN propagates
        d = vmax;
    }
    p = p - h.step_size * (m / (sqrtf(d) / h.bc2_sqrt + h.eps));
    if (soft) tgt = tgt * h.one_minus_tau + p * h.tau;
}

__global__ __launch_bounds__(WG) void update(const Table t) {
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
    const bool amsgrad = X != nullptr, soft = T != nullptr;
    const Hyper h{t.w1, t.beta2, t.w2, t.eps, t.scalars[0], t.scalars[1], t.tau, t.one_minus_tau};
    const float coef = t.rec->coef;
    const int64_t base = (int64_t)(blk - t.first[j]) * BLOCK_ELEMS;     // < 2^31: numel fits int32
    const int64_t i0 = base + (int64_t)threadIdx.x * VEC;
    if (((t.vec >> j) & 1u) && i0 + VEC <= n) {
        float4 p = *(const float4 *)(P + i0), g = *(const float4 *)(G + i0), m = *(const float4 *)(M + i0),
               v = *(const float4 *)(V + i0), x{}, y{};
        if (amsgrad) x = *(const float4 *)(X + i0);
        if (soft) y = *(const float4 *)(T + i0);
        element(h, amsgrad, soft, p.x, g.x * coef, m.x, v.x, x.x, y.x);
        element(h, amsgrad, soft, p.y, g.y * coef, m.y, v.y, x.y, y.y);
        element(h, amsgrad, soft, p.z, g.z * coef, m.z, v.z, x.z, y.z);
        element(h, amsgrad, soft, p.w, g.w * coef, m.w, v.w, x.w, y.w);
        *(float4 *)(P + i0) = p;
        *(float4 *)(M + i0) = m;
        *(float4 *)(V + i0) = v;
        if (amsgrad) *(float4 *)(X + i0) = x;
        if (soft) *(float4 *)(T + i0) = y;
        return;
    }
    // scalar path: an unaligned tensor takes its block's elements with a stride of WG; in an aligned tensor only the thread
    // that holds the last < 4 elements arrives here with anything to do
    const bool strided = !((t.vec >> j) & 1u);
    for (int k = 0; k < VEC; ++k) {
        const int64_t i = strided ? base + (int64_t)k * WG + threadIdx.x : i0 + k;
        if (i >= n) break;
        float p = P[i], m = M[i], v = V[i], x = 0.f, y = 0.f;
        const float g = G[i] * coef;
        if (amsgrad) x = X[i];
        if (soft) y = T[i];
        element(h, amsgrad, soft, p, g, m, v, x, y);
        P[i] = p;
        M[i] = m;
        V[i] = v;
        if (amsgrad) X[i] = x;
        if (soft) T[i] = y;
    }
}

// The block numbers of one group; false on a bad count.  Every tensor starts a block of its own.
static bool plan(int n, const int64_t *numel, int32_t *count, int32_t *first, int64_t &blocks) {
    if (n < 1 || n > MAXT || !numel) return false;
    blocks = 0;
    for (int i = 0; i < n; ++i) {
        if (numel[i] < 1 || numel[i] > INT32_MAX) return false;
        count[i] = (int32_t)numel[i];
        first[i] = (int32_t)blocks;
        blocks += (numel[i] + BLOCK_ELEMS - 1) / BLOCK_ELEMS;     // <= 16 · 2^21
    }
    return true;
}

// Checks one group as uavx_optim_adam checks its arguments and fills its two tables.
static bool fill(const uavx_clip_group &g, Table &t, NormTable &nt, int64_t &blocks) {
    if (!g.params || !g.grads || !g.exp_avg || !g.exp_avg_sq || !plan(g.n, g.numel, t.numel, t.first, blocks)) return false;
    if (!g.step || !g.scalars || !aligned(g.step, 8) || !aligned(g.scalars, 8)) return false;
    if (!(g.lr >= 0.0) || !isfinite(g.lr) || !(g.eps >= 0.0) || !isfinite(g.eps)) return false;
    if (!(g.beta1 >= 0.0 && g.beta1 < 1.0) || !(g.beta2 >= 0.0 && g.beta2 < 1.0)) return false;
    if (g.targets && !unit(g.tau)) return false;
    t.n = nt.n = g.n;
    for (int i = 0; i < g.n; ++i) {
        const void *ps[6] = {g.params[i], g.grads[i], g.exp_avg[i], g.exp_avg_sq[i],
                             g.max_exp_avg_sq ? g.max_exp_avg_sq[i] : nullptr, g.targets ? g.targets[i] : nullptr};
        if (!ps[0] || !ps[1] || !ps[2] || !ps[3] || (g.max_exp_avg_sq && !ps[4])) return false;
        bool v16 = true;
        for (const void *q : ps) {
            if (!aligned(q, 4)) return false;
            v16 = v16 && aligned(q, 16);
        }
        t.p[i] = g.params[i];
        t.g[i] = nt.g[i] = g.grads[i];
        t.m[i] = g.exp_avg[i];
        t.v[i] = g.exp_avg_sq[i];
        t.vmax[i] = (float *)ps[4];
        t.target[i] = (float *)ps[5];
        t.vec |= (uint32_t)v16 << i;
        nt.vec |= (uint32_t)aligned(ps[1], 16) << i;
        nt.numel[i] = t.numel[i];
        nt.first[i] = t.first[i];
    }
    t.w1 = (float)(1.0 - g.beta1);
    t.beta2 = (float)g.beta2;
    t.w2 = (float)(1.0 - g.beta2);
    t.eps = (float)g.eps;
    t.tau = (float)g.tau;
    t.one_minus_tau = (float)(1.0 - g.tau);
    t.scalars = g.scalars;
    return true;
}

}  // namespace uavx_clip_k

using namespace uavx_clip_k;

extern "C" {

UAVX_BUILD_MARKER(UAVX_CLIP_SRC_HASH);

int uavx_clip_version(void) { return UAVX_CLIP_VERSION; }

int uavx_clip_workspace_bytes(int groups, const uavx_clip_group *g, int64_t *bytes) {
    if (groups < 1 || groups > UAVX_CLIP_MAX_GROUPS || !g || !bytes) return UAVX_ACTOR_ERR_INVALID_ARG;
    int64_t total = 0;
    for (int k = 0; k < groups; ++k) {
        int32_t count[MAXT], first[MAXT];
        int64_t blocks = 0;
        if (!plan(g[k].n, g[k].numel, count, first, blocks)) return UAVX_ACTOR_ERR_INVALID_ARG;
        total += blocks;
    }
    *bytes = total * (int64_t)sizeof(double);
    return UAVX_ACTOR_OK;
}

int uavx_clip_step(int groups, const uavx_clip_group *g, double *partials, int64_t partials_bytes, const float *max_norm,
                   uavx_clip_record *rec, void *stream) {
    if (groups < 1 || groups > UAVX_CLIP_MAX_GROUPS || !g) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (!partials || !max_norm || !rec || !aligned(partials, 8) || !aligned(max_norm, 8) || !aligned(rec, 8))
        return UAVX_ACTOR_ERR_INVALID_ARG;
    static thread_local Table tabs[UAVX_CLIP_MAX_GROUPS];
    static thread_local NormTable norms[UAVX_CLIP_MAX_GROUPS];
    int64_t blocks[UAVX_CLIP_MAX_GROUPS], total = 0;
    for (int k = 0; k < groups; ++k) {
        tabs[k] = Table{};
        norms[k] = NormTable{};
        if (!fill(g[k], tabs[k], norms[k], blocks[k])) return UAVX_ACTOR_ERR_INVALID_ARG;
        tabs[k].rec = rec;
        norms[k].partials = partials + total;
        total += blocks[k];                      // <= 16 · 16 · 2^21
    }
    if (partials_bytes < total * (int64_t)sizeof(double)) return UAVX_ACTOR_ERR_INVALID_ARG;
    const hipStream_t st = (hipStream_t)stream;
    int rc = UAVX_ACTOR_OK;
    for (int k = 0; k < groups && rc == UAVX_ACTOR_OK; ++k) rc = launch(sumsq, blocks[k], WG, st, norms[k]);
    for (int k = 0; k < groups && rc == UAVX_ACTOR_OK; ++k) {
        if (k == 0)
            rc = launch(finish, 1, WG, st, (const double *)partials, total, max_norm, rec, g[k].step, g[k].scalars, g[k].lr,
                        g[k].beta1, g[k].beta2);
        else
            rc = launch(adam_prologue, 1, 64, st, g[k].step, g[k].scalars, g[k].lr, g[k].beta1, g[k].beta2);
        if (rc == UAVX_ACTOR_OK) rc = launch(update, blocks[k], WG, st, tabs[k]);
    }
    return rc;
}

}  // extern "C"

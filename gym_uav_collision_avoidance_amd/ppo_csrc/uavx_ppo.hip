// PPO's sampling and loss heads (include/uavx_ppo.h): what lies between the networks' GEMMs, as one launch
// (sample) and two (loss).
//
//   sample   one thread per row: σ = expf(ℓ), u = μ + σ·ε, a = tanhf(u), log π of the stored u.
//   rows     one thread per minibatch row: gathers the row's u, log π_old, adv, ret and weight through idx, writes the
//            ratio, and the workgroup leaves its four float64 sums (w, w·surr, w·q, w·log π) in partial[k][workgroup].
//   grads    every workgroup totals the weights itself (same order, same bits) -> D; its threads evaluate their rows
//            again -- the same device function on the same inputs, so the same bits -- and write the three gradients.
//            Workgroup 0 totals the other three sums and writes the scalars.
//
// Built with -ffp-contract=off: every operation is one rounding.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/uavx_ppo.h"
#include "../common_csrc/uavx_block_reduce.hpp"
#include "../common_csrc/uavx_entry.hpp"

namespace uavx_ppo_k {

using namespace uavx_common;

constexpr int WG = UAVX_PPO_BLOCK, WAVES = WG / WAVE;
static_assert(WG == 256, "the header documents four wavefronts per workgroup");
constexpr float HALF_LOG_2PI = 0.91893853320467274178f, LOG_2 = 0.69314718055994530942f;

// one action dimension of the log density; leaves z and expf(−ℓ) for the gradients
__device__ inline float log_pi_dim(float mu, float l, float u, float &z, float &inv) {
    inv = expf(-l);
    z = (u - mu) * inv;
    const float gauss = (((-0.5f * z) * z) - l) - HALF_LOG_2PI;
    const float x = -2.0f * u;
    const float sp = fmaxf(x, 0.0f) + log1pf(expf(-fabsf(x)));
    const float squash = 2.0f * ((LOG_2 - u) - sp);
    return gauss - squash;
}

struct Density {
    float logp, z0, z1, inv0, inv1;
};

__device__ inline Density log_pi(float2 mu, float2 l, float2 u) {
    Density d;
    const float t0 = log_pi_dim(mu.x, l.x, u.x, d.z0, d.inv0);
    const float t1 = log_pi_dim(mu.y, l.y, u.y, d.z1, d.inv1);
    d.logp = t0 + t1;
    return d;
}

__global__ __launch_bounds__(WG) void sample(const float2 *__restrict__ mean, const float2 *__restrict__ log_std,
                                              const float2 *__restrict__ eps, int32_t rows, float2 *__restrict__ u_out,
                                              float *__restrict__ logp_out, float2 *__restrict__ action_out) {
    const int64_t b = (int64_t)blockIdx.x * WG + threadIdx.x;
    if (b >= rows) return;
    const float2 mu = mean[b], l = log_std[b], e = eps[b];
    float2 u, a;
    u.x = mu.x + expf(l.x) * e.x;
    u.y = mu.y + expf(l.y) * e.y;
    a.x = tanhf(u.x);
    a.y = tanhf(u.y);
    u_out[b] = u;
    action_out[b] = a;
    logp_out[b] = log_pi(mu, l, u).logp;
}

struct Args {
    const float2 *mean;
    const float2 *log_std;
    const float *v;
    const int64_t *idx;        // NULL: the identity
    const float2 *u;
    const float *logp_old;
    const float *adv;
    const float *ret;
    const float *weight;
    float *ratio;
    float *scalars;
    float2 *g_mean;
    float2 *g_log_std;
    float *g_v;
    double *partial;           // workspace: [4][blocks] float64 -- w, w·surr, w·q, w·log π
    int32_t B;
    int32_t blocks;
    float lo, hi;              // the clip band
    float vf_coef, ent_coef;
};

// everything of a row that both launches need
struct Row {
    Density d;
    float r, a, w, dv;         // ratio, advantage, weight, v − ret
    float surr;
    bool pass;
};

__device__ inline Row row(const Args &a, int64_t b) {
    const int64_t j = a.idx ? a.idx[b] : b;
    Row x;
    x.d = log_pi(a.mean[b], a.log_std[b], a.u[j]);
    x.r = expf(x.d.logp - a.logp_old[j]);
    x.a = a.adv[j];
    x.w = a.weight[j];
    x.dv = a.v[b] - a.ret[j];
    const float s1 = x.r * x.a;
    const float s2 = fminf(fmaxf(x.r, a.lo), a.hi) * x.a;
    x.surr = s1 < s2 ? s1 : s2;
    x.pass = (a.lo <= x.r && x.r <= a.hi) || s1 < s2;
    return x;
}

__global__ __launch_bounds__(WG) void rows(const Args a) {
    __shared__ double part[4][WAVES];
    const int64_t b = (int64_t)blockIdx.x * WG + threadIdx.x;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    if (b < a.B) {
        const Row x = row(a, b);
        a.ratio[b] = x.r;
        const double w = (double)x.w;
        s[0] = w;
        s[1] = w * (double)x.surr;
        s[2] = w * (double)(0.5f * (x.dv * x.dv));
        s[3] = w * (double)x.d.logp;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double t = block_sum<WG>(s[k], part[k]);
        if (threadIdx.x == 0) a.partial[(int64_t)k * a.blocks + blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(WG) void grads(const Args a) {
    __shared__ double part[4][WAVES];
    const double W = total<WG>(a.partial, a.blocks, part[0]);
    const double D = W < 1.0 ? 1.0 : W;           // max(1, W); a NaN W stays a NaN, as under torch's clamp
    if (blockIdx.x == 0) {                         // uniform over the workgroup
        const double S = total<WG>(a.partial + a.blocks, a.blocks, part[1]);
        const double Q = total<WG>(a.partial + 2 * (int64_t)a.blocks, a.blocks, part[2]);
        const double P = total<WG>(a.partial + 3 * (int64_t)a.blocks, a.blocks, part[3]);
        if (threadIdx.x == 0) {
            a.scalars[0] = (float)(-S / D);
            a.scalars[1] = (float)(Q / D);
            a.scalars[2] = (float)(-P / D);
            a.scalars[3] = (float)W;
        }
    }
    const int64_t b = (int64_t)blockIdx.x * WG + threadIdx.x;
    if (b >= a.B) return;
    const Row x = row(a, b);
    const float k = (float)((double)x.w / D);
    const float g_lp = k * (a.ent_coef - (x.pass ? x.a * x.r : 0.0f));
    float2 gm, gl;
    gm.x = (g_lp * x.d.z0) * x.d.inv0;
    gm.y = (g_lp * x.d.z1) * x.d.inv1;
    gl.x = g_lp * ((x.d.z0 * x.d.z0) - 1.0f);
    gl.y = g_lp * ((x.d.z1 * x.d.z1) - 1.0f);
    a.g_mean[b] = gm;
    a.g_log_std[b] = gl;
    a.g_v[b] = (k * a.vf_coef) * x.dv;
}

static bool count(int64_t n) { return n >= 1 && n <= INT32_MAX; }

static bool coefficient(double x) { return x >= 0.0 && x <= 1.7976931348623157e308; }     // false for NaN and inf

}  // namespace uavx_ppo_k

using namespace uavx_ppo_k;

extern "C" {

UAVX_BUILD_MARKER(UAVX_PPO_SRC_HASH);

int uavx_ppo_version(void) { return UAVX_PPO_VERSION; }

int uavx_ppo_sample(const float *mean, const float *log_std, const float *eps, int64_t rows_, float *u_out, float *logp_out,
                    float *action_out, void *stream) {
    if (!count(rows_)) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (!mean || !log_std || !eps || !u_out || !logp_out || !action_out) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (!aligned(mean, 8) || !aligned(log_std, 8) || !aligned(eps, 8) || !aligned(u_out, 8) || !aligned(action_out, 8) ||
        !aligned(logp_out, 4))
        return UAVX_ACTOR_ERR_INVALID_ARG;
    return launch(sample, (rows_ + WG - 1) / WG, WG, (hipStream_t)stream, (const float2 *)mean, (const float2 *)log_std,
                  (const float2 *)eps, (int32_t)rows_, (float2 *)u_out, logp_out, (float2 *)action_out);
}

int uavx_ppo_loss_workspace_bytes(int64_t B, int64_t *bytes) {
    if (!bytes || !count(B)) return UAVX_ACTOR_ERR_INVALID_ARG;
    *bytes = ((B + WG - 1) / WG) * 32;
    return UAVX_ACTOR_OK;
}

int uavx_ppo_loss(const float *mean, const float *log_std, const float *v, const int64_t *idx, int64_t B, const float *u,
                  const float *logp_old, const float *adv, const float *ret, const float *weight, int64_t R, double clip,
                  double vf_coef, double ent_coef, float *ratio, float *scalars, float *g_mean, float *g_log_std, float *g_v,
                  void *workspace, int64_t workspace_bytes, void *stream) {
    if (!count(B) || !count(R) || (!idx && B > R)) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (!mean || !log_std || !v || !u || !logp_old || !adv || !ret || !weight) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (!ratio || !scalars || !g_mean || !g_log_std || !g_v || !workspace) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (!aligned(mean, 8) || !aligned(log_std, 8) || !aligned(u, 8) || !aligned(g_mean, 8) || !aligned(g_log_std, 8) ||
        !aligned(idx, 8) || !aligned(workspace, 8))
        return UAVX_ACTOR_ERR_INVALID_ARG;
    if (!aligned(v, 4) || !aligned(logp_old, 4) || !aligned(adv, 4) || !aligned(ret, 4) || !aligned(weight, 4) ||
        !aligned(ratio, 4) || !aligned(scalars, 4) || !aligned(g_v, 4))
        return UAVX_ACTOR_ERR_INVALID_ARG;
    if (!(clip > 0.0) || !coefficient(clip) || !coefficient(vf_coef) || !coefficient(ent_coef)) return UAVX_ACTOR_ERR_INVALID_ARG;
    const int64_t blocks = (B + WG - 1) / WG;
    if (workspace_bytes < blocks * 32) return UAVX_ACTOR_ERR_INVALID_ARG;
    Args a{};
    a.mean = (const float2 *)mean;
    a.log_std = (const float2 *)log_std;
    a.v = v;
    a.idx = idx;
    a.u = (const float2 *)u;
    a.logp_old = logp_old;
    a.adv = adv;
    a.ret = ret;
    a.weight = weight;
    a.ratio = ratio;
    a.scalars = scalars;
    a.g_mean = (float2 *)g_mean;
    a.g_log_std = (float2 *)g_log_std;
    a.g_v = g_v;
    a.partial = (double *)workspace;
    a.B = (int32_t)B;
    a.blocks = (int32_t)blocks;
    a.lo = (float)(1.0 - clip);
    a.hi = (float)(1.0 + clip);
    a.vf_coef = (float)vf_coef;
    a.ent_coef = (float)ent_coef;
    const hipStream_t st = (hipStream_t)stream;
    const int rc = launch(rows, blocks, WG, st, a);
    return rc != UAVX_ACTOR_OK ? rc : launch(grads, blocks, WG, st, a);
}

}  // extern "C"

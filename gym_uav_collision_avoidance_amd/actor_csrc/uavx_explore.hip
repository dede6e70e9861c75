// The exploration launch (include/uavx_explore.h): warm-up and random actions, SAC / TD3 Gaussian action noise and DDPG's
// Ornstein-Uhlenbeck process behind the RAW output of uavx_actor_forward.  DESIGN.md §20.
//
//   act    one thread per row, 256-thread workgroups, no LDS, no barriers, no atomics.  A thread issues every load of its row
//          (the 16-byte state, the raw row, the flag byte, the fed normals, the probability slot) before the Philox rounds
//          and the arithmetic that wait for them, and ends with at most three vector stores.
//
// The unit is built with -ffp-contract=off: every operation below is one rounding.  tanhf and expf are the calls of
// uavx_actor.hip's SAC_SAMPLE / ADD_CLAMP epilogues on the same operands, so a row fed the same noise is bit-equal to them;
// log, sqrt, cos and sin on doubles are float64.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/uavx_explore.h"
#include "uavx_actor_impl.hpp"

namespace uavx_explore_k {

using uavx_actor_k::clampf;

constexpr int BLOCK = 256;

struct alignas(16) Row {
    double x;
    uint32_t n, reserved;
};
static_assert(sizeof(Row) == UAVX_EXPLORE_STATE_BYTES, "one 16-byte load and store per row");
struct alignas(16) Pair {
    double a, b;
};

struct Args {
    const float *raw;
    float *out;
    Row *state;
    const Pair *normals;
    Pair *normals_out;
    const uint8_t *flags;
    const float *prob_dev;
    int64_t raw_stride, out_stride, flag_stride, warmup;
    uint64_t row_offset;
    double s, theta, dt, mean, x_initial;     // s = sigma·sqrt(dt)
    uint32_t rows, rows_per_env, flag_mask, k0, k1;
    float prob, noise_std;
};

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t w[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

template <int KIND>
__global__ __launch_bounds__(BLOCK) void act(const Args a) {
    const uint32_t row = blockIdx.x * BLOCK + threadIdx.x;
    if (row >= a.rows) return;
    // every load of the row, before anything waits
    Row st = a.state[row];
    float y0, y1, l0 = 0.f, l1 = 0.f;
    if (KIND == UAVX_ACTOR_SAC) {
        const float4 v = *reinterpret_cast<const float4 *>(a.raw + (int64_t)row * a.raw_stride);
        y0 = v.x; y1 = v.y; l0 = v.z; l1 = v.w;
    } else {
        const float2 v = *reinterpret_cast<const float2 *>(a.raw + (int64_t)row * a.raw_stride);
        y0 = v.x; y1 = v.y;
    }
    const uint32_t flag = a.flags ? a.flags[(int64_t)(row / a.rows_per_env) * a.flag_stride] : 0u;
    Pair nz{0.0, 0.0};
    if (a.normals) nz = a.normals[row];
    const float p = a.prob_dev ? *a.prob_dev : a.prob;

    const uint64_t g = a.row_offset + row;
    uint32_t w[4];
    philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), st.n, 0u, a.k0, a.k1, w);
    constexpr double INV32 = 1.0 / 4294967296.0;
    if (!a.normals) {
        const double u1 = ((double)w[0] + 1.0) * INV32, u2 = (double)w[1] * INV32;
        const double r = sqrt(-2.0 * log(u1)), t = 6.283185307179586 * u2;
        nz.a = r * cos(t);
        nz.b = r * sin(t);
    }
    if (flag & a.flag_mask) st.x = a.x_initial;
    bool random = (int64_t)st.n < a.warmup;
    if (!random && p > 0.f) {
        uint32_t b[4];
        philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), st.n, 1u, a.k0, a.k1, b);
        random = (double)b[0] * INV32 < (double)p;
    }
    float2 o;
    if (random) {
        o.x = (float)(-1.0 + 2.0 * ((double)w[2] * INV32));
        o.y = (float)(-1.0 + 2.0 * ((double)w[3] * INV32));
    } else if (KIND == UAVX_ACTOR_SAC) {
        o.x = tanhf(y0 + expf(l0) * (float)nz.a);
        o.y = tanhf(y1 + expf(l1) * (float)nz.b);
    } else if (KIND == UAVX_ACTOR_TD3) {
        o.x = clampf(tanhf(y0) + a.noise_std * (float)nz.a, -1.f, 1.f);
        o.y = clampf(tanhf(y1) + a.noise_std * (float)nz.b, -1.f, 1.f);
    } else {
        st.x = (st.x + (a.theta * (a.mean - st.x)) * a.dt) + a.s * nz.a;
        o.x = (float)fmin(fmax((double)tanhf(y0) + st.x, -1.0), 1.0);
        o.y = (float)fmin(fmax((double)tanhf(y1) + st.x, -1.0), 1.0);
    }
    st.n += 1u;
    a.state[row] = st;
    *reinterpret_cast<float2 *>(a.out + (int64_t)row * a.out_stride) = o;
    if (a.normals_out) a.normals_out[row] = nz;
}

static bool aligned(const void *p, uintptr_t n) { return ((uintptr_t)p & (n - 1)) == 0; }
static bool nonneg(double v) { return v >= 0.0 && isfinite(v); }

}  // namespace uavx_explore_k

using namespace uavx_explore_k;

extern "C" {

int uavx_explore_version(void) { return UAVX_EXPLORE_VERSION; }

int uavx_explore_act(const uavx_explore_args *g, void *stream) {
    if (!g) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (g->kind != UAVX_ACTOR_SAC && g->kind != UAVX_ACTOR_TD3 && g->kind != UAVX_ACTOR_DDPG) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (g->rows < 1 || g->rows > UAVX_EXPLORE_MAX_ROWS || g->row_offset < 0 || g->warmup_steps < 0)
        return UAVX_ACTOR_ERR_INVALID_ARG;
    if (!g->raw || !g->out || !g->state) return UAVX_ACTOR_ERR_INVALID_ARG;
    const int cols = g->kind == UAVX_ACTOR_SAC ? 4 : 2;
    if (!aligned(g->state, 16) || !aligned(g->raw, 4 * cols) || g->raw_stride < cols || g->raw_stride % cols)
        return UAVX_ACTOR_ERR_INVALID_ARG;
    if (!aligned(g->out, 8) || g->out_stride < 2 || g->out_stride % 2) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (g->raw_stride > INT64_MAX / UAVX_EXPLORE_MAX_ROWS || g->out_stride > INT64_MAX / UAVX_EXPLORE_MAX_ROWS)
        return UAVX_ACTOR_ERR_INVALID_ARG;
    if (!aligned(g->normals, 16) || !aligned(g->normals_out, 16) || !aligned(g->random_prob_dev, 4))
        return UAVX_ACTOR_ERR_INVALID_ARG;
    if (!(g->random_prob >= 0.f && g->random_prob <= 1.f)) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (!nonneg(g->noise_std) || !nonneg(g->ou_sigma) || !nonneg(g->ou_dt)) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (!isfinite(g->ou_theta) || !isfinite(g->ou_mean) || !isfinite(g->ou_x_initial)) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (g->reset_flags) {
        if (g->rows_per_env < 1 || g->rows % g->rows_per_env != 0) return UAVX_ACTOR_ERR_INVALID_ARG;
        if (g->reset_mask < 1 || g->reset_mask > 255) return UAVX_ACTOR_ERR_INVALID_ARG;
        if (g->reset_stride < 1 || g->reset_stride > INT64_MAX / UAVX_EXPLORE_MAX_ROWS) return UAVX_ACTOR_ERR_INVALID_ARG;
    }
    Args a{};
    a.raw = g->raw;
    a.out = g->out;
    a.state = static_cast<Row *>(g->state);
    a.normals = reinterpret_cast<const Pair *>(g->normals);
    a.normals_out = reinterpret_cast<Pair *>(g->normals_out);
    a.flags = g->reset_flags;
    a.prob_dev = g->random_prob_dev;
    a.raw_stride = g->raw_stride;
    a.out_stride = g->out_stride;
    a.flag_stride = g->reset_flags ? g->reset_stride : 0;
    a.warmup = g->warmup_steps;
    a.row_offset = (uint64_t)g->row_offset;
    a.s = g->ou_sigma * sqrt(g->ou_dt);
    a.theta = g->ou_theta;
    a.dt = g->ou_dt;
    a.mean = g->ou_mean;
    a.x_initial = g->ou_x_initial;
    a.rows = (uint32_t)g->rows;
    a.rows_per_env = g->reset_flags ? (uint32_t)g->rows_per_env : 1u;
    a.flag_mask = g->reset_flags ? (uint32_t)g->reset_mask : 0u;
    a.k0 = (uint32_t)g->seed;
    a.k1 = (uint32_t)(g->seed >> 32);
    a.prob = g->random_prob;
    a.noise_std = g->noise_std;
    const dim3 grid((uint32_t)((g->rows + BLOCK - 1) / BLOCK)), block(BLOCK);
    hipStream_t s = (hipStream_t)stream;
    if (g->kind == UAVX_ACTOR_SAC) hipLaunchKernelGGL(act<UAVX_ACTOR_SAC>, grid, block, 0, s, a);
    else if (g->kind == UAVX_ACTOR_TD3) hipLaunchKernelGGL(act<UAVX_ACTOR_TD3>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(act<UAVX_ACTOR_DDPG>, grid, block, 0, s, a);
    return hipGetLastError() == hipSuccess ? UAVX_ACTOR_OK : UAVX_ACTOR_ERR_HIP;
}

}  // extern "C"

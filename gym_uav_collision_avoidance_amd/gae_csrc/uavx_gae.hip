// GAE(λ) over the device ring and its normalisation (include/uavx_gae.h) as one or three launches.
//
//   1. walk        one thread per column q = e·N + i, adjacent lanes adjacent columns: every row access is one coalesced
//                  run in the time-major ring.  The thread walks its column's window newest to oldest.  What a row needs
//                  from memory (reward, done byte, value, the env's flags) does not depend on the carry, so the rows are
//                  fetched ROWS at a time, and the next group is in flight while the recurrence runs over this one: the
//                  dependent chain per row is a multiply and an add in float64, not a memory round trip.  V[s1] and
//                  skip(k+1) are what the previous row loaded.  With adv_norm the thread also sums its column's valid
//                  advantages and the workgroup leaves sum[blk] and cnt[blk].
//   2. spread      every workgroup totals sum[] and cnt[] itself (same order, same bits), forms the mean, and its threads
//                  sum (a − mean)² over their columns in the walk's order -> sq[blk].  Workgroup 0 writes stats n, mean.
//   3. normalise   every workgroup totals sq[] itself, forms std, and its threads write adv_norm over their columns.
//                  Workgroup 0 writes stats std.
//
// Built with -ffp-contract=off: every operation is one rounding; `/` and sqrt in float64 are correctly rounded.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/uavx_gae.h"
#include "../common_csrc/uavx_block_reduce.hpp"
#include "../common_csrc/uavx_entry.hpp"
#include "../common_csrc/uavx_ring_view.hpp"

namespace uavx_gae_k {

using namespace uavx_common;

constexpr int WG = UAVX_GAE_BLOCK, WAVES = WG / WAVE, ROWS = 8;
static_assert(WG == 256, "the header documents four wavefronts per workgroup");

struct Args : RingView {
    const float *values;
    float *adv;
    float *ret;
    uint8_t *valid;
    float *adv_norm;           // NULL: no normalisation
    uavx_gae_stats *stats;
    double *sum;               // workspace: blocks float64, blocks float64, blocks int64
    double *sq;
    long long *cnt;
    int32_t first;             // slot of step count − 1
    int32_t boot;              // slot of the state after it: count mod slots
    int32_t steps;
    double gamma, gl;          // γ and γ·λ
};

struct Rows {
    float r[ROWS], v[ROWS];
    uint32_t d[ROWS], f[ROWS];     // done byte; bit 0 skip, bit 1 ended
};

// loads rows s, s − 1, ... (n of them, wrapping) of column `col` of env `e`; leaves s at the row after the last
__device__ inline void fetch(const Args &a, Rows &b, int32_t &s, int n, int32_t col, int32_t e) {
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
        if (j < n) {
            const int64_t off = (int64_t)s * a.plane + col;
            b.r[j] = a.rew[off];
            b.v[j] = a.values[off];
            b.d[j] = a.done[off];
            b.f[j] = flags(a, s, e);
            s = prev_slot(a, s);
        }
    }
}

__global__ __launch_bounds__(WG) void walk(const Args a) {
    __shared__ double psum[WAVES];
    __shared__ long long pcnt[WAVES];
    const Column c = column<WG>(a);
    const int32_t col = c.col, e = c.e;
    double sum = 0.0;
    long long cnt = 0;
    if (c.learn) {
        Rows cur, nxt{};
        int32_t s = a.first, out = a.first, left = a.steps;
        fetch(a, cur, s, left < ROWS ? left : ROWS, col, e);
        float vnext = a.values[(int64_t)a.boot * a.plane + col];
        bool cut = true;           // k + 1 >= count at the newest row; afterwards skip(k + 1, e)
        double carry = 0.0;
        while (left > 0) {
            const int n = left < ROWS ? left : ROWS;
            left -= n;
            if (left > 0) fetch(a, nxt, s, left < ROWS ? left : ROWS, col, e);
#pragma unroll
            for (int j = 0; j < ROWS; ++j) {
                if (j < n) {
                    const int64_t off = (int64_t)out * a.plane + col;
                    const double v = (double)cur.v[j];
                    float fa = 0.f, fr = 0.f;
                    const bool skip = cur.f[j] & 1u;
                    if (skip) {
                        carry = 0.0;
                    } else {
                        const bool d = cur.d[j] & 1u;
                        const double b = d ? 0.0 : a.gamma * (double)vnext;
                        const double delta = ((double)cur.r[j] + b) - v;
                        const bool stop = d || (cur.f[j] & 2u) || cut;
                        const double A = stop ? delta : delta + a.gl * carry;
                        fa = (float)A;
                        fr = (float)(A + v);
                        carry = A;
                        sum += (double)fa;
                        ++cnt;
                    }
                    a.adv[off] = fa;
                    a.ret[off] = fr;
                    a.valid[off] = skip ? 0 : 1;
                    cut = skip;
                    vnext = cur.v[j];
                    out = prev_slot(a, out);
                }
            }
            cur = nxt;
        }
    } else if (c.in) {
        int32_t out = a.first;
        for (int32_t j = 0; j < a.steps; ++j) {
            const int64_t off = (int64_t)out * a.plane + col;
            a.adv[off] = 0.f;
            a.ret[off] = 0.f;
            a.valid[off] = 0;
            out = prev_slot(a, out);
        }
    }
    if (!a.adv_norm) return;       // uniform over the launch
    const double S = block_sum<WG>(sum, psum);
    const long long C = block_sum<WG>(cnt, pcnt);
    if (threadIdx.x == 0) {
        a.sum[blockIdx.x] = S;
        a.cnt[blockIdx.x] = C;
    }
}

__global__ __launch_bounds__(WG) void spread(const Args a) {
    __shared__ double psum[WAVES], psq[WAVES];
    __shared__ long long pcnt[WAVES];
    const long long n = total<WG>(a.cnt, a.blocks, pcnt);
    const double S = total<WG>(a.sum, a.blocks, psum);
    const double mean = n > 0 ? S / (double)n : 0.0;
    const Column c = column<WG>(a);
    const int32_t col = c.col;
    double sq = 0.0;
    if (c.learn) {
        const float *__restrict__ adv = a.adv;
        const uint8_t *__restrict__ valid = a.valid;
        int32_t s = a.first;
        for (int32_t j0 = 0; j0 < a.steps; j0 += ROWS) {     // ROWS rows' loads in flight, summed in the walk's order
            float x[ROWS];
            uint32_t v[ROWS];
#pragma unroll
            for (int j = 0; j < ROWS; ++j) {
                v[j] = 0;
                if (j0 + j < a.steps) {
                    const int64_t off = (int64_t)s * a.plane + col;
                    x[j] = adv[off];
                    v[j] = valid[off];
                    s = prev_slot(a, s);
                }
            }
#pragma unroll
            for (int j = 0; j < ROWS; ++j) {
                if (v[j]) {
                    const double dev = (double)x[j] - mean;
                    sq += dev * dev;
                }
            }
        }
    }
    const double Q = block_sum<WG>(sq, psq);
    if (threadIdx.x != 0) return;
    a.sq[blockIdx.x] = Q;
    if (blockIdx.x == 0) {
        a.stats->n = n;
        a.stats->mean = mean;
    }
}

__global__ __launch_bounds__(WG) void normalise(const Args a) {
    __shared__ double psq[WAVES];
    const double Q = total<WG>(a.sq, a.blocks, psq);
    const long long n = a.stats->n;
    const double mean = a.stats->mean;
    const double std = n >= 2 ? sqrt(Q / (double)(n - 1)) : 0.0;
    const double denom = std + 1e-8;
    if (blockIdx.x == 0 && threadIdx.x == 0) a.stats->std = std;
    const Column c = column<WG>(a);
    if (!c.in) return;
    const int32_t col = c.col;
    const float *__restrict__ adv = a.adv;
    const uint8_t *__restrict__ valid = a.valid;
    float *__restrict__ out = a.adv_norm;
    int32_t s = a.first;
    for (int32_t j0 = 0; j0 < a.steps; j0 += ROWS) {         // ROWS rows' loads in flight ahead of their stores
        float x[ROWS];
        uint32_t v[ROWS];
        int64_t off[ROWS];
#pragma unroll
        for (int j = 0; j < ROWS; ++j) {
            if (j0 + j < a.steps) {
                off[j] = (int64_t)s * a.plane + col;
                x[j] = adv[off[j]];
                v[j] = valid[off[j]];
                s = prev_slot(a, s);
            }
        }
#pragma unroll
        for (int j = 0; j < ROWS; ++j)
            if (j0 + j < a.steps) out[off[j]] = v[j] ? (float)(((double)x[j] - mean) / denom) : 0.f;
    }
}

}  // namespace uavx_gae_k

using namespace uavx_gae_k;

extern "C" {

UAVX_BUILD_MARKER(UAVX_GAE_SRC_HASH);

int uavx_gae_version(void) { return UAVX_GAE_VERSION; }

int uavx_gae_workspace_bytes(const uavx_gae_ring *ring, int64_t *bytes) {
    int64_t blocks = 0;
    if (!bytes || !plan<WG>(ring, blocks)) return UAVX_ACTOR_ERR_INVALID_ARG;
    *bytes = blocks * 24;
    return UAVX_ACTOR_OK;
}

int uavx_gae_compute(const uavx_gae_ring *ring, const float *values, int64_t count, int64_t steps, double gamma,
                     double lambda, float *adv, float *ret, uint8_t *valid, float *adv_norm, uavx_gae_stats *stats,
                     void *workspace, int64_t workspace_bytes, void *stream) {
    Args a{};
    if (!ring_view<WG>(ring, a)) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (!a.rew || !values || !adv || !ret || !valid) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (!aligned(a.rew, 4) || !aligned(values, 4) || !aligned(adv, 4) || !aligned(ret, 4) || !aligned(adv_norm, 4))
        return UAVX_ACTOR_ERR_INVALID_ARG;
    if (count < 1 || steps < 1 || steps > count || steps > a.slots - 1) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (!unit(gamma) || !unit(lambda)) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (adv_norm) {
        if (!stats || !workspace || !aligned(stats, 8) || !aligned(workspace, 8)) return UAVX_ACTOR_ERR_INVALID_ARG;
        if (workspace_bytes < (int64_t)a.blocks * 24) return UAVX_ACTOR_ERR_INVALID_ARG;
    }
    a.values = values;
    a.adv = adv;
    a.ret = ret;
    a.valid = valid;
    a.adv_norm = adv_norm;
    a.stats = stats;
    a.sum = (double *)workspace;
    a.sq = a.sum + a.blocks;
    a.cnt = (long long *)(a.sq + a.blocks);
    a.first = (int32_t)((count - 1) % a.slots);
    a.boot = (int32_t)(count % a.slots);
    a.steps = (int32_t)steps;
    a.gamma = gamma;
    a.gl = gamma * lambda;
    const hipStream_t st = (hipStream_t)stream;
    int rc = launch(walk, a.blocks, WG, st, a);
    if (rc == UAVX_ACTOR_OK && adv_norm) rc = launch(spread, a.blocks, WG, st, a);
    if (rc == UAVX_ACTOR_OK && adv_norm) rc = launch(normalise, a.blocks, WG, st, a);
    return rc;
}

}  // extern "C"

// Running observation and return statistics over the device ring and the two calls that apply them (include/uavx_norm.h,
// DESIGN.md §30).  A fold is three launches, an apply call one.
//
//   1. first pass   one thread per column q = e·N + i, adjacent lanes adjacent columns, walking its column's steps oldest to
//                   newest.  Returns: what a row needs from memory (reward, done byte, the env's flags) does not depend on
//                   the carry, so the rows are fetched ROWS at a time and the next group is in flight while the recurrence
//                   runs over this one (as uavx_gae.hip's walk; the dependent chain per row is a multiply and an add in
//                   float64).  Observations: a thread reads the F consecutive floats of its row -- a wavefront's lanes cover
//                   one contiguous run -- OROWS rows' loads in flight, into F accumulators.  The workgroup leaves sum[f][blk]
//                   and cnt[blk].
//   2. second pass  every workgroup totals sum[] and cnt[] itself (same order, same bits), forms the batch mean, and its
//                   threads sum the squared deviations in the first pass's order -> sq[f][blk].  The returns walk starts
//                   again from the carry the call found and stores the new carry at its end.
//   3. merge        ONE workgroup totals cnt[], sum[] and sq[]; thread f merges feature f into the record (Chan's update).
//
// Built with -ffp-contract=off: every operation is one rounding; `/` and sqrt in float64 are correctly rounded.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/uavx_norm.h"
#include "../common_csrc/uavx_block_reduce.hpp"
#include "../common_csrc/uavx_entry.hpp"
#include "../common_csrc/uavx_ring_view.hpp"

namespace uavx_norm_k {

using namespace uavx_common;

constexpr int WG = UAVX_NORM_BLOCK, WAVES = WG / WAVE, ROWS = 8, OROWS = 4, MAXF = UAVX_NORM_MAX_FEATURES;
static_assert(WG == 256, "the header documents four wavefronts per workgroup");

struct Fold : RingView {
    const float *obs;
    double *carry;
    uavx_norm_record *rec;
    double *sum;               // workspace: features × blocks float64, the same again, blocks int64
    double *sq;
    long long *cnt;
    int32_t start;             // slot of step first
    int32_t prev;              // slot of step first − 1; −1 when first = 0
    int32_t steps;
    int32_t features;
    double gamma;
};

// does the row before the fold's first park this column's agent in the fold's first row?
__device__ inline bool parked_at_first(const Fold &a, int32_t col, int32_t e) {
    if (a.prev < 0) return false;
    const uint32_t d = a.done[(int64_t)a.prev * a.plane + col];
    return (d & 1u) && !(flags(a, a.prev, e) & 3u);
}

// ---- returns ---------------------------------------------------------------------------------------------------------------

struct Rows {
    float r[ROWS];
    uint32_t d[ROWS], f[ROWS];     // done byte; bit 0 skip, bit 1 ended
};

// loads rows s, s + 1, ... (n of them, wrapping) of column `col` of env `e`; leaves s at the row after the last
__device__ inline void fetch(const Fold &a, Rows &b, int32_t &s, int n, int32_t col, int32_t e) {
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
        if (j < n) {
            const int64_t off = (int64_t)s * a.plane + col;
            b.r[j] = a.rew[off];
            b.d[j] = a.done[off];
            b.f[j] = flags(a, s, e);
            s = next_slot(a, s);
        }
    }
}

// the forward walk of one column from the carry in memory: SECOND = false sums R and counts, SECOND = true sums (R − mean)².
// Returns the carry after the newest row.
template <bool SECOND>
__device__ inline double walk(const Fold &a, int32_t col, int32_t e, double mean, double &acc, long long &cnt) {
    Rows cur, nxt{};
    int32_t s = a.start, left = a.steps;
    fetch(a, cur, s, left < ROWS ? left : ROWS, col, e);
    bool parked = parked_at_first(a, col, e);
    double C = a.carry[col];
    while (left > 0) {
        const int n = left < ROWS ? left : ROWS;
        left -= n;
        if (left > 0) fetch(a, nxt, s, left < ROWS ? left : ROWS, col, e);
#pragma unroll
        for (int j = 0; j < ROWS; ++j) {
            if (j < n) {
                const bool skip = cur.f[j] & 1u, end = cur.f[j] & 2u, d = cur.d[j] & 1u;
                if (skip || parked) {
                    C = 0.0;
                } else {
                    const double R = (double)cur.r[j] + a.gamma * C;
                    if (SECOND) {
                        const double dev = R - mean;
                        acc += dev * dev;
                    } else {
                        acc += R;
                        ++cnt;
                    }
                    C = (d || end) ? 0.0 : R;
                }
                parked = d && !skip && !end;
            }
        }
        cur = nxt;
    }
    return C;
}

__global__ __launch_bounds__(WG) void ret_sum(const Fold a) {
    __shared__ double psum[WAVES];
    __shared__ long long pcnt[WAVES];
    const Column c = column<WG>(a);
    double sum = 0.0;
    long long cnt = 0;
    if (c.learn) walk<false>(a, c.col, c.e, 0.0, sum, cnt);
    const double S = block_sum<WG>(sum, psum);
    const long long N = block_sum<WG>(cnt, pcnt);
    if (threadIdx.x == 0) {
        a.sum[blockIdx.x] = S;
        a.cnt[blockIdx.x] = N;
    }
}

__global__ __launch_bounds__(WG) void ret_sq(const Fold a) {
    __shared__ double psum[WAVES], psq[WAVES];
    __shared__ long long pcnt[WAVES];
    const long long n = total<WG>(a.cnt, a.blocks, pcnt);
    const double S = total<WG>(a.sum, a.blocks, psum);
    const double mean = n > 0 ? S / (double)n : 0.0;
    const Column c = column<WG>(a);
    double sq = 0.0;
    long long unused = 0;
    if (c.learn) a.carry[c.col] = walk<true>(a, c.col, c.e, mean, sq, unused);
    const double Q = block_sum<WG>(sq, psq);
    if (threadIdx.x == 0) a.sq[blockIdx.x] = Q;
}

// ---- observations ----------------------------------------------------------------------------------------------------------

// SECOND = false: sum[f][blk] and cnt[blk]; SECOND = true: sq[f][blk] around the batch mean every workgroup forms itself
template <int F, bool SECOND>
__global__ __launch_bounds__(WG) void obs_pass(const Fold a) {
    __shared__ double part[MAXF][WAVES], tpart[MAXF][WAVES], smean[MAXF];
    __shared__ long long pcnt[WAVES];
    double mean[F];
#pragma unroll
    for (int f = 0; f < F; ++f) mean[f] = 0.0;
    if (SECOND) {
        const long long n = total<WG>(a.cnt, a.blocks, pcnt);
        for (int f = 0; f < F; ++f) {
            const double S = total<WG>(a.sum + (int64_t)f * a.blocks, a.blocks, tpart[f]);
            if (threadIdx.x == 0) smean[f] = n > 0 ? S / (double)n : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int f = 0; f < F; ++f) mean[f] = smean[f];
    }
    const Column c = column<WG>(a);
    double acc[F];
#pragma unroll
    for (int f = 0; f < F; ++f) acc[f] = 0.0;
    long long cnt = 0;
    if (c.learn) {
        const float *__restrict__ obs = a.obs;
        bool parked = parked_at_first(a, c.col, c.e);
        int32_t s = a.start;
        for (int32_t j0 = 0; j0 < a.steps; j0 += OROWS) {    // OROWS rows' loads in flight, summed oldest first
            float x[OROWS][F];
            uint32_t d[OROWS], fl[OROWS];
#pragma unroll
            for (int j = 0; j < OROWS; ++j) {
                d[j] = 0;
                fl[j] = 1u;                                  // rows past the fold's last: no sample
                if (j0 + j < a.steps) {
                    const int64_t off = (int64_t)s * a.plane + c.col;
                    d[j] = a.done[off];
                    fl[j] = flags(a, s, c.e);
                    const float *__restrict__ row = obs + off * F;
#pragma unroll
                    for (int f = 0; f < F; ++f) x[j][f] = row[f];
                    s = next_slot(a, s);
                }
            }
#pragma unroll
            for (int j = 0; j < OROWS; ++j) {
                if (!(fl[j] & 1u) && !parked) {
#pragma unroll
                    for (int f = 0; f < F; ++f) {
                        if (SECOND) {
                            const double dev = (double)x[j][f] - mean[f];
                            acc[f] += dev * dev;
                        } else {
                            acc[f] += (double)x[j][f];
                        }
                    }
                    ++cnt;
                }
                parked = (d[j] & 1u) && !(fl[j] & 3u);
            }
        }
    }
    double *out = SECOND ? a.sq : a.sum;
#pragma unroll
    for (int f = 0; f < F; ++f) {
        const double S = block_sum<WG>(acc[f], part[f]);
        if (threadIdx.x == 0) out[(int64_t)f * a.blocks + blockIdx.x] = S;
    }
    if (!SECOND) {
        const long long N = block_sum<WG>(cnt, pcnt);
        if (threadIdx.x == 0) a.cnt[blockIdx.x] = N;
    }
}

// ---- merge -----------------------------------------------------------------------------------------------------------------

// one workgroup: thread f merges the batch of feature f into the record (returns: one feature, the record's second part)
__global__ __launch_bounds__(WG) void merge(const Fold a, const int returns) {
    __shared__ double psum[MAXF][WAVES], psq[MAXF][WAVES];
    __shared__ long long pcnt[WAVES];
    const long long nb = total<WG>(a.cnt, a.blocks, pcnt);
    double S = 0.0, Q = 0.0;
    for (int f = 0; f < a.features; ++f) {
        const double s = total<WG>(a.sum + (int64_t)f * a.blocks, a.blocks, psum[f]);
        const double q = total<WG>(a.sq + (int64_t)f * a.blocks, a.blocks, psq[f]);
        if ((int)threadIdx.x == f) {
            S = s;
            Q = q;
        }
    }
    if (nb <= 0 || (int)threadIdx.x >= a.features) return;       // an empty batch leaves the record's bits alone
    const int f = threadIdx.x;
    int64_t *n = returns ? &a.rec->n_ret : &a.rec->n_obs;
    double *mean = returns ? &a.rec->mean_ret : &a.rec->mean[f];
    double *M2 = returns ? &a.rec->M2_ret : &a.rec->M2[f];
    const long long na = *n, nn = na + nb;
    const double mean_b = S / (double)nb;
    const double delta = mean_b - *mean;
    const double w = (double)nb / (double)nn;
    const double t1 = *M2 + Q, t2 = delta * delta, t3 = (double)na * w;
    *mean = *mean + delta * w;
    *M2 = t1 + t2 * t3;
    // every thread 0 .. F − 1 read n above, within one wavefront (F <= 16): thread 0 stores it after they all have
    __builtin_amdgcn_wave_barrier();
    if (f == 0) *n = nn;
}

// ---- apply -----------------------------------------------------------------------------------------------------------------

struct Apply {
    const uavx_norm_record *rec;
    const float *in;
    float *out;
    int64_t vec;               // float4 groups, one per thread; 0 when in or out is not 16-byte aligned
    int64_t total;             // elements; those from 4·vec on are one per thread
    int32_t features;
    double eps;
    float clip;
};

__device__ inline float clamp(float y, float c) { return y > c ? c : (y < -c ? -c : y); }     // a NaN passes

template <bool RETURNS>
__global__ __launch_bounds__(WG) void apply(const Apply a) {
    __shared__ double smean[MAXF], sden[MAXF];
    if ((int)threadIdx.x < a.features) {
        const int f = threadIdx.x;
        const long long n = RETURNS ? a.rec->n_ret : a.rec->n_obs;
        const double M2 = RETURNS ? a.rec->M2_ret : a.rec->M2[f];
        const double var = n > 0 ? M2 / (double)n : 1.0;
        smean[f] = RETURNS ? 0.0 : (n > 0 ? a.rec->mean[f] : 0.0);
        sden[f] = sqrt(var + a.eps);
    }
    __syncthreads();
    const int64_t t = (int64_t)blockIdx.x * WG + threadIdx.x;
    if (t < a.vec) {
        const float4 x = reinterpret_cast<const float4 *>(a.in)[t];
        const float in[4] = {x.x, x.y, x.z, x.w};
        float out[4];
        int f = RETURNS ? 0 : (int)((t * 4) % a.features);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double z = RETURNS ? (double)in[j] / sden[0] : ((double)in[j] - smean[f]) / sden[f];
            out[j] = clamp((float)z, a.clip);
            if (!RETURNS) f = f + 1 == a.features ? 0 : f + 1;
        }
        reinterpret_cast<float4 *>(a.out)[t] = make_float4(out[0], out[1], out[2], out[3]);
        return;
    }
    const int64_t i = a.vec * 4 + (t - a.vec);
    if (i >= a.total) return;
    const int f = RETURNS ? 0 : (int)(i % a.features);
    const double z = RETURNS ? (double)a.in[i] / sden[0] : ((double)a.in[i] - smean[f]) / sden[f];
    a.out[i] = clamp((float)z, a.clip);
}

// everything the two folds check alike, and the arguments they share
static bool fold_args(const uavx_norm_ring *ring, int64_t features, int64_t first, int64_t count, uavx_norm_record *record,
                      void *workspace, int64_t workspace_bytes, Fold &a) {
    if (!ring_view<WG>(ring, a)) return false;
    const int64_t blocks = a.blocks;
    if (features < 1 || features > MAXF) return false;
    if (first < 0 || count <= first || count - first > a.slots - 1) return false;
    if (!record || !workspace || !aligned(record, 8) || !aligned(workspace, 8)) return false;
    if (workspace_bytes < 8 * (2 * features + 1) * blocks) return false;
    a.rec = record;
    a.sum = (double *)workspace;
    a.sq = a.sum + features * blocks;
    a.cnt = (long long *)(a.sq + features * blocks);
    a.start = (int32_t)(first % a.slots);
    a.prev = first >= 1 ? (int32_t)((first - 1) % a.slots) : -1;
    a.steps = (int32_t)(count - first);
    a.features = (int32_t)features;
    return true;
}

template <int F>
static int launch_obs(const Fold &a, hipStream_t st) {
    const int rc = launch(obs_pass<F, false>, a.blocks, WG, st, a);
    return rc != UAVX_ACTOR_OK ? rc : launch(obs_pass<F, true>, a.blocks, WG, st, a);
}

static int apply_call(bool returns, const uavx_norm_record *record, const float *in, float *out, int64_t total,
                      int64_t features, double eps, double clip, void *stream) {
    if (!record || !in || !out || !aligned(record, 8) || !aligned(in, 4) || !aligned(out, 4)) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (!(eps >= 0.0) || !isfinite(eps) || !(clip > 0.0) || !isfinite(clip)) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (out != in && out < in + total && in < out + total) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (total == 0) return UAVX_ACTOR_OK;
    Apply a{};
    a.rec = record;
    a.in = in;
    a.out = out;
    a.vec = aligned(in, 16) && aligned(out, 16) ? total / 4 : 0;
    a.total = total;
    a.features = (int32_t)features;
    a.eps = eps;
    a.clip = (float)clip;
    const int64_t threads = a.vec + (total - 4 * a.vec);
    return launch(returns ? apply<true> : apply<false>, (threads + WG - 1) / WG, WG, (hipStream_t)stream, a);
}

}  // namespace uavx_norm_k

using namespace uavx_norm_k;

extern "C" {

UAVX_BUILD_MARKER(UAVX_NORM_SRC_HASH);

int uavx_norm_version(void) { return UAVX_NORM_VERSION; }

int uavx_norm_workspace_bytes(const uavx_norm_ring *ring, int64_t features, int64_t *bytes) {
    int64_t blocks = 0;
    if (!bytes || !plan<WG>(ring, blocks) || features < 1 || features > MAXF) return UAVX_ACTOR_ERR_INVALID_ARG;
    *bytes = 8 * (2 * features + 1) * blocks;
    return UAVX_ACTOR_OK;
}

int uavx_norm_fold_obs(const uavx_norm_ring *ring, const float *obs, int64_t features, int64_t first, int64_t count,
                       uavx_norm_record *record, void *workspace, int64_t workspace_bytes, void *stream) {
    Fold a{};
    if (!fold_args(ring, features, first, count, record, workspace, workspace_bytes, a)) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (!obs || !aligned(obs, 4)) return UAVX_ACTOR_ERR_INVALID_ARG;
    a.obs = obs;
    const hipStream_t st = (hipStream_t)stream;
    int rc = UAVX_ACTOR_OK;
    switch (features) {
#define UAVX_NORM_CASE(F) case F: rc = launch_obs<F>(a, st); break;
        UAVX_NORM_CASE(1) UAVX_NORM_CASE(2) UAVX_NORM_CASE(3) UAVX_NORM_CASE(4) UAVX_NORM_CASE(5) UAVX_NORM_CASE(6)
        UAVX_NORM_CASE(7) UAVX_NORM_CASE(8) UAVX_NORM_CASE(9) UAVX_NORM_CASE(10) UAVX_NORM_CASE(11) UAVX_NORM_CASE(12)
        UAVX_NORM_CASE(13) UAVX_NORM_CASE(14) UAVX_NORM_CASE(15) UAVX_NORM_CASE(16)
#undef UAVX_NORM_CASE
    }
    return rc != UAVX_ACTOR_OK ? rc : launch(merge, 1, WG, st, a, 0);
}

int uavx_norm_fold_returns(const uavx_norm_ring *ring, int64_t first, int64_t count, double gamma, double *carry,
                           uavx_norm_record *record, void *workspace, int64_t workspace_bytes, void *stream) {
    Fold a{};
    if (!fold_args(ring, 1, first, count, record, workspace, workspace_bytes, a)) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (!a.rew || !aligned(a.rew, 4) || !carry || !aligned(carry, 8) || !unit(gamma)) return UAVX_ACTOR_ERR_INVALID_ARG;
    a.carry = carry;
    a.gamma = gamma;
    const hipStream_t st = (hipStream_t)stream;
    int rc = launch(ret_sum, a.blocks, WG, st, a);
    if (rc == UAVX_ACTOR_OK) rc = launch(ret_sq, a.blocks, WG, st, a);
    return rc != UAVX_ACTOR_OK ? rc : launch(merge, 1, WG, st, a, 1);
}

int uavx_norm_apply_obs(const uavx_norm_record *record, const float *in, float *out, int64_t rows, int64_t features,
                        double eps, double clip, void *stream) {
    if (features < 1 || features > MAXF || rows < 0 || rows > (INT64_C(1) << 38) / features) return UAVX_ACTOR_ERR_INVALID_ARG;
    return apply_call(false, record, in, out, rows * features, features, eps, clip, stream);
}

int uavx_norm_scale_rewards(const uavx_norm_record *record, const float *in, float *out, int64_t count, double eps,
                            double clip, void *stream) {
    if (count < 0 || count > (INT64_C(1) << 38)) return UAVX_ACTOR_ERR_INVALID_ARG;
    return apply_call(true, record, in, out, count, 1, eps, clip, stream);
}

}  // extern "C"

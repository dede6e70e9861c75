// Replay sampler (include/uavx_replay.h): DeviceReplay.sample from the ring to the learner's batch.  DESIGN.md §16.
//
//   rows <= 1024   sample_small   one workgroup, one thread per row: both draws and both skip flags, the choice, then the
//                                 in-batch fallback from the waves' validity ballots kept in LDS, then the gather.  A row
//                                 that takes another row's draw recomputes it from u (rare, and cheaper than 12 KiB of LDS).
//   rows  > 1024   sample_draw    blocks of 1024 rows: writes every row's chosen (slot, env, agent, valid) and the block's
//                                 first / last valid row into the workspace.
//                  sample_gather  the same blocks: a row without a valid row before it in its own block takes the last
//                                 valid row of the nearest earlier block that has one, found from a 1024-bit map of the
//                                 block summaries built once per workgroup (only by workgroups whose first row is invalid);
//                                 then the same for the rows after it.  No workgroup waits on another: the kernel boundary
//                                 is the only ordering between the two phases, and every search is a bounded loop.
//
// Rows move as 8-byte accesses: observation rows are 40 bytes, action rows 8.  Built with -ffp-contract=off; the index is
// one float32 multiply truncated toward zero, as torch's `(r * n).long()`.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/uavx_replay.h"

namespace uavx_replay_k {

constexpr int WG = UAVX_REPLAY_SINGLE_ROWS, WAVES = WG / 64, OBS = 10;
constexpr int64_t MAX_BLOCKS = UAVX_REPLAY_MAX_ROWS / WG;
static_assert(MAX_BLOCKS <= WG, "one thread per block summary");

struct Args {
    const float *obs, *act, *rew;
    const uint8_t *done, *skip, *trunc, *ended;      // skip == NULL: flags packed into done
    int32_t L, E, N, NL;
    int64_t count;
    const int64_t *count_dev;
    const float *u;
    int32_t rows;
    float *state, *action, *reward, *next_state, *mask;
    uint8_t *truncated, *ended_out;
    int2 *summary;           // per block of WG rows: first and last valid row of the batch, −1 without one
    int4 *picks;             // per row: slot, env, agent, valid
};

struct Pick {
    int32_t s, e, i;
    bool valid;
};

// trunc(u · n) clamped into [0, n − 1], n in [1, 2^31): NaN and negatives give 0, anything at or past n its top
__device__ inline int32_t pick(float u, int32_t n) {
    const float x = u * (float)n;
    if (!(x >= 0.f)) return 0;
    if (x >= 2147483648.f) return n - 1;
    const int32_t k = (int32_t)x;
    return k < n - 1 ? k : n - 1;
}

// the sampling window: span steps, the oldest of them in slot lo_mod
__device__ inline void window(const Args &a, int32_t &lo_mod, int32_t &span) {
    int64_t c = a.count_dev ? *a.count_dev : a.count;
    if (c < 1) c = 1;
    const int64_t T = a.L - 1, lo = c > T ? c - T : 0;
    span = (int32_t)(c - lo);
    lo_mod = (int32_t)(lo % a.L);
}

__device__ inline bool skipped(const Args &a, int32_t s, int32_t e) {
    const int64_t se = (int64_t)s * a.E + e;
    return a.skip ? a.skip[se] != 0 : (a.done[se * a.N] & 2) != 0;
}

// the draw row j ends up with after the redraw (steps 1 and 2)
__device__ inline Pick draw(const Args &a, int64_t j, int32_t lo_mod, int32_t span) {
    const int64_t R = a.rows;
    const float u0 = a.u[j], u1 = a.u[R + j], u2 = a.u[2 * R + j];
    const float v0 = a.u[3 * R + j], v1 = a.u[4 * R + j], v2 = a.u[5 * R + j];
    int64_t s0 = (int64_t)lo_mod + pick(u0, span), s1 = (int64_t)lo_mod + pick(v0, span);
    if (s0 >= a.L) s0 -= a.L;
    if (s1 >= a.L) s1 -= a.L;
    const int32_t e0 = pick(u1, a.E), e1 = pick(v1, a.E);
    const bool bad0 = skipped(a, (int32_t)s0, e0), bad1 = skipped(a, (int32_t)s1, e1);
    Pick p;
    p.s = bad0 ? (int32_t)s1 : (int32_t)s0;
    p.e = bad0 ? e1 : e0;
    p.i = pick(bad0 ? v2 : u2, a.NL);
    p.valid = !(bad0 && bad1);
    return p;
}

// publishes the wave's validity ballot; after the barrier bal[w] holds wave w's
__device__ inline uint64_t publish(bool valid, uint64_t *bal) {
    const uint64_t b = __ballot(valid);
    if ((threadIdx.x & 63) == 0) bal[threadIdx.x >> 6] = b;
    __syncthreads();
    return b;
}

// the last valid thread before this (invalid) one in the workgroup, −1 without one
__device__ inline int before_in_block(uint64_t mine, const uint64_t *bal) {
    const int lane = threadIdx.x & 63;
    int w = threadIdx.x >> 6;
    uint64_t m = mine & ((1ull << lane) - 1);
    for (;;) {
        if (m) return w * 64 + 63 - __clzll((long long)m);
        if (--w < 0) return -1;
        m = bal[w];
    }
}

// the first valid thread after this one in the workgroup, −1 without one
__device__ inline int after_in_block(uint64_t mine, const uint64_t *bal, int waves) {
    const int lane = threadIdx.x & 63;
    int w = threadIdx.x >> 6;
    uint64_t m = mine & ~((2ull << lane) - 1);
    for (;;) {
        if (m) return w * 64 + __ffsll((unsigned long long)m) - 1;
        if (++w >= waves) return -1;
        m = bal[w];
    }
}

__device__ inline void gather(const Args &a, int64_t j, int32_t s, int32_t e, int32_t i) {
    const int32_t s1 = s + 1 == a.L ? 0 : s + 1;
    const int64_t se = (int64_t)s * a.E + e, cell = se * a.N + i, next = ((int64_t)s1 * a.E + e) * a.N + i;
    const float2 *__restrict__ x = (const float2 *)(a.obs + cell * OBS);
    const float2 *__restrict__ y = (const float2 *)(a.obs + next * OBS);
    float2 xs[OBS / 2], ys[OBS / 2];
#pragma unroll
    for (int k = 0; k < OBS / 2; ++k) {
        xs[k] = x[k];
        ys[k] = y[k];
    }
    const float2 act = *(const float2 *)(a.act + cell * 2);
    const float rew = a.rew[cell];
    const uint8_t done = a.done[cell];
    uint8_t tr = 0, en = 0;
    if (a.truncated) {
        if (a.skip) {
            tr = a.trunc[se] != 0;
            en = a.ended[se] != 0;
        } else {
            const uint8_t b = a.done[se * a.N];
            tr = (b >> 3) & 1;
            en = (b >> 2) & 1;
        }
    }
    float2 *__restrict__ xo = (float2 *)(a.state + j * OBS);
    float2 *__restrict__ yo = (float2 *)(a.next_state + j * OBS);
#pragma unroll
    for (int k = 0; k < OBS / 2; ++k) {
        xo[k] = xs[k];
        yo[k] = ys[k];
    }
    *(float2 *)(a.action + j * 2) = act;
    a.reward[j] = rew;
    a.mask[j] = 1.0f - (float)(done & 1);
    if (a.truncated) {
        a.truncated[j] = tr;
        a.ended_out[j] = en;
    }
}

__global__ __launch_bounds__(WG) void sample_small(const Args a) {
    __shared__ uint64_t bal[WAVES];
    const int j = threadIdx.x;
    int32_t lo_mod, span;
    window(a, lo_mod, span);
    Pick p{0, 0, 0, false};
    if (j < a.rows) p = draw(a, j, lo_mod, span);
    const uint64_t mine = publish(p.valid, bal);
    if (j >= a.rows) return;
    if (!p.valid) {
        int src = before_in_block(mine, bal);
        if (src < 0) src = after_in_block(mine, bal, blockDim.x >> 6);
        if (src < 0) src = a.rows - 1;
        if (src != j) p = draw(a, src, lo_mod, span);
    }
    gather(a, j, p.s, p.e, p.i);
}

__global__ __launch_bounds__(WG) void sample_draw(const Args a) {
    __shared__ uint64_t bal[WAVES];
    const int64_t base = (int64_t)blockIdx.x * WG, j = base + threadIdx.x;
    int32_t lo_mod, span;
    window(a, lo_mod, span);
    Pick p{0, 0, 0, false};
    if (j < a.rows) {
        p = draw(a, j, lo_mod, span);
        a.picks[j] = make_int4(p.s, p.e, p.i, p.valid ? 1 : 0);
    }
    publish(p.valid, bal);
    if (threadIdx.x != 0) return;
    int first = -1, last = -1;
    for (int w = 0; w < WAVES; ++w) {
        const uint64_t m = bal[w];
        if (!m) continue;
        if (first < 0) first = (int)base + w * 64 + __ffsll((unsigned long long)m) - 1;
        last = (int)base + w * 64 + 63 - __clzll((long long)m);
    }
    a.summary[blockIdx.x] = make_int2(first, last);
}

__global__ __launch_bounds__(WG) void sample_gather(const Args a) {
    __shared__ uint64_t bal[WAVES], has[WAVES];
    const int64_t base = (int64_t)blockIdx.x * WG, j = base + threadIdx.x;
    const int blocks = (a.rows + WG - 1) / WG;
    int4 p = make_int4(0, 0, 0, 0);
    if (j < a.rows) p = a.picks[j];
    const uint64_t mine = publish(p.w != 0, bal);
    // rows in front of the block's first valid row look at the other blocks; uniform over the workgroup
    int prev_last = -1, next_first = -1;
    if (!(bal[0] & 1)) {
        const int t = threadIdx.x;
        publish(t < blocks && a.summary[t].y >= 0, has);
        const int b = blockIdx.x;
        int w = b >> 6;
        uint64_t m = has[w] & ((1ull << (b & 63)) - 1);
        for (;;) {
            if (m) {
                prev_last = a.summary[w * 64 + 63 - __clzll((long long)m)].y;
                break;
            }
            if (--w < 0) break;
            m = has[w];
        }
        w = b >> 6;
        m = has[w] & ~((2ull << (b & 63)) - 1);
        for (;;) {
            if (m) {
                next_first = a.summary[w * 64 + __ffsll((unsigned long long)m) - 1].x;
                break;
            }
            if (++w >= WAVES) break;
            m = has[w];
        }
    }
    if (j >= a.rows) return;
    if (p.w == 0) {
        const int in_before = before_in_block(mine, bal);
        int64_t src = in_before >= 0 ? base + in_before : prev_last;
        if (src < 0) {
            const int in_after = after_in_block(mine, bal, WAVES);
            src = in_after >= 0 ? base + in_after : next_first;
        }
        if (src < 0) src = a.rows - 1;
        if (src != j) p = a.picks[src];
    }
    gather(a, j, p.x, p.y, p.z);
}

static bool aligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

static int64_t summary_bytes(int64_t rows) { return ((rows + WG - 1) / WG * (int64_t)sizeof(int2) + 15) / 16 * 16; }

static int64_t workspace_bytes(int64_t rows) {
    return rows <= WG ? 0 : summary_bytes(rows) + rows * (int64_t)sizeof(int4);
}

}  // namespace uavx_replay_k

using namespace uavx_replay_k;

extern "C" {

int uavx_replay_version(void) { return UAVX_REPLAY_VERSION; }

int uavx_replay_workspace_bytes(int64_t rows, int64_t *bytes) {
    if (!bytes || rows < 0 || rows > UAVX_REPLAY_MAX_ROWS) return UAVX_ACTOR_ERR_INVALID_ARG;
    *bytes = workspace_bytes(rows);
    return UAVX_ACTOR_OK;
}

int uavx_replay_sample(const uavx_replay_ring *ring, int64_t count, const int64_t *count_dev, const float *u, int64_t rows,
                       float *state, float *action, float *reward, float *next_state, float *mask, uint8_t *truncated,
                       uint8_t *ended, void *workspace, int64_t workspace_bytes_given, void *stream) {
    if (!ring || !ring->obs || !ring->act || !ring->rew || !ring->done) return UAVX_ACTOR_ERR_INVALID_ARG;
    const int flags = (ring->skip != nullptr) + (ring->trunc != nullptr) + (ring->ended != nullptr);
    if (flags != 0 && flags != 3) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (ring->slots < 2 || ring->slots > INT32_MAX || ring->envs < 1 || ring->envs > INT32_MAX || ring->agents < 1 ||
        ring->agents > INT32_MAX || ring->learners < 1 || ring->learners > ring->agents)
        return UAVX_ACTOR_ERR_INVALID_ARG;
    if (!aligned(ring->obs, 8) || !aligned(ring->act, 8) || !aligned(ring->rew, 4)) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (count_dev ? !aligned(count_dev, 8) : count < 1) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (rows < 0 || rows > UAVX_REPLAY_MAX_ROWS) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (rows == 0) return UAVX_ACTOR_OK;
    if (!u || !state || !action || !reward || !next_state || !mask || (truncated == nullptr) != (ended == nullptr))
        return UAVX_ACTOR_ERR_INVALID_ARG;
    if (!aligned(u, 4) || !aligned(state, 8) || !aligned(action, 8) || !aligned(next_state, 8) || !aligned(reward, 4) ||
        !aligned(mask, 4))
        return UAVX_ACTOR_ERR_INVALID_ARG;
    const int64_t need = workspace_bytes(rows);
    if (need > 0 && (!workspace || workspace_bytes_given < need || !aligned(workspace, 16))) return UAVX_ACTOR_ERR_INVALID_ARG;

    Args a{};
    a.obs = ring->obs;
    a.act = ring->act;
    a.rew = ring->rew;
    a.done = ring->done;
    a.skip = ring->skip;
    a.trunc = ring->trunc;
    a.ended = ring->ended;
    a.L = (int32_t)ring->slots;
    a.E = (int32_t)ring->envs;
    a.N = (int32_t)ring->agents;
    a.NL = (int32_t)ring->learners;
    a.count = count;
    a.count_dev = count_dev;
    a.u = u;
    a.rows = (int32_t)rows;
    a.state = state;
    a.action = action;
    a.reward = reward;
    a.next_state = next_state;
    a.mask = mask;
    a.truncated = truncated;
    a.ended_out = ended;
    const hipStream_t st = (hipStream_t)stream;
    if (rows <= WG) {
        hipLaunchKernelGGL(sample_small, dim3(1), dim3((unsigned)((rows + 63) / 64 * 64)), 0, st, a);
        return hipGetLastError() == hipSuccess ? UAVX_ACTOR_OK : UAVX_ACTOR_ERR_HIP;
    }
    a.summary = (int2 *)workspace;
    a.picks = (int4 *)((char *)workspace + summary_bytes(rows));
    const unsigned blocks = (unsigned)((rows + WG - 1) / WG);
    hipLaunchKernelGGL(sample_draw, dim3(blocks), dim3(WG), 0, st, a);
    if (hipGetLastError() != hipSuccess) return UAVX_ACTOR_ERR_HIP;
    hipLaunchKernelGGL(sample_gather, dim3(blocks), dim3(WG), 0, st, a);
    return hipGetLastError() == hipSuccess ? UAVX_ACTOR_OK : UAVX_ACTOR_ERR_HIP;
}

}  // extern "C"

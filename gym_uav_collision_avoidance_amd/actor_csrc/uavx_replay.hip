// Replay sampler: a draw from the ring, uniform or recency-weighted, to one row of a one-step or an n-step batch.  One set of
// kernels behind both C interfaces: include/uavx_nstep.h is the validation and launch path, and
// include/uavx_replay.h (DeviceReplay.sample, §16) forwards to it with n_step = 1, gamma = 1, recency = 0 and three columns
// of uniforms.
//
//   rows <= 1024   sample_small   one workgroup, one thread per row: both draws and both skip flags, the choice, then the
//                                 in-batch fallback from the waves' validity ballots kept in LDS, then the walk and gather.
//                                 A row that takes another row's draw recomputes it from u (rare, and cheaper than 12 KiB
//                                 of LDS).
//   rows  > 1024   sample_draw    blocks of 1024 rows: writes every row's chosen (slot, env, agent, step in the window) and
//                                 the block's first / last valid row into the workspace.
//                  sample_gather  the same blocks: a row without a valid row before it in its own block takes the last
//                                 valid row of the nearest earlier block that has one, found from a 1024-bit map of the
//                                 block summaries built once per workgroup (only by workgroups whose first row is invalid);
//                                 then the same for the rows after it; then the walk and gather.  No workgroup waits on
//                                 another: the kernel boundary is the only ordering between the two phases, and every
//                                 search is a bounded loop.
//
// The walk (nstep_walk of ../common_csrc/uavx_replay_walk.hpp, which uavx_keywalk.hip runs from a prioritized sample's keys as
// well).  Once (k, e, i) is chosen every address of the walk is known: step j lies in slot s + j (minus slots past the
// wrap: one compare, no division), clamped to the last step that both n_step and the ring's head allow, so that every load
// is inside the window whatever the flags will say.  The rew, done and flag loads of ALL steps are issued together and
// unconditionally, with the start row's observation and action, and the stop is resolved in registers afterwards (a load
// under a run-time condition is branched around and waited for one by one: uavx_grad_impl.hpp).  Only next_state, whose
// slot is k + len, waits for that resolution: two round trips to memory whatever n_step is, and one when the kernel is
// built for a single step.  The kernels are instantiated for every n_step of 1..8 and for both flag layouts: a walk costs
// the load instructions of its own steps and no more (each is 64 scattered lines per wave, and that, not latency, is
// what a longer walk pays for), and the layout is not tested per load.  A single step loads one row's observation, action,
// reward and done byte and the next slot's observation, and its flags only when they are asked for; −0 + 1·(double)r and
// (1 − d)·1 round back to r and to 1 − (float)d, so the <1, *> kernels ARE the one-step sampler.
//
// Rows move as 8-byte accesses: observation rows are 40 bytes, action rows 8.  Built with -ffp-contract=off: the index is
// one float32 multiply truncated toward zero, as torch's `(r * n).long()`, the return a float64 multiply and a float64 add
// per step.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/uavx_nstep.h"
#include "../common_csrc/uavx_entry.hpp"
#include "../common_csrc/uavx_replay_ring.hpp"
#include "../common_csrc/uavx_replay_walk.hpp"

namespace uavx_replay_k {

using namespace uavx_common;

static_assert(UAVX_REPLAY_MAX_ROWS == UAVX_NSTEP_MAX_ROWS && UAVX_REPLAY_SINGLE_ROWS == UAVX_NSTEP_SINGLE_ROWS,
              "one workspace layout and one launch shape behind both interfaces");
constexpr int WG = UAVX_NSTEP_SINGLE_ROWS, WAVES = WG / 64;
constexpr int64_t MAX_BLOCKS = UAVX_NSTEP_MAX_ROWS / WG;
static_assert(MAX_BLOCKS <= WG, "one thread per block summary");

struct Args : ReplayView {
    const float *u;
    int32_t cols, n;
    double gamma;
    float recency;
    int32_t rows;
    float *state, *action, *reward, *next_state, *mask;
    uint8_t *length, *truncated, *ended_out;
    int2 *summary;           // per block of WG rows: first and last valid row of the batch, −1 without one
    int4 *picks;             // per row: slot, env, agent, and the step's place in the window (−1: not valid)
};

struct Pick {
    int32_t s, e, i, kk;     // kk = k − lo in [0, span)
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

__device__ inline bool skipped(const Args &a, int32_t s, int32_t e) {
    const int64_t se = (int64_t)s * a.E + e;
    return a.skip ? a.skip[se] != 0 : (a.done[se * a.N] & 2) != 0;
}

// the draw row j ends up with after the redraw (steps 1 and 2)
__device__ inline Pick draw(const Args &a, int64_t j, int32_t lo_mod, int32_t span) {
    const int64_t R = a.rows;
    const float *u = a.u + j, *v = a.u + (int64_t)a.cols * R + j;      // first draw, redraw: planes of R floats
    const float u0 = u[0], u1 = u[R], u2 = u[2 * R], v0 = v[0], v1 = v[R], v2 = v[2 * R];
    int32_t k0 = pick(u0, span), k1 = pick(v0, span);
    if (a.cols == 5) {       // uniform over the launch
        const float u3 = u[3 * R], u4 = u[4 * R], v3 = v[3 * R], v4 = v[4 * R];
        const int32_t b0 = pick(u3, span), b1 = pick(v3, span);
        if (u4 < a.recency && b0 > k0) k0 = b0;
        if (v4 < a.recency && b1 > k1) k1 = b1;
    }
    int64_t s0 = (int64_t)lo_mod + k0, s1 = (int64_t)lo_mod + k1;
    if (s0 >= a.L) s0 -= a.L;
    if (s1 >= a.L) s1 -= a.L;
    const int32_t e0 = pick(u1, a.E), e1 = pick(v1, a.E);
    const bool bad0 = skipped(a, (int32_t)s0, e0), bad1 = skipped(a, (int32_t)s1, e1);
    Pick p;
    p.s = bad0 ? (int32_t)s1 : (int32_t)s0;
    p.e = bad0 ? e1 : e0;
    p.i = pick(bad0 ? v2 : u2, a.NL);
    p.kk = bad0 ? k1 : k0;
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

// the walk from (s, e, i), kk steps into a window of span, and the row's outputs (steps 3 and 4).  NMAX >= n_step (the launch picks NMAX == n_step).
template <int NMAX, bool PACKED>
__device__ inline void gather(const Args &a, int64_t j, int32_t s, int32_t e, int32_t i, int32_t kk, int32_t span) {
    // the last step the walk can reach: n_step − 1, or the newest step of the ring if that comes first
    const int32_t rem = span - 1 - kk;
    nstep_walk<NMAX, PACKED, true>(a, j, s, e, i, NMAX == 1 ? 0 : (rem < a.n - 1 ? rem : a.n - 1));
}

template <int NMAX, bool PACKED>
__global__ __launch_bounds__(WG) void sample_small(const Args a) {
    __shared__ uint64_t bal[WAVES];
    const int j = threadIdx.x;
    const ReplayWindow w = window(a);
    const int32_t lo_mod = w.lo_mod, span = w.span;
    Pick p{0, 0, 0, 0, false};
    if (j < a.rows) p = draw(a, j, lo_mod, span);
    const uint64_t mine = publish(p.valid, bal);
    if (j >= a.rows) return;
    if (!p.valid) {
        int src = before_in_block(mine, bal);
        if (src < 0) src = after_in_block(mine, bal, blockDim.x >> 6);
        if (src < 0) src = a.rows - 1;
        if (src != j) p = draw(a, src, lo_mod, span);
    }
    gather<NMAX, PACKED>(a, j, p.s, p.e, p.i, p.kk, span);
}

__global__ __launch_bounds__(WG) void sample_draw(const Args a) {
    __shared__ uint64_t bal[WAVES];
    const int64_t base = (int64_t)blockIdx.x * WG, j = base + threadIdx.x;
    const ReplayWindow w = window(a);
    const int32_t lo_mod = w.lo_mod, span = w.span;
    Pick p{0, 0, 0, 0, false};
    if (j < a.rows) {
        p = draw(a, j, lo_mod, span);
        // the step's place in the window rides with the validity: kk + 1 when valid, −(kk + 1) when not
        a.picks[j] = make_int4(p.s, p.e, p.i, p.valid ? p.kk + 1 : -(p.kk + 1));
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

template <int NMAX, bool PACKED>
__global__ __launch_bounds__(WG) void sample_gather(const Args a) {
    __shared__ uint64_t bal[WAVES], has[WAVES];
    const int64_t base = (int64_t)blockIdx.x * WG, j = base + threadIdx.x;
    const int blocks = (a.rows + WG - 1) / WG;
    const int32_t span = NMAX == 1 ? 1 : span_of(a);     // the walk's; the slot rotation was sample_draw's business
    int4 p = make_int4(0, 0, 0, 0);
    if (j < a.rows) p = a.picks[j];
    const uint64_t mine = publish(p.w > 0, bal);
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
    if (p.w <= 0) {
        const int in_before = before_in_block(mine, bal);
        int64_t src = in_before >= 0 ? base + in_before : prev_last;
        if (src < 0) {
            const int in_after = after_in_block(mine, bal, WAVES);
            src = in_after >= 0 ? base + in_after : next_first;
        }
        if (src < 0) src = a.rows - 1;
        if (src != j) p = a.picks[src];
    }
    gather<NMAX, PACKED>(a, j, p.x, p.y, p.z, (p.w < 0 ? -p.w : p.w) - 1, span);
}

using Kernel = void (*)(const Args);

// [packed][n_step − 1]
#define UAVX_NSTEP_ROW(K, P) {K<1, P>, K<2, P>, K<3, P>, K<4, P>, K<5, P>, K<6, P>, K<7, P>, K<8, P>}
static const Kernel SMALL[2][UAVX_NSTEP_MAX] = {UAVX_NSTEP_ROW(sample_small, false), UAVX_NSTEP_ROW(sample_small, true)};
static const Kernel GATHER[2][UAVX_NSTEP_MAX] = {UAVX_NSTEP_ROW(sample_gather, false), UAVX_NSTEP_ROW(sample_gather, true)};
#undef UAVX_NSTEP_ROW

static int64_t summary_bytes(int64_t rows) { return ((rows + WG - 1) / WG * (int64_t)sizeof(int2) + 15) / 16 * 16; }

static int64_t workspace_bytes(int64_t rows) {
    return rows <= WG ? 0 : summary_bytes(rows) + rows * (int64_t)sizeof(int4);
}

}  // namespace uavx_replay_k

using namespace uavx_replay_k;

extern "C" {

int uavx_replay_version(void) { return UAVX_REPLAY_VERSION; }

int uavx_nstep_version(void) { return UAVX_NSTEP_VERSION; }

int uavx_nstep_workspace_bytes(int64_t rows, int64_t *bytes) {
    if (!bytes || rows < 0 || rows > UAVX_NSTEP_MAX_ROWS) return UAVX_ACTOR_ERR_INVALID_ARG;
    *bytes = workspace_bytes(rows);
    return UAVX_ACTOR_OK;
}

int uavx_replay_workspace_bytes(int64_t rows, int64_t *bytes) { return uavx_nstep_workspace_bytes(rows, bytes); }

int uavx_nstep_sample(const uavx_nstep_args *g, void *stream) {
    if (!g) return UAVX_ACTOR_ERR_INVALID_ARG;
    Args a{};
    if (!replay_view(g->ring, g->count, g->count_dev, a)) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (g->n_step < 1 || g->n_step > UAVX_NSTEP_MAX) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (!(g->gamma > 0.0 && g->gamma <= 1.0)) return UAVX_ACTOR_ERR_INVALID_ARG;              // a NaN is refused too
    if (!(g->recency >= 0.f && g->recency <= 1.f)) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (g->u_cols != 5 && !(g->u_cols == 3 && g->recency == 0.f)) return UAVX_ACTOR_ERR_INVALID_ARG;
    const int64_t rows = g->rows;
    if (rows < 0 || rows > UAVX_NSTEP_MAX_ROWS) return UAVX_ACTOR_ERR_INVALID_ARG;
    if ((g->truncated == nullptr) != (g->ended == nullptr)) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (rows == 0) return UAVX_ACTOR_OK;
    if (!g->u || !g->state || !g->action || !g->reward || !g->next_state || !g->mask) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (!aligned(g->u, 4) || !aligned(g->state, 8) || !aligned(g->action, 8) || !aligned(g->next_state, 8) ||
        !aligned(g->reward, 4) || !aligned(g->mask, 4))
        return UAVX_ACTOR_ERR_INVALID_ARG;
    const int64_t need = workspace_bytes(rows);
    if (need > 0 && (!g->workspace || g->workspace_bytes < need || !aligned(g->workspace, 16)))
        return UAVX_ACTOR_ERR_INVALID_ARG;

    a.u = g->u;
    a.cols = g->u_cols;
    a.n = g->n_step;
    a.gamma = g->gamma;
    a.recency = g->recency;
    a.rows = (int32_t)rows;
    a.state = g->state;
    a.action = g->action;
    a.reward = g->reward;
    a.next_state = g->next_state;
    a.mask = g->mask;
    a.length = g->length;
    a.truncated = g->truncated;
    a.ended_out = g->ended;
    const int packed = a.skip == nullptr, level = a.n - 1;
    const hipStream_t st = (hipStream_t)stream;
    if (rows <= WG) return launch(SMALL[packed][level], 1, (int)((rows + 63) / 64 * 64), st, a);
    a.summary = (int2 *)g->workspace;
    a.picks = (int4 *)((char *)g->workspace + summary_bytes(rows));
    const int64_t blocks = (rows + WG - 1) / WG;
    const int rc = launch(sample_draw, blocks, WG, st, a);
    return rc != UAVX_ACTOR_OK ? rc : launch(GATHER[packed][level], blocks, WG, st, a);
}

// One step, uniform draws, three columns of uniforms, no length.  With rows = 0 this entry has always answered before it
// looked at the output flags, and uavx_nstep_sample looks at that pair first: they are not handed on then.
int uavx_replay_sample(const uavx_replay_ring *ring, int64_t count, const int64_t *count_dev, const float *u, int64_t rows,
                       float *state, float *action, float *reward, float *next_state, float *mask, uint8_t *truncated,
                       uint8_t *ended, void *workspace, int64_t workspace_bytes_given, void *stream) {
    uavx_nstep_args g{};
    g.ring = ring;
    g.count = count;
    g.count_dev = count_dev;
    g.u = u;
    g.u_cols = 3;
    g.n_step = 1;
    g.gamma = 1.0;
    g.recency = 0.f;
    g.rows = rows;
    g.state = state;
    g.action = action;
    g.reward = reward;
    g.next_state = next_state;
    g.mask = mask;
    g.length = nullptr;
    g.truncated = rows == 0 ? nullptr : truncated;
    g.ended = rows == 0 ? nullptr : ended;
    g.workspace = workspace;
    g.workspace_bytes = workspace_bytes_given;
    return uavx_nstep_sample(&g, stream);
}

}  // extern "C"

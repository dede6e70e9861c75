// The n-step walk from sampled keys (include/uavx_keywalk.h): behind uavx_prio_sample, one launch that reads
// each row's key and overwrites the row's reward, next_state, mask and flags with the n-step values.
//
//   walk_rows<NSTEP, PACKED>   one thread per row, workgroups of 256.  The thread loads its key, decodes (k, e, i), and
//                              leaves (writing length = 0, if asked) when the key is negative or names a step outside the
//                              window.  Otherwise every address of the walk is known: step t lies in slot s + min(t, top),
//                              top = min(NSTEP − 1, c − 1 − k), minus slots past the wrap (one compare, no division), so
//                              every load is inside the window whatever the flags will say.  The rew, done and flag loads of
//                              ALL steps are issued together and unconditionally, and the stop is resolved in registers
//                              afterwards, each step computed and then selected (uavx_replay.hip has the same walk, and
//                              DESIGN.md §22 what the compiler does to other shapes of it).  Only next_state, whose slot is
//                              k + len, waits for that resolution: three dependent round trips to memory per row whatever
//                              NSTEP is -- key, walk, next state -- and two when the kernel is built for a single step,
//                              whose next slot is known with the key.
//
// Instantiated for every n_step of 1..8 and for both flag layouts: a walk costs the load instructions of its own steps and
// no more, and the layout is not tested per load.  Rows move as 8-byte accesses (observation rows are 40 bytes).  Built
// with -ffp-contract=off: the return is a float64 multiply and a float64 add per step.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "../../include/uavx_keywalk.h"

namespace uavx_keywalk_k {

constexpr int WG = 256, OBS = 10;

struct Args {
    const float *obs, *rew;
    const uint8_t *done, *skip, *trunc, *ended;      // skip == NULL: flags packed into done
    int32_t L, E, N, NL;
    int64_t count;
    const int64_t *count_dev;
    const int64_t *key;
    int32_t rows;
    double gamma;
    float *reward, *next_state, *mask;
    uint8_t *length, *truncated, *ended_out;
};

template <int NSTEP, bool PACKED>
__global__ __launch_bounds__(WG) void walk_rows(const Args a) {
    const int64_t j = (int64_t)blockIdx.x * WG + threadIdx.x;
    if (j >= a.rows) return;
    const int64_t q = a.key[j];
    int64_t c = a.count_dev ? *a.count_dev : a.count;
    if (c < 1) c = 1;
    const int64_t T = a.L - 1, lo = c > T ? c - T : 0;
    const int64_t per = (int64_t)a.E * a.NL;          // <= 2^31 − 1: the host checked
    const int64_t k = q < 0 ? -1 : q / per;
    if (k < lo || k >= c) {                           // ignored: nothing of the ring is read, nothing else written
        if (a.length) a.length[j] = 0;
        return;
    }
    const uint32_t rest = (uint32_t)(q - k * per), e = rest / (uint32_t)a.NL, i = rest - e * (uint32_t)a.NL;
    const uint32_t L = (uint32_t)a.L;
    const uint32_t kk = (uint32_t)(k - lo);           // < span <= slots − 1
    uint32_t s = (uint32_t)(lo % a.L) + kk;           // < 2·slots <= 2^32 − 2
    if (s >= L) s -= L;
    // the last step the walk can reach: NSTEP − 1, or the newest step of the ring if that comes first
    const int64_t rem = c - 1 - k;
    const uint32_t top = NSTEP == 1 ? 0u : (uint32_t)(rem < NSTEP - 1 ? rem : NSTEP - 1);
    const int64_t se0 = (int64_t)s * a.E + e;
    const bool flags = a.truncated != nullptr;
    float rew[NSTEP];
    uint8_t dn[NSTEP], sk[NSTEP], en[NSTEP], tr[NSTEP];      // PACKED: sk holds agent 0's done byte, en and tr are not used
#pragma unroll
    for (int t = 0; t < NSTEP; ++t) {
        uint32_t st = s + ((uint32_t)t < top ? (uint32_t)t : top);      // st < 2·slots: top <= span − 1 <= slots − 2
        if (st >= L) st -= L;
        const int64_t se = (int64_t)st * a.E + e, cell = se * a.N + i;
        rew[t] = a.rew[cell];
        dn[t] = a.done[cell];
        if (NSTEP == 1) {
            // a single step stops by itself: its flags are only outputs, loaded below when they are asked for
            sk[t] = en[t] = tr[t] = 0;
        } else if (PACKED) {
            sk[t] = a.done[se * a.N];
        } else {
            sk[t] = a.skip[se];
            en[t] = a.ended[se];
            tr[t] = a.trunc[se];                         // wanted or not: a load under `flags` would be waited for by itself
        }
    }
    // every load above is issued before the first of them is waited for: left to itself the scheduler starts resolving
    // step 0 after half the loads, which puts a wait for memory between the two halves.  (A single step resolves nothing,
    // and its next_state load belongs with the others.)
    if (NSTEP > 1) __builtin_amdgcn_sched_barrier(0);

    // the stop, in registers: nothing below loads, and every step is computed and then selected, so that there is no
    // conditional block for the compiler to sink a step's loads into
    double R = -0.0, g = 1.0;                            // −0 + x is x for every x, a reward of −0 included
    uint32_t len = 1;
    bool run = true;
    uint8_t d_last = 0, tr_last = 0, en_last = 0;
#pragma unroll
    for (int t = 0; t < NSTEP; ++t) {
        const bool ended = PACKED ? (sk[t] & 4) != 0 : en[t] != 0;
        const bool trunc = PACKED ? (sk[t] & 8) != 0 : tr[t] != 0;
        bool stop = t == NSTEP - 1 || (uint32_t)t >= top || (dn[t] & 1) || ended;
        if (t + 1 < NSTEP) stop = stop || (PACKED ? (sk[t + 1] & 2) != 0 : sk[t + 1] != 0);
        const double Rt = R + g * (double)rew[t], gt = g * a.gamma;
        R = run ? Rt : R;
        d_last = run ? (uint8_t)(dn[t] & 1) : d_last;
        tr_last = run ? (uint8_t)trunc : tr_last;
        en_last = run ? (uint8_t)ended : en_last;
        run = run && !stop;
        g = run ? gt : g;
        len = run ? (uint32_t)t + 2 : len;
    }

    uint32_t s1 = s + len;                               // len <= top + 1 <= span <= slots − 1
    if (s1 >= L) s1 -= L;
    const float2 *__restrict__ y = (const float2 *)(a.obs + (((int64_t)s1 * a.E + e) * a.N + i) * OBS);
    float2 ys[OBS / 2];
#pragma unroll
    for (int m = 0; m < OBS / 2; ++m) ys[m] = y[m];
    if (NSTEP == 1 && flags) {                           // behind the row's other loads, as the one-step sampler has them
        if (PACKED) {
            const uint8_t b = a.done[se0 * a.N];
            tr_last = (b >> 3) & 1;
            en_last = (b >> 2) & 1;
        } else {
            tr_last = a.trunc[se0] != 0;
            en_last = a.ended[se0] != 0;
        }
    }
    float2 *__restrict__ yo = (float2 *)(a.next_state + j * OBS);
#pragma unroll
    for (int m = 0; m < OBS / 2; ++m) yo[m] = ys[m];
    a.reward[j] = (float)R;
    a.mask[j] = (float)((1.0 - (double)d_last) * g);
    if (a.length) a.length[j] = (uint8_t)len;
    if (flags) {
        a.truncated[j] = tr_last;
        a.ended_out[j] = en_last;
    }
}

using Kernel = void (*)(const Args);

// [packed][n_step − 1]
#define UAVX_KEYWALK_ROW(P) {walk_rows<1, P>, walk_rows<2, P>, walk_rows<3, P>, walk_rows<4, P>, walk_rows<5, P>, \
                             walk_rows<6, P>, walk_rows<7, P>, walk_rows<8, P>}
static const Kernel WALK[2][UAVX_KEYWALK_MAX_STEP] = {UAVX_KEYWALK_ROW(false), UAVX_KEYWALK_ROW(true)};
#undef UAVX_KEYWALK_ROW

static bool aligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace uavx_keywalk_k

using namespace uavx_keywalk_k;

extern "C" {

#ifndef UAVX_KEYWALK_SRC_HASH
#define UAVX_KEYWALK_SRC_HASH ""
#endif
// the loader (_keywalk_lib.py) finds this marker in the file without mapping it
__attribute__((used)) static const char kBuildInfo[] = "UAVX_KEYWALK_SRC_HASH=" UAVX_KEYWALK_SRC_HASH;

int uavx_keywalk_version(void) { return UAVX_KEYWALK_VERSION; }

int uavx_keywalk(const uavx_keywalk_args *g, void *stream) {
    if (!g) return UAVX_ACTOR_ERR_INVALID_ARG;
    const uavx_replay_ring *ring = g->ring;
    if (!ring || !ring->obs || !ring->act || !ring->rew || !ring->done) return UAVX_ACTOR_ERR_INVALID_ARG;
    const int ring_flags = (ring->skip != nullptr) + (ring->trunc != nullptr) + (ring->ended != nullptr);
    if (ring_flags != 0 && ring_flags != 3) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (ring->slots < 2 || ring->slots > INT32_MAX || ring->envs < 1 || ring->envs > INT32_MAX || ring->agents < 1 ||
        ring->agents > INT32_MAX || ring->learners < 1 || ring->learners > ring->agents)
        return UAVX_ACTOR_ERR_INVALID_ARG;
    // envs·learners <= 2^31 − 1 (what is left of a key after its step is a 32-bit number), and the observation array's
    // slots·envs·agents·40 bytes below 2^63, without overflowing on the way
    if (ring->learners > INT32_MAX / ring->envs) return UAVX_ACTOR_ERR_INVALID_ARG;
    const int64_t most = INT64_MAX / (OBS * (int64_t)sizeof(float));
    if (ring->envs > most / ring->slots || ring->agents > most / (ring->slots * ring->envs))
        return UAVX_ACTOR_ERR_INVALID_ARG;
    if (!aligned(ring->obs, 8) || !aligned(ring->act, 8) || !aligned(ring->rew, 4)) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (g->count_dev ? !aligned(g->count_dev, 8) : g->count < 1) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (g->n_step < 1 || g->n_step > UAVX_KEYWALK_MAX_STEP) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (!(g->gamma >= 0.0 && g->gamma <= 1.0)) return UAVX_ACTOR_ERR_INVALID_ARG;             // a NaN is refused too
    const int64_t rows = g->rows;
    if (rows < 0 || rows > UAVX_KEYWALK_MAX_ROWS) return UAVX_ACTOR_ERR_INVALID_ARG;
    if ((g->truncated == nullptr) != (g->ended == nullptr)) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (rows == 0) return UAVX_ACTOR_OK;
    if (!g->key || !g->reward || !g->next_state || !g->mask) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (!aligned(g->key, 8) || !aligned(g->next_state, 8) || !aligned(g->reward, 4) || !aligned(g->mask, 4))
        return UAVX_ACTOR_ERR_INVALID_ARG;

    Args a{};
    a.obs = ring->obs;
    a.rew = ring->rew;
    a.done = ring->done;
    a.skip = ring->skip;
    a.trunc = ring->trunc;
    a.ended = ring->ended;
    a.L = (int32_t)ring->slots;
    a.E = (int32_t)ring->envs;
    a.N = (int32_t)ring->agents;
    a.NL = (int32_t)ring->learners;
    a.count = g->count;
    a.count_dev = g->count_dev;
    a.key = g->key;
    a.rows = (int32_t)rows;
    a.gamma = g->gamma;
    a.reward = g->reward;
    a.next_state = g->next_state;
    a.mask = g->mask;
    a.length = g->length;
    a.truncated = g->truncated;
    a.ended_out = g->ended;
    const int packed = ring->skip == nullptr;
    const unsigned blocks = (unsigned)((rows + WG - 1) / WG);
    hipLaunchKernelGGL(WALK[packed][g->n_step - 1], dim3(blocks), dim3(WG), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? UAVX_ACTOR_OK : UAVX_ACTOR_ERR_HIP;
}

}  // extern "C"

// The n-step walk from sampled keys (include/uavx_keywalk.h): behind uavx_prio_sample, one launch that reads
// each row's key and overwrites the row's reward, next_state, mask and flags with the n-step values.
//
//   walk_rows<NSTEP, PACKED>   one thread per row, workgroups of 256.  The thread loads its key, decodes (k, e, i), and
//                              leaves (writing length = 0, if asked) when the key is negative or names a step outside the
//                              window.  Otherwise every address of the walk is known: step t lies in slot s + min(t, top),
//                              top = min(NSTEP − 1, c − 1 − k), minus slots past the wrap (one compare, no division), so
//                              every load is inside the window whatever the flags will say.  The rew, done and flag loads of
//                              ALL steps are issued together and unconditionally, and the stop is resolved in registers
//                              afterwards, each step computed and then selected: nstep_walk of
//                              ../common_csrc/uavx_replay_walk.hpp, the function uavx_replay.hip's samplers run (DESIGN.md §22
//                              has what the compiler does to other shapes of it).  Only next_state, whose slot is
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
#include "../common_csrc/uavx_entry.hpp"
#include "../common_csrc/uavx_replay_ring.hpp"
#include "../common_csrc/uavx_replay_walk.hpp"

namespace uavx_keywalk_k {

using namespace uavx_common;

constexpr int WG = 256, OBS = 10;

struct Args : ReplayView {
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
    const ReplayWindow w = window(a);
    const int64_t per = (int64_t)a.E * a.NL;          // <= 2^31 − 1: the host checked
    const int64_t k = q < 0 ? -1 : q / per;
    if (k < w.lo || k >= w.c) {                       // ignored: nothing of the ring is read, nothing else written
        if (a.length) a.length[j] = 0;
        return;
    }
    const uint32_t rest = (uint32_t)(q - k * per), e = rest / (uint32_t)a.NL, i = rest - e * (uint32_t)a.NL;
    uint32_t s = (uint32_t)w.lo_mod + (uint32_t)(k - w.lo);       // k − lo < span <= slots − 1, so s < 2·slots <= 2^32 − 2
    if (s >= (uint32_t)a.L) s -= (uint32_t)a.L;
    // the last step the walk can reach: NSTEP − 1, or the newest step of the ring if that comes first
    const int64_t rem = w.c - 1 - k;
    const uint32_t top = NSTEP == 1 ? 0u : (uint32_t)(rem < NSTEP - 1 ? rem : NSTEP - 1);
    nstep_walk<NSTEP, PACKED, false>(a, j, s, e, i, top);
}

using Kernel = void (*)(const Args);

// [packed][n_step − 1]
#define UAVX_KEYWALK_ROW(P) {walk_rows<1, P>, walk_rows<2, P>, walk_rows<3, P>, walk_rows<4, P>, walk_rows<5, P>, \
                             walk_rows<6, P>, walk_rows<7, P>, walk_rows<8, P>}
static const Kernel WALK[2][UAVX_KEYWALK_MAX_STEP] = {UAVX_KEYWALK_ROW(false), UAVX_KEYWALK_ROW(true)};
#undef UAVX_KEYWALK_ROW

}  // namespace uavx_keywalk_k

using namespace uavx_keywalk_k;

extern "C" {

UAVX_BUILD_MARKER(UAVX_KEYWALK_SRC_HASH);

int uavx_keywalk_version(void) { return UAVX_KEYWALK_VERSION; }

int uavx_keywalk(const uavx_keywalk_args *g, void *stream) {
    if (!g) return UAVX_ACTOR_ERR_INVALID_ARG;
    Args a{};
    if (!replay_view(g->ring, g->count, g->count_dev, a)) return UAVX_ACTOR_ERR_INVALID_ARG;
    const uavx_replay_ring *ring = g->ring;
    // envs·learners <= 2^31 − 1 (what is left of a key after its step is a 32-bit number), and the observation array's
    // slots·envs·agents·40 bytes below 2^63, without overflowing on the way
    if (ring->learners > INT32_MAX / ring->envs) return UAVX_ACTOR_ERR_INVALID_ARG;
    const int64_t most = INT64_MAX / (OBS * (int64_t)sizeof(float));
    if (ring->envs > most / ring->slots || ring->agents > most / (ring->slots * ring->envs))
        return UAVX_ACTOR_ERR_INVALID_ARG;
    if (g->n_step < 1 || g->n_step > UAVX_KEYWALK_MAX_STEP) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (!unit(g->gamma)) return UAVX_ACTOR_ERR_INVALID_ARG;
    const int64_t rows = g->rows;
    if (rows < 0 || rows > UAVX_KEYWALK_MAX_ROWS) return UAVX_ACTOR_ERR_INVALID_ARG;
    if ((g->truncated == nullptr) != (g->ended == nullptr)) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (rows == 0) return UAVX_ACTOR_OK;
    if (!g->key || !g->reward || !g->next_state || !g->mask) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (!aligned(g->key, 8) || !aligned(g->next_state, 8) || !aligned(g->reward, 4) || !aligned(g->mask, 4))
        return UAVX_ACTOR_ERR_INVALID_ARG;

    a.key = g->key;
    a.rows = (int32_t)rows;
    a.gamma = g->gamma;
    a.reward = g->reward;
    a.next_state = g->next_state;
    a.mask = g->mask;
    a.length = g->length;
    a.truncated = g->truncated;
    a.ended_out = g->ended;
    return launch(WALK[a.skip == nullptr][g->n_step - 1], (rows + WG - 1) / WG, WG, (hipStream_t)stream, a);
}

}  // extern "C"

// The replay ring (uavx_replay_ring of include/uavx_replay.h) as a kernel of libuavx_actor.so's replay unit, of libuavx_prio.so
// or of libuavx_keywalk.so sees it: the fields, the sampling window derived from the step count, and the host
// checks that fill the view from the public struct.  What an entry checks beyond them -- its own overflow limit, its range of
// gamma -- stays with the entry.
#pragma once
#include <stdint.h>
#include "../../include/uavx_replay.h"

namespace uavx_common {

struct ReplayView {
    const float *obs, *rew, *act;
    const uint8_t *done, *skip, *trunc, *ended;      // skip == NULL: flags packed into done
    int32_t L, E, N, NL;                             // slots, envs, agents, learners
    int64_t count;
    const int64_t *count_dev;                        // read in count's place when set
};

// the sampling window: steps [lo, c), span of them, the oldest in slot lo_mod
struct ReplayWindow {
    int64_t c, lo;
    int32_t lo_mod, span;
};

// the steps written so far, at least 1
__device__ inline int64_t steps_of(const ReplayView &v) {
    const int64_t c = v.count_dev ? *v.count_dev : v.count;
    return c < 1 ? 1 : c;
}

__device__ inline ReplayWindow window(const ReplayView &v) {
    ReplayWindow w;
    const int64_t T = v.L - 1;
    w.c = steps_of(v);
    w.lo = w.c > T ? w.c - T : 0;
    w.span = (int32_t)(w.c - w.lo);
    w.lo_mod = (int32_t)(w.lo % v.L);
    return w;
}

// the window's span alone: no 64-bit remainder
__device__ inline int32_t span_of(const ReplayView &v) {
    const int64_t c = steps_of(v), T = v.L - 1;
    return (int32_t)(c > T ? T : c);
}

// checks what every entry over the ring checks -- the arrays and their alignment (obs and act rows move as 8-byte accesses),
// the flag arrays all or none, the sizes within int32, the count -- and fills the view; false on a bad ring
static bool replay_view(const uavx_replay_ring *ring, int64_t count, const int64_t *count_dev, ReplayView &v) {
    if (!ring || !ring->obs || !ring->act || !ring->rew || !ring->done) return false;
    const uavx_replay_ring &r = *ring;
    const int flags = (r.skip != nullptr) + (r.trunc != nullptr) + (r.ended != nullptr);
    if (flags != 0 && flags != 3) return false;
    if (r.slots < 2 || r.slots > INT32_MAX || r.envs < 1 || r.envs > INT32_MAX || r.agents < 1 || r.agents > INT32_MAX ||
        r.learners < 1 || r.learners > r.agents)
        return false;
    if ((((uintptr_t)r.obs | (uintptr_t)r.act) & 7) != 0 || ((uintptr_t)r.rew & 3) != 0) return false;
    if (count_dev ? ((uintptr_t)count_dev & 7) != 0 : count < 1) return false;
    v.obs = r.obs;
    v.act = r.act;
    v.rew = r.rew;
    v.done = r.done;
    v.skip = r.skip;
    v.trunc = r.trunc;
    v.ended = r.ended;
    v.L = (int32_t)r.slots;
    v.E = (int32_t)r.envs;
    v.N = (int32_t)r.agents;
    v.NL = (int32_t)r.learners;
    v.count = count;
    v.count_dev = count_dev;
    return true;
}

}  // namespace uavx_common

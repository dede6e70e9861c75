// The device ring as a kernel of libuavx_gae.so or libuavx_norm.so sees it: the fields, how a thread finds
// its column, the flags of an env's row, the two steps round the ring, and the host checks that fill the view from either
// library's public ring struct.
#pragma once
#include <stdint.h>

namespace uavx_common {

struct RingView {
    const float *rew;
    const uint8_t *done;
    const uint8_t *skip;       // NULL (with ended): flags packed into done
    const uint8_t *ended;
    int64_t plane;             // envs · agents: the elements of one slot
    int32_t columns;           // = plane
    int32_t agents, learners;
    int32_t envs;
    int32_t slots;
    int32_t blocks;            // workgroups, one thread per column
};

// bit 0 skip, bit 1 ended of (slot s, env e)
__device__ inline uint32_t flags(const RingView &a, int32_t s, int32_t e) {
    if (a.skip) {
        const int64_t fo = (int64_t)s * a.envs + e;
        return (a.skip[fo] ? 1u : 0u) | (a.ended[fo] ? 2u : 0u);
    }
    return ((uint32_t)a.done[(int64_t)s * a.plane + (int64_t)e * a.agents] >> 1) & 3u;
}

__device__ inline int32_t prev_slot(const RingView &a, int32_t s) { return s == 0 ? a.slots - 1 : s - 1; }
__device__ inline int32_t next_slot(const RingView &a, int32_t s) { return s + 1 == a.slots ? 0 : s + 1; }

// the column q = e·N + i of the calling thread; col and e are 0 past the last column
struct Column {
    int32_t col, e;
    bool in, learn;            // a column of the ring; of one of its learners
};

template <int WG>
__device__ inline Column column(const RingView &a) {
    const int64_t q = (int64_t)blockIdx.x * WG + threadIdx.x;
    Column c;
    c.in = q < a.columns;
    c.col = c.in ? (int32_t)q : 0;
    c.e = c.col / a.agents;
    c.learn = c.in && c.col - c.e * a.agents < a.learners;
    return c;
}

// the number of workgroups of a ring; false on a bad shape.  R: uavx_gae_ring or uavx_norm_ring
template <int WG, class R>
static bool plan(const R *r, int64_t &blocks) {
    if (!r || r->envs < 1 || r->agents < 1 || r->envs > INT32_MAX || r->agents > INT32_MAX) return false;
    if (r->envs * r->agents > INT32_MAX) return false;
    blocks = (r->envs * r->agents + WG - 1) / WG;
    return true;
}

// checks what every walk over the ring needs and fills the view; false on a bad ring.  rew is copied unchecked: not every
// caller reads it.
template <int WG, class R>
static bool ring_view(const R *ring, RingView &v) {
    int64_t blocks = 0;
    if (!plan<WG>(ring, blocks)) return false;
    const R &r = *ring;
    if (r.slots < 2 || r.slots > INT32_MAX || r.learners < 1 || r.learners > r.agents) return false;
    if (!r.done || (r.skip == nullptr) != (r.ended == nullptr)) return false;
    v.rew = r.rew;
    v.done = r.done;
    v.skip = r.skip;
    v.ended = r.ended;
    v.plane = r.envs * r.agents;
    v.columns = (int32_t)v.plane;
    v.agents = (int32_t)r.agents;
    v.learners = (int32_t)r.learners;
    v.envs = (int32_t)r.envs;
    v.slots = (int32_t)r.slots;
    v.blocks = (int32_t)blocks;
    return true;
}

}  // namespace uavx_common

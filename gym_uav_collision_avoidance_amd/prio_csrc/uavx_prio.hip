// Prioritized replay (include/uavx_prio.h): the priority table's refresh and the rebuild of its partial
// sums, the proportional draw with its gather, and the feedback of TD errors.
//
//   refresh  refresh_leaves  workgroups of 256 threads over 4 096 entries each: a wavefront takes 64 consecutive entries per
//                            iteration (one level-1 node), 16 iterations with all their loads issued first; it applies the
//                            refresh rule, stores an entry that changed and reduces the 64 values to the node's sum; the
//                            four wavefronts' sums make the workgroup's level-2 node, its smallest positive entry and its
//                            count of positive entries.
//            refresh_top     ONE workgroup of 1 024 threads: levels 3 and 4 from level 2 (at most 16 384 nodes), the total,
//                            p_min, valid and seen.  The kernel boundary is the only ordering between the two.
//   sample   sample_rows     16 lanes per row, four rows per wavefront.  At each level the row's lanes load the 64 children
//                            of the current node, four each; a prefix sum over the 16 lanes in uint64 and a ballot find
//                            the lane, and that lane the child, whose inclusive sum first exceeds what is left of the
//                            target; a level with a single node is skipped.  The search is a chain of dependent loads,
//                            so what a launch of many rows pays for is latency: four rows per wavefront keep four times
//                            the rows in flight that one would.  Then lanes 0..4 copy the state, 5..9 the next state, 10
//                            the action and 11 the scalars.
//   update   update_clear    stores 0 to the entry of every row that is still in the window
//            update_max      atomic unsigned max of the row's priority into its entry, and of the wavefront's largest into
//                            p_max: ordinary vector atomics on integers, the result is the maximum whatever the order.
//
// All sums are uint64 over uint32 entries: exact, so no order of the reduction changes a bit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/uavx_prio.h"
#include "../common_csrc/uavx_entry.hpp"
#include "../common_csrc/uavx_replay_ring.hpp"

namespace uavx_prio_k {

using namespace uavx_common;

constexpr int FAN = 64, OBS = 10;
constexpr int LEAF_WG = 256, LEAF_WAVES = LEAF_WG / 64, LEAF_ITERS = FAN / LEAF_WAVES;      // 4 096 entries per workgroup
constexpr int TOP_WG = 1024, TOP_WAVES = TOP_WG / 64;
constexpr int64_t MAX_N3 = UAVX_PRIO_MAX_ENTRIES / FAN / FAN / FAN;                          // 256
constexpr int SAMPLE_WG = 256, GROUP = 16, PER = FAN / GROUP;      // lanes per row, children per lane
constexpr int UPDATE_WG = 256;

struct Levels {
    int64_t n, n1, n2, n3, n4;       // entries and nodes per level
    uint64_t *l1, *l2, *l3, *l4;
    uint32_t *bmin, *bvalid;         // per level-2 node
};

using Ring = ReplayView;
using Window = ReplayWindow;

// the step slot s belongs to: the k in [lo, lo + slots) with k % slots == s (inside the window when k < c)
__device__ inline int64_t step_of(const Window &w, int32_t s, int32_t L) {
    int32_t d = s - w.lo_mod;
    if (d < 0) d += L;
    return w.lo + d;
}

__device__ inline uint64_t shfl64(uint64_t v, int src, int width = 64) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, width);
    const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, width);
    return ((uint64_t)hi << 32) | lo;
}

__device__ inline uint64_t shfl_xor64(uint64_t v, int m) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m);
    return ((uint64_t)hi << 32) | lo;
}

__device__ inline uint64_t shfl_up64(uint64_t v, int d, int width = 64) {
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d, width);
    const uint32_t hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d, width);
    return ((uint64_t)hi << 32) | lo;
}

// the sum over the wavefront, in every lane
__device__ inline uint64_t wave_sum(uint64_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += shfl_xor64(v, m);
    return v;
}

__device__ inline uint32_t wave_min(uint32_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, m);
        v = o < v ? o : v;
    }
    return v;
}

__device__ inline uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, m);
        v = o > v ? o : v;
    }
    return v;
}

// ---- refresh ---------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(LEAF_WG) void refresh_leaves(const Ring r, uint32_t *__restrict__ table, const Levels lv,
                                                          const uavx_prio_record *__restrict__ rec) {
    __shared__ uint64_t s_sum[LEAF_WAVES];
    __shared__ uint32_t s_min[LEAF_WAVES], s_valid[LEAF_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Window w = window(r);
    const uint32_t p_max = rec->p_max;
    const int64_t seen = rec->seen, fresh = seen > w.lo ? seen : w.lo;
    const uint32_t per_slot = (uint32_t)r.E * (uint32_t)r.NL;       // < 2^26: the table has at most that many entries
    uint64_t block_sum = 0;
    uint32_t my_min = 0xffffffffu, valid = 0;
    // every load of the wavefront's 16 nodes is issued before the first is used: the stores and the reductions below would
    // otherwise put a round trip to memory into each iteration
    const int64_t node0 = (int64_t)blockIdx.x * FAN + wave * LEAF_ITERS;
    uint32_t old[LEAF_ITERS];
    uint8_t flag[LEAF_ITERS], rule[LEAF_ITERS];                      // rule: 0 outside the window, 1 fresh, 2 keeps its value
#pragma unroll
    for (int t = 0; t < LEAF_ITERS; ++t) {
        const int64_t f = (node0 + t) * FAN + lane;
        old[t] = 0;
        flag[t] = rule[t] = 0;
        if (f < lv.n) {
            const uint32_t s = (uint32_t)f / per_slot, rest = (uint32_t)f - s * per_slot, e = rest / (uint32_t)r.NL;
            const int64_t se = (int64_t)s * r.E + e, k = step_of(w, (int32_t)s, r.L);
            flag[t] = r.skip ? r.skip[se] : (uint8_t)(r.done[se * r.N] & 2);
            old[t] = table[f];
            rule[t] = k >= w.c ? 0 : k >= fresh ? 1 : 2;
        }
    }
#pragma unroll
    for (int t = 0; t < LEAF_ITERS; ++t) {
        const int64_t node = node0 + t, f = node * FAN + lane;
        uint32_t p = old[t];
        if (rule[t] == 0 || flag[t]) p = 0;
        else if (rule[t] == 1) p = p_max;
        if (p != old[t]) table[f] = p;                               // never past the table: there old and p are both 0
        const uint64_t sum = wave_sum(p);
        if (lane == 0 && node < lv.n1) lv.l1[node] = sum;
        block_sum += sum;
        if (p && p < my_min) my_min = p;
        valid += (uint32_t)__popcll(__ballot(p != 0));
    }
    my_min = wave_min(my_min);
    if (lane == 0) {
        s_sum[wave] = block_sum;
        s_min[wave] = my_min;
        s_valid[wave] = valid;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t sum = 0;
        uint32_t mn = 0xffffffffu, v = 0;
        for (int k = 0; k < LEAF_WAVES; ++k) {
            sum += s_sum[k];
            mn = s_min[k] < mn ? s_min[k] : mn;
            v += s_valid[k];
        }
        lv.l2[blockIdx.x] = sum;
        lv.bmin[blockIdx.x] = mn;
        lv.bvalid[blockIdx.x] = v;
    }
}

__global__ __launch_bounds__(TOP_WG) void refresh_top(const Ring r, const Levels lv, uavx_prio_record *__restrict__ rec) {
    __shared__ uint64_t s3[MAX_N3], s4[FAN], s_valid[TOP_WAVES];
    __shared__ uint32_t s_min[TOP_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t j = wave; j < lv.n3; j += TOP_WAVES) {
        const int64_t c = j * FAN + lane;
        const uint64_t sum = wave_sum(c < lv.n2 ? lv.l2[c] : 0);
        if (lane == 0) {
            lv.l3[j] = sum;
            s3[j] = sum;
        }
    }
    uint32_t mn = 0xffffffffu;
    uint64_t valid = 0;
    for (int64_t b = threadIdx.x; b < lv.n2; b += TOP_WG) {
        const uint32_t m = lv.bmin[b];
        mn = m < mn ? m : mn;
        valid += lv.bvalid[b];
    }
    mn = wave_min(mn);
    valid = wave_sum(valid);
    if (lane == 0) {
        s_min[wave] = mn;
        s_valid[wave] = valid;
    }
    __syncthreads();
    if (wave < lv.n4) {
        const int64_t c = (int64_t)wave * FAN + lane;
        const uint64_t sum = wave_sum(c < lv.n3 ? s3[c] : 0);
        if (lane == 0) {
            lv.l4[wave] = sum;
            s4[wave] = sum;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t total = 0, v = 0;
        uint32_t m = 0xffffffffu;
        for (int64_t k = 0; k < lv.n4; ++k) total += s4[k];
        for (int k = 0; k < TOP_WAVES; ++k) {
            m = s_min[k] < m ? s_min[k] : m;
            v += s_valid[k];
        }
        rec->total = total;
        rec->p_min = v ? m : 0;                  // 2^32 − 1 is a priority too: `valid` says whether there is a minimum
        rec->valid = v;
        rec->seen = window(r).c;
    }
}

// ---- sample ----------------------------------------------------------------------------------------------------------------

struct SampleArgs {
    const float *u;
    int32_t rows, stratified;
    float beta;
    const float *beta_dev;
    float *state, *action, *reward, *next_state, *mask;
    uint8_t *truncated, *ended_out;
    int64_t *key;
    float *weight;
};

// One level of the search, by the GROUP lanes of a row: lane l holds the PER children l·PER .. l·PER + PER − 1 of the node in
// v (0 past `count`).  -> the first child whose inclusive prefix sum exceeds `left` (the last child if none does: a table
// that disagrees with its sums), with `left` reduced by the sum of the children before it.
static_assert(GROUP < 32 && GROUP * PER == FAN, "the group's ballot bits fit a 32-bit mask");

template <typename V>
__device__ inline int descend(const V (&v)[PER], int count, uint64_t &left) {
    const int l = threadIdx.x & (GROUP - 1);
    uint64_t mine = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) mine += v[k];
    uint64_t inc = mine;
#pragma unroll
    for (int d = 1; d < GROUP; d <<= 1) {
        const uint64_t o = shfl_up64(inc, d, GROUP);
        if (l >= d) inc += o;
    }
    const uint64_t hits = __ballot(inc > left) >> ((threadIdx.x & 63) & ~(GROUP - 1));
    const uint32_t hit = (uint32_t)hits & ((1u << GROUP) - 1);
    const int owner = hit ? __ffs(hit) - 1 : (count - 1) / PER;
    // every lane resolves its own children as if it were the owner; the owner's answer is the one handed round
    uint64_t rem = left - (inc - mine);
    int c = PER - 1;
    bool found = false;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const bool here = !found && rem < v[k];
        c = here ? k : c;
        found = found || here;
        rem = found ? rem : rem - v[k];
    }
    c += l * PER;
    c = c < count ? c : count - 1;
    left = shfl64(rem, owner, GROUP);
    return __shfl(c, owner, GROUP);
}

template <typename V>
__device__ inline void children(V (&v)[PER], const V *__restrict__ level, int64_t base, int count) {
    const int first = (threadIdx.x & (GROUP - 1)) * PER;
#pragma unroll
    for (int k = 0; k < PER; ++k) v[k] = first + k < count ? level[base + first + k] : 0;
}

// a level of `n` nodes: the children of `node` -> the chosen child's index in the level
template <typename V>
__device__ inline int64_t level_step(const V *__restrict__ level, int64_t n, int64_t node, uint64_t &left) {
    const int64_t base = node * FAN, rest = n - base;
    const int count = rest < FAN ? (int)rest : FAN;
    V v[PER];
    children(v, level, base, count);
    return base + descend(v, count, left);
}

__global__ __launch_bounds__(SAMPLE_WG) void sample_rows(const Ring r, const uint32_t *__restrict__ table, const Levels lv,
                                                         const uavx_prio_record *__restrict__ rec, const SampleArgs a) {
    const int l = threadIdx.x & (GROUP - 1);
    const int64_t row = ((int64_t)blockIdx.x * SAMPLE_WG + threadIdx.x) / GROUP;
    if (((int64_t)blockIdx.x * SAMPLE_WG + (threadIdx.x & ~63)) / GROUP >= a.rows) return;      // the wavefront's first row
    const bool live = row < a.rows;
    const int64_t j = live ? row : a.rows - 1;       // idle groups of the last wavefront go through the motions
    const Window w = window(r);
    const uint64_t total = rec->total;
    const int64_t per_slot = (int64_t)r.E * r.NL;
    int32_t s, e, i;
    int64_t key = -1;
    uint32_t p = 0;
    if (total == 0) {
        s = (int32_t)((w.c - 1) % r.L);
        e = i = 0;
    } else {
        const double uj = (double)a.u[j];
        const double t = a.stratified ? ((double)j + uj) / (double)a.rows : uj;
        uint64_t left;
        if (!(t > 0.0)) left = 0;
        else if (t >= 1.0) left = total - 1;
        else {
            left = (uint64_t)floor(t * (double)total);
            if (left > total - 1) left = total - 1;
        }
        int64_t node = 0;                            // a level with a single node is not searched
        if (lv.n4 > 1) node = level_step(lv.l4, lv.n4, 0, left);
        if (lv.n3 > 1) node = level_step(lv.l3, lv.n3, node, left);
        if (lv.n2 > 1) node = level_step(lv.l2, lv.n2, node, left);
        if (lv.n1 > 1) node = level_step(lv.l1, lv.n1, node, left);
        const int64_t base = node * FAN, rest = lv.n - base;
        const int count = rest < FAN ? (int)rest : FAN;
        uint32_t v[PER];
        children(v, table, base, count);
        const int c = descend(v, count, left);
        const int64_t f = base + c;
#pragma unroll
        for (int k = 0; k < PER; ++k) p = c % PER == k ? v[k] : p;       // a select: no indexed register array
        p = (uint32_t)__shfl((int)p, c / PER, GROUP);
        s = (int32_t)(f / per_slot);
        const int32_t rest_f = (int32_t)(f - (int64_t)s * per_slot);
        e = rest_f / r.NL;
        i = rest_f - e * r.NL;
        key = step_of(w, s, r.L) * per_slot + rest_f;
    }
    if (!live) return;
    int32_t s1 = s + 1;
    if (s1 >= r.L) s1 -= r.L;
    const int64_t se = (int64_t)s * r.E + e, cell = se * r.N + i, cell1 = ((int64_t)s1 * r.E + e) * r.N + i;
    static_assert(GROUP >= 2 * (OBS / 2) + 2, "state, next state, action and the scalars each have their lanes");
    if (l < OBS / 2) {
        ((float2 *)(a.state + j * OBS))[l] = ((const float2 *)(r.obs + cell * OBS))[l];
    } else if (l < OBS) {
        ((float2 *)(a.next_state + j * OBS))[l - OBS / 2] = ((const float2 *)(r.obs + cell1 * OBS))[l - OBS / 2];
    } else if (l == OBS) {
        *(float2 *)(a.action + j * 2) = *(const float2 *)(r.act + cell * 2);
    } else if (l == OBS + 1) {
        float weight = 0.f;
        if (p) {
            const float beta = a.beta_dev ? *a.beta_dev : a.beta;
            weight = (float)pow((double)rec->p_min / (double)p, (double)beta);
        }
        a.reward[j] = r.rew[cell];
        a.mask[j] = 1.f - (float)(r.done[cell] & 1);
        a.key[j] = key;
        a.weight[j] = weight;
        if (a.truncated) {
            uint8_t tr, en;
            if (r.skip) {
                tr = r.trunc[se] != 0;
                en = r.ended[se] != 0;
            } else {
                const uint8_t b = r.done[se * r.N];
                tr = (b >> 3) & 1;
                en = (b >> 2) & 1;
            }
            a.truncated[j] = tr;
            a.ended_out[j] = en;
        }
    }
}

// ---- update ----------------------------------------------------------------------------------------------------------------

struct UpdateArgs {
    const int64_t *key;
    const float *q, *y;
    int64_t y_stride;
    int32_t rows, towers;
    double alpha, eps;
};

// the entry row j addresses, −1 if the row is ignored
__device__ inline int64_t entry_of(const Ring &r, const Window &w, int64_t key) {
    if (key < 0) return -1;
    const int64_t per_slot = (int64_t)r.E * r.NL, k = key / per_slot;
    if (k < w.lo || k >= w.c) return -1;
    return (k % r.L) * per_slot + (key - k * per_slot);
}

__global__ __launch_bounds__(UPDATE_WG) void update_clear(const Ring r, uint32_t *__restrict__ table, const UpdateArgs a) {
    const int64_t j = (int64_t)blockIdx.x * UPDATE_WG + threadIdx.x;
    if (j >= a.rows) return;
    const int64_t f = entry_of(r, window(r), a.key[j]);
    if (f >= 0) table[f] = 0;
}

__global__ __launch_bounds__(UPDATE_WG) void update_max(const Ring r, uint32_t *__restrict__ table,
                                                        uavx_prio_record *__restrict__ rec, const UpdateArgs a) {
    const int64_t j = (int64_t)blockIdx.x * UPDATE_WG + threadIdx.x;
    uint32_t p = 0;
    if (j < a.rows) {
        const int64_t f = entry_of(r, window(r), a.key[j]);
        if (f >= 0) {
            float d = a.q[j];
            if (a.y) {
                const float y = a.y[j * a.y_stride];
                d = fabsf(d - y);
                if (a.towers == 2) {
                    const float d1 = fabsf(a.q[(int64_t)a.rows + j] - y);
                    d = (d1 > d || d1 != d1) ? d1 : d;       // a NaN in either tower stays
                }
            } else {
                d = fabsf(d);
            }
            const double b = (double)d + a.eps;
            // a delta that is not finite is settled first, whatever alpha: NaN gives 1 and +inf the top (pow(x, 0) would
            // make both 1.0)
            const double x = (a.alpha == 1.0 ? b : a.alpha == 0.0 ? 1.0 : pow(b, a.alpha)) * 65536.0 + 0.5;
            if (b != b) p = 1;
            else if (b == INFINITY) p = 0xffffffffu;
            else if (!(x >= 1.0)) p = 1;
            else if (x >= 4294967295.0) p = 0xffffffffu;
            else p = (uint32_t)floor(x);
            atomicMax(table + f, p);
        }
    }
    const uint32_t top = wave_max(p);
    if ((threadIdx.x & 63) == 0 && top) atomicMax(&rec->p_max, top);
}

// ---- host ------------------------------------------------------------------------------------------------------------------

static int64_t up16(int64_t b) { return (b + 15) / 16 * 16; }

// the levels' sizes and, with a base, their places in the caller's memory -> bytes
static int64_t carve(int64_t n, void *base, Levels &lv) {
    lv.n = n;
    lv.n1 = (n + FAN - 1) / FAN;
    lv.n2 = (lv.n1 + FAN - 1) / FAN;
    lv.n3 = (lv.n2 + FAN - 1) / FAN;
    lv.n4 = (lv.n3 + FAN - 1) / FAN;
    char *p = (char *)base;
    int64_t off = 0;
    lv.l1 = (uint64_t *)(p + off); off += up16(lv.n1 * 8);
    lv.l2 = (uint64_t *)(p + off); off += up16(lv.n2 * 8);
    lv.l3 = (uint64_t *)(p + off); off += up16(lv.n3 * 8);
    lv.l4 = (uint64_t *)(p + off); off += up16(lv.n4 * 8);
    lv.bmin = (uint32_t *)(p + off); off += up16(lv.n2 * 4);
    lv.bvalid = (uint32_t *)(p + off); off += up16(lv.n2 * 4);
    return off;
}

// everything a call checks of the shared state; fills r and lv
static int check_state(const uavx_prio_state *st, Ring &r, Levels &lv) {
    if (!st || !replay_view(st->ring, st->count, st->count_dev, r)) return UAVX_ACTOR_ERR_INVALID_ARG;
    const uavx_replay_ring *ring = st->ring;
    // slots·envs·learners <= 2^26, without overflowing on the way
    if (ring->envs > UAVX_PRIO_MAX_ENTRIES / ring->slots ||
        ring->learners > UAVX_PRIO_MAX_ENTRIES / (ring->slots * ring->envs))
        return UAVX_ACTOR_ERR_INVALID_ARG;
    if (!st->table || !aligned(st->table, 4) || !st->sums || !aligned(st->sums, 16) || !st->rec || !aligned(st->rec, 8))
        return UAVX_ACTOR_ERR_INVALID_ARG;
    if (st->sums_bytes < carve(ring->slots * ring->envs * ring->learners, st->sums, lv)) return UAVX_ACTOR_ERR_INVALID_ARG;
    return UAVX_ACTOR_OK;
}

}  // namespace uavx_prio_k

using namespace uavx_prio_k;

extern "C" {

UAVX_BUILD_MARKER(UAVX_PRIO_SRC_HASH);

int uavx_prio_version(void) { return UAVX_PRIO_VERSION; }

int uavx_prio_state_bytes(int64_t entries, int64_t *bytes) {
    if (!bytes || entries < 1 || entries > UAVX_PRIO_MAX_ENTRIES) return UAVX_ACTOR_ERR_INVALID_ARG;
    Levels lv;
    *bytes = carve(entries, nullptr, lv);
    return UAVX_ACTOR_OK;
}

int uavx_prio_refresh(const uavx_prio_state *state, void *stream) {
    Ring r{};
    Levels lv{};
    int rc = check_state(state, r, lv);
    if (rc != UAVX_ACTOR_OK) return rc;
    const hipStream_t st = (hipStream_t)stream;
    rc = launch(refresh_leaves, lv.n2, LEAF_WG, st, r, state->table, lv, state->rec);
    return rc != UAVX_ACTOR_OK ? rc : launch(refresh_top, 1, TOP_WG, st, r, lv, state->rec);
}

int uavx_prio_sample(const uavx_prio_state *state, const uavx_prio_sample_args *g, void *stream) {
    Ring r{};
    Levels lv{};
    const int rc = check_state(state, r, lv);
    if (rc != UAVX_ACTOR_OK) return rc;
    if (!g) return UAVX_ACTOR_ERR_INVALID_ARG;
    const int64_t rows = g->rows;
    if (rows < 0 || rows > UAVX_PRIO_MAX_ROWS) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (g->stratified != 0 && g->stratified != 1) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (g->beta_dev ? !aligned(g->beta_dev, 4) : !unit(g->beta)) return UAVX_ACTOR_ERR_INVALID_ARG;
    if ((g->truncated == nullptr) != (g->ended == nullptr)) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (rows == 0) return UAVX_ACTOR_OK;
    if (!g->u || !g->state || !g->action || !g->reward || !g->next_state || !g->mask || !g->key || !g->weight)
        return UAVX_ACTOR_ERR_INVALID_ARG;
    if (!aligned(g->u, 4) || !aligned(g->state, 8) || !aligned(g->action, 8) || !aligned(g->next_state, 8) ||
        !aligned(g->reward, 4) || !aligned(g->mask, 4) || !aligned(g->key, 8) || !aligned(g->weight, 4))
        return UAVX_ACTOR_ERR_INVALID_ARG;
    SampleArgs a{};
    a.u = g->u;
    a.rows = (int32_t)rows;
    a.stratified = g->stratified;
    a.beta = g->beta;
    a.beta_dev = g->beta_dev;
    a.state = g->state;
    a.action = g->action;
    a.reward = g->reward;
    a.next_state = g->next_state;
    a.mask = g->mask;
    a.truncated = g->truncated;
    a.ended_out = g->ended;
    a.key = g->key;
    a.weight = g->weight;
    const int64_t per_block = SAMPLE_WG / GROUP;
    return launch(sample_rows, (rows + per_block - 1) / per_block, SAMPLE_WG, (hipStream_t)stream, r, state->table, lv,
                  state->rec, a);
}

int uavx_prio_update(const uavx_prio_state *state, const int64_t *key, const float *q, int32_t towers, const float *y,
                     int64_t y_stride, int64_t rows, double alpha, double eps, void *stream) {
    Ring r{};
    Levels lv{};
    int rc = check_state(state, r, lv);
    if (rc != UAVX_ACTOR_OK) return rc;
    if (rows < 0 || rows > UAVX_PRIO_MAX_ROWS) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (towers < 1 || towers > UAVX_PRIO_MAX_TOWERS || (!y && towers != 1)) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (y && y_stride < 1) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (!unit(alpha) || !(eps > 0.0) || !(eps < INFINITY)) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (rows == 0) return UAVX_ACTOR_OK;
    if (!key || !aligned(key, 8) || !q || !aligned(q, 4) || !aligned(y, 4)) return UAVX_ACTOR_ERR_INVALID_ARG;
    UpdateArgs a{};
    a.key = key;
    a.q = q;
    a.y = y;
    a.y_stride = y_stride;
    a.rows = (int32_t)rows;
    a.towers = towers;
    a.alpha = alpha;
    a.eps = eps;
    const hipStream_t st = (hipStream_t)stream;
    const int64_t blocks = (rows + UPDATE_WG - 1) / UPDATE_WG;
    rc = launch(update_clear, blocks, UPDATE_WG, st, r, state->table, a);
    return rc != UAVX_ACTOR_OK ? rc : launch(update_max, blocks, UPDATE_WG, st, r, state->table, state->rec, a);
}

}  // extern "C"

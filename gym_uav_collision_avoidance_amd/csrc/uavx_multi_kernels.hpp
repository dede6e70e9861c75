// uavx_multi_kernels.hpp -- the __global__ kernels behind the C ABI (step_kernel lives with step_agent in uavx_multi_step.hpp):
// step_ex / step_k / observe / reset, the extension and state-exchange plumbing, the float64-position mode (uavx_multi_f64.hpp),
// the self test and the polar conversion.  Included by uavx_multi.hip inside namespace uavx, last of the device parts.

// uavx_step_ex: the step launch plus the trainer loop's bookkeeping (polar action conversion,
// episode returns, next-step auto-reset).  Same step_agent body as step_kernel.
// Register budget (profiles/r02_ab_notes.md): one agent record instead of three and the statistics fold read back at the end
// took the variant with bodies from 83 to 72 VGPRs and the N = 8 one from 89 to 79; with the staging path (stage_ahead) in the
// same kernel the variant with bodies is bounded at 6 wavefronts per SIMD (74 VGPRs, no spill; 7 = 72 VGPRs with scratch
// reloads in the hot path: 22.3 -> 23.8 us).  The same kind of bound on the N = 8 variant spills in its hot path, not applied.
#ifndef UAVX_EXB
#define UAVX_EXB 8
#endif
#ifndef UAVX_EX8B
#define UAVX_EX8B 8    // the 8-UAV specialisation: 65 536 x 8 is exactly 8 wavefronts per SIMD
#endif
#define UAVX_EX_KERNEL step_ex_kernel
#define UAVX_EX_REF false
#include "uavx_step_ex.hpp"
#undef UAVX_EX_KERNEL
#undef UAVX_EX_REF
#define UAVX_EX_KERNEL step_ex_ref_kernel
#define UAVX_EX_REF true
#include "uavx_step_ex.hpp"
#undef UAVX_EX_KERNEL
#undef UAVX_EX_REF

// K consecutive steps per launch from an action tape (open-loop rollouts): agent state stays in
// registers, only actions are read and obs/rew/done written per step.
template <int NT, bool ACT64, int W>
__global__ __launch_bounds__(kWave * W) void step_k_kernel(MultiParams p, const void *__restrict__ actions, int evaluate,
                                                           int K, int tape_out, float *__restrict__ obs_out,
                                                           float *__restrict__ rew_out, uint8_t *__restrict__ done_out) {
    using LDS = LdsT<false, W>;
    __shared__ LDS lds;
    const int N = NT ? NT : p.N;
    const LaneMap m = lane_map<NT, false, W>(p);
    AgentRegs s = {};
    if (m.active) load_agent(p, m.a, s);
    const uint32_t flags_in = s.flags;
    const size_t A = (size_t)p.E * N;
    uint32_t reach_acc = 0, coll_acc = 0, nonfin_acc = 0;
    for (int k = 0; k < K; k++) {
        double ax = 0.0, ay = 0.0;
        const size_t abytes = (ACT64 ? 16 : 8) * A * k;
        if (m.active) load_action<ACT64>(reinterpret_cast<const char *>(actions) + abytes, m.a, ax, ay);
        float o[10], rew;
        uint32_t dn, re, ce;
        step_agent<NT, false>(p, p, m, lds, s, ax, ay, evaluate, o, rew, dn, re, ce);
        reach_acc += re;
        coll_acc += ce;
        nonfin_acc += !(fabsf(rew) < INFINITY) ? 1u : 0u;
        if (tape_out || k == K - 1) {
            const size_t off = tape_out ? (size_t)k * A : 0;
            if (m.active) {
                (rew_out + off)[m.a] = rew;
                (done_out + off)[m.a] = (uint8_t)dn;
            }
            store_obs_block<NT>(p, m, lds, o, obs_out + off * UAVX_OBS_DIM);
        } else {
            group_sync<LDS::kW>();
        }
    }
    if (m.active) {
        store_agent(p, m.a, s, flags_in);
        if (reach_acc) atomicAdd(&p.reach[m.e], reach_acc);  // MUW:221
        if (coll_acc) atomicAdd(&p.coll[m.e], coll_acc);     // MUW:209
        if (nonfin_acc) atomicAdd(&p.nonfin[m.e], nonfin_acc);
        if (m.lane == 0) atomicAdd(&p.wave_steps[m.wave], (uint32_t)K);  // MUW:238
    }
}

template <int NT, bool EXT, int W>
__global__ __launch_bounds__(kWave * W) void observe_kernel(MultiParams p, float *__restrict__ obs_out) {
    using LDS = LdsT<EXT, W>;
    __shared__ LDS lds;
    const LaneMap m = lane_map<NT, EXT, W>(p);
    AgentRegs s = {};
    if (m.active) load_agent(p, m.a, s);
    const WorldLims w = world_lims<EXT>(p, s.flags);
    const float tdx = s.tx - s.x, tdy = s.ty - s.y;
    const float dist_t = norm32(tdx, tdy);
    const float theta = atan2_fast((float)s.vy, (float)s.vx);
    const float dth = wrap_pi(atan2_fast(tdy, tdx) - theta);
    if (EXT && p.B > 0) stage_bodies<false>(p, m, lds, s.flags, false, 0u, 0u);
    if (m.active) {
        lds.pos[m.rbase + m.i] = make_float4(s.x, s.y, s.x, s.y);
        lds.theta[m.rbase + m.i] = theta;
    }
    group_sync<LDS::kW>();
    const Neigh nb = scan_neighbours<NT, false>(w.sq_sense, m, lds, s.x, s.y);
    const float speed = __builtin_amdgcn_sqrtf((float)fma(s.vy, s.vy, s.vx * s.vx));
    float o[10];
    assemble_obs(p, w, m, lds, nb, s.x, s.y, speed, theta, dist_t, dth, o);
    if (EXT && (s.flags & kFlagInactive)) {
#pragma unroll
        for (int k = 0; k < UAVX_OBS_DIM; k++) o[k] = 0.f;
    }
    store_obs_block<NT>(p, m, lds, o, obs_out);
}

// MUW:116-168 for the masked envs, same lane-per-agent mapping and sampler as the in-step auto-reset.
template <int NT, bool EXT, int W>
__global__ __launch_bounds__(kWave * W) void reset_kernel(MultiParams p, const uint8_t *__restrict__ mask, uint64_t seed) {
    using LDS = LdsT<EXT, W>;
    __shared__ LDS lds;
    const LaneMap m = lane_map<NT, EXT, W>(p);
    const bool go = m.active && (!mask || mask[m.e] != 0);
    if (!group_any<W>(go)) return;
    AgentRegs s = {};
    uint4 rec = make_uint4(0, 0, 0, 0);
    if (go) rec = p.env_rec[m.e];
    const uint32_t episode = rec.y & ~kRecEnded;
    EpisodeFold fold = {};
    uint32_t wc = 0;
    if (go && m.i == 0) {  // statistics words requested before the draw, consumed after it
        fold = fold_load(p, m.e);
        wc = p.wave_steps[m.wave];
    }
    reset_envs_wave<NT, EXT>(p, m, lds, go, episode, (uint32_t)seed, (uint32_t)(seed >> 32), s, p.body_pos, p.body_leg, p.lvl_cur);
    if (go) {
        p.pos[m.a] = make_float2(s.x, s.y);
        p.vel[m.a] = make_double2(0.0, 0.0);
        p.goal[m.a] = Goal{s.tx, s.ty, s.init_d, s.flags};
        if (m.i == 0) {
            fold_store(p, m.e, wc - rec.x, make_float2(__uint_as_float(rec.z), __uint_as_float(rec.w)), fold);
            p.env_rec[m.e] = make_uint4(wc, episode + 1u, 0u, 0u);  // MUW:166 steps = 0, new episode, no running return
        }
    }
}

// extension plumbing: level table upload, per-env level arrays, body records
__global__ __launch_bounds__(64) void upload_levels_kernel(LevelParams *dst, LevelTable t) {
    if (threadIdx.x < UAVX_MAX_LEVELS) dst[threadIdx.x] = t.l[threadIdx.x];
}
__global__ __launch_bounds__(kBlock) void env_levels_kernel(MultiParams p, const uint8_t *set_next, uint8_t *get_cur) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= p.E) return;
    if (set_next) p.lvl_next[e] = set_next[e];
    if (get_cur) get_cur[e] = p.lvl_cur[e];
}
// public body record (include/uavx.h): UAVX_BODY_DIM = 6 floats {x, y, dx, dy, heading, legs}
__global__ __launch_bounds__(kBlock) void bodies_kernel(MultiParams p, const float *set, float *get) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= p.E * p.B) return;
    if (set) {
        const float *r = set + i * UAVX_BODY_DIM;
        p.body_pos[i] = make_float2(r[0], r[1]);
        p.body_leg[i] = make_float4(r[2], r[3], r[4], r[5]);
    }
    if (get) {
        const float2 q = p.body_pos[i];
        const float4 leg = p.body_leg[i];
        float *r = get + i * UAVX_BODY_DIM;
        r[0] = q.x; r[1] = q.y; r[2] = leg.x; r[3] = leg.y; r[4] = leg.z; r[5] = leg.w;
    }
}

__global__ __launch_bounds__(kBlock) void episode_stats_kernel(MultiParams p, uint32_t *counts, float *returns, int clear) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= p.E) return;
    if (clear) {
        p.fin_counts[e] = make_uint4(0, 0, 0, 0);
        p.fin_returns[e] = make_float2(0.f, 0.f);
        return;
    }
    if (counts) {
        const uint4 c = p.fin_counts[e];
        counts[4 * e] = c.x; counts[4 * e + 1] = c.y; counts[4 * e + 2] = c.z; counts[4 * e + 3] = c.w;
    }
    if (returns) {
        const float2 f = p.fin_returns[e];
        returns[2 * e] = f.x; returns[2 * e + 1] = f.y;
    }
}

__global__ __launch_bounds__(kBlock) void get_state_kernel(MultiParams p, uavx_state_view v) {
    const int64_t a = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t A = p.E * p.N;
    if (a < A) {
        const float2 d = p.pos[a];
        const Goal g = p.goal[a];
        if (v.loc) { v.loc[2 * a] = d.x; v.loc[2 * a + 1] = d.y; }
        if (v.prev_d) v.prev_d[a] = (g.flags & kFlagPrevOvr) ? p.prev_ovr[a] : natural_prev_d(g.flags, d.x, d.y, g.tx, g.ty);
        if (v.flags) v.flags[a] = (uint8_t)(g.flags & kFlagPublic);
        if (v.vel) { const double2 w = p.vel[a]; v.vel[2 * a] = w.x; v.vel[2 * a + 1] = w.y; }
        if (v.tgt) { v.tgt[2 * a] = g.tx; v.tgt[2 * a + 1] = g.ty; }
        if (v.init_d) v.init_d[a] = g.init_d;
    }
    if (a < p.E && v.counters) {
        const uint4 rec = p.env_rec[a];
        v.counters[4 * a + 0] = p.wave_steps[a / p.epw] - rec.x; v.counters[4 * a + 1] = p.reach[a];
        v.counters[4 * a + 2] = p.coll[a];  v.counters[4 * a + 3] = rec.y & ~kRecEnded;
    }
}

// Overwrites any subset of the UAVAgent fields.  prev_distance keeps the VALUE the reference would hold: a
// field the caller does not pass stays what it was (e.g. poking only .location leaves prev_distance stale,
// test_sac_multi_plot_trajectory.py:43-49), and whenever that value is not the one derived from the new
// (flags, location, target) it is parked in prev_ovr[] behind the PREVD_OVR bit until the next step.
__global__ __launch_bounds__(kBlock) void set_state_kernel(MultiParams p, uavx_state_view v) {
    const int64_t a = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t A = p.E * p.N;
    const bool agent_fields = v.loc || v.vel || v.tgt || v.init_d || v.prev_d || v.flags;
    if (a < A && agent_fields) {
        float2 d = p.pos[a];
        Goal g = p.goal[a];
        const float old_prev = (g.flags & kFlagPrevOvr) ? p.prev_ovr[a] : natural_prev_d(g.flags, d.x, d.y, g.tx, g.ty);
        if (v.loc) { d.x = v.loc[2 * a]; d.y = v.loc[2 * a + 1]; }
        if (v.tgt) { g.tx = v.tgt[2 * a]; g.ty = v.tgt[2 * a + 1]; }
        if (v.init_d) g.init_d = v.init_d[a];
        uint32_t flags = g.flags & ~kFlagPrevOvr;
        if (v.flags) flags = ((uint32_t)v.flags[a] & kFlagPublic) | (g.flags & kLevelMask);  // a caller-set done flag is not "just finished"
        const float want = v.prev_d ? v.prev_d[a] : old_prev;
        const float nat = natural_prev_d(flags, d.x, d.y, g.tx, g.ty);
        if (__float_as_uint(want) != __float_as_uint(nat)) {
            flags |= kFlagPrevOvr;
            p.prev_ovr[a] = want;
        }
        g.flags = flags;
        p.pos[a] = d;
        p.goal[a] = g;
        if (v.vel) p.vel[a] = make_double2(v.vel[2 * a], v.vel[2 * a + 1]);
    }
    if (a < p.E && v.counters) {
        uint4 rec = p.env_rec[a];
        rec.x = p.wave_steps[a / p.epw] - v.counters[4 * a + 0];
        rec.y = (rec.y & kRecEnded) | (v.counters[4 * a + 3] & ~kRecEnded);
        p.env_rec[a] = rec;
        p.reach[a] = v.counters[4 * a + 1]; p.coll[a] = v.counters[4 * a + 2];
    }
}

#include "uavx_multi_f64.hpp"

// uavx_selftest(): sqrt_rn() against the compiler's IEEE sqrtf on every float32 bit pattern 0 ... 0x7f800000 (all
// non-negative values and +inf) plus the NaN / negative patterns of one exponent; counts differing results.
__global__ __launch_bounds__(256) void sqrt_selftest_kernel(unsigned long long *mismatches) {
    const uint32_t stride = gridDim.x * blockDim.x;
    unsigned int bad = 0;
    for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b <= 0x7f800000ull + 0x00800000ull; b += stride) {
        const float s = __uint_as_float((uint32_t)b);     // the last 2^23 patterns are NaNs
        const uint32_t got = __float_as_uint(sqrt_rn(s)), want = __float_as_uint(sqrtf(s));
        const bool both_nan = (got & 0x7fffffffu) > 0x7f800000u && (want & 0x7fffffffu) > 0x7f800000u;
        bad += (got != want && !both_nan) ? 1u : 0u;
    }
    if (bad) atomicAdd(mismatches, (unsigned long long)bad);
}

// uavx_polar_commands(): the reference polar conversion alone, one action per thread
template <bool ACT64>
__global__ __launch_bounds__(kBlock) void polar_commands_kernel(const void *__restrict__ actions, int64_t n, float scale,
                                                                double2 *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    double ax, ay;
    if (ACT64) {
        const double2 v = reinterpret_cast<const double2 *>(actions)[i];
        ax = v.x; ay = v.y;
    } else {
        const float2 v = reinterpret_cast<const float2 *>(actions)[i];
        ax = (double)v.x; ay = (double)v.y;
    }
    polar_to_command_ref<ACT64>(scale, ax, ay);
    out[i] = make_double2(ax, ay);
}

// uavx_multi_step.hpp -- one env step of one agent (observation, scripted bodies, step_agent) and the one-step kernel
// step_kernel.  Included by uavx_multi.hip inside namespace uavx, after uavx_multi_scan.hpp.

// MUW:60-109 in float32 (angles compared on the circle; see DESIGN.md numerics).
template <class LDS, class H>
__device__ __forceinline__ void assemble_obs(const H &h, const WorldLims &w, const LaneMap &m, const LDS &lds,
                                             const Neigh &nb, float nx, float ny, float speed, float theta, float dist_t,
                                             float dth, float o[10]) {
    o[0] = speed * h.inv_vmax_norm;  // MUW:62
    o[1] = theta * kInvPi;           // MUW:64
    o[2] = dist_t * w.inv_diag;      // MUW:68
    o[3] = dth * kInvPi;             // MUW:72
    // absent neighbour: d=1, bearing (pi + theta) - theta wraps to +-pi -> +-1 (one point on the circle), heading 0
    const bool has1 = nb.j1 >= 0, has2 = nb.j2 >= 0;
    const int i1 = m.rbase + (has1 ? nb.j1 : 0), i2 = m.rbase + (has2 ? nb.j2 : 0);
    const float4 q1 = lds.pos[i1], q2 = lds.pos[i2];
    const float t1 = lds.theta[i1], t2 = lds.theta[i2];
    const float b1 = wrap_unit(atan2_fast(q1.w - ny, q1.z - nx) - theta);  // MUW:78-81
    const float b2 = wrap_unit(atan2_fast(q2.w - ny, q2.z - nx) - theta);  // MUW:88-91
    const float h1 = wrap_unit(t1 - theta);                                // MUW:82-85
    const float h2 = wrap_unit(t2 - theta);                                // MUW:92-95
    o[4] = has1 ? nb.d1 * w.inv_sense : 1.f;                                      // MUW:77
    o[5] = has1 ? b1 : 1.f;
    o[6] = has1 ? h1 : 0.f;
    o[7] = has2 ? nb.d2 * w.inv_sense : 1.f;                                      // MUW:87
    o[8] = has2 ? b2 : 1.f;
    o[9] = has2 ? h2 : 0.f;
}

// Wave-cooperative store of the wave's contiguous obs block (cnt*40 B starting at slot a0): the
// lane-major [64][10] tile is staged in LDS and written back with lane-contiguous vector stores.
// Even N: a0 and cnt are even, so the block is 16-byte aligned and a whole number of float4
// (uavx_create/step check the 16-byte alignment of the caller's obs pointer); otherwise float2.
// FLAT (step_kernel at N = 4; -DUAVX_OBSFLAT=0: off, A/B): the three store rounds without their
// `f < nfloat` guards, so that the three LDS reads are issued together and the three stores follow instead of read -> wait ->
// store -> restore EXEC three times in series.  Only the last workgroup can be partial; its rows beyond cnt lie at or above
// nslot (a0 + cnt = E * N) and cnt * 40 B is a multiple of 16, so those stores are dropped whole by the buffer bounds check.
// The tile is 2.5 rounds long: the upper half of the third round reads the tile's last row (in bounds) and stores out of range.
#ifndef UAVX_OBSFLAT
#define UAVX_OBSFLAT 1
#endif
template <int NT, class LDS, bool FLAT = false>
__device__ __forceinline__ void store_obs_block(uint32_t nslot, int n_agents, const LaneMap &m, LDS &lds, const float o[10],
                                                float *obs_out) {   // nslot = E * N, n_agents = N (read when NT == 0)
    constexpr int T = kWave * LDS::kW;
    float *stage = lds.obs + m.obs0;
    if (m.active) {
        float2 *dst = reinterpret_cast<float2 *>(stage + m.lane * UAVX_OBS_DIM);
#pragma unroll
        for (int k = 0; k < 5; k++) dst[k] = make_float2(o[2 * k], o[2 * k + 1]);
    }
    group_sync<LDS::kW>();
    const int nfloat = m.cnt * UAVX_OBS_DIM;
    const rsrc_t r = make_rsrc(obs_out, nslot * (UAVX_OBS_DIM * 4u));
    const uint32_t gbase = m.a0 * (UAVX_OBS_DIM * 4u);  // byte offset of the workgroup's block
    if constexpr (UAVX_OBSFLAT && FLAT && NT != 0 && NT % 2 == 0 && LDS::kW == 1) {
        constexpr int kTile = kWave * UAVX_OBS_DIM;
        static_assert(kTile % 4 == 0 && 3 * T * 4 >= kTile, "three rounds of float4 cover the tile");
        float4 v[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int f = (k * T + m.lane) * 4;
            v[k] = *reinterpret_cast<const float4 *>(stage + ((k + 1) * T * 4 <= kTile ? f : min(f, kTile - 4)));
        }
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int f = (k * T + m.lane) * 4;
            const uint32_t off = gbase + f * 4u;
            store16_wt(r, ((k + 1) * T * 4 <= kTile || f < kTile) ? off : nslot * (UAVX_OBS_DIM * 4u), v[k]);
        }
    } else if (NT ? (NT % 2 == 0) : ((n_agents & 1) == 0)) {   // uniform: even N => 16-byte aligned block of whole float4
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int f = (k * T + m.lane) * 4;
            if (f < nfloat) store16_wt(r, gbase + f * 4u, *reinterpret_cast<const float4 *>(stage + f));
        }
    } else {
        // odd N: the block starts 8 bytes off a 16-byte boundary in every second workgroup and ends likewise.  16-byte
        // stores for the aligned middle, one 8-byte store for a misaligned head / tail (8-byte write-through stores run at
        // 0.54-0.70x the 16-byte rate: round 1 wrote the whole block that way)
        const int head = (gbase & 8u) ? 2 : 0;          // uniform over the workgroup
        const int mid = (nfloat - head) / 4;              // float4 count
        const int tail = head + mid * 4;                  // first float after the middle (nfloat - tail is 0 or 2)
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int q = k * T + m.lane;
            if (q < mid) {
                const float *src = stage + head + q * 4;   // only 8-byte aligned in LDS: two ds_read_b64
                const float2 lo = *reinterpret_cast<const float2 *>(src), hi = *reinterpret_cast<const float2 *>(src + 2);
                store16_wt(r, gbase + (uint32_t)(head + q * 4) * 4u, make_float4(lo.x, lo.y, hi.x, hi.y));
            }
        }
        if (m.lane == 0 && head) store8_wt(r, gbase, *reinterpret_cast<const float2 *>(stage));
        if (m.lane == 1 && tail < nfloat) store8_wt(r, gbase + (uint32_t)tail * 4u, *reinterpret_cast<const float2 *>(stage + tail));
    }
    group_sync<LDS::kW>();
}
template <int NT, class LDS>
__device__ __forceinline__ void store_obs_block(const MultiParams &p, const LaneMap &m, LDS &lds, const float o[10],
                                                float *obs_out) {
    store_obs_block<NT>((uint32_t)p.E * (uint32_t)p.N, p.N, m, lds, o, obs_out);
}

// configs[4] extension: a body starts a leg at (x, y) towards waypoint (wx, wy) -- include/uavx.h, uavx_set_body_rule; float32,
// no FMA, IEEE division and square root, restated bit for bit by the oracle (body_leg).  Off the per-step path (reset, and one
// env step in `period`).
__device__ __forceinline__ float4 make_leg(float body_step, float x, float y, float wx, float wy) {
    const float dx = wx - x, dy = wy - y;
    const float d = norm32(dx, dy);
    float4 leg = make_float4(0.f, 0.f, 0.f, 0.f);
    if (d > 0.f) {
        const float sc = body_step / d;
        leg.x = dx * sc; leg.y = dy * sc;
        leg.w = floorf(d / body_step);   // body_step == 0 (static obstacle): +inf legs of zero displacement
    }
    leg.z = atan2_exact(dy, dx);
    return leg;
}

// configs[4] extension: the scripted bodies of this lane's env.  Body b is handled by the env's learner lane b % L in trip
// b / L: position (8 B) and leg record (16 B) loaded, moved when MOVE -- the bodies move BEFORE the learners of the env's
// sequential loop, so the collision tests and the observations of this step both see the new positions --, staged into its
// neighbour row {x, y, x, y} + heading, position stored back (8 B) if it moved.  A body that does not take part (b >= the
// level's b_active) is staged at +inf.
//   ready   the env was re-initialised by this call: its bodies' rows were staged by the reset path, they do not move.
template <bool MOVE, class LDS, bool LATEW = false>
__device__ __forceinline__ void stage_bodies(const MultiParams &p, const LaneMap &m, LDS &lds, uint32_t flags, bool ready,
                                             uint32_t steps, uint32_t ep_draw) {
    const int L = p.N;
    const bool leveled = p.n_levels > 0;
    const LevelParams *lv = &p.levels[(flags & kLevelMask) >> kLevelShift];   // read only when a curriculum is installed
    const int b_active = m.active ? (leveled ? lv->b_active : p.B) : 0;
    const uint32_t kk = steps & (uint32_t)p.body_pmask;     // steps of the current leg that lie behind the body
    const bool retarget = MOVE && steps != 0u && kk == 0u;  // a new waypoint every `period` steps
    const float kf = (float)kk;
#pragma unroll 1
    for (int k = 0; k < p.kb; k++) {
        const int b = k * L + m.i;
        const bool valid = m.active && b < p.B && !ready;
        const bool on = valid && b < b_active;
        const uint32_t gi = m.e * (uint32_t)p.B + (uint32_t)b;
        float2 q = make_float2(INFINITY, INFINITY);
        float4 leg = make_float4(0.f, 0.f, 0.f, 0.f);
        if (on) { q = p.body_pos[gi]; leg = p.body_leg[gi]; }
        if (on && retarget) {
            // (once per `period` steps: LATEW fetches what this needs from the kernel arguments here, not at the top)
            const ResetCandidates c = reset_candidates((uint64_t)LATE(LATEW, p, env_offset) + m.e, (uint32_t)(L + b),
                                                       0x80000000u | (steps >> p.body_pshift), ep_draw, LATE(LATEW, p, body_k0),
                                                       LATE(LATEW, p, body_k1), leveled ? lv->lox : LATE(LATEW, p, lox),
                                                       leveled ? lv->loy : LATE(LATEW, p, loy), leveled ? lv->hix : LATE(LATEW, p, hix),
                                                       leveled ? lv->hiy : LATE(LATEW, p, hiy));
            leg = make_leg(p.body_step, q.x, q.y, c.sx, c.sy);
            p.body_leg[gi] = leg;
        }
        if (MOVE && on && kf < leg.w) {
            q.x = q.x + leg.x; q.y = q.y + leg.y;
            p.body_pos[gi] = q;
        }
        if (valid) {
            lds.pos[m.rbase + L + b] = make_float4(q.x, q.y, q.x, q.y);
            lds.theta[m.rbase + L + b] = leg.z;
        }
    }
}

// One env step for this lane's agent (state in registers).  MUW:177-241.
//   frozen: the env was re-initialised by this call (auto-reset); the agent only observes.
//   EXT: env_steps / ep_draw = the env's step count before this step and the episode index its reset drew with
//        (scripted bodies); frozen envs had their bodies' rows staged by the reset path.
//   h: where the straight-line path reads the handle's parameters: `p` itself (compiler-placed loads of the argument segment) or
//      a HotParams the kernel fetched (step_kernel); same member names
template <int NT, bool EXT, class LDS, bool LATEW = false, bool SQ = false, class H = MultiParams>   // SQ: see scan_neighbours
__device__ __forceinline__ void step_agent(const MultiParams &p, const H &h, const LaneMap &m, LDS &lds, AgentRegs &s, double ax,
                                           double ay, int evaluate, float o[10], float &rew, uint32_t &done_out,
                                           uint32_t &reach_ev, uint32_t &coll_ev, bool frozen = false,
                                           uint32_t env_steps = 0, uint32_t ep_draw = 0) {
    const float sq_sense = sense_limit<EXT>(p, h, s.flags);
    const bool was_done = (s.flags & UAVX_FLAG_DONE) != 0;
    const bool parked = EXT && (s.flags & kFlagInactive) != 0;  // extension: learner switched off by its env's level
    if (!frozen) s.flags &= ~(kFlagPrevOvr | kFlagJustDone);  // from here on prev_distance is the natural one again
    const float ox = s.x, oy = s.y;
    float pd = 0.f, d = 0.f;  // AG:24-25: a done agent returns (0, 0) and does not move
    if (!was_done && !frozen && !parked) {
        axis_update(ax, h.tau, h.rtau, h.recip_ok != 0, h.amax, h.vmax, s.vx, s.x);  // AG:26-29
        axis_update(ay, h.tau, h.rtau, h.recip_ok != 0, h.amax, h.vmax, s.vy, s.y);
        pd = s.prev_d;                                       // AG:32
    }
    const float tdx = s.tx - s.x, tdy = s.ty - s.y;
    const float dist_t = norm32(tdx, tdy);                   // AG:33 / MUW:67
    if (!was_done) d = dist_t;
    // heading; finish() only rescales the velocity (AG:40), so one atan2 serves reward and obs
    const float theta = atan2_fast((float)s.vy, (float)s.vx);   // MUW:63,185
    const float dth = wrap_pi(atan2_fast(tdy, tdx) - theta);    // MUW:184-186 == MUW:69-71

    if (m.active) {
        lds.pos[m.rbase + m.i] = make_float4(ox, oy, s.x, s.y);   // a parked learner sits at +inf
        lds.theta[m.rbase + m.i] = theta;
    }
    if (EXT && p.B > 0) stage_bodies<true, LDS, LATEW>(p, m, lds, s.flags, frozen, env_steps, ep_draw);
    group_sync<LDS::kW>();
    const Neigh nb = scan_neighbours<NT, true, LDS, SQ>(sq_sense, m, lds, s.x, s.y);
    const WorldLims w = world_lims<EXT>(p, h, s.flags);

    // reward shaping, MUW:188-195 (float32, reciprocals instead of divisions; |error| << 1e-5)
    const float inv_init = __builtin_amdgcn_rcpf(s.init_d);
    float r = -0.01f * fminf(h.vmax_norm * inv_init, 1.0f);  // MUW:189
    r += (50.0f * h.inv_vmax_norm) * (pd - d);               // MUW:190 (pd - d is a float32 subtraction there too)
    const float frac = d * inv_init * (1.0f / 1.5f);         // MUW:192,194
    r *= (r > 0.f) ? (1.0f - frac) : (1.0f + frac);
    r -= 0.01f * fabsf(dth);                                 // MUW:195

    // collisions, MUW:197-210 (exact threshold tests on the squared distance)
    const bool collision = nb.step_sq_min <= w.sq_two_r;     // MUW:203  dist <= 2R
    if (collision) r = -2.0f;                                // MUW:204
    coll_ev = 0;
    if (nb.step_sq_min <= h.sq_hard && !(s.flags & (UAVX_FLAG_DONE | UAVX_FLAG_COLLIDED)) && !frozen) {  // MUW:207-208
        coll_ev = 1;                                         // MUW:209
        s.flags |= UAVX_FLAG_COLLIDED;                       // MUW:210
    }
    // termination, MUW:213-227
    const double sq = fma(s.vy, s.vy, s.vx * s.vx);          // MUW:214 (np.linalg.norm's float64 dot)
    const bool oob = !(s.x >= w.lo_x && s.x <= w.hi_x && s.y >= w.lo_y && s.y <= w.hi_y);  // MUW:213,224 (exact float32 form)
    float speed = __builtin_amdgcn_sqrtf((float)sq);         // obs feature only
    reach_ev = 0;
    if (frozen) {
        done_out = 0;
        r = 0.f;
    } else if (d < 0.5f && !collision && sq < h.speed_sq_lim) {     // MUW:218
        done_out = 1;
        reach_ev = was_done ? 0u : 1u;                       // MUW:220-221
        s.flags |= UAVX_FLAG_DONE | (was_done ? 0u : kFlagJustDone);  // AG:39
        const double nv = sqrt(sq);                          // AG:40
        double fx = s.vx / nv * 0.001, fy = s.vy / nv * 0.001;
        if (fx != fx || fy != fy) { fx = 0.0; fy = 0.0; }    // AG:41-42
        s.vx = fx; s.vy = fy;
        speed = __builtin_amdgcn_sqrtf((float)fma(fy, fy, fx * fx));
        r += 10.0f;                                          // MUW:223
    } else if (oob) {
        done_out = evaluate ? 0u : 1u;                       // MUW:224-225
    } else {
        done_out = 0;
    }
    if (!frozen) s.prev_d = d;                               // MUW:229
    rew = r;
    assemble_obs(h, w, m, lds, nb, s.x, s.y, speed, theta, dist_t, dth, o);  // MUW:233-235
    if (parked) {  // extension: a parked learner reports an all-zero observation, no reward, done
#pragma unroll
        for (int k = 0; k < UAVX_OBS_DIM; k++) o[k] = 0.f;
        rew = 0.f;
        done_out = frozen ? 0u : 1u;
    }
}

template <bool ACT64>
__device__ __forceinline__ void load_action(const void *__restrict__ actions, uint32_t a, double &ax, double &ay) {
    if (ACT64) {
        const double2 v = reinterpret_cast<const double2 *>(actions)[a];
        ax = v.x; ay = v.y;
    } else {
        const float2 v = reinterpret_cast<const float2 *>(actions)[a];
        ax = (double)v.x; ay = (double)v.y;
    }
}

// One env step per launch (the RL loop's shape: the policy runs between two launches).
// The arguments the FIRST instructions need -- command pointer, the base of the state allocation and the 32-bit offsets of its
// arrays, the numbers the lane mapping is made of -- are LEADING SCALAR kernel arguments: gfx950 preloads those into SGPRs before
// the wavefront starts (Makefile: -mllvm -amdgpu-kernarg-preload-count), so the state loads are the first thing a wavefront does
// instead of waiting for a scalar load of the argument segment.  A/B, same library, three runs each (profiles/r04_ab_notes.md
// section 10): 65 536 x 4 5.76 -> 5.56 us, x 8 10.4 -> 10.0, x 2 4.19 -> 4.09, 32 768 x 4 4.53 -> 4.35.
// The REST of the argument struct: a scheduling barrier behind the state loads was meant to put its scalar loads behind them.
// What the compiler emitted was those loads behind the WAIT for the state loads (it places a load of the invariant segment at
// its first use, and the barrier only fences what is in front of it): eleven s_load between the first `s_waitcnt vmcnt(0)` and
// the first LDS write of the 4-UAV kernel, the one for tau / rtau / amax / vmax followed at once by `s_waitcnt lgkmcnt(0)` -- a
// second round trip that every wavefront of the launch's single round paid at the same moment.  The plain variants (step_fetches)
// now fetch what the straight-line path needs THEMSELVES, between the state loads and that wait (fetch_step_args), and read
// nothing else of the arguments outside rare branches; tests/test_step_isa_host.py holds the instruction order.
// The variants with bodies / levels keep the compiler-placed loads.  Numbers: profiles/r12_karg_ab.md.
// (with bodies the allocator lands on 65 VGPRs = 7 wavefronts per SIMD; asking for 8 gives 62 without a spill)
#ifndef UAVX_STEPB
#define UAVX_STEPB 8
#endif
// What step_kernel's straight-line path needs of its argument segment, fetched by the kernel itself: three scalar loads through
// the laundered segment pointer (late_kargs), issued behind the state loads and in front of the wait for them.
//   dwordx8  at p.tau    tau, rtau, amax, vmax
//   dwordx16 at p.lo_x   lo_x .. hi_y, speed_sq_lim, sq_sense .. inv_diag, (two_r_reset,) recip_ok, (N)
//   dwordx8  behind p    evaluate, (padding,) obs_out, rew_out, done_out
// The body then reads these copies ONLY: one remaining read of `p.tau` or `rew_out` hands the compiler a second, invariant load
// that it places where it likes.  The rare branches (prev_ovr, the reach / coll / nonfin counters) fetch their pointer inside
// the branch.
constexpr uint32_t kStepLead = 56;   // MultiParams' place in step_kernel's argument segment (behind the preloaded scalars)
typedef uint32_t karg_x8 __attribute__((ext_vector_type(8), aligned(4)));
typedef uint32_t karg_x16 __attribute__((ext_vector_type(16), aligned(4)));
struct StepArgs {
    HotParams h;
    int evaluate;
    float *obs_out, *rew_out;
    uint8_t *done_out;
};
__device__ __forceinline__ double karg_f64(uint32_t lo, uint32_t hi) { return __hiloint2double((int)hi, (int)lo); }
template <class T>
__device__ __forceinline__ T *karg_ptr64(uint32_t lo, uint32_t hi) { return reinterpret_cast<T *>(((uint64_t)hi << 32) | lo); }
__device__ __forceinline__ StepArgs fetch_step_args() {
    const karg_ptr ka = late_kargs();
    const karg_x8 k = late_karg<karg_x8>(kStepLead + (uint32_t)offsetof(MultiParams, tau), ka);
    const karg_x16 l = late_karg<karg_x16>(kStepLead + (uint32_t)offsetof(MultiParams, lo_x), ka);
    const karg_x8 io = late_karg<karg_x8>(kStepLead + (uint32_t)sizeof(MultiParams), ka);
    // an (empty) reader of all three, HERE: without it the compiler sinks each load to its first use, behind the wait for the state
    asm volatile("" ::"s"(k), "s"(l), "s"(io));
    StepArgs a;
    a.h.tau = karg_f64(k[0], k[1]); a.h.rtau = karg_f64(k[2], k[3]); a.h.amax = karg_f64(k[4], k[5]); a.h.vmax = karg_f64(k[6], k[7]);
    a.h.lo_x = __uint_as_float(l[0]); a.h.lo_y = __uint_as_float(l[1]); a.h.hi_x = __uint_as_float(l[2]); a.h.hi_y = __uint_as_float(l[3]);
    a.h.speed_sq_lim = karg_f64(l[4], l[5]);
    a.h.sq_sense = __uint_as_float(l[6]); a.h.sq_two_r = __uint_as_float(l[7]); a.h.sq_hard = __uint_as_float(l[8]);
    a.h.inv_sense = __uint_as_float(l[9]); a.h.vmax_norm = __uint_as_float(l[10]); a.h.inv_vmax_norm = __uint_as_float(l[11]);
    a.h.inv_diag = __uint_as_float(l[12]);
    a.h.recip_ok = (int)l[14];
    a.evaluate = (int)io[0];
    a.obs_out = karg_ptr64<float>(io[2], io[3]); a.rew_out = karg_ptr64<float>(io[4], io[5]); a.done_out = karg_ptr64<uint8_t>(io[6], io[7]);
    return a;
}
static_assert(sizeof(MultiParams) % 8 == 0, "fetch_step_args: `int evaluate` starts where MultiParams ends, the three pointers 8 bytes on");
// Which variants fetch that way (-DUAVX_KFETCH=0: none, A/B).  The plain one-wavefront-tile variants do.  The variants with
// scripted bodies / levels do not: they sit at 78 scalar registers with six already parked in VGPR lanes, and 32 more held from
// the top would cost them their eighth wavefront.
#ifndef UAVX_KFETCH
#define UAVX_KFETCH 1
#endif
template <int NT, bool EXT, int W, int T>
constexpr bool step_fetches() { return UAVX_KFETCH && !EXT; }
// The 4-UAV one-step kernel stores positions and rewards as quad-packed 16-byte write-through rows (-DUAVX_PACKWT=0: the plain
// 8-byte / 4-byte stores, A/B).  Numbers: profiles/r13_packed_rows_ab.md.
#ifndef UAVX_PACKWT
#define UAVX_PACKWT 1
#endif
// The tail of the same kernel (the two 4-UAV one-step instantiations only); numbers: profiles/r14_tail_ab.md.
//   UAVX_TAILCOLD  flags word changed | arrival | hard collision | non-finite reward as ONE wave-uniform test and one scalar
//                  branch; the four bodies sit in the block behind it (=0: four masked regions in line)
//   UAVX_DONEROW   the env's four done bytes assembled in the quad and stored by its first lane as one write-through dword
//                  (=0: one plain byte store per lane)
// UAVX_CEIL_NOCOUNT / UAVX_CEIL_NODONE: ceiling builds for timing ONLY -- the step counter's increment / the done store
// compiled out, wrong step counts / dones.  Never under a test.  (The counter's ceiling is 0.06 us; a load at the head and a
// write-through store at the tail in place of its atomic measured 0.36 us SLOWER and is not kept.)
#ifndef UAVX_TAILCOLD
#define UAVX_TAILCOLD 1
#endif
#ifndef UAVX_DONEROW
#define UAVX_DONEROW 1
#endif
#ifndef UAVX_CEIL_NOCOUNT
#define UAVX_CEIL_NOCOUNT 0
#endif
#ifndef UAVX_CEIL_NODONE
#define UAVX_CEIL_NODONE 0
#endif
// T > 1: T independent one-wavefront tiles per workgroup (own LDS slice, wavefront-level ordering only) -- fewer workgroups for
// the dispatcher to place.  Pays only where one-wavefront workgroups fill every slot exactly once and live short (65 536 x 8:
// the 2.3 us over which 8 192 workgroups are placed is a large share of a 6 us wavefront); see tiles_for().
template <int NT, bool ACT64, bool EXT, int W, int T = 1>
__global__ __launch_bounds__(kWave * W * T, (EXT && W == 1) ? UAVX_STEPB : 1) void step_kernel(
    const void *__restrict__ actions, char *slab, uint32_t off_vel, uint32_t off_goal, uint32_t off_rec, uint32_t off_wsteps,
    uint32_t num_envs, uint32_t n_agents, uint32_t envs_per_group, uint32_t magic, uint32_t nslots, MultiParams p, int evaluate_arg,
    float *__restrict__ obs_arg, float *__restrict__ rew_arg, uint8_t *__restrict__ done_arg) {
    static_assert(T == 1 || W == 1, "tiles are one-wavefront workgroups side by side");
    using LDS = std::conditional_t<(T > 1), LdsTiles<T>, LdsT<EXT, W>>;
    static_assert(T == 1 || !EXT, "tiles: the plain variants only");
    __shared__ LDS lds;
    const uint32_t tile = T > 1 ? (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave)) : 0u;   // (a scalar)
    // 4 UAVs, one step: state rows through buffer resources (16 scalar registers for the four of them; the other variants have none
    // to spare) and the squared-distance neighbour scan (scan_neighbours)
    constexpr bool BUF = NT == 4 && !EXT && T == 1;
    constexpr bool FETCH = step_fetches<NT, EXT, W, T>();
    constexpr bool TAILCOLD = BUF && UAVX_TAILCOLD;
    float2 *const pos_b = reinterpret_cast<float2 *>(slab);
    double2 *const vel_b = reinterpret_cast<double2 *>(slab + off_vel);
    Goal *const goal_b = reinterpret_cast<Goal *>(slab + off_goal);
    const uint32_t nslot = num_envs * n_agents;   // E*N < 2^26 (uavx_create): every byte offset below fits 32 bits
    const rsrc_t r_act = make_rsrc(actions, nslot * (ACT64 ? 16u : 8u));
    const rsrc_t r_pos = make_rsrc(slab, nslot * 8u), r_vel = make_rsrc(slab + off_vel, nslot * 16u);
    const rsrc_t r_goal = make_rsrc(slab + off_goal, nslot * 16u);
    const uint32_t wave_id = blockIdx.x * T + tile;
    const LaneMap m = lane_map_from<NT, EXT, W>(num_envs, (int)n_agents, (int)envs_per_group, (int)magic, (int)nslots, wave_id,
                                                T > 1 ? threadIdx.x % kWave : threadIdx.x, tile);
    AgentRegs s = {};
    double ax = 0.0, ay = 0.0;
    uint4 rec = make_uint4(0, 0, 0, 0);
    uint32_t wave_count = 0;
    StepArgs ka = {};   // (FETCH only)
    {
        // Unconditional (idle lanes of the last workgroup read slot 0 and drop what they compute): the requests leave in front
        // of every scalar load of the argument struct.  The command goes first: prev_distance is arithmetic on the state, and
        // a load placed behind that would start a second memory round trip after the first one has come back.
        const uint32_t el = m.active ? m.e : 0u, al = m.active ? m.a : 0u;
        if (EXT) {  // the bodies' waypoint schedule runs on the env's step count and episode index
            rec = reinterpret_cast<const uint4 *>(slab + off_rec)[el];
            wave_count = reinterpret_cast<const uint32_t *>(slab + off_wsteps)[wave_id];
        }
        // BUF: buffer loads, one 32-bit lane offset per row size on top of the scalar bases (a global load needs a 64-bit
        // address per lane and array)
        if (!BUF) {
            load_action<ACT64>(actions, al, ax, ay);
            const float2 d = pos_b[al];
            const double2 v = vel_b[al];
            const Goal g = goal_b[al];
            if constexpr (FETCH) ka = fetch_step_args();
            __builtin_amdgcn_sched_barrier(0);
            s.x = d.x; s.y = d.y; s.vx = v.x; s.vy = v.y;
            s.tx = g.tx; s.ty = g.ty; s.init_d = g.init_d; s.flags = g.flags;
        } else {
            if (ACT64) {
                const u32x4 c = __builtin_amdgcn_raw_buffer_load_b128(r_act, al * 16u, 0, 0);
                ax = __hiloint2double(c.y, c.x); ay = __hiloint2double(c.w, c.z);
            } else {
                const u32x2 c = __builtin_amdgcn_raw_buffer_load_b64(r_act, al * 8u, 0, 0);
                ax = (double)__uint_as_float(c.x); ay = (double)__uint_as_float(c.y);
            }
            const u32x2 d = __builtin_amdgcn_raw_buffer_load_b64(r_pos, al * 8u, 0, 0);
            const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r_vel, al * 16u, 0, 0);
            const u32x4 g = __builtin_amdgcn_raw_buffer_load_b128(r_goal, al * 16u, 0, 0);
            if constexpr (FETCH) ka = fetch_step_args();
            __builtin_amdgcn_sched_barrier(0);
            s.x = __uint_as_float(d.x); s.y = __uint_as_float(d.y);
            s.vx = __hiloint2double(v.y, v.x); s.vy = __hiloint2double(v.w, v.z);
            s.tx = __uint_as_float(g.x); s.ty = __uint_as_float(g.y); s.init_d = __uint_as_float(g.z); s.flags = g.w;
        }
        s.prev_d = natural_prev_d(s.flags, s.x, s.y, s.tx, s.ty);
        if (m.active && (s.flags & kFlagPrevOvr)) s.prev_d = p.prev_ovr[m.a];  // rare: only after a caller poked the state
    }
    float *const obs_out = FETCH ? ka.obs_out : obs_arg, *const rew_out = FETCH ? ka.rew_out : rew_arg;
    uint8_t *const done_out = FETCH ? ka.done_out : done_arg;
    const int evaluate = FETCH ? ka.evaluate : evaluate_arg;
    const uint32_t flags_in = s.flags;
    float o[10], rew;
    uint32_t dn, re, ce;
    if constexpr (FETCH)
        step_agent<NT, EXT, LDS, false, BUF>(p, ka.h, m, lds, s, ax, ay, evaluate, o, rew, dn, re, ce, false, wave_count - rec.x,
                                             ((rec.y & ~kRecEnded) - 1u) & ~kRecEnded);
    else
        step_agent<NT, EXT, LDS, false, BUF>(p, p, m, lds, s, ax, ay, evaluate, o, rew, dn, re, ce, false, wave_count - rec.x,
                                             ((rec.y & ~kRecEnded) - 1u) & ~kRecEnded);
    if (m.active) {
        if (!BUF) {
            if (!(EXT && (flags_in & kFlagInactive))) {
                if constexpr (FETCH) store_agent(nslot, pos_b, vel_b, goal_b, m.a, s, flags_in);
                else store_agent(p, pos_b, vel_b, goal_b, m.a, s, flags_in);
            }
            rew_out[m.a] = rew;
            done_out[m.a] = (uint8_t)dn;
        } else {   // store_agent() through the buffer resources of the loads
            store16_wt(r_vel, m.a * 16u, make_double2(s.vx, s.vy));
            const rsrc_t r_rew = make_rsrc(rew_out, nslot * 4u);
#if UAVX_PACKWT
            // Positions and rewards leave as 16-byte write-through rows too, assembled in registers: with N = 4 the lanes that
            // hold 16 contiguous bytes are neighbours in a quad (positions: lanes 2k, 2k+1; rewards: lanes 4g .. 4g+3).
            // A quad is ONE WHOLE ENV (whole envs are packed from thread 0 and slot = a0 + lane, lane_map_from), so inside
            // `m.active` it is entirely live -- every DPP source lane is enabled -- and a row lies wholly inside nslot.
            // Positions: agents 0 and 1 of the env store the rows of slots {0, 1} and {2, 3} (one compare on m.i; all four
            // dwords arrive by DPP, so the row needs no copy of the lane's own x, y into a register quad)
            const uint32_t ux = __float_as_uint(s.x), uy = __float_as_uint(s.y);
            const float4 prow = make_float4(__uint_as_float(quad_perm<0, 2, 0, 2>(ux)), __uint_as_float(quad_perm<0, 2, 0, 2>(uy)),
                                            __uint_as_float(quad_perm<1, 3, 1, 3>(ux)), __uint_as_float(quad_perm<1, 3, 1, 3>(uy)));
            const float4 rrow = make_float4(rew, quad_perm_lane(rew, 1), quad_perm_lane(rew, 2), quad_perm_lane(rew, 3));
            if (m.i < 2) store16_wt(r_pos, (m.a + (uint32_t)m.i) * 8u, prow);
            // the reward array may be the caller's (out=, a replay-ring slot): rows only if it starts on a 16-byte boundary, else
            // one dword per lane as before.  `mis` is uniform (a scalar test of the pointer: 0, or at least 4) and rides in the
            // leaders' compare -- m.i == mis holds for agent 0 of an aligned array only -- so that the common path stays
            // straight-line code under one EXEC mask, no scalar branch out and back
#if UAVX_DONEROW && !UAVX_CEIL_NODONE
            // The env's four done bytes (0 / 1 each) leave with the reward row, as one write-through dword from the same lane:
            // two DPP steps ({d0 | d1 << 8, d2 | d3 << 8} in lanes 4g and 4g + 2, then the pair of pairs in lane 4g).  The
            // leader's slot m.a is a multiple of 4 and its env lies wholly inside nslot.  A caller's done array that does not
            // start on a 4-byte boundary gets its byte stores: its low address bits ride in `mis` too (one compare, one masked
            // region and one fallback branch for both arrays; either array misaligned sends both down the narrow stores)
            const rsrc_t r_done = make_rsrc(done_out, nslot);
            const uint32_t dpair = dn | (quad_perm<1, 1, 3, 3>(dn) << 8);
            const uint32_t drow = dpair | (quad_perm<2, 2, 2, 2>(dpair) << 16);
            const uint32_t mis = (((uint32_t)reinterpret_cast<uintptr_t>(rew_out) & 15u) |
                                  ((uint32_t)reinterpret_cast<uintptr_t>(done_out) & 3u)) << 2;
            if (__builtin_expect((uint32_t)m.i == mis, 1)) {
                store16_wt(r_rew, m.a * 4u, rrow);
                __builtin_amdgcn_raw_buffer_store_b32(drow, r_done, m.a, 0, kAuxSc1);
            }
            if (__builtin_expect(mis != 0u, 0)) {
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(rew), r_rew, m.a * 4u, 0, 0);
                __builtin_amdgcn_raw_buffer_store_b8((uint8_t)dn, r_done, m.a, 0, 0);
            }
#else
            const uint32_t mis = ((uint32_t)reinterpret_cast<uintptr_t>(rew_out) & 15u) << 2;
            if (__builtin_expect((uint32_t)m.i == mis, 1)) store16_wt(r_rew, m.a * 4u, rrow);
            if (__builtin_expect(mis != 0u, 0)) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(rew), r_rew, m.a * 4u, 0, 0);
#endif
#else
            const u32x2 d = {__float_as_uint(s.x), __float_as_uint(s.y)};
            __builtin_amdgcn_raw_buffer_store_b64(d, r_pos, m.a * 8u, 0, 0);
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(rew), r_rew, m.a * 4u, 0, 0);
#endif
            if constexpr (!TAILCOLD)
                if (s.flags != flags_in) __builtin_amdgcn_raw_buffer_store_b32(s.flags, r_goal, m.a * 16u + 12u, 0, 0);
#if !(UAVX_PACKWT && UAVX_DONEROW) && !UAVX_CEIL_NODONE
            __builtin_amdgcn_raw_buffer_store_b8((uint8_t)dn, make_rsrc(done_out, nslot), m.a, 0, 0);
#endif
        }
        // The rare events.  TAILCOLD: ONE wave-uniform test on the common path and one scalar branch; the four bodies sit behind
        // it.  An arrival sets DONE where it was clear and a counted collision sets COLLIDED where it was clear (step_agent), so
        // `flags changed` already covers `re | ce`: the test is (flags changed) | (non-finite reward)
        const bool nonfinite = !(fabsf(rew) < INFINITY);   // the tripwire of test_ddpg_multi.py:114-130, per env
        if (!TAILCOLD || __builtin_expect(__any((s.flags != flags_in) | nonfinite), 0)) {
            if constexpr (TAILCOLD)
                if (s.flags != flags_in) __builtin_amdgcn_raw_buffer_store_b32(s.flags, r_goal, m.a * 16u + 12u, 0, 0);
            // (FETCH: the counters' pointers are fetched inside their rare branches)
            // TAILCOLD: the increment and the env index are made opaque here, so that the three branches share one register
            // each instead of setting up their own (static vector instructions: tests/test_step4_isa_budget.py)
            if constexpr (TAILCOLD) {
                uint32_t one = 1u;
                uint64_t ei = m.e;
                asm volatile("" : "+v"(one), "+v"(ei));
                if (re) atomicAdd(&karg_if<FETCH>(p.reach, kStepLead + (uint32_t)offsetof(MultiParams, reach))[ei], one);   // MUW:221
                if (ce) atomicAdd(&karg_if<FETCH>(p.coll, kStepLead + (uint32_t)offsetof(MultiParams, coll))[ei], one);     // MUW:209
                if (nonfinite) atomicAdd(&karg_if<FETCH>(p.nonfin, kStepLead + (uint32_t)offsetof(MultiParams, nonfin))[ei], one);
            } else {
                if (re) atomicAdd(&karg_if<FETCH>(p.reach, kStepLead + (uint32_t)offsetof(MultiParams, reach))[m.e], 1u);   // MUW:221
                if (ce) atomicAdd(&karg_if<FETCH>(p.coll, kStepLead + (uint32_t)offsetof(MultiParams, coll))[m.e], 1u);     // MUW:209
                if (nonfinite) atomicAdd(&karg_if<FETCH>(p.nonfin, kStepLead + (uint32_t)offsetof(MultiParams, nonfin))[m.e], 1u);
            }
        }
        if (!(BUF && UAVX_CEIL_NOCOUNT) && m.lane == 0) {
            uint32_t *const ws = reinterpret_cast<uint32_t *>(slab + off_wsteps);
            if (EXT) ws[m.wave] = wave_count + 1u;             // single writer: this wave (MUW:238)
            else atomicAdd(&ws[m.wave], 1u);                   // MUW:238 for every env of this wave (no-return)
        }
    }
    // (E, N: the preloaded leading scalars.  Flat store rounds at N = 4 only: at N = 2 and 8 the changed register allocation moved
    //  the prev_ovr branch's scalar load next to its wait in the kernel's head, which tests/test_step_isa_host.py holds)
    if constexpr (FETCH) store_obs_block<NT, LDS, NT == 4>(nslot, (int)n_agents, m, lds, o, obs_out);
    else store_obs_block<NT>(p, m, lds, o, obs_out);
}

// uavx_step_ex.hpp -- the kernel of uavx_step_ex, included by uavx_multi.hip once per action-mode family (no include guard):
//   UAVX_EX_KERNEL step_ex_kernel,     UAVX_EX_REF false : UAVX_ACTION_CARTESIAN / UAVX_ACTION_POLAR (action_mode read at run time)
//   UAVX_EX_KERNEL step_ex_ref_kernel, UAVX_EX_REF true  : UAVX_ACTION_POLAR_REFERENCE
// One text, two kernels: the double cos / sin of the reference conversion lives only in the second, and the first is the
// same function it was before that mode existed (a __device__ body behind two thin kernels compiled differently: the
// kernel-argument copy moved the register allocation of every variant).
template <int NT, bool ACT64, bool EXT, int W, int T = 1>   // T: one-wavefront tiles per workgroup (see step_kernel)
__global__ __launch_bounds__(kWave * W * T, (W != 1) ? 1 : (EXT ? UAVX_EXB : (NT == 8 ? UAVX_EX8B : 1))) void UAVX_EX_KERNEL(const void *__restrict__ actions, char *slab, uint32_t off_vel, uint32_t off_goal,
                                                            uint32_t off_rec, uint32_t off_wsteps, uint32_t num_envs, uint32_t stage_first,
                                                            uint32_t pf_blocks, uint32_t step_first, uint32_t shape_packed, uint32_t magic,
                                                            MultiParams p, StepExtra x, int evaluate,
                                                            float *__restrict__ obs_out, float *__restrict__ rew_out_arg,
                                                            uint8_t *__restrict__ done_out_arg) {
    // The first twelve parameters (kExLead = 56 bytes: all 14 dwords the preload takes) are LEADING SCALARS -- shape_packed =
    // agents | envs per workgroup << 8 | neighbour slots per env << 16 --: gfx950 preloads them into SGPRs before the wavefront
    // starts (see step_kernel), so the staging / step decision and the first loads -- env record, step counter, command,
    // state -- need no scalar load of the argument segment.  The state arrays are one allocation: its base + 32-bit offsets
    // (uavx_create checks they fit) instead of five pointers; the END of the kernel stores through the same registers, so the
    // register-tight variants no longer fetch those pointers a second time.
    static_assert(kExLead == 2 * sizeof(void *) + 10 * sizeof(uint32_t), "leading scalar arguments of step_ex_kernel");
    static_assert(T == 1 || W == 1, "tiles are one-wavefront workgroups side by side");
    using LDS = std::conditional_t<(T > 1), LdsTiles<T>, LdsT<EXT, W>>;
    static_assert(T == 1 || !EXT, "tiles: the plain variants only");
    __shared__ LDS lds;
    const uint32_t tile = T > 1 ? (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave)) : 0u;   // (a scalar)
    const int N = NT ? NT : (int)(shape_packed & 0xFFu);
    float2 *const pos_b = reinterpret_cast<float2 *>(slab);
    double2 *const vel_b = reinterpret_cast<double2 *>(slab + off_vel);
    Goal *const goal_b = reinterpret_cast<Goal *>(slab + off_goal);
    uint4 *const rec_b = reinterpret_cast<uint4 *>(slab + off_rec);
    uint32_t *const wsteps_b = reinterpret_cast<uint32_t *>(slab + off_wsteps);
    // Register-tight variants (one resident round of 8 192 wavefronts needs 8 per SIMD: 64 VGPRs and 80 SGPRs): arguments that
    // only a rare branch or the END of the kernel needs are fetched there (LATE) instead of living in scalar registers across
    // the step -- bounded to 8 wavefronts per SIMD the compiler otherwise parks them in VGPR lanes (v_writelane / v_readlane
    // in the hot path: 65 536 x 8 fused 13.9 -> 15.5 us in round 3).
    constexpr bool kTight = (EXT || NT == 8) && W == 1;
    constexpr int kLate = kTight ? UAVX_LATE_EX : 0;   // LATE() sites of this variant
    constexpr bool kLateR = (kLate & 8) != 0;
    {
        // the staging workgroups of the launch: [stage_first, stage_first + pf_blocks) -- in front of the env-workgroups or
        // behind them (uavx_step_ex picks; one unsigned compare serves both)
        const uint32_t sb = blockIdx.x - stage_first;
        if (sb < pf_blocks) {   // uniform per workgroup
            if (T > 1 && tile != 0u) return;   // a staging workgroup is ONE wavefront of work: the other tiles leave
            // The staging path reads its arguments through the laundered segment pointer: left to itself the compiler hoists
            // THOSE scalar loads in front of this branch, into the prologue of every step wavefront, and with 80 SGPRs parks
            // them in VGPR lanes there (20 v_writelane at the top of step_ex_kernel<8>).
#ifndef UAVX_STAGE_LAUNDER
#define UAVX_STAGE_LAUNDER 3     // 0: off, 1: the 8-UAV specialisation, 2: also the variants with bodies / levels, 3: every variant
#endif
            // (A/B, profiles/r04_ab_notes.md: 65 536 x 8 fused 13.95 -> 13.55 us.  Every variant since the leading arguments
            //  are preloaded: the branch above is decided from registers, and hoisted staging loads + their wait in front of
            //  it would hold up the first state loads of every step wavefront again)
            if constexpr (UAVX_LATE && ((UAVX_STAGE_LAUNDER >= 1 && W == 1 && NT == 8 && !EXT) || (UAVX_STAGE_LAUNDER >= 2 && W == 1 && EXT) || UAVX_STAGE_LAUNDER >= 3)) {
                typedef const __attribute__((address_space(4))) MultiParams KP;
                typedef const __attribute__((address_space(4))) StepExtra KX;
                const karg_ptr ka = late_kargs();
                stage_ahead<NT, EXT, W>(*(KP *)(ka + kExLead), *(KX *)(ka + kExLead + sizeof(MultiParams)), lds, sb);
            } else {
                stage_ahead<NT, EXT, W>(p, x, lds, sb);
            }
            return;
        }
    }
    // (everything the mapping needs arrived in registers with the wavefront)
    const LaneMap m = lane_map_from<NT, EXT, W>(num_envs, N, (int)((shape_packed >> 8) & 0xFFu), (int)magic,
                                                (int)(shape_packed >> 16),
                                                (blockIdx.x - step_first) * T + tile,
                                                T > 1 ? threadIdx.x % kWave : threadIdx.x, tile);
#ifdef UAVX_STAMPS
    unsigned long long stamps[7] = {};
    STAMP(0);
    g_dbg_fallback = 0;
#endif
    AgentRegs s = {};
    double ax = 0.0, ay = 0.0;
    // The env record is requested FIRST and the 48 B of agent state after it: vmcnt retires in issue order, so the
    // (rare) re-initialisation below can start as soon as the small load is back and runs underneath the
    // state loads of the launch-wide read burst.  The wave's step counter comes through the scalar cache.
    // Unconditional (idle lanes of the last workgroup read slot 0 and drop what they compute): the requests leave in front of
    // every scalar load of the argument structs (scheduling barrier below).
    uint4 rec0 = make_uint4(0, 0, 0, 0);
    uint32_t wave_count;
    if constexpr (kTight) {
        // (at the 64-VGPR edge the unconditional form below costs a spill: these variants keep the loads under `active`)
        if (m.active) rec0 = rec_b[m.e];
        wave_count = wsteps_b[m.wave];
        __builtin_amdgcn_sched_barrier(0);
        if (m.active) {
            load_action<ACT64>(actions, m.a, ax, ay);
            const float2 d = pos_b[m.a];
            const double2 v = vel_b[m.a];
            const Goal g = goal_b[m.a];
            s.x = d.x; s.y = d.y; s.vx = v.x; s.vy = v.y;
            s.tx = g.tx; s.ty = g.ty; s.init_d = g.init_d; s.flags = g.flags;
            s.prev_d = natural_prev_d(s.flags, s.x, s.y, s.tx, s.ty);
            if (s.flags & kFlagPrevOvr) s.prev_d = p.prev_ovr[m.a];
        }
    } else {
        const uint32_t el = m.active ? m.e : 0u, al = m.active ? m.a : 0u;
        rec0 = rec_b[el];
        wave_count = wsteps_b[m.wave];
        // the command is requested BEFORE the state: prev_distance is arithmetic on what was loaded, and a load placed behind
        // that would start a second memory round trip after the first one has come back
        load_action<ACT64>(actions, al, ax, ay);
        const float2 d = pos_b[al];
        const double2 v = vel_b[al];
        const Goal g = goal_b[al];
        __builtin_amdgcn_sched_barrier(0);
        s.x = d.x; s.y = d.y; s.vx = v.x; s.vy = v.y;
        s.tx = g.tx; s.ty = g.ty; s.init_d = g.init_d; s.flags = g.flags;
        s.prev_d = natural_prev_d(s.flags, s.x, s.y, s.tx, s.ty);
        if (m.active && (s.flags & kFlagPrevOvr)) s.prev_d = p.prev_ovr[m.a];  // rare: only after a caller poked the state
    }
    __builtin_amdgcn_sched_barrier(0);
    if (!m.active) rec0.y = 0u;   // an idle lane holds env 0's record: it must not take part in a re-initialisation
    const bool do_reset = (rec0.y & kRecEnded) != 0;
    const uint32_t episode = rec0.y & ~kRecEnded;
    uint32_t steps_v = wave_count - rec0.x;
    // Register budget (the variants with 8 agents / bodies sit at the 64-VGPR edge of 8 wavefronts per SIMD): a
    // re-initialised env's record is written straight over the loaded one (`s`), and what the statistics fold needs is
    // read back from `rec` and memory at the END of the launch, by the (rare) lanes that need it.
    const bool wave_resets = group_any<W>(do_reset);   // uniform over the workgroup
    if (wave_resets) {  // wave-uniform: at least one env of this wave starts a new episode
        // A wave that re-initialises an env has a few hundred more instructions to issue than its three SIMD
        // mates and would finish last (launch time = slowest wave): let it issue ahead of them for the rest
        // of its life; the mates lose only issue slots they had to spare.
        __builtin_amdgcn_s_setprio(3);
        // The layout was normally drawn ahead of time by a staging workgroup (16-byte copies); only a miss -- first use, a
        // changed seed / world, an episode that ended within two or three launches of its start -- draws here.
        // Everything the parked layout consists of is requested together with its tag, before the tag is looked at: the
        // wavefront is one memory round trip behind its mates instead of five (record -> tag -> agents -> bodies, trip by
        // trip), and a launch is as long as its slowest wavefront.
        // (what only this branch needs from the kernel arguments -- seed, staging arrays -- is fetched here, LATE())
        LATE_BASE(kLateR, ka);
        const uint32_t seed_lo = LATE_X_AT(kLateR, ka, x, seed_lo), seed_hi = LATE_X_AT(kLateR, ka, x, seed_hi);
        const uint4 *const stage_tag = LATE_AT(kLateR, ka, p, stage_tag);
        const float4 *const stage_agent = LATE_AT(kLateR, ka, p, stage_agent);
        const float2 *const stage_bpos = EXT ? LATE_AT(kLateR, ka, p, stage_bpos) : nullptr;
        const float4 *const stage_bleg = EXT ? LATE_AT(kLateR, ka, p, stage_bleg) : nullptr;
        bool hit = false;
        uint4 tag = make_uint4(0, 0, 0, 0);
        float4 st = make_float4(0.f, 0.f, 0.f, 0.f);
        float2 bq0 = make_float2(0.f, 0.f), bq1 = bq0;
        float4 bl0 = make_float4(0.f, 0.f, 0.f, 0.f), bl1 = bl0;
        // the parked layout of episode `episode` lives in slot episode & 1 of the (slot-major) staging arrays
        const uint32_t sl = episode & 1u;
        const uint32_t sbase = sl * (uint32_t)p.E * (uint32_t)p.B + m.e * (uint32_t)p.B;   // first staged body of this env
        if (do_reset && LATE_X_AT(kLateR, ka, x, use_stage)) {
            tag = stage_tag[sl * (uint32_t)p.E + m.e];
            st = stage_agent[sl * (uint32_t)p.E * (uint32_t)N + m.a];
            if (EXT) {   // the first two body trips (all of them up to B = 2 L); further ones below
                if (m.i < p.B) { bq0 = stage_bpos[sbase + (uint32_t)m.i]; bl0 = stage_bleg[sbase + (uint32_t)m.i]; }
                if (N + m.i < p.B) { bq1 = stage_bpos[sbase + (uint32_t)(N + m.i)]; bl1 = stage_bleg[sbase + (uint32_t)(N + m.i)]; }
            }
            hit = stage_hit(tag, stage_want<EXT>(p, m.e, episode, seed_lo, seed_hi));
        }
        const uint32_t hit_lvl = tag.w & 0xFFu;
        if (EXT && hit) {   // the bodies of a parked layout: staged -> live, and into the env's LDS rows (frees their registers first)
            if (m.i == 0) LATE_AT(kLateR, ka, p, lvl_cur)[m.e] = (uint8_t)hit_lvl;
            auto place = [&](int k, float2 q, float4 leg) {
                const int b = k * N + m.i;
                if (b < p.B) {
                    const uint32_t gi = m.e * (uint32_t)p.B + (uint32_t)b;
                    p.body_pos[gi] = q;
                    p.body_leg[gi] = leg;
                    lds.pos[m.rbase + N + b] = make_float4(q.x, q.y, q.x, q.y);
                    lds.theta[m.rbase + N + b] = leg.z;
                }
            };
            place(0, bq0, bl0);
            place(1, bq1, bl1);
#pragma unroll 1
            for (int k = 2; k < p.kb; k++) {
                const int b = k * N + m.i;
                const uint32_t gi = sbase + (uint32_t)min(b, p.B - 1);
                place(k, stage_bpos[gi], stage_bleg[gi]);
            }
        }
#ifndef UAVX_X_NOMISS
        if (group_any<W>(do_reset && !hit)) {
            // The accept / reject chain needs some forty registers of its own.  Inlined into the step with the loaded state
            // and command alive across it, it set the register count of the WHOLE kernel (74 with scripted bodies: 6
            // wavefronts per SIMD instead of 8).  So nothing loaded at the top of the launch is carried across it: a wavefront
            // that draws a layout in place reads the command and the state of its other envs AGAIN afterwards -- one more
            // memory round trip on that (rare) wavefront instead of 10 registers on every wavefront of every launch.
            const bool draw = do_reset && !hit;
            AgentRegs t = {};
            reset_envs_wave<NT, EXT>(p, m, lds, draw, episode, seed_lo, seed_hi, t, p.body_pos, p.body_leg, LATE_AT(kLateR, ka, p, lvl_cur));
            asm volatile("" ::: "memory");   // (the loads below must not be folded into the ones at the top)
            AgentRegs r = {};
            ax = 0.0; ay = 0.0;
            if (m.active) {   // (rare path: the state arrays through the argument struct, not the preloaded registers)
                load_action<ACT64>(actions, m.a, ax, ay);
                if (!do_reset) load_agent(p, m.a, r);
            }
            s = draw ? t : r;
        }
#endif
        if (hit) {
            s.x = st.x; s.y = st.y; s.tx = st.z; s.ty = st.w;
            s.vx = 0.0; s.vy = 0.0; s.flags = 0;                 // MUW:120-123
            // whether the learner is parked is read off the layout itself (a parked learner is staged at +inf), not off the
            // level table: a table rewritten since the layout was drawn (uavx_set_curriculum under a graph captured before
            // it, whose launches still carry the old world version and so still accept the old layouts) then cannot produce a
            // learner that takes part without a position
            bool parked = false;
            if (EXT) {
                parked = st.x == INFINITY;
                s.flags = (hit_lvl << kLevelShift) | (parked ? kFlagInactive : 0u);
            }
            s.init_d = s.prev_d = parked ? INFINITY : norm32(s.tx - s.x, s.ty - s.y);  // MUW:154-155
        }
        if (do_reset) {
            Goal *goal_w = goal_b;
            if constexpr (kLateR && UAVX_LATE) goal_w = LATE_AT(true, ka, p, goal);
            goal_w[m.a] = Goal{s.tx, s.ty, s.init_d, s.flags};
            steps_v = 0;                                           // MUW:166
        }
    }
    STAMP(1);
    const uint32_t flags_in = s.flags;
    if constexpr (UAVX_EX_REF) polar_to_command_ref<ACT64>(p.vmax_norm, ax, ay);
    else if (x.action_mode == UAVX_ACTION_POLAR) polar_to_command(p, (float)ax, (float)ay, ax, ay);
    float o[10], rew;
    uint32_t dn, re, ce;
    // a freshly re-initialised env draws its bodies' waypoints with the episode index `episode`, a running one with the
    // index its own reset used (one less than the stored one)
    step_agent<NT, EXT, LDS, (kLate & 2) != 0>(p, p, m, lds, s, ax, ay, evaluate, o, rew, dn, re, ce, do_reset, steps_v,
                                               (episode - (do_reset ? 0u : 1u)) & ~kRecEnded);
    // episode end test for the NEXT call (test_sac_multi.py:67,112,116)
    bool all_done;
    if (W == 1) {
        const unsigned long long done_bits = __ballot(dn != 0);
        const unsigned long long group = (N >= 64) ? ~0ull : ((1ull << N) - 1ull);
        all_done = ((done_bits >> m.base) & group) == group;
    } else {  // the env may span two wavefronts: count its done agents in LDS (obs tile scratch, free until the final store)
        int *cnt = reinterpret_cast<int *>(lds.obs) + m.g;
        if (m.i == 0) *cnt = 0;
        __syncthreads();
        if (m.active && dn != 0) atomicAdd(cnt, 1);
        __syncthreads();
        all_done = *cnt == N;
        __syncthreads();
    }
    if (x.track_returns) {
        if (m.active) lds.theta[m.rbase + m.i] = do_reset ? 0.f : rew * (1.0f - (float)dn);  // test_sac_multi.py:157
        group_sync<LDS::kW>();
    }
    // The observation tile leaves FIRST: its ten registers per lane are free for the bookkeeping below, and the 40 B per
    // agent of write-through stores drain underneath it.  (The tile never overlaps the theta rows the score sum below reads:
    // separate arrays, or -- with scripted bodies -- the first 2 560 B of a union whose theta rows start at byte 3 072.)
    store_obs_block<NT>(p, m, lds, o, obs_out);
    float2 *pos_p = pos_b;
    double2 *vel_p = vel_b;
    Goal *goal_p = goal_b;
    uint4 *rec_p = rec_b;
    uint32_t *wsteps_p = wsteps_b;
    float *rew_out = rew_out_arg;
    uint8_t *done_out = done_out_arg;
    if constexpr (kLateR && UAVX_LATE) {
        // (register-tight variants: neither the preloaded base + offsets nor the output pointers stay alive across the step --
        //  the pointers the tail stores through are fetched from the argument struct here; A/B at 65 536 x 8 fused: holding
        //  the six preloaded registers instead cost 12.7 -> 13.2 us)
        LATE_BASE(true, kt);
        pos_p = LATE_AT(true, kt, p, pos); vel_p = LATE_AT(true, kt, p, vel); goal_p = LATE_AT(true, kt, p, goal);
        rec_p = LATE_AT(true, kt, p, env_rec); wsteps_p = LATE_AT(true, kt, p, wave_steps);
        rew_out = late_karg<float *>(kIoRew, kt); done_out = late_karg<uint8_t *>(kIoDone, kt);
    }
    if (m.active) {
        if (!(EXT && (s.flags & kFlagInactive))) store_agent(p, pos_p, vel_p, goal_p, m.a, s, flags_in);
        else if (do_reset) { pos_p[m.a] = make_float2(s.x, s.y); vel_p[m.a] = make_double2(0.0, 0.0); }  // parked at +inf
        rew_out[m.a] = rew;
        // episode end test for the NEXT call (test_sac_multi.py:67,112,116); meaningful in the env's first lane
        const uint32_t steps_next = do_reset ? 0u : steps_v + 1u;
        const bool terminal = (x.reset_policy == UAVX_RESET_AGENT0_DONE && dn != 0) ||
                              (x.reset_policy == UAVX_RESET_ALL_DONE && all_done);          // test_sac_multi.py:112,116
        const bool capped = x.step_cap != 0 && steps_next >= x.step_cap;                   // :17,67
        const bool ended = (terminal || capped) && !do_reset;
        // UAVX_FLAGS_IN_DONE: reset_mask / ended / truncated ride in bits 1..3 of the done byte of the env's agent 0 -- a
        // byte of a line this launch writes in full anyway -- instead of three more one-byte-per-env arrays, each a partial
        // line write per env (A/B at 65 536 x 4: the three byte stores are 0.28 us of a 7 us launch)
        uint32_t dbyte = dn;
        if (x.flags_in_done && m.i == 0) dbyte |= (do_reset ? 2u : 0u) | (ended ? 4u : 0u) | ((ended && !terminal) ? 8u : 0u);
        done_out[m.a] = (uint8_t)dbyte;
        if (re) atomicAdd(&LATE(kLate & 1, p, reach)[m.e], 1u);                // MUW:221
        if (ce) atomicAdd(&LATE(kLate & 1, p, coll)[m.e], 1u);                 // MUW:209
        if (!(fabsf(rew) < INFINITY)) atomicAdd(&LATE(kLate & 1, p, nonfin)[m.e], 1u);
        if (m.lane == 0) wsteps_p[m.wave] = wave_count + 1u;  // single writer: this wave (MUW:238)
        if (m.i == 0) {
            // With scripted bodies the env record is read AGAIN here by the one lane that rewrites it, instead of being
            // carried through the step in four registers of every lane (nothing has written it since the load at the top of
            // the launch): that kernel fits 64 VGPRs that way, i.e. 8 wavefronts per SIMD and ONE resident round for the
            // 8 192 wavefronts of a 65 536-env launch.  The other variants have registers to spare and keep it.
            const uint4 rec = (EXT || NT == 8) ? rec_p[m.e] : rec0;
            float2 run = do_reset ? make_float2(0.f, 0.f) : make_float2(__uint_as_float(rec.z), __uint_as_float(rec.w));
            if (!x.flags_in_done) {   // (three pointers nobody needs before this line: fetched here)
                uint8_t *const rm = LATE_X(kLateR, x, reset_mask), *const en = LATE_X(kLateR, x, ended), *const tr = LATE_X(kLateR, x, truncated);
                if (rm) rm[m.e] = do_reset ? 1 : 0;
                if (en) en[m.e] = ended ? 1 : 0;
                if (tr) tr[m.e] = (ended && !terminal) ? 1 : 0;
            }
            uint4 out = rec;
            if (do_reset) {  // fold the ended episode, start the new one: steps == 0 after this launch (MUW:166)
                fold_store<(kLate & 4) != 0>(p, m.e, wave_count - rec.x, make_float2(__uint_as_float(rec.z), __uint_as_float(rec.w)),
                                             fold_load<(kLate & 4) != 0>(p, m.e));
                out.x = wave_count + 1u;
                out.y = episode + 1u;
            }
            out.y = (out.y & ~kRecEnded) | (ended ? kRecEnded : 0u);
            if (x.track_returns) {
                float score = 0.f;
                for (int j = 0; j < N; j++) score += lds.theta[m.rbase + j];
                run.x += do_reset ? 0.f : rew;               // test_sac_multi.py:106 score += rewards[0]
                run.y += score;
            }
            out.z = __float_as_uint(run.x); out.w = __float_as_uint(run.y);
            if (out.x != rec.x || out.y != rec.y || out.z != rec.z || out.w != rec.w) rec_p[m.e] = out;
        }
    }
#ifdef UAVX_STAMPS
    STAMP(2);
    stamp_log(stamps, (wave_resets ? 1u : 0u) | (g_dbg_fallback ? 4u : 0u));
#endif
}

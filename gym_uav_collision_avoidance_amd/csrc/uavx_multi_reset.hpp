// uavx_multi_reset.hpp -- episode start: the accept / reject chain of reset (reset_envs_wave), the episode fold, the polar
// conversion, the diagnostic stamps and the layouts drawn ahead (stage_ahead).  Included by uavx_multi.hip inside namespace uavx,
// after uavx_multi_step.hpp.

// One round of the accept/reject chain: does any agent of the workgroup clash, and which is the lowest-indexed clashing
// agent of MY env?  One wavefront per workgroup: a ballot.  Several: an LDS min per env (scratch in the obs tile, which is
// only used at the very end of a launch) and a workgroup-wide OR.  Returns false when nobody clashes (uniform).
template <class LDS, class MAP>
__device__ __forceinline__ bool lowest_clash(const MAP &m, LDS &lds, unsigned long long group, bool clash, int &low) {
    if (LDS::kW == 1) {
        const unsigned long long bits = __ballot(clash);
        const unsigned long long mine = (bits >> m.base) & group;     // clashing agents of my env
        low = mine ? (int)__builtin_ctzll(mine) : 64;
        return bits != 0ull;
    } else {
        int *slot = reinterpret_cast<int *>(lds.obs) + m.g;
        if (m.i == 0) *slot = 64;
        __syncthreads();
        if (clash) atomicMin(slot, m.i);
        const bool any = __syncthreads_or(clash ? 1 : 0) != 0;
        low = *slot;
        return any;
    }
}

// ||a - b|| <= float32(2R) on the squared distance (exact: sqrtf is monotone, limit from sq_limit_le)
__device__ __forceinline__ bool too_close(float sq_two_r, float ax, float ay, float bx, float by) {
    const float dx = ax - bx, dy = ay - by;
    const float xx = dx * dx, yy = dy * dy;
    return xx + yy <= sq_two_r;
}

// MUW:116-155 for the envs of this wave flagged `go` (all lanes of an env agree), wave-cooperative.
// Every lane draws its agent's first start/target candidates with ONE Philox call.  The reference's
// sequential accept/reject chain (agent i keeps the first candidate that is clear of the ACCEPTED points of
// agents j < i, MUW:127-153) is replayed without a per-agent turn loop: all lanes test their current
// candidate against the lower-indexed ones at once; if any clash, only the LOWEST-indexed clashing agent of
// each env redraws (everyone below it is already final, everyone above it still holds its first candidate),
// and the test repeats.  With no clash — the common case, probability ~N^2*pi*R^2/area — that is one pass for
// the start points and one for the targets; each clash costs one more pass.  (A per-agent turn loop here
// made 6 % of the resets take thousands of cycles, and with ~100 resets per launch that long tail was in
// EVERY launch: +3 us at 65 536 x 4.)  Same distribution as the reference; the stream layout is
// reset_candidates(), restated by the CPU test oracle.
// EXT (include/uavx.h, curriculum + bodies): the env first takes its level; learners >= the level's n_active are parked;
// the level's bodies then draw their start points in slot order by the same chain, trip by trip (body b belongs to
// lane b % L, trip b / L), against the learners' accepted starts and the lower-indexed bodies, and take waypoint 0.
// Body records (position + leg 0) are stored by this function, and the bodies' neighbour rows of a re-initialised env are
// left in LDS in their staged form ({x, y, x, y} + heading; +inf for a body that does not take part): stage_bodies skips them.
// bpos_out / bleg_out / lvl_out: where the body records and the env's level go -- the live arrays (p.body_pos, p.body_leg,
// p.lvl_cur), or the staging area of a pre-drawn layout (p.stage_bpos, p.stage_bleg, nullptr: the level then only travels
// in s.flags).
#ifndef UAVX_CHAINROWS
#define UAVX_CHAINROWS 4
#endif
constexpr int kChainRows = UAVX_CHAINROWS;   // rows of accepted points a clash test reads per trip (8-byte halves of the rows: the points only)
template <int NT, bool EXT, class LDS>
__device__ __forceinline__ void reset_envs_wave(const MultiParams &p, const LaneMap &m, LDS &lds, bool go,
                                                uint32_t episode, uint32_t k0, uint32_t k1, AgentRegs &s,
                                                float2 *bpos_out, float4 *bleg_out, uint8_t *lvl_out) {
    const int N = NT ? NT : p.N;
    float4 *row = &lds.pos[m.rbase];
    const uint64_t ge = (uint64_t)p.env_offset + m.e;
    const unsigned long long group = (N >= 64) ? ~0ull : ((1ull << N) - 1ull);
    double lox = p.lox, loy = p.loy, hix = p.hix, hiy = p.hiy;
    float sq2r = p.sq_two_r;
    uint32_t lvl = 0;
    int nl = N, nb = 0;
    if (EXT) {
        if (go && p.n_levels > 0) {
            if (p.level_lo >= 0) {  // randomized-reset curriculum: uniform in [lo, hi] from the env's pseudo-slot 0xFFFF
                uint32_t o[4];
                reset_words(ge, 0xFFFFu, 0u, episode, k0, k1, o);
                lvl = (uint32_t)p.level_lo + __umulhi(o[0], (uint32_t)(p.level_hi - p.level_lo + 1));
            } else {
                lvl = p.lvl_next[m.e];
            }
            lvl = min(lvl, (uint32_t)(p.n_levels - 1));
        }
        nb = p.B;
        if (p.n_levels > 0) {
            const LevelParams *lv = &p.levels[lvl];
            lox = lv->lox; loy = lv->loy; hix = lv->hix; hiy = lv->hiy;
            sq2r = lv->sq_two_r;
            nl = lv->n_active; nb = lv->b_active;
        }
    }
    const bool gl = go && m.i < nl;  // this lane's learner takes part
    ResetCandidates c = {0.f, 0.f, 0.f, 0.f};
    if (gl) {
        c = reset_candidates(ge, m.i, 0u, episode, k0, k1, lox, loy, hix, hiy);
        row[m.i] = make_float4(c.sx, c.sy, c.tx, c.ty);
    }
    group_sync<LDS::kW>();
#pragma unroll 1
    for (int phase = 0; phase < 2; phase++) {  // 0: start points MUW:126-137, 1: targets MUW:140-153
        uint32_t attempt = 0;
#pragma unroll 1
        for (;;) {
            bool clash = false;
            if (gl) {
                const float qx = phase ? c.tx : c.sx, qy = phase ? c.ty : c.sy;
                clash = phase ? too_close(sq2r, qx, qy, c.sx, c.sy) : false;                       // MUW:146
#pragma unroll 1
                for (int j0 = 0; j0 < m.i; j0 += kChainRows) {  // several rows per trip (LDS round trips bound this loop)
                    float2 o[kChainRows];
#pragma unroll
                    for (int u = 0; u < kChainRows; u++) {
                        const float4 *r4 = &row[min(j0 + u, m.i - 1)];
                        o[u] = *reinterpret_cast<const float2 *>(phase ? &r4->z : &r4->x);
                    }
#pragma unroll
                    for (int u = 0; u < kChainRows; u++) clash = clash || too_close(sq2r, o[u].x, o[u].y, qx, qy);  // MUW:135,151
                }
            }
            int low;   // lowest-indexed clashing agent of my env (>= N: none)
            if (!lowest_clash<LDS>(m, lds, group, clash, low)) break;
            const bool redraw = gl && m.i == low;
            group_sync<LDS::kW>();
            if (redraw) {  // the lowest-indexed clashing agent takes its next candidate
                const ResetCandidates r = reset_candidates(ge, m.i, ++attempt, episode, k0, k1, lox, loy, hix, hiy);
                if (phase) { c.tx = r.tx; c.ty = r.ty; row[m.i].z = c.tx; row[m.i].w = c.ty; }
                else { c.sx = r.sx; c.sy = r.sy; row[m.i].x = c.sx; row[m.i].y = c.sy; }
            }
            group_sync<LDS::kW>();
        }
    }
    if (EXT) {
#pragma unroll 1
        for (int k = 0; k < p.kb; k++) {
            const int b = k * N + m.i;
            const bool on = go && b < nb;
            const int slot = N + b;
            uint32_t attempt = 0;
            float qx = 0.f, qy = 0.f;
            if (on) {
                const ResetCandidates r = reset_candidates(ge, (uint32_t)slot, 0u, episode, k0, k1, lox, loy, hix, hiy);
                qx = r.sx; qy = r.sy;
                row[slot].x = qx; row[slot].y = qy;
            }
            group_sync<LDS::kW>();
#pragma unroll 1
            for (;;) {
                bool clash = false;
                if (on) {
                    // against the learners' accepted start points (rows 0..nl-1) and the lower-indexed bodies (rows
                    // N..N+b-1), four rows per trip: the loop is bound by LDS round trips, not by arithmetic, and the
                    // slowest resetting wave of a launch is what the whole launch waits for
                    const int cnt = nl + b;
#pragma unroll 1
                    for (int j0 = 0; j0 < cnt; j0 += kChainRows) {
                        float2 o[kChainRows];
#pragma unroll
                        for (int u = 0; u < kChainRows; u++) {
                            const int j = min(j0 + u, cnt - 1);
                            o[u] = *reinterpret_cast<const float2 *>(&row[j < nl ? j : N + (j - nl)].x);
                        }
#pragma unroll
                        for (int u = 0; u < kChainRows; u++) clash = clash || too_close(sq2r, o[u].x, o[u].y, qx, qy);
                    }
                }
                int low;
                if (!lowest_clash<LDS>(m, lds, group, clash, low)) break;
                const bool redraw = on && m.i == low;
                group_sync<LDS::kW>();
                if (redraw) {
                    const ResetCandidates r = reset_candidates(ge, (uint32_t)slot, ++attempt, episode, k0, k1, lox, loy, hix, hiy);
                    qx = r.sx; qy = r.sy;
                    row[slot].x = qx; row[slot].y = qy;
                }
                group_sync<LDS::kW>();
            }
            if (go && b < p.B) {
                float2 q = make_float2(INFINITY, INFINITY);    // a body that does not take part
                float4 leg = make_float4(0.f, 0.f, 0.f, 0.f);
                if (on) {
                    const ResetCandidates w0 = reset_candidates(ge, (uint32_t)slot, 0x80000000u, episode & ~kRecEnded, p.body_k0,
                                                                p.body_k1, lox, loy, hix, hiy);
                    q = make_float2(qx, qy);
                    leg = make_leg(p.body_step, qx, qy, w0.sx, w0.sy);   // leg 0: towards waypoint 0
                }
                row[slot] = make_float4(q.x, q.y, q.x, q.y);
                lds.theta[m.rbase + slot] = leg.z;
                bpos_out[m.e * (uint32_t)p.B + (uint32_t)b] = q;
                bleg_out[m.e * (uint32_t)p.B + (uint32_t)b] = leg;
            }
        }
    }
    group_sync<LDS::kW>();
    if (go) {
        s.x = c.sx; s.y = c.sy; s.tx = c.tx; s.ty = c.ty;
        s.init_d = s.prev_d = norm32(c.tx - c.sx, c.ty - c.sy);  // MUW:154-155
        s.vx = 0.0; s.vy = 0.0; s.flags = 0;                      // MUW:120-123
        if (EXT) {
            s.flags = lvl << kLevelShift;
            if (!gl) {  // parked learner: never a neighbour (+inf), reports obs 0 / reward 0 / done 1
                s.x = s.y = INFINITY; s.tx = s.ty = 0.f;
                s.init_d = s.prev_d = INFINITY;
                s.flags |= kFlagInactive;
            }
            if (m.i == 0 && lvl_out) lvl_out[m.e] = (uint8_t)lvl;
        }
    }
}

// What a parked layout must have been drawn for to serve env e's next reset: {episode index, seed, level rule | world
// version | valid}.  With an installed curriculum and the random window off the level is the one assigned to the env.
template <bool EXT, class P>   // P: MultiParams, or the same struct seen through the laundered kernel-argument pointer
__device__ __forceinline__ uint4 stage_want(const P &p, uint32_t e, uint32_t episode, uint32_t k0, uint32_t k1) {
    uint32_t lvl = 0xFFu;   // "drawn by the layout itself" (random window) or no curriculum
    if (EXT && p.n_levels > 0 && p.level_lo < 0) lvl = min((uint32_t)p.lvl_next[e], (uint32_t)(p.n_levels - 1));
    return make_uint4(episode, k0, k1, kStageValid | ((p.world_version & 0x7FFFFFu) << 8) | lvl);
}
__device__ __forceinline__ bool stage_hit(uint4 have, uint4 want) {   // the level byte of `have` is the level it drew
    const bool lvl_ok = (want.w & 0xFFu) == 0xFFu || (want.w & 0xFFu) == (have.w & 0xFFu);
    return have.x == want.x && have.y == want.y && have.z == want.z && (have.w >> 8) == (want.w >> 8) && lvl_ok;
}

// An episode of env e ends (reset): fold its counters into the per-env statistics the evaluation
// loop reads (test_sac_multi.py:157,164-165) and clear the running values.  One lane per env.
struct EpisodeFold {
    uint4 c; float2 f; uint32_t reach, coll;
};
template <bool LATEF = false>
__device__ __forceinline__ EpisodeFold fold_load(const MultiParams &p, uint32_t e) {  // all loads up front: one latency
    EpisodeFold v;
    LATE_BASE(LATEF, ka);
    v.c = LATE_AT(LATEF, ka, p, fin_counts)[e]; v.f = LATE_AT(LATEF, ka, p, fin_returns)[e];
    v.reach = LATE_AT(LATEF, ka, p, reach)[e]; v.coll = LATE_AT(LATEF, ka, p, coll)[e];
    return v;
}
// An episode of env e ends (reset): fold its counters into the per-env statistics the evaluation loop reads
// (test_sac_multi.py:157,164-165) and clear them (MUW:167-168).  One lane per env; the caller rewrites env_rec.
template <bool LATEF = false>
__device__ __forceinline__ void fold_store(const MultiParams &p, uint32_t e, uint32_t steps, float2 run, EpisodeFold v) {
    LATE_BASE(LATEF, ka);
    if (steps != 0) {
        v.c.x += 1; v.c.y += steps; v.c.z += v.reach; v.c.w += v.coll;
        v.f.x += run.x; v.f.y += run.y;
        LATE_AT(LATEF, ka, p, fin_counts)[e] = v.c;
        LATE_AT(LATEF, ka, p, fin_returns)[e] = v.f;
    }
    LATE_AT(LATEF, ka, p, reach)[e] = 0; LATE_AT(LATEF, ka, p, coll)[e] = 0;  // MUW:167-168
    LATE_AT(LATEF, ka, p, nonfin)[e] = 0;
}

// test_sac_multi.py:77-80 in float32: a in [-1,1]^2 -> velocity command.
__device__ __forceinline__ void polar_to_command(const MultiParams &p, float a0, float a1, double &ax, double &ay) {
    const float v = fmaf(a0, 0.5f, 0.5f) * p.vmax_norm;
    float sn, cs;
    sincospi32(a1, sn, cs);
    ax = (double)(v * cs);
    ay = (double)(v * sn);
}

#ifdef UAVX_STAMPS
// diagnostic build (tools/exp_stamps.py): every wavefront of a uavx_step_ex launch logs {start, mid, end, kind | xcc << 8 | block << 16}
__device__ unsigned long long g_stamps[8 * 16384];
__device__ unsigned int g_stamp_n;
// (s_memtime counts per compute unit: differences inside one wavefront only; slot 6 carries the 100 MHz s_memrealtime of the
//  wavefront's first and last stamp, low words, which IS one clock for the whole device: the launch's dispatch timeline)
#define STAMP(k) do { stamps[k] = __builtin_amdgcn_s_memtime(); if ((k) == 0) stamps[6] = __builtin_amdgcn_s_memrealtime() & 0xFFFFFFFFull; } while (0)
__device__ __forceinline__ void stamp_log(unsigned long long *st, unsigned int kind) {
    if ((threadIdx.x & 63) != 0) return;
    st[6] |= (unsigned long long)__builtin_amdgcn_s_memrealtime() << 32;
    unsigned int xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    const unsigned int k = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64;   // a slot per wavefront: no shared counter to queue on
    if (k < 16384) {
        for (int t = 0; t < 7; t++) g_stamps[8 * k + t] = st[t];
        g_stamps[8 * k + 7] = 0x80000000ull << 32 | kind | ((xcc & 15u) << 8) | ((unsigned long long)blockIdx.x << 16);
    }
    if (k == 0) g_stamp_n = gridDim.x * (blockDim.x / 64);
}
#else
#define STAMP(k)
#endif

// Layouts drawn ahead of time, inside the step launch.  The layout of an env's NEXT episode is a pure function of (seed,
// global env, episode index, level rule); re-initialising an env from a parked layout costs 16-byte copies, drawing it in
// place costs a serial accept / reject chain on ONE wavefront that the whole launch then waits for (with 16 scripted bodies:
// 8 us for a lucky env running alone on its SIMD, 19 us for the unluckiest of the ~100 envs that reset in a launch).  So
// pf_blocks extra workgroups of every auto-resetting uavx_step_ex launch draw instead of stepping -- in front of the
// env-workgroups or behind them (uavx_step_ex decides by the shape of the launch).  A launch is as long as its slowest
// wavefront, so what matters is how long ONE staging workgroup lives and whom it keeps waiting, not how many there are
// (per-wavefront timelines on the device-wide clock: tools/exp_stamps.py, profiles/r03_ab_notes.md):
//   * a staging workgroup alternates between two short jobs.  SCAN (no hints left from its last launch): one window of 64 W
//     envs, a lane each -- record and the tags of the env's two parked layouts, one memory round trip -- and the first few
//     envs that miss a layout are written down as HINTS {env, episode} in the workgroup's own eight slots (no atomics, nobody
//     else writes them); 2.5 us.  DRAW (the next launch finds the hints with one scalar load, a few hundred cycles): the
//     hinted layouts are drawn at once.  Until this round one workgroup scanned AND drew in the same launch: 9 us with the
//     chain waiting behind the scan's round trip at the most congested moment of the launch;
//   * a hint is one launch old, so whether the layout is still wanted and whether its slot may be written NOW is decided from
//     the env's record and the slot's tag as THIS launch finds them (the rule below) -- those two loads are requested before
//     the Philox rounds and waited for in front of the stores, the whole chain runs under them on the hinted (env, episode),
//     and a layout that fails the test is not stored.  Hints can be stale, lost or doubled: results never depend on them;
//   * an env keeps TWO parked layouts, for its next episode (index y, slot y & 1) and the one after: consuming one leaves
//     the other in place, so how soon a layout is parked again (a few launches: window rotation + one for the hint) is not
//     critical and an env draws in place only at first use, after a changed seed / world, or when two of its episodes end
//     within those few launches;
//   * DRAW maps ONE LANE PER SLOT of the neighbour model (S = L + B lanes per layout, learners and bodies alike; up to
//     min(floor(64 W / S), 8) layouts per workgroup): every slot draws its candidates in the same fused Philox loop and the
//     chain is one fixed-point iteration over all start points followed by one over the learners' targets (round 2 mapped a
//     lane per learner and walked the bodies in ceil(B / L) sequential trips, each with its own Philox calls and clash loops).
//     A full invalidation -- creation, a new seed or world -- is worked off at about pf_blocks / 2 workgroups' worth of
//     layouts per launch while the envs that need one meanwhile draw in place as before (same result either way).
// Safe against the step workgroups of the SAME launch: those read the staging arrays only of an env they re-initialise, i.e.
// one whose record carried the "ended" mark when the launch began, and only slot y & 1 of it -- and exactly that slot of
// exactly those envs is left alone here (nothing orders our stores against another workgroup's loads inside a launch); their
// other slot (episode y + 1) may be drawn at any time.  INVARIANT this rests on: a step workgroup clears the mark (its
// env_rec store, the last thing it does) only after every load it made from the staging arrays has returned -- the record's
// new "ended" bit is computed from the step's done flags, which are computed from the loaded layout, so the store cannot be
// issued earlier; a staging workgroup that sees the mark cleared (and the episode index moved on) may therefore overwrite
// the consumed slot at once.  The rule does not care WHEN in the launch the record is read, which is what lets the staging
// workgroups run behind the env-workgroups as well as in front of them.  (tests/test_gpu_ext.py steps with caps of 1 and 2
// and staging in every launch for that overlap, on both positions.)
struct StageMap {   // lane-per-slot mapping of a staging workgroup (the fields lowest_clash() reads are named as in LaneMap)
    int i, base, g, rbase;
    bool active;
    uint32_t e;
};
template <int NT, bool EXT, int W, class LDS, class P, class X>   // P / X: MultiParams / StepExtra, plain or in the kernel-argument address space
__device__ __forceinline__ void stage_ahead(const P &p, const X &x, LDS &lds, uint32_t sb) {   // sb: which staging workgroup
#ifdef UAVX_STAMPS
    unsigned long long stamps[7] = {};
    STAMP(0);
#endif
    const int L = NT ? NT : p.N;
    const int S = EXT ? p.nslots : L;                 // lanes per layout
    const int epg = min((kWave * W) / S, kHintJobs);    // layouts a staging workgroup draws at once
    uint32_t *cnt = reinterpret_cast<uint32_t *>(lds.obs);        // job list: word 0 = count, job g = {env, episode} in words 1 + 2 g, 2 + 2 g
    // ---- what did this workgroup's last scan find?  Its own hint slots, ONE scalar load (wave-uniform, through the scalar
    // cache: a few hundred cycles at a moment when a vector load queues behind the first loads of every wavefront of the launch)
    typedef uint32_t HintWords __attribute__((ext_vector_type(2 * kHintJobs)));
    HintWords hw;
    uint2 *myhints = x.hints + (size_t)sb * kHintJobs;
    asm volatile("s_load_dwordx16 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(hw) : "s"(myhints) : "memory");
    int n = 0;
#pragma unroll
    for (int k = 0; k < kHintJobs; k++) {      // uniform: scalar code, the list itself goes to LDS through lane 0
        const uint32_t he = hw[2 * k], hp = hw[2 * k + 1];
        if (k < epg && he != 0u && he <= (uint32_t)p.E) {
            if (threadIdx.x == 0) { cnt[1 + 2 * n] = he - 1u; cnt[2 + 2 * n] = hp; }
            n++;
        }
    }
    if (n == 0) {
        // ---- scan: one window of 64 W envs, a lane each; what it finds is drawn by THIS workgroup in the NEXT launch ----
        const uint32_t span = kWave * W;
        const uint32_t windows = ((uint32_t)p.E + span - 1u) / span;
        // Which window?  Staging workgroup b owns the windows b, b + pf_blocks, b + 2 pf_blocks ... and looks at one of them per
        // launch, picked by the low bits of the clock: any window is as good as any other (results never depend on what is
        // parked; nothing on the host or in device memory counts launches, so a captured graph behaves like eager calls).
        const uint32_t turns = (windows + x.pf_blocks - 1u) / x.pf_blocks;
        const uint32_t turn = __builtin_amdgcn_readfirstlane((uint32_t)(__builtin_amdgcn_s_memtime() >> 7)) % turns;
        const uint32_t se = ((sb + turn * x.pf_blocks) % windows) * span + threadIdx.x;
        uint32_t want_ep = 0;
        bool need = false;
        if (se < (uint32_t)p.E) {
            const uint32_t y = p.env_rec[se].y;
            const uint32_t ep = y & ~kRecEnded;
            const uint4 t0 = p.stage_tag[se], t1 = p.stage_tag[(uint32_t)p.E + se];
            const uint4 ta = (ep & 1u) ? t1 : t0, tb = (ep & 1u) ? t0 : t1;      // tags of the slots of episodes ep / ep + 1
            const bool miss_a = !(y & kRecEnded) && !stage_hit(ta, stage_want<EXT>(p, se, ep, x.seed_lo, x.seed_hi));
            const bool miss_b = !stage_hit(tb, stage_want<EXT>(p, se, (ep + 1u) & ~kRecEnded, x.seed_lo, x.seed_hi));
            need = miss_a || miss_b;
            want_ep = miss_a ? ep : ((ep + 1u) & ~kRecEnded);
        }
        if (threadIdx.x == 0) cnt[0] = 0u;
        group_sync<W>();
        if (need) {   // the first epg of them (which ones does not matter; the rest is found again when the window comes round)
            const uint32_t k = atomicAdd(cnt, 1u);
            if ((int)k < epg) myhints[k] = make_uint2(se + 1u, want_ep);
        }
#ifdef UAVX_STAMPS
        STAMP(1); STAMP(2);
        stamp_log(stamps, __any(need) ? 11u : 10u);   // scanned: left hints / nothing to draw
#endif
        return;
    }
    if (threadIdx.x == 0) cnt[0] = (uint32_t)n;
    // the level table (at most 16 x 80 B) rides along into LDS: the chain then reads its env's box from there instead of from
    // memory (a dependent load behind the level draw)
    // (16 levels x 5 float4 = 80 rows behind the 64 rows the chain of a one-wavefront workgroup works on; EXT kernels have 192)
    constexpr int kLvlF4 = (int)(sizeof(LevelParams) / 16);
    constexpr bool kLvlLds = EXT && W == 1 && LDS::kRows >= kWave + UAVX_MAX_LEVELS * kLvlF4;
    static_assert(UAVX_MAX_LEVELS * kLvlF4 <= 2 * kWave, "the level table is two rows per lane");
    // requested here, put into LDS behind the Philox rounds (the loads' latency rides under those)
    float4 lvl_row0 = make_float4(0.f, 0.f, 0.f, 0.f), lvl_row1 = lvl_row0;
    if (kLvlLds && p.n_levels > 0) {
        const int last = p.n_levels * kLvlF4 - 1;
        lvl_row0 = reinterpret_cast<const float4 *>(p.levels)[min((int)threadIdx.x, last)];
        lvl_row1 = reinterpret_cast<const float4 *>(p.levels)[min((int)threadIdx.x + kWave, last)];
    }
    group_sync<W>();
    // The hints are marked "taken" only BEHIND this barrier: `n` must be the same in every wavefront of the workgroup (W > 1:
    // each wavefront reads the slots with its own scalar load above), and a clear in front of the barrier could reach memory
    // before a late sibling's load -- that wavefront would see n == 0, take the scan path and leave the others alone at the
    // barriers of the chain.  NO store to the hint slots may be placed in front of this barrier.
    if ((int)threadIdx.x < kHintJobs) myhints[threadIdx.x] = make_uint2(0u, 0u);   // taken
    // ---- the chain, one lane per slot ----
    StageMap m;
    uint32_t episode = 0;
    {
        const int lane = threadIdx.x;
        const int g = (lane * p.magic_s) >> 16;       // floor(lane / S) for lane < 256 (host test)
        m.i = lane - g * S;
        m.g = g < n ? g : 0;
        m.active = g < n;
        m.base = m.active ? (g * S) & (kWave - 1) : 0;
        m.rbase = m.active ? g * S : 0;
        m.e = m.active ? cnt[1 + 2 * g] : 0u;
        episode = m.active ? cnt[2 + 2 * g] : 0u;
    }
    const bool go = m.active;
    // A hint is one launch old: is the layout still wanted, and may its slot be written NOW?  Same rule as the scan applies --
    // the env's record and the slot's tag as THIS launch finds them (see the invariant above) -- but the two loads are only
    // waited for in front of the stores: the Philox rounds, the level and the whole chain run meanwhile on the hinted
    // (env, episode), and a layout that fails the test is simply not stored.
    const uint32_t rec_y = p.env_rec[m.e].y;
    const uint4 tag_now = p.stage_tag[(episode & 1u) * (uint32_t)p.E + m.e];
    group_sync<W>();   // (the job list lives in words the chain's scratch reuses)
    STAMP(1);
    __builtin_amdgcn_s_setprio(3);   // a serial chain the launch must not end up waiting for: issue ahead of the SIMD mates
    const uint32_t k0 = x.seed_lo, k1 = x.seed_hi;
    const uint64_t ge = (uint64_t)p.env_offset + m.e;
    const unsigned long long group = (S >= 64) ? ~0ull : ((1ull << S) - 1ull);
    const bool learner = m.i < L;
    // Every Philox stream whose counter is known up front runs in ONE rolled loop (four independent multiply chains fill each
    // other's latency; called one after the other they were four loops of dependent multiplies): the slot's first and second
    // candidates (attempts 0 and 1: most layouts need a redraw somewhere, few slots need two), the env's level, and -- bodies --
    // waypoint 0.  Further attempts of a slot are drawn on demand.
    uint32_t cw[4][4];
    {
        const uint32_t e_lo = (uint32_t)ge, e_hi = (uint32_t)(ge >> 32) & 0xFFFFu;
        uint32_t st[4][4] = {{e_lo, e_hi | ((uint32_t)m.i << 16), 0u, episode},             // candidates, attempt 0
                             {e_lo, e_hi | ((uint32_t)m.i << 16), 1u, episode},             // candidates, attempt 1
                             {e_lo, e_hi | (0xFFFFu << 16), 0u, episode},                   // level of the episode (pseudo-slot 0xFFFF)
                             {e_lo, e_hi | ((uint32_t)m.i << 16), 0x80000000u, episode}};   // waypoint 0 (bodies; key = the body seed)
        uint32_t ka0 = k0, ka1 = k1, kb0 = p.body_k0, kb1 = p.body_k1;
#pragma unroll 1
        for (int r = 0; r < 10; r++) {   // Philox4x32-10, the rounds of reset_words()
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint64_t p0 = (uint64_t)0xD2511F53u * st[q][0];
                const uint64_t p1 = (uint64_t)0xCD9E8D57u * st[q][2];
                const uint32_t n0 = (uint32_t)(p1 >> 32) ^ st[q][1] ^ (q == 3 ? kb0 : ka0);
                const uint32_t n2 = (uint32_t)(p0 >> 32) ^ st[q][3] ^ (q == 3 ? kb1 : ka1);
                st[q][1] = (uint32_t)p1; st[q][3] = (uint32_t)p0; st[q][0] = n0; st[q][2] = n2;
            }
            ka0 += 0x9E3779B9u; ka1 += 0xBB67AE85u; kb0 += 0x9E3779B9u; kb1 += 0xBB67AE85u;
        }
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int k = 0; k < 4; k++) cw[q][k] = st[q][k];
    }
    STAMP(3);
    if (kLvlLds && p.n_levels > 0) {
        const int t = (int)threadIdx.x;
        if (t < p.n_levels * kLvlF4) lds.pos[kWave + t] = lvl_row0;
        if (t + kWave < p.n_levels * kLvlF4) lds.pos[2 * kWave + t] = lvl_row1;
        group_sync<W>();
    }
    double lox = p.lox, loy = p.loy, hix = p.hix, hiy = p.hiy;
    float sq2r = p.sq_two_r;
    uint32_t lvl = 0;
    int nl = L, nb = EXT ? p.B : 0;
    if (EXT && p.n_levels > 0) {   // MUW:116 extended: the env takes its level first (every lane of the env computes the same one)
        if (go) {
            lvl = (p.level_lo >= 0) ? (uint32_t)p.level_lo + __umulhi(cw[2][0], (uint32_t)(p.level_hi - p.level_lo + 1)) : (uint32_t)p.lvl_next[m.e];
            lvl = min(lvl, (uint32_t)(p.n_levels - 1));
        }
        const LevelParams *lv = kLvlLds ? reinterpret_cast<const LevelParams *>(&lds.pos[kWave]) + lvl : &p.levels[lvl];
        lox = lv->lox; loy = lv->loy; hix = lv->hix; hiy = lv->hiy;
        sq2r = lv->sq_two_r;
        nl = lv->n_active; nb = lv->b_active;
    }
    const double bx = hix - lox, by = hiy - loy, inv32 = 1.0 / 4294967296.0;
    auto point = [&](uint32_t wx, uint32_t wy, float &px, float &py) {   // lo + (hi - lo) * U cast to float32, as reset_candidates()
        px = (float)(lox + bx * ((double)wx * inv32));
        py = (float)(loy + by * ((double)wy * inv32));
    };
    const bool part = go && (learner ? m.i < nl : m.i - L < nb);   // this lane's slot takes part in the episode
    float4 *row = &lds.pos[m.rbase];
    ResetCandidates c = {INFINITY, INFINITY, INFINITY, INFINITY};    // a slot that does not take part never clashes with anyone
    if (part) { point(cw[0][0], cw[0][1], c.sx, c.sy); point(cw[0][2], cw[0][3], c.tx, c.ty); }
    if (go) row[m.i] = make_float4(c.sx, c.sy, c.tx, c.ty);
    group_sync<LDS::kW>();
    STAMP(4);
#pragma unroll 1
    for (int phase = 0; phase < 2; phase++) {  // 0: all start points in slot order (MUW:126-137, bodies after learners), 1: targets MUW:140-153
        uint32_t attempt = 0;
        const bool mine = part && (phase == 0 || learner);
        const int below = phase ? min(m.i, L) : m.i;     // lower-indexed slots whose accepted point mine must keep clear of
        float qx = phase ? c.tx : c.sx, qy = phase ? c.ty : c.sy;
        // which lower-indexed slots this one is too close to: a bit each.  The whole row of tests is made ONCE; a redraw
        // changes one point of the env, so afterwards every lane re-tests against that point only.
        unsigned long long cm = 0ull;
        bool self = mine && phase && too_close(sq2r, qx, qy, c.sx, c.sy);                          // MUW:146
        if (mine) {
#pragma unroll 1
            for (int j0 = 0; j0 < below; j0 += kChainRows) {
                float2 o[kChainRows];
#pragma unroll
                for (int u = 0; u < kChainRows; u++) {
                    const float4 *r4 = &row[min(j0 + u, below - 1)];
                    o[u] = *reinterpret_cast<const float2 *>(phase ? &r4->z : &r4->x);
                }
#pragma unroll
                for (int u = 0; u < kChainRows; u++)
                    if (j0 + u < below && too_close(sq2r, o[u].x, o[u].y, qx, qy)) cm |= 1ull << (j0 + u);  // MUW:135,151
            }
        }
#pragma unroll 1
        for (;;) {
            int low;   // lowest-indexed clashing slot of my env (everything below it is final, everything above keeps its candidate)
            if (!lowest_clash<LDS>(m, lds, group, mine && (self || cm != 0ull), low)) break;
            const bool redraw = mine && m.i == low;
            group_sync<LDS::kW>();
            if (redraw) {
                float rx, ry;
                if (++attempt == 1u) {
                    point(phase ? cw[1][2] : cw[1][0], phase ? cw[1][3] : cw[1][1], rx, ry);
                } else {
                    const ResetCandidates r = reset_candidates(ge, (uint32_t)m.i, attempt, episode, k0, k1, lox, loy, hix, hiy);
                    rx = phase ? r.tx : r.sx; ry = phase ? r.ty : r.sy;
                }
                qx = rx; qy = ry;
                if (phase) { c.tx = rx; c.ty = ry; row[m.i].z = rx; row[m.i].w = ry; self = too_close(sq2r, rx, ry, c.sx, c.sy); }
                else { c.sx = rx; c.sy = ry; row[m.i].x = rx; row[m.i].y = ry; }
            }
            group_sync<LDS::kW>();
            if (W == 1) {
                // everybody re-tests against the ONE point of its env that moved: slots above it update that bit of theirs, the
                // slots below it answer for the redrawn slot's own row of tests (the test is symmetric) through a ballot
                const bool any_low = low < S;
                const float4 *r4 = &row[any_low ? low : 0];
                const float2 np = *reinterpret_cast<const float2 *>(phase ? &r4->z : &r4->x);
                const bool t = mine && any_low && m.i != low && too_close(sq2r, np.x, np.y, qx, qy);
                const unsigned long long bits = __ballot(t && m.i < low);
                if (any_low && m.i > low) cm = (cm & ~(1ull << low)) | ((unsigned long long)t << low);
                if (redraw) cm = (bits >> m.base) & ((1ull << low) - 1ull);
            } else if (mine) {   // an env may span two wavefronts: the full row of tests again
                cm = 0ull;
#pragma unroll 1
                for (int j0 = 0; j0 < below; j0++) {
                    const float4 *r4 = &row[j0];
                    const float2 o = *reinterpret_cast<const float2 *>(phase ? &r4->z : &r4->x);
                    if (too_close(sq2r, o.x, o.y, qx, qy)) cm |= 1ull << j0;
                }
            }
        }
    }
    STAMP(5);
    const uint32_t ep_now = rec_y & ~kRecEnded;
    const bool wanted = go && ((episode == ep_now && !(rec_y & kRecEnded)) || episode == ((ep_now + 1u) & ~kRecEnded)) &&
                        !stage_hit(tag_now, stage_want<EXT>(p, m.e, episode, k0, k1));
    if (wanted) {
        const uint32_t sl = episode & 1u;   // the slot of this episode's layout
        if (learner) {   // a parked learner sits at +inf with target 0 (what reset_envs_wave leaves in its record)
            p.stage_agent[(sl * (uint32_t)p.E + m.e) * (uint32_t)L + (uint32_t)m.i] =
                part ? make_float4(c.sx, c.sy, c.tx, c.ty) : make_float4(INFINITY, INFINITY, 0.f, 0.f);
        } else if (EXT) {
            float2 q = make_float2(INFINITY, INFINITY);    // a body that does not take part
            float4 leg = make_float4(0.f, 0.f, 0.f, 0.f);
            if (part) {
                float wx, wy;
                point(cw[3][0], cw[3][1], wx, wy);
                q = make_float2(c.sx, c.sy);
                leg = make_leg(p.body_step, c.sx, c.sy, wx, wy);   // leg 0: towards waypoint 0
            }
            const uint32_t gi = (sl * (uint32_t)p.E + m.e) * (uint32_t)p.B + (uint32_t)(m.i - L);
            p.stage_bpos[gi] = q;
            p.stage_bleg[gi] = leg;
        }
    }
    // the tag goes last, behind every store of the layout it vouches for (it is read by a LATER launch, across a kernel
    // boundary; the order only matters for whoever inspects the arrays while this launch runs: nobody does)
    group_sync<W>();
    if (wanted && m.i == 0) {
        uint4 tag = stage_want<EXT>(p, m.e, episode, k0, k1);
        tag.w = (tag.w & ~0xFFu) | (EXT ? lvl : 0u);   // the level it drew
        p.stage_tag[(episode & 1u) * (uint32_t)p.E + m.e] = tag;
    }
#ifdef UAVX_STAMPS
    STAMP(2);
    stamp_log(stamps, 13u);   // drew layouts
#endif
}

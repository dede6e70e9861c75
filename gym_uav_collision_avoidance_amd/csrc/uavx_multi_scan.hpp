// uavx_multi_scan.hpp -- lane mapping, LDS tiles, agent load / store and the neighbour scans.  Included by uavx_multi.hip inside
// namespace uavx, after uavx_multi_params.hpp.

struct LaneMap {
    int lane;        // thread in its workgroup (the lane when the workgroup is one wavefront)
    int i, base;     // agent index in its env, first lane of the env's group
    int rbase, nslots;  // first LDS neighbour row of the env, rows per env (N unless the env has scripted bodies)
    int nlearn;         // the first nlearn rows of an env are agents with a lane each (= N)
    int g;              // env index within the workgroup
    bool active;
    uint32_t e, a;   // env, agent slot (E*N < 2^26, checked by uavx_create)
    uint32_t a0;     // first agent slot of this workgroup
    uint32_t wave;   // workgroup index (= index into wave_steps)
    int obs0;        // first float of this wavefront's obs staging tile in lds.obs (0 unless the workgroup holds several tiles)
    int cnt;         // active agent slots in this workgroup: threads [0, cnt), slots [a0, a0 + cnt)
};

// Work mapping of one launch: a workgroup of W wavefronts holds epw = floor(64 W / N) whole envs, one thread per agent,
// packed from thread 0 (so agent slot = a0 + thread id).  W = 1 everywhere except for agent counts that would leave
// many lanes of a single wavefront idle (N = 24: 48 of 64; three wavefronts hold 8 envs with none idle).
template <int NT, bool EXT = false, int W = 1>
__device__ __forceinline__ LaneMap lane_map_from(uint32_t E, int n_agents, int envs_per_group, int magic, int nslots, uint32_t wave,
                                                 uint32_t lane = threadIdx.x, uint32_t tile = 0u) {
    LaneMap m;
    const int N = NT ? NT : n_agents;
    const int epw = NT ? (kWave / (NT ? NT : 1)) : envs_per_group;
    m.lane = lane;                   // thread in its workgroup (= lane for W == 1; tiled workgroups pass their lane)
    int g;
    if (NT) {
        g = m.lane / (NT ? NT : 1);
        m.i = m.lane % (NT ? NT : 1);
    } else {
        g = (m.lane * magic) >> 16;  // floor(thread / N) for thread < 256
        m.i = m.lane - g * N;
    }
    m.wave = wave;
    const uint32_t e0 = wave * epw;
    const uint32_t envs_here = e0 < E ? min(E - e0, (uint32_t)epw) : 0u;
    m.e = e0 + g;
    m.active = (uint32_t)g < envs_here;
    m.base = m.active ? (g * N) & (kWave - 1) : 0;  // first lane of the env's group in its wavefront (W == 1: ballot shifts)
    m.g = m.active ? g : 0;
    m.nslots = EXT ? nslots : N;
    m.nlearn = N;
    m.rbase = (m.active ? g * m.nslots : 0) + (int)tile * kWave;  // idle lanes still execute the LDS scan: keep it in bounds
    m.obs0 = (int)tile * (kWave * UAVX_OBS_DIM);
    m.a0 = e0 * N;
    m.a = m.a0 + m.lane;            // whole envs are packed from thread 0: slot = a0 + thread
    m.cnt = (int)envs_here * N;
    return m;
}
template <int NT, bool EXT = false, int W = 1>
__device__ __forceinline__ LaneMap lane_map(const MultiParams &p, uint32_t wave = blockIdx.x) {   // wave: env-workgroup index
    return lane_map_from<NT, EXT, W>((uint32_t)p.E, p.N, p.epw, p.magic, p.nslots, wave);
}

struct AgentRegs {
    float x, y, prev_d;
    uint32_t flags;
    float tx, ty, init_d;
    double vx, vy;
};

// LDS of one workgroup (W wavefronts; W > 1 only on the runtime-N path, see pick_group_waves()).
template <bool EXT, int W = 1>
struct LdsT {
    static constexpr int kW = W;
    static constexpr int kRows = (EXT && kExtSlots > kWave * W) ? kExtSlots : kWave * W;
    float4 pos[kRows];            // {old.x, old.y, new.x, new.y} per neighbour slot
    float theta[kRows];           // heading atan2(vy, vx)
    float obs[kWave * W * UAVX_OBS_DIM];
};
// With scripted bodies the neighbour rows alone are 3.8 KB per wavefront; the obs staging tile shares their bytes: it is
// written after the last read of the rows (one wavefront per workgroup: DS operations execute in issue order), so the
// workgroup needs 3 840 B instead of 6 400 B and a CU holds 28 wavefronts (the register limit) instead of 25.
template <>
struct LdsT<true, 1> {
    static constexpr int kW = 1;
    static constexpr int kRows = kExtSlots;
    union {
        struct {
            float4 pos[kRows];
            float theta[kRows];
        };
        float obs[kWave * UAVX_OBS_DIM];
    };
};
// All cross-agent traffic of an env stays inside its workgroup.  With one wavefront per workgroup a compiler-level
// ordering point is enough (wave_lds_sync); an env that spans two wavefronts needs the workgroup barrier.
template <int W>
__device__ __forceinline__ void group_sync() {
    if (W == 1) wave_lds_sync();
    else __syncthreads();
}
template <int W>
__device__ __forceinline__ bool group_any(bool v) {   // same answer in every thread of the workgroup
    if (W == 1) return __ballot(v) != 0ull;
    return __syncthreads_or(v ? 1 : 0) != 0;
}
using Lds = LdsT<false>;
// T one-wavefront TILES side by side in one workgroup (step_kernel / step_ex_kernel, T > 1): tile t owns rows [64 t, 64 t + 64)
// of each array -- the tile offset rides in the lane map's row base and obs0, so no LDS address needs a register of its own --
// and orders its traffic at wavefront level like a one-wavefront workgroup (kW = 1).
template <int T>
struct LdsTiles {
    static constexpr int kW = 1;
    static constexpr int kRows = kWave * T;
    float4 pos[kRows];
    float theta[kRows];
    float obs[kWave * T * UAVX_OBS_DIM];
};

// World limits of this lane's env: kernel arguments, or (EXT) the level its flags word names -- two 16-byte loads from a
// table every lane of the chip shares, i.e. an L1/L2 hit whose latency hides under the kinematics.
// d_sense alone (all the neighbour scan needs): the other seven limits are fetched AFTER the scan, where they are used --
// per-lane values loaded at the top of the step stayed in eight registers across the scan, the most register-hungry stretch
// (h: the handle's own limits as the caller holds them -- `p` itself, or step_kernel's fetched copies, HotParams)
template <bool EXT, class H>
__device__ __forceinline__ float sense_limit(const MultiParams &p, const H &h, uint32_t flags) {
    if (EXT && p.n_levels > 0) return p.levels[(flags & kLevelMask) >> kLevelShift].sq_sense;
    return h.sq_sense;
}
template <bool EXT, class H>
__device__ __forceinline__ WorldLims world_lims(const MultiParams &p, const H &h, uint32_t flags) {
    WorldLims w;
    if (EXT && p.n_levels > 0) {   // uniform: no curriculum installed -> the handle's own world, as in the plain kernels
        const float4 *t = reinterpret_cast<const float4 *>(&p.levels[(flags & kLevelMask) >> kLevelShift]);
        const float4 a = t[0], b = t[1];
        w.lo_x = a.x; w.lo_y = a.y; w.hi_x = a.z; w.hi_y = a.w;
        w.sq_sense = b.x; w.sq_two_r = b.y; w.inv_sense = b.z; w.inv_diag = b.w;
    } else {
        w.lo_x = h.lo_x; w.lo_y = h.lo_y; w.hi_x = h.hi_x; w.hi_y = h.hi_y;
        w.sq_sense = h.sq_sense; w.sq_two_r = h.sq_two_r; w.inv_sense = h.inv_sense; w.inv_diag = h.inv_diag;
    }
    return w;
}
template <bool EXT>
__device__ __forceinline__ WorldLims world_lims(const MultiParams &p, uint32_t flags) {
    return world_lims<EXT>(p, p, flags);
}

// Agent slots are addressed with 32-bit lane offsets from scalar base pointers (saddr + voffset
// addressing; uavx_create rejects E*N >= 2^26).
// prev_distance as the reference would hold it for this (flags, position, target)
__device__ __forceinline__ float natural_prev_d(uint32_t flags, float x, float y, float tx, float ty) {
    const float d = norm32(tx - x, ty - y);
    return ((flags & UAVX_FLAG_DONE) && !(flags & kFlagJustDone)) ? 0.f : d;
}

__device__ __forceinline__ void load_agent(const MultiParams &p, uint32_t a, AgentRegs &s) {
    const float2 d = p.pos[a];
    const double2 v = p.vel[a];
    const Goal g = p.goal[a];
    s.x = d.x; s.y = d.y;
    s.vx = v.x; s.vy = v.y;
    s.tx = g.tx; s.ty = g.ty; s.init_d = g.init_d; s.flags = g.flags;
    s.prev_d = natural_prev_d(s.flags, s.x, s.y, s.tx, s.ty);
    if (s.flags & kFlagPrevOvr) s.prev_d = p.prev_ovr[a];  // rare: only after a caller poked the state
}
// flags_in: the flags word as loaded (the word is stored only if the step changed it)
// (pos / vel / goal: p's arrays, handed over separately because the register-tight kernels fetch those pointers again at
//  their end instead of holding them in scalar registers from the loads at the top on, see LATE())
// (nslot = E * N, from whichever kernel arguments the caller has at hand)
__device__ __forceinline__ void store_agent(uint32_t nslot, float2 *pos, double2 *vel, Goal *goal, uint32_t a, const AgentRegs &s,
                                            uint32_t flags_in) {
    // velocity: 16 B per lane, written through (sc1) like the obs tile so that it drains during the launch instead
    // of at the kernel boundary (A/B at 65536x4: 6.71 -> 6.21 us); the 8-byte position store stays plain
    // (narrow sc1 stores are slow: 6.29 us with both)
    store16_wt(make_rsrc(vel, nslot * 16u), a * 16u, make_double2(s.vx, s.vy));
    pos[a] = make_float2(s.x, s.y);
    if (s.flags != flags_in) goal[a].flags = s.flags;
}
__device__ __forceinline__ void store_agent(const MultiParams &p, float2 *pos, double2 *vel, Goal *goal, uint32_t a,
                                            const AgentRegs &s, uint32_t flags_in) {
    store_agent((uint32_t)p.E * (uint32_t)p.N, pos, vel, goal, a, s, flags_in);
}
__device__ __forceinline__ void store_agent(const MultiParams &p, uint32_t a, const AgentRegs &s, uint32_t flags_in) {
    store_agent(p, p.pos, p.vel, p.goal, a, s, flags_in);
}

// Neighbour scan of one agent over the other N-1 agents of its env (positions staged in LDS).
//  * obs part (AG:44-64 as used by MUW:75-95): the two nearest strictly within d_sense at FINAL
//    positions, ascending by the float32 distance, ties -> lower index (agents are visited in
//    ascending index order and only a strictly smaller distance displaces an entry);
//  * STEP part (MUW:198-210): the reference tests the nearest in-range agents against the thresholds
//    2R and 1.0, so only the MINIMUM in-range distance under the Gauss-Seidel rule (j<i moved, j>i
//    not yet) matters.  sqrtf is monotone, so every threshold test is done on the squared distance
//    fl(dx*dx)+fl(dy*dy) against a host-computed exact float32 limit (no sqrt on this part).
struct Neigh {
    float d1, d2;
    int j1, j2;
    float step_sq_min;
};

template <int NT, bool STEP, class LDS>
__device__ __forceinline__ Neigh scan_neighbours_exact(float sq_sense, const LaneMap &m, const LDS &lds, float nx,
                                                       float ny) {
    const int N = NT ? NT : m.nslots;
    Neigh r;
    r.d1 = r.d2 = INFINITY;
    r.j1 = r.j2 = -1;
    r.step_sq_min = INFINITY;
    const float4 *row = &lds.pos[m.rbase];
    // Branch-free: out-of-range agents enter the insertion with distance +inf, which never displaces.
    auto visit = [&](int j, float4 q) {
        const float dxn = q.z - nx, dyn = q.w - ny;  // target_agent.location - self.location (AG:51)
        const float ax = dxn * dxn, ay = dyn * dyn;
        const float sn = ax + ay;
        if (STEP) {
            const float dxo = q.x - nx, dyo = q.y - ny;
            const float bx = dxo * dxo, by = dyo * dyo;
            const float so = bx + by;
            const float ss = (j < m.i) ? sn : so;      // j<i already moved this step, j>i not yet
            r.step_sq_min = fminf(r.step_sq_min, (ss < sq_sense) ? ss : INFINITY);
        }
        const float dn = (sn < sq_sense) ? sqrt_rn(sn) : INFINITY;  // AG:51-52 (IEEE-rounded sqrt)
        const bool lt1 = dn < r.d1, lt2 = dn < r.d2;
        r.d2 = lt1 ? r.d1 : (lt2 ? dn : r.d2);
        r.j2 = lt1 ? r.j1 : (lt2 ? j : r.j2);
        r.d1 = lt1 ? dn : r.d1;
        r.j1 = lt1 ? j : r.j1;
    };
    if (NT) {
        // all N-1 LDS reads are issued before the first use (one lgkmcnt wait instead of N-1)
        constexpr int M = NT > 1 ? NT - 1 : 1;
        float4 q[M];
        int js[M];
#pragma unroll
        for (int k = 0; k < NT - 1; k++) {
            js[k] = k + (k >= m.i ? 1 : 0);  // ascending over the other agents, self skipped
            q[k] = row[js[k]];
        }
#pragma unroll
        for (int k = 0; k < NT - 1; k++) visit(js[k], q[k]);
    } else {
        for (int k = 0; k < N - 1; k++) {
            const int j = k + (k >= m.i ? 1 : 0);
            visit(j, row[j]);
        }
    }
    return r;
}

__device__ __forceinline__ uint32_t med3_u32(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r;
    asm("v_med3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// The same result for N = 4 with square roots of the two winners only (at N = 5 the kept third key and the inlined fallback
// cost the fused multi-step kernel a wavefront per SIMD).  The visits keep the three smallest SQUARED
// distances s1 <= s2 <= s3 (out of range: +inf), ties -> lower index (ascending visits, strict compares), which is the
// order by (s, index).  sqrtf is monotone, so the reference's order by (float32 distance, index) (AG:52-62) can differ from it
// only where two roots are EQUAL: for the first two that is decided here exactly (equal roots -> lower index first); the third
// can only displace the second if its root equals the second's, which needs s3 within a few ulps of s2 (equal roots of s and
// s' need |s - s'| < 2^-22 s, at most four ulps of s): any lane with s3 - s2 <= 8 ulps sends its wavefront through the exact
// scan (never on random layouts; symmetric ones such as reset(circular=True) take it).  Bit-identical to scan_neighbours_exact.
template <int NT, bool STEP, class LDS>
__device__ __forceinline__ Neigh scan_neighbours_sq(float sq_sense, const LaneMap &m, const LDS &lds, float nx, float ny) {
    static_assert(NT == 4, "three other agents");
    const float4 *row = &lds.pos[m.rbase];
    constexpr uint32_t kInfBits = 0x7f800000u;
    uint32_t s1 = kInfBits, s2 = kInfBits, s3 = kInfBits;
    float step_min = INFINITY;
    int j1 = -1, j2 = -1;
    constexpr int M = NT - 1;
    float4 q[M];
    int js[M];
#pragma unroll
    for (int k = 0; k < M; k++) {   // all LDS reads in front of the first use
        js[k] = k + (k >= m.i ? 1 : 0);
        q[k] = row[js[k]];
    }
#pragma unroll
    for (int k = 0; k < M; k++) {
        const int j = js[k];
        const float dxn = q[k].z - nx, dyn = q[k].w - ny;   // target_agent.location - self.location (AG:51)
        const float ax = dxn * dxn, ay = dyn * dyn;
        const float sn0 = ax + ay;
        if (STEP) {
            const float dxo = q[k].x - nx, dyo = q[k].y - ny;
            const float bx = dxo * dxo, by = dyo * dyo;
            const float so = bx + by;
            step_min = fminf(step_min, (j < m.i) ? sn0 : so);   // j<i already moved this step, j>i not yet; d_sense below
        }
        // AG:52 (NaN: out).  Non-negative floats and +inf order like their bit patterns: the three smallest are kept with
        // integer min / median (fminf / fmaxf would canonicalise every operand first)
        const uint32_t sn = (sn0 < sq_sense) ? __float_as_uint(sn0) : kInfBits;
        const bool lt1 = sn < s1, lt2 = sn < s2;
        j2 = lt1 ? j1 : (lt2 ? j : j2);
        j1 = lt1 ? j : j1;
        s3 = med3_u32(s2, s3, sn);
        s2 = med3_u32(s1, s2, sn);
        s1 = min(s1, sn);
    }
    Neigh r;
    r.step_sq_min = (step_min < sq_sense) ? step_min : INFINITY;
    r.d1 = sqrt_rn(__uint_as_float(s1));   // +inf stays +inf
    r.d2 = sqrt_rn(__uint_as_float(s2));
    const bool swap = r.d1 == r.d2 && j2 < j1;   // equal roots: lower index first (both in range: j2 >= 0)
    r.j1 = swap ? j2 : j1;
    r.j2 = swap ? j1 : j2;
    const bool near_tie = m.active && s3 < kInfBits && s3 - s2 <= 8u;
    if (__builtin_expect(__any(near_tie), 0)) return scan_neighbours_exact<NT, STEP>(sq_sense, m, lds, nx, ny);
    return r;
}

// Same result for N > 5 (and the N = 8 specialisation) at about half the per-neighbour cost: the scan keeps the
// three smallest KEYS, key = (bits of the squared distance with the low 6 bits replaced by a name of the neighbour), with
// one v_min_u32 + two v_med3_u32 per neighbour instead of a compare/select insertion of (distance, index)
// pairs, and takes square roots only of the two winners (their exact squared distances are recomputed from LDS).
// Non-negative floats order like their bit patterns and NaN / +inf patterns sort above every finite value, so
// keys order by (squared distance truncated to 2^-17 relative, name).  sqrtf is monotone and two squared
// distances whose truncations differ by two or more steps have different float32 roots, so the order by key
// equals the reference's order by (float32 distance, index) (AG:52-62) unless two of the kept keys are within
// one truncation step of each other at or below the sensing limit -- then (about 1 wave in 1000 on random
// layouts; always on symmetric ones like reset(circular=True)) the wave falls back to the exact scan.  An agent
// outside the kept three can only belong in the top two if the third key is within a step of the second, which
// is one of the fallback conditions.  Bit-identical to scan_neighbours_exact.  A slot that does not take part
// (parked learner, inactive body: extension) is staged at +inf: its key sorts above every real one and its
// squared distance fails every threshold.
#ifdef UAVX_STAMPS
__shared__ int g_dbg_fallback;   // diagnostic build: this workgroup took the exact scan / the finish() branch (bits 0 / 1)
#endif

// SQ: the one-step kernel at N = 4 takes scan_neighbours_sq (the fused kernels keep the exact scan: there the inlined fallback
// cost registers -- step_k_kernel<4> 69 -> 78 VGPRs with two scalars spilled into VGPR lanes, step_ex_kernel<4> 50 -> 57)
template <int NT, bool STEP, class LDS, bool SQ = false>
__device__ __forceinline__ Neigh scan_neighbours(float sq_sense, const LaneMap &m, const LDS &lds, float nx,
                                                 float ny) {
    if (SQ && NT == 4) return scan_neighbours_sq<4, STEP>(sq_sense, m, lds, nx, ny);
    if (NT != 0 && NT <= 5) return scan_neighbours_exact<NT, STEP>(sq_sense, m, lds, nx, ny);
    const int N = NT ? NT : m.nslots;
    if (NT == 0 && N <= 5) return scan_neighbours_exact<NT, STEP>(sq_sense, m, lds, nx, ny);  // <= 4 others: nothing to save
    const float4 *row = &lds.pos[m.rbase];
    uint32_t k1 = 0xffffffffu, k2 = 0xffffffffu, k3 = 0xffffffffu;
    float step_min = INFINITY;
    // The low 6 bits of a key only have to NAME the neighbour (two keys that agree above them are a near tie and take the
    // exact scan): they hold c = the neighbour's rank among the OTHER slots of the env (slot j = c + (c >= i)), which is
    // the same number in every lane -- the row address is then the lane's base + 16 c (+ 16 from agent i upwards) and the
    // key needs no per-lane index register.
    // (the mask sits in a VGPR so that the wave-uniform name can be the one scalar operand of a single v_and_or_b32)
    uint32_t keep;
    asm("v_mov_b32 %0, 0xffffffc0" : "=v"(keep));
    auto visit = [&](uint32_t c, bool below, float4 q) {   // below: slot < m.i (already moved in this step)
        const float dxn = q.z - nx, dyn = q.w - ny;
        const float ax = dxn * dxn, ay = dyn * dyn;
        const float sn = ax + ay;
        if (STEP) {
            const float dxo = q.x - nx, dyo = q.y - ny;
            const float bx = dxo * dxo, by = dyo * dyo;
            const float so = bx + by;
            step_min = fminf(step_min, below ? sn : so);  // fminf drops NaN; the d_sense test follows the loop
        }
        uint32_t key;
        asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(key) : "v"(sn), "v"(keep), "s"(c));
        k3 = med3_u32(k2, k3, key);
        k2 = med3_u32(k1, k2, key);
        k1 = min(k1, key);
    };
    const char *rowb = reinterpret_cast<const char *>(row);
    auto other = [&](int c, bool below) {   // the c-th other slot of the env as seen from agent i
        return *reinterpret_cast<const float4 *>(rowb + c * 16 + (below ? 0 : 16));
    };
    if (NT) {  // compile-time N: the LDS reads of a batch are issued before its first use
#ifndef UAVX_SCANBATCH
#define UAVX_SCANBATCH 7
#endif
        constexpr int M = NT > 1 ? NT - 1 : 1;
        constexpr int BATCH = M < UAVX_SCANBATCH ? M : UAVX_SCANBATCH;
#pragma unroll
        for (int c0 = 0; c0 < NT - 1; c0 += BATCH) {
            float4 q[BATCH];
#pragma unroll
            for (int c = 0; c < BATCH; c++)
                if (c0 + c < NT - 1) q[c] = other(c0 + c, c0 + c < m.i);
#pragma unroll
            for (int c = 0; c < BATCH; c++)
                if (c0 + c < NT - 1) visit((uint32_t)(c0 + c), c0 + c < m.i, q[c]);
        }
    } else {
        // two neighbours per trip, written out (inline asm is convergent in HIP, which rules out the unroll pragma)
        const int NL = m.nlearn;   // slots [0, NL) are agents with a lane each; [NL, N) scripted bodies (extension)
        int c = 0;
        for (; c + 1 < NL - 1; c += 2) {
            const bool la = c < m.i, lb = c + 1 < m.i;
            const float4 qa = other(c, la), qb = other(c + 1, lb);
            visit((uint32_t)c, la, qa);
            visit((uint32_t)c + 1u, lb, qb);
        }
        if (c < NL - 1) {
            const bool la = c < m.i;
            visit((uint32_t)c, la, other(c, la));
            c++;
        }
        // bodies sit above every learner and have moved before any of them: ONE squared distance serves the collision test
        // and the observation, and the Gauss-Seidel select folds away (rows {x, y, x, y}: 8-byte reads of the upper half)
        auto body = [&](uint32_t c, int r) {
            const float2 q = *reinterpret_cast<const float2 *>(&row[r].z);
            const float dxn = q.x - nx, dyn = q.y - ny;
            const float ax = dxn * dxn, ay = dyn * dyn;
            const float sn = ax + ay;
            if (STEP) step_min = fminf(step_min, sn);
            uint32_t key;
            asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(key) : "v"(sn), "v"(keep), "s"(c));
            k3 = med3_u32(k2, k3, key);
            k2 = med3_u32(k1, k2, key);
            k1 = min(k1, key);
        };
        for (; c + 1 < N - 1; c += 2) {
            body((uint32_t)c, c + 1);
            body((uint32_t)c + 1u, c + 2);
        }
        if (c < N - 1) body((uint32_t)c, c + 1);
    }
    // N > 5: at least five neighbours were visited, so k1..k3 are real keys
    const uint32_t t1 = k1 >> 6, t2 = k2 >> 6, t3 = k3 >> 6, ts = __float_as_uint(sq_sense) >> 6;
    const bool near_tie = m.active && ((t2 - t1 <= 1u && t1 <= ts) || (t3 - t2 <= 1u && t2 <= ts));
#ifdef UAVX_STAMPS
    if (__any(near_tie)) g_dbg_fallback = 1;
#endif
    const int c1 = (int)(k1 & 63u), c2 = (int)(k2 & 63u);
    const int j1 = c1 + (c1 >= m.i ? 1 : 0), j2 = c2 + (c2 >= m.i ? 1 : 0);
    const float4 q1 = row[j1], q2 = row[j2];
    const float ex1 = q1.z - nx, ey1 = q1.w - ny, ex2 = q2.z - nx, ey2 = q2.w - ny;
    const float mx1 = ex1 * ex1, my1 = ey1 * ey1, mx2 = ex2 * ex2, my2 = ey2 * ey2;
    const float s1 = mx1 + my1, s2 = mx2 + my2;
    const bool in1 = s1 < sq_sense, in2 = s2 < sq_sense;  // AG:52
    Neigh r;
    r.step_sq_min = (step_min < sq_sense) ? step_min : INFINITY;
    r.d1 = in1 ? sqrt_rn(s1) : INFINITY;
    r.d2 = in2 ? sqrt_rn(s2) : INFINITY;
    r.j1 = in1 ? j1 : -1;
    r.j2 = in2 ? j2 : -1;
    // Near ties (about one wavefront in 800 on random layouts; every wavefront of a symmetric one): the two nearest of a TIED
    // LANE are found again, exactly, by the whole wavefront -- lane t takes the tied agent's t-th neighbour, float32 distance
    // with the IEEE root, and two 64-bit minimum reductions over (distance bits, slot) give the reference's order (AG:52-62:
    // ascending distance, ties -> lower index).  About 150 instructions per tied lane.  Round 2 sent the whole wavefront
    // through the compare / select scan instead (+700 instructions, +43 % on the wavefront's life): with ~10 such wavefronts
    // in every 65 536-env launch those were the ones each launch ended with (tools/exp_stamps.py).  The minimum for the
    // collision tests (step_sq_min) is exact on the key path as it is.
    unsigned long long tied = __ballot(near_tie);
    if (__popcll(tied) > 6) return scan_neighbours_exact<NT, STEP>(sq_sense, m, lds, nx, ny);   // a symmetric layout: everybody ties
    while (tied != 0ull) {   // wave-uniform
        const int tl = (int)__builtin_ctzll(tied);
        tied &= tied - 1ull;
        const float ax = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(nx), tl));
        const float ay = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ny), tl));
        const float lim = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sq_sense), tl));
        const int ti = __builtin_amdgcn_readlane(m.i, tl), trb = __builtin_amdgcn_readlane(m.rbase, tl);
        const int t = (int)(threadIdx.x & (kWave - 1));
        const bool mine = t < N - 1;
        const int j = mine ? t + (t >= ti ? 1 : 0) : ti;                     // idle lanes look at the agent itself (distance 0, masked out)
        const float4 q = lds.pos[trb + j];
        const float dx = q.z - ax, dy = q.w - ay;
        const float xx = dx * dx, yy = dy * dy;
        const float sn = xx + yy;
        const float dn = sqrt_rn(sn);                                       // (wave-uniform inside: every lane calls it)
        unsigned long long key = (mine && sn < lim) ? ((unsigned long long)__float_as_uint(dn) << 32) | (uint32_t)j : ~0ull;   // AG:52
        auto wave_min = [](unsigned long long k) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const uint32_t hi = __shfl_xor((uint32_t)(k >> 32), off), lo = __shfl_xor((uint32_t)k, off);
                const unsigned long long o = ((unsigned long long)hi << 32) | lo;
                k = o < k ? o : k;
            }
            return k;
        };
        const unsigned long long m1 = wave_min(key);
        const unsigned long long m2 = wave_min(key == m1 ? ~0ull : key);
        if (t == tl) {
            r.d1 = m1 == ~0ull ? INFINITY : __uint_as_float((uint32_t)(m1 >> 32));
            r.j1 = m1 == ~0ull ? -1 : (int)(uint32_t)m1;
            r.d2 = m2 == ~0ull ? INFINITY : __uint_as_float((uint32_t)(m2 >> 32));
            r.j2 = m2 == ~0ull ? -1 : (int)(uint32_t)m2;
        }
    }
    return r;
}

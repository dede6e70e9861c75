// uavx_multi_host.hpp -- the extern "C" entry points of include/uavx.h for MultiUAVWorld2D (all but the snapshot calls and the
// self test: uavx_multi_snapshot.hpp): argument checks, then a launch through uavx_multi_launch.hpp.  Included by uavx_multi.hip
// at file scope, behind uavx_multi_launch.hpp.

extern "C" {

int uavx_version(void) { return UAVX_VERSION; }

#ifndef UAVX_SRC_HASH
#define UAVX_SRC_HASH ""
#endif
static const char kBuildInfo[] = "UAVX_SRC_HASH=" UAVX_SRC_HASH;   // the loader finds this marker in the file without mapping it
const char *uavx_build_info(void) { return kBuildInfo + 14; }
int uavx_polar_commands(const void *actions, int action_dtype, int64_t n, float scale, double *out, void *stream) {
    if (n < 0 || (n > 0 && (!actions || !out))) return UAVX_ERR_INVALID_ARG;
    if (action_dtype != UAVX_F32 && action_dtype != UAVX_F64) return UAVX_ERR_INVALID_ARG;
    if ((reinterpret_cast<uintptr_t>(actions) & (action_dtype == UAVX_F64 ? 15u : 7u)) || (reinterpret_cast<uintptr_t>(out) & 15u))
        return UAVX_ERR_INVALID_ARG;
    if (n == 0) return UAVX_OK;
    const auto kernel = action_dtype == UAVX_F64 ? &polar_commands_kernel<true> : &polar_commands_kernel<false>;
    return launch_items((uavx_handle *)nullptr, kernel, n, static_cast<hipStream_t>(stream), actions, n, scale, reinterpret_cast<double2 *>(out));
}

const char *uavx_strerror(int status) {
    switch (status) {
        case UAVX_OK: return "ok";
        case UAVX_ERR_INVALID_ARG: return "invalid argument";
        case UAVX_ERR_HIP: return "HIP runtime error";
        case UAVX_ERR_NO_DEVICE: return "no HIP device";
        case UAVX_ERR_UNSUPPORTED: return "unsupported";
        case UAVX_ERR_ALLOC: return "allocation failed";
        default: return "unknown status";
    }
}

int uavx_create(const uavx_config *cfg, int64_t num_envs, int64_t env_offset, int device, uavx_handle **out) {
    if (!cfg || !out || num_envs <= 0 || env_offset < 0) return UAVX_ERR_INVALID_ARG;
    if (cfg->num_agents < 1 || cfg->num_agents > UAVX_MAX_AGENTS) return UAVX_ERR_INVALID_ARG;
    if (cfg->num_bodies < 0 || cfg->num_agents + cfg->num_bodies > UAVX_MAX_AGENTS) return UAVX_ERR_INVALID_ARG;
    if (!config_valid(cfg)) return UAVX_ERR_INVALID_ARG;
    if (num_envs * (int64_t)cfg->num_agents >= (int64_t(1) << 26)) return UAVX_ERR_UNSUPPORTED;  // 32-bit byte offsets (obs: 40 B/agent)
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return UAVX_ERR_NO_DEVICE;
    if (device < 0 || device >= ndev) return UAVX_ERR_INVALID_ARG;
    uavx_handle *h = new (std::nothrow) uavx_handle();
    if (!h) return UAVX_ERR_ALLOC;
    h->cfg = *cfg;
    h->device = device;
    h->slab = nullptr;
    MultiParams &p = h->p;
    std::memset(&p, 0, sizeof p);
    const int N = cfg->num_agents;
    derive_world_params(*cfg, p);
    h->wl = derive_wide_limits(*cfg);
    const int B = cfg->num_bodies;
    p.N = N;
    p.B = B; p.nslots = N + B; p.kb = (B + N - 1) / N;
    h->gw = B > 0 ? 1 : pick_group_waves(N);
    if (const char *gv = getenv("UAVX_GW")) {   // A/B switch: wavefronts per workgroup of the runtime-N kernels
        const int w = atoi(gv);
        if (w >= 1 && w <= 4 && B == 0 && !(N == 1 || N == 2 || N == 4 || N == 5 || N == 8)) h->gw = w;
    }
    p.epw = std::min(kWave * h->gw / N, kExtSlots / (N + B));  // an EXT wave keeps epw * (L + B) neighbour rows in LDS
    p.magic = 65536 / N + 1;
    p.E = num_envs;
    p.env_offset = env_offset;
    h->ext = B > 0;
    // layouts drawn ahead: a staging workgroup draws up to min(floor(64 W / S), 8) layouts every other launch (it scans in
    // between), and there are enough of them for E / 128 layouts per launch -- what a batch whose episodes last 128 steps on
    // average consumes (a random-initialised actor: 170-190 steps at 4 UAVs, tools/closed_loop.py; shorter episodes draw the
    // excess in place): one per 32 env-workgroups at 4 UAVs, per 64 at 8, per 16 with 8 learners + 16 bodies.  At ~70 episode
    // ends per launch (bench.py --fused) the launch time is flat from 16 to 256 (4 UAVs) / 8 to 64 (8 + 16); with ~350 per launch
    // 64 at 4 UAVs already falls behind (env launch of the closed loop 8.0 -> 9.4 us).
    {
        const int lps = std::min(kHintJobs, std::max(1, kWave * h->gw / (N + B)));
        h->prefetch_every = std::max(1, 64 * lps / std::max(1, p.epw));
    }
    apply_body_rule(h);
    h->levels.l[0] = make_level(*cfg, nullptr, N, B);

    DeviceGuard guard(device);
    hipError_t e = guard.err;
    if (e != hipSuccess) { delete h; return UAVX_ERR_HIP; }
    const size_t A = (size_t)num_envs * N, E = (size_t)num_envs;
    size_t off = 0;
    const size_t o_pos = off;  off = align_up(off + A * sizeof(float2), 256);
    const size_t o_ovr = off;  off = align_up(off + A * sizeof(float), 256);
    const size_t o_vel = off;  off = align_up(off + A * sizeof(double2), 256);
    const size_t o_goal = off; off = align_up(off + A * sizeof(Goal), 256);
    const size_t o_steps = off; off = align_up(off + E * sizeof(uint4), 256);
    const size_t o_wsteps = off; off = align_up(off + ((E + p.epw - 1) / p.epw) * 4, 256);
    const size_t o_reach = off; off = align_up(off + E * 4, 256);
    const size_t o_coll = off;  off = align_up(off + E * 4, 256);
    const size_t o_nonfin = off; off = align_up(off + E * 4, 256);
    const size_t o_finc = off;  off = align_up(off + E * sizeof(uint4), 256);
    const size_t o_finr = off;  off = align_up(off + E * sizeof(float2), 256);
    const size_t o_bpos = off;  off = align_up(off + E * (size_t)B * sizeof(float2), 256);
    const size_t o_bleg = off;  off = align_up(off + E * (size_t)B * sizeof(float4), 256);
    const size_t o_lcur = off;  off = align_up(off + E, 256);
    const size_t o_lnext = off; off = align_up(off + E, 256);
    const size_t o_levels = off; off = align_up(off + sizeof(LevelTable), 256);
    const size_t o_sagent = off; off = align_up(off + 2 * A * sizeof(float4), 256);
    const size_t o_sbpos = off;  off = align_up(off + 2 * E * (size_t)B * sizeof(float2), 256);
    const size_t o_sbleg = off;  off = align_up(off + 2 * E * (size_t)B * sizeof(float4), 256);
    const size_t o_stag = off;   off = align_up(off + 2 * E * sizeof(uint4), 256);
    const size_t o_hint = off;   off = align_up(off + ((E + p.epw - 1) / p.epw + 1) * kHintJobs * sizeof(uint2), 256);   // (staging workgroups <= env-workgroups)
    // step_ex_kernel addresses the state arrays as slab base + 32-bit offsets (leading scalar kernel arguments)
    static_assert(sizeof(size_t) >= 8, "64-bit host");
    if (o_pos != 0 || o_wsteps >= (size_t(1) << 32)) { delete h; return UAVX_ERR_UNSUPPORTED; }
    h->off_vel = (uint32_t)o_vel; h->off_goal = (uint32_t)o_goal; h->off_rec = (uint32_t)o_steps; h->off_wsteps = (uint32_t)o_wsteps;
    if (p.epw > 255 || p.nslots > 255) { delete h; return UAVX_ERR_UNSUPPORTED; }   // (packed into one leading argument; <= 64 today)
    e = hipMalloc(&h->slab, off);
    if (e != hipSuccess) { delete h; return UAVX_ERR_ALLOC; }
    h->slab_bytes = off;
    e = hipMemset(h->slab, 0, off);
    if (e != hipSuccess) { (void)hipFree(h->slab); delete h; return UAVX_ERR_HIP; }
    char *b = static_cast<char *>(h->slab);
    p.pos = reinterpret_cast<float2 *>(b + o_pos);
    p.prev_ovr = reinterpret_cast<float *>(b + o_ovr);
    p.vel = reinterpret_cast<double2 *>(b + o_vel);
    p.goal = reinterpret_cast<Goal *>(b + o_goal);
    p.env_rec = reinterpret_cast<uint4 *>(b + o_steps);
    p.wave_steps = reinterpret_cast<uint32_t *>(b + o_wsteps);
    p.reach = reinterpret_cast<uint32_t *>(b + o_reach);
    p.coll = reinterpret_cast<uint32_t *>(b + o_coll);
    p.nonfin = reinterpret_cast<uint32_t *>(b + o_nonfin);
    p.fin_counts = reinterpret_cast<uint4 *>(b + o_finc);
    p.fin_returns = reinterpret_cast<float2 *>(b + o_finr);
    p.body_pos = reinterpret_cast<float2 *>(b + o_bpos);
    p.body_leg = reinterpret_cast<float4 *>(b + o_bleg);
    p.lvl_cur = reinterpret_cast<uint8_t *>(b + o_lcur);
    p.lvl_next = reinterpret_cast<uint8_t *>(b + o_lnext);
    h->levels_dev = reinterpret_cast<LevelParams *>(b + o_levels);
    p.levels = h->levels_dev;
    p.n_levels = 0; p.level_lo = -1; p.level_hi = -1;
    p.stage_agent = reinterpret_cast<float4 *>(b + o_sagent);
    p.stage_bpos = reinterpret_cast<float2 *>(b + o_sbpos);
    p.stage_bleg = reinterpret_cast<float4 *>(b + o_sbleg);
    p.stage_tag = reinterpret_cast<uint4 *>(b + o_stag);   // zero-filled: no layout is valid yet
    h->hints = reinterpret_cast<uint2 *>(b + o_hint);      // zero-filled: no hints
    if (const char *sb = getenv("UAVX_STAGE_BEHIND")) h->stage_behind = atoi(sb);
    {
        int cus = 0, tpc = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess &&
            hipDeviceGetAttribute(&tpc, hipDeviceAttributeMaxThreadsPerMultiProcessor, device) == hipSuccess && cus > 0 && tpc >= kWave)
            h->wave_slots = cus * (tpc / kWave);
    }
    {
        // Pairs of one-wavefront tiles per workgroup (the 8-UAV specialisation only): measured in one session (r03_ab_notes.md,
        // r04_ab_notes.md section 11), they pay where the launch fills the wavefront slots ONCE -- 65 536 x 8: 8 192 workgroups
        // take the dispatcher 2.3 us to place, half as many 1.2 -- and cost a few percent where it runs in two rounds or leaves
        // half the slots free (the pairs then land unevenly on the SIMDs of an issue-bound launch).
        const long waves = (long)wave_grid(h).x;
        h->tiles = (N == 8 && !h->ext && h->gw == 1 && waves % 2 == 0 && 2 * waves > (long)h->wave_slots && waves <= (long)h->wave_slots) ? 2 : 1;
        if (const char *tv = getenv("UAVX_TILES")) {   // A/B switch
            const int t = atoi(tv);
            if (t == 1 || (t == 2 && N == 8 && !h->ext && h->gw == 1 && waves % 2 == 0)) h->tiles = t;
        }
    }
    p.magic_s = 65536 / (N + B) + 1;
    p.world_version = 1;
    hipLaunchKernelGGL(upload_levels_kernel, dim3(1), dim3(64), 0, 0, h->levels_dev, h->levels);  // level 0 = the config
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(0);
    if (e != hipSuccess) { (void)hipFree(h->slab); delete h; return UAVX_ERR_HIP; }
    *out = h;
    return UAVX_OK;
}

int uavx_destroy(uavx_handle *h) {
    if (!h) return UAVX_ERR_INVALID_ARG;
    if (h->slab) {
        DeviceGuard guard(h->device);
        (void)hipFree(h->slab);
        if (h->wide_slab) (void)hipFree(h->wide_slab);
    }
    delete h;
    return UAVX_OK;
}

int uavx_set_config(uavx_handle *h, const uavx_config *cfg) {
    if (!h || !cfg) return UAVX_ERR_INVALID_ARG;
    if (cfg->num_agents != h->p.N) return fail(h, UAVX_ERR_INVALID_ARG, "uavx_set_config: num_agents is fixed at creation");
    if (!config_valid(cfg)) return fail(h, UAVX_ERR_INVALID_ARG, "uavx_set_config: parameter out of range");
    if (cfg->num_bodies != h->p.B) return fail(h, UAVX_ERR_INVALID_ARG, "uavx_set_config: num_bodies is fixed at creation");
    if (h->ext && h->p.n_levels > 0)
        return fail(h, UAVX_ERR_UNSUPPORTED, "uavx_set_config: a curriculum is installed; change the world through uavx_set_curriculum");
    h->cfg = *cfg;
    derive_world_params(*cfg, h->p);  // kernel arguments are taken by value at launch: later launches see the new world
    h->wl = derive_wide_limits(*cfg);
    apply_body_rule(h);
    h->p.world_version++;             // pre-drawn layouts of the old world are stale
    return UAVX_OK;   // host-only: without a curriculum the EXT kernels take the world from their arguments too
}

int uavx_num_bodies(const uavx_handle *h) { return h ? h->p.B : -1; }

int uavx_set_prefetch(uavx_handle *h, int every) {
    if (!h || every < 0) return UAVX_ERR_INVALID_ARG;
    h->prefetch_every = every;
    return UAVX_OK;
}

int uavx_set_body_rule(uavx_handle *h, const uavx_body_rule *rule) {
    if (!h || !rule) return UAVX_ERR_INVALID_ARG;
    if (!(rule->speed >= 0) || rule->period < 1 || (rule->period & (rule->period - 1)) != 0)
        return fail(h, UAVX_ERR_INVALID_ARG, "uavx_set_body_rule: speed must be >= 0 and period a power of two");
    h->rule = *rule;
    apply_body_rule(h);
    h->p.world_version++;
    return UAVX_OK;
}

int uavx_set_curriculum(uavx_handle *h, const uavx_level *levels, int32_t n_levels, int32_t level_lo, int32_t level_hi,
                        void *stream) {
    if (!h) return UAVX_ERR_INVALID_ARG;
    if (n_levels < 0 || n_levels > UAVX_MAX_LEVELS || (n_levels > 0 && !levels))
        return fail(h, UAVX_ERR_INVALID_ARG, "uavx_set_curriculum: 0 <= n_levels <= UAVX_MAX_LEVELS");
    if (h->wide) return fail(h, UAVX_ERR_UNSUPPORTED, "uavx_set_curriculum: not available for float64-position episodes");
    if (n_levels > 0 && level_lo >= 0 && (level_hi < level_lo || level_hi >= n_levels))
        return fail(h, UAVX_ERR_INVALID_ARG, "uavx_set_curriculum: need 0 <= level_lo <= level_hi < n_levels (or level_lo < 0)");
    for (int i = 0; i < n_levels; i++) {
        const uavx_level &l = levels[i];
        if (!(l.x_size > 0 && l.y_size > 0 && l.d_sense > 0 && l.collider_radius >= 0) || l.n_active < 1 ||
            l.n_active > h->p.N || l.b_active < 0 || l.b_active > h->p.B)
            return fail(h, UAVX_ERR_INVALID_ARG, "uavx_set_curriculum: level parameter out of range");
    }
    UAVX_ENTER(h);
    if (n_levels == 0) {
        h->levels.l[0] = make_level(h->cfg, nullptr, h->p.N, h->p.B);
    } else {
        for (int i = 0; i < n_levels; i++) h->levels.l[i] = make_level(h->cfg, &levels[i], h->p.N, h->p.B);
    }
    const int rc = launch(h, upload_levels_kernel, dim3(1), dim3(64), static_cast<hipStream_t>(stream), h->levels_dev, h->levels);
    if (rc != UAVX_OK) return rc;
    h->p.world_version++;
    h->p.n_levels = n_levels;
    h->p.level_lo = n_levels > 0 ? level_lo : -1;
    h->p.level_hi = n_levels > 0 ? level_hi : -1;
    h->ext = h->p.B > 0 || n_levels > 0;
    return UAVX_OK;
}

int uavx_set_env_levels(uavx_handle *h, const uint8_t *levels, void *stream) {
    if (!h || !levels) return UAVX_ERR_INVALID_ARG;
    UAVX_ENTER(h);
    return launch_items(h, env_levels_kernel, h->p.E, static_cast<hipStream_t>(stream), h->p, levels, (uint8_t *)nullptr);
}

int uavx_get_env_levels(uavx_handle *h, uint8_t *levels, void *stream) {
    if (!h || !levels) return UAVX_ERR_INVALID_ARG;
    UAVX_ENTER(h);
    return launch_items(h, env_levels_kernel, h->p.E, static_cast<hipStream_t>(stream), h->p, (const uint8_t *)nullptr, levels);
}

static int bodies_exchange(uavx_handle *h, const float *set, float *get, void *stream) {
    if (h->p.B == 0) return fail(h, UAVX_ERR_UNSUPPORTED, "the handle has no scripted bodies");
    if ((reinterpret_cast<uintptr_t>(set) | reinterpret_cast<uintptr_t>(get)) & 3u)
        return fail(h, UAVX_ERR_INVALID_ARG, "body records must be 4-byte aligned");
    UAVX_ENTER(h);
    return launch_items(h, bodies_kernel, h->p.E * h->p.B, static_cast<hipStream_t>(stream), h->p, set, get);
}
int uavx_get_bodies(uavx_handle *h, float *records, void *stream) {
    if (!h || !records) return UAVX_ERR_INVALID_ARG;
    return bodies_exchange(h, nullptr, records, stream);
}
int uavx_set_bodies(uavx_handle *h, const float *records, void *stream) {
    if (!h || !records) return UAVX_ERR_INVALID_ARG;
    return bodies_exchange(h, records, nullptr, stream);
}

const char *uavx_last_error(const uavx_handle *h) { return h ? h->err.c_str() : "null handle"; }
int64_t uavx_num_envs(const uavx_handle *h) { return h ? h->p.E : -1; }
int uavx_num_agents(const uavx_handle *h) { return h ? h->p.N : -1; }
static int launch_observe(uavx_handle *h, float *obs, hipStream_t st) {
    if (h->wide) return launch_items(h, observe64_kernel, h->p.E, st, h->p, h->w, h->wl, obs);
    return dispatch(h, ObserveLaunch{h, wave_grid(h), st, obs});
}

int uavx_observe(uavx_handle *h, float *obs, void *stream) {
    if (!h) return UAVX_ERR_INVALID_ARG;
    if (!obs || (reinterpret_cast<uintptr_t>(obs) & 15u))
        return fail(h, UAVX_ERR_INVALID_ARG, "uavx_observe: obs is NULL or not 16-byte aligned");
    UAVX_ENTER(h);
    return launch_observe(h, obs, static_cast<hipStream_t>(stream));
}

int uavx_reset(uavx_handle *h, const uint8_t *mask, uint64_t seed, float *obs, void *stream) {
    if (!h) return UAVX_ERR_INVALID_ARG;
    UAVX_ENTER(h);
    if (obs && (reinterpret_cast<uintptr_t>(obs) & 15u))
        return fail(h, UAVX_ERR_INVALID_ARG, "uavx_reset: obs not 16-byte aligned");
    if (h->wide && mask)
        return fail(h, UAVX_ERR_UNSUPPORTED, "uavx_reset: a masked reset would mix float32 and float64 episodes in one handle");
    h->wide = false;  // MUW:126,131,144: reset() installs float32 arrays again
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = dispatch(h, ResetLaunch{h, wave_grid(h), st, mask, seed});
    if (rc != UAVX_OK || !obs) return rc;
    return launch_observe(h, obs, st);
}

static int launch_step64(uavx_handle *h, const void *actions, int action_dtype, int action_mode, int track_returns, int evaluate,
                  float *obs, float *rew, uint8_t *done, hipStream_t st) {
    const bool f64 = action_dtype == UAVX_F64;
    const auto kernel = action_mode == UAVX_ACTION_POLAR_REFERENCE ? (f64 ? &step64_ref_kernel<true> : &step64_ref_kernel<false>)
                                                                   : (f64 ? &step64_kernel<true> : &step64_kernel<false>);
    return launch_items(h, kernel, h->p.E, st, h->p, h->w, h->wl, actions, action_mode, track_returns, evaluate, obs, rew, done);
}

int uavx_step_k(uavx_handle *h, int k, const void *actions, int action_dtype, int evaluate, int tape_out, float *obs,
                float *rew, uint8_t *done, void *stream) {
    if (!h) return UAVX_ERR_INVALID_ARG;
    if (!actions || !obs || !rew || !done) return fail(h, UAVX_ERR_INVALID_ARG, "uavx_step: NULL buffer");
    if (k < 1) return fail(h, UAVX_ERR_INVALID_ARG, "uavx_step_k: k < 1");
    if (action_dtype != UAVX_F32 && action_dtype != UAVX_F64)
        return fail(h, UAVX_ERR_INVALID_ARG, "uavx_step: action_dtype must be UAVX_F32 or UAVX_F64");
    if ((reinterpret_cast<uintptr_t>(obs) & 15u) || (reinterpret_cast<uintptr_t>(actions) & (action_dtype == UAVX_F64 ? 15u : 7u)) ||
        (reinterpret_cast<uintptr_t>(rew) & 3u))
        return fail(h, UAVX_ERR_INVALID_ARG, "uavx_step: obs must be 16-byte aligned, actions 8 (float32) / 16 (float64), rew 4");
    UAVX_ENTER(h);
    if (h->wide) {
        if (k != 1) return fail(h, UAVX_ERR_UNSUPPORTED, "uavx_step_k: k > 1 is not available for float64-position episodes");
        return launch_step64(h, actions, action_dtype, UAVX_ACTION_CARTESIAN, 0, evaluate, obs, rew, done,
                             static_cast<hipStream_t>(stream));
    }
    if (h->ext && k != 1)
        return fail(h, UAVX_ERR_UNSUPPORTED, "uavx_step_k: k > 1 is not available with scripted bodies / a curriculum");
    return dispatch(h, StepLaunch{h, wave_grid(h), static_cast<hipStream_t>(stream), actions, action_dtype, evaluate, k, tape_out, obs, rew, done});
}

int uavx_step(uavx_handle *h, const void *actions, int action_dtype, int evaluate, float *obs, float *rew,
              uint8_t *done, void *stream) {
    return uavx_step_k(h, 1, actions, action_dtype, evaluate, 0, obs, rew, done, stream);
}

int uavx_step_ex(uavx_handle *h, const uavx_step_args *a, void *stream) {
    if (!h || !a) return UAVX_ERR_INVALID_ARG;
    if (!a->actions || !a->obs || !a->rew || !a->done) return fail(h, UAVX_ERR_INVALID_ARG, "uavx_step_ex: NULL buffer");
    if (a->action_dtype != UAVX_F32 && a->action_dtype != UAVX_F64)
        return fail(h, UAVX_ERR_INVALID_ARG, "uavx_step_ex: action_dtype must be UAVX_F32 or UAVX_F64");
    if (a->action_mode != UAVX_ACTION_CARTESIAN && a->action_mode != UAVX_ACTION_POLAR &&
        a->action_mode != UAVX_ACTION_POLAR_REFERENCE)
        return fail(h, UAVX_ERR_INVALID_ARG, "uavx_step_ex: unknown action_mode");
    if (a->reset_policy < UAVX_RESET_NEVER || a->reset_policy > UAVX_RESET_ALL_DONE)
        return fail(h, UAVX_ERR_INVALID_ARG, "uavx_step_ex: unknown reset_policy");
    if (a->flags_mode != UAVX_FLAGS_ARRAYS && a->flags_mode != UAVX_FLAGS_IN_DONE)
        return fail(h, UAVX_ERR_INVALID_ARG, "uavx_step_ex: unknown flags_mode");
    if ((reinterpret_cast<uintptr_t>(a->obs) & 15u) || (reinterpret_cast<uintptr_t>(a->actions) & (a->action_dtype == UAVX_F64 ? 15u : 7u)) ||
        (reinterpret_cast<uintptr_t>(a->rew) & 3u))
        return fail(h, UAVX_ERR_INVALID_ARG, "uavx_step_ex: obs must be 16-byte aligned, actions 8 (float32) / 16 (float64), rew 4");
    UAVX_ENTER(h);
    if (h->wide) {
        if (a->reset_policy != UAVX_RESET_NEVER || a->step_cap != 0)
            return fail(h, UAVX_ERR_UNSUPPORTED, "uavx_step_ex: no auto-reset / step cap for float64-position episodes");
        if (a->reset_mask) UAVX_HIP(h, hipMemsetAsync(a->reset_mask, 0, (size_t)h->p.E, static_cast<hipStream_t>(stream)));
        if (a->ended) UAVX_HIP(h, hipMemsetAsync(a->ended, 0, (size_t)h->p.E, static_cast<hipStream_t>(stream)));
        if (a->truncated) UAVX_HIP(h, hipMemsetAsync(a->truncated, 0, (size_t)h->p.E, static_cast<hipStream_t>(stream)));
        return launch_step64(h, a->actions, a->action_dtype, a->action_mode, a->track_returns, a->evaluate, a->obs, a->rew,
                             a->done, static_cast<hipStream_t>(stream));
    }
    StepExtra x;
    x.action_mode = a->action_mode; x.reset_policy = a->reset_policy; x.track_returns = a->track_returns;
    x.step_cap = a->step_cap; x.seed_lo = (uint32_t)a->seed; x.seed_hi = (uint32_t)(a->seed >> 32);
    x.reset_mask = a->reset_mask;
    x.ended = a->ended; x.truncated = a->truncated;
    x.flags_in_done = (a->flags_mode == UAVX_FLAGS_IN_DONE) ? 1 : 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid = wave_grid(h);
    // auto-resetting call: the launch carries staging workgroups that draw the layouts of the next episodes (stage_ahead)
    const bool resets = a->reset_policy != UAVX_RESET_NEVER || a->step_cap != 0;
    x.use_stage = (h->prefetch_every > 0 && resets) ? 1 : 0;
    x.pf_blocks = 0; x.pf_groups = grid.x;
    x.stage_first = 0; x.step_first = 0;
    x.hints = h->hints;
    // env-workgroups of the launch: pairs of tiles divide evenly (uavx_create); a handle that has since been given a curriculum
    // runs the kernels with levels, which keep one tile per workgroup
    const unsigned step_blocks = grid.x / (unsigned)launch_tiles(h);
    dim3 blocks(step_blocks);
    if (x.use_stage) {
        x.pf_blocks = (grid.x + (unsigned)h->prefetch_every - 1u) / (unsigned)h->prefetch_every;
        blocks.x = step_blocks + x.pf_blocks;
        // Where in the launch?  Workgroups are dispatched in block order.  While the env-workgroups leave wavefront slots free
        // (65 536 x 4: 4 096 of 8 192) the staging workgroups go IN FRONT and run beside them.  When the env-workgroups alone fill
        // every slot (65 536 x 8, with or without bodies: exactly 8 192 one-wavefront workgroups), whatever comes on top waits
        // for a slot: in front, 512 step wavefronts start 4-12 us late -- the ones behind a drawing workgroup last, and the
        // launch ends with them (per-wavefront timelines, tools/exp_stamps.py: 19.5 us from first start to last end against
        // 17.1 without staging).  BEHIND the env-workgroups the staging workgroups start when the first step wavefronts retire
        // (11 us) and work in the shadow of the ones still running (their ends spread over 10-18 us): nothing that steps is
        // displaced.  Measured in one session, in front / behind: 8 learners + 16 bodies with levels 22.0 / 21.5 us, without
        // levels 22.3 / 21.8, 8 UAVs 13.8 / 13.5; 4 UAVs 7.03 / 7.02, half-full and multi-round launches within 1 %.  Workgroups
        // of several wavefronts (24 UAVs: 42 / 53 us) stay in front: their chain runs on __syncthreads and is long.
        const bool behind = h->stage_behind < 0 ? (h->gw == 1 && (long)grid.x + (long)x.pf_blocks > (long)h->wave_slots) : h->stage_behind != 0;
        if (behind) x.stage_first = step_blocks; else x.step_first = x.pf_blocks;
    }
    return dispatch(h, StepExLaunch{h, blocks, st, x, a});
}

#ifdef UAVX_STAMPS
extern "C" int uavx_debug_stamps(unsigned long long *host_out, unsigned int *n) {  // debug builds only
    hipDeviceSynchronize();
    hipMemcpyFromSymbol(n, HIP_SYMBOL(g_stamp_n), sizeof(unsigned int));
    hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * 8 * 16384);
    unsigned int zero = 0;
    hipMemcpyToSymbol(HIP_SYMBOL(g_stamp_n), &zero, sizeof zero);
    void *dst = nullptr;
    hipGetSymbolAddress(&dst, HIP_SYMBOL(g_stamps));
    hipMemset(dst, 0, sizeof(unsigned long long) * 8 * 16384);
    return 0;
}
#endif

int uavx_get_nonfinite(uavx_handle *h, uint32_t *counts, void *stream) {
    if (!h || !counts) return UAVX_ERR_INVALID_ARG;
    UAVX_ENTER(h);
    UAVX_HIP(h, hipMemcpyAsync(counts, h->p.nonfin, (size_t)h->p.E * 4, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
    return UAVX_OK;
}

int uavx_get_episode_stats(uavx_handle *h, uint32_t *counts, float *returns, void *stream) {
    if (!h) return UAVX_ERR_INVALID_ARG;
    UAVX_ENTER(h);
    return launch_items(h, episode_stats_kernel, h->p.E, static_cast<hipStream_t>(stream), h->p, counts, returns, 0);
}

int uavx_clear_episode_stats(uavx_handle *h, void *stream) {
    if (!h) return UAVX_ERR_INVALID_ARG;
    UAVX_ENTER(h);
    return launch_items(h, episode_stats_kernel, h->p.E, static_cast<hipStream_t>(stream), h->p, (uint32_t *)nullptr, (float *)nullptr, 1);
}

static int wide_exchange(uavx_handle *h, const uavx_state_view &v, const uavx_state_view_f64 &v64, int set, hipStream_t st) {
    const int rc = launch_items(h, wide_exchange_kernel, agent_slots(h), st, h->p, h->w, v, v64, set);
    if (rc != UAVX_OK || !v.counters) return rc;
    {  // env counters live in the shared arrays: the float32-mode kernels handle them
        uavx_state_view c;
        std::memset(&c, 0, sizeof c);
        c.counters = v.counters;
        return launch_items(h, set ? set_state_kernel : get_state_kernel, agent_slots(h), st, h->p, c);
    }
}

int uavx_get_state(uavx_handle *h, const uavx_state_view *dst, void *stream) {
    if (!h || !dst) return UAVX_ERR_INVALID_ARG;
    UAVX_ENTER(h);
    if (h->wide) return wide_exchange(h, *dst, uavx_state_view_f64{}, 0, static_cast<hipStream_t>(stream));
    return launch_items(h, get_state_kernel, agent_slots(h), static_cast<hipStream_t>(stream), h->p, *dst);
}

int uavx_set_state(uavx_handle *h, const uavx_state_view *src, void *stream) {
    if (!h || !src) return UAVX_ERR_INVALID_ARG;
    UAVX_ENTER(h);
    if (h->wide) return wide_exchange(h, *src, uavx_state_view_f64{}, 1, static_cast<hipStream_t>(stream));
    return launch_items(h, set_state_kernel, agent_slots(h), static_cast<hipStream_t>(stream), h->p, *src);
}

int uavx_get_position_mode(const uavx_handle *h) { return h ? (h->wide ? UAVX_POS_F64 : UAVX_POS_F32) : UAVX_ERR_INVALID_ARG; }

int uavx_set_position_mode(uavx_handle *h, int mode, void *stream) {
    if (!h) return UAVX_ERR_INVALID_ARG;
    if (mode != UAVX_POS_F32 && mode != UAVX_POS_F64) return fail(h, UAVX_ERR_INVALID_ARG, "uavx_set_position_mode: unknown mode");
    UAVX_ENTER(h);
    if ((mode == UAVX_POS_F64) == h->wide) return UAVX_OK;
    if (mode == UAVX_POS_F64 && h->ext)
        return fail(h, UAVX_ERR_UNSUPPORTED, "uavx_set_position_mode: float64-position episodes are not available with scripted bodies / a curriculum");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (mode == UAVX_POS_F64) {
        if (!h->wide_slab) {  // 48 B per agent, once per handle
            const size_t A = (size_t)h->p.E * h->p.N;
            const size_t o_tgt = align_up(A * sizeof(double2), 256), o_init = o_tgt + align_up(A * sizeof(double2), 256);
            const size_t o_prev = o_init + align_up(A * sizeof(double), 256), total = o_prev + align_up(A * sizeof(double), 256);
            if (hipMalloc(&h->wide_slab, total) != hipSuccess) {
                h->wide_slab = nullptr;
                return fail(h, UAVX_ERR_ALLOC, "uavx_set_position_mode: hipMalloc of the float64 arrays failed");
            }
            char *b = static_cast<char *>(h->wide_slab);
            h->w.pos = reinterpret_cast<double2 *>(b);
            h->w.tgt = reinterpret_cast<double2 *>(b + o_tgt);
            h->w.init_d = reinterpret_cast<double *>(b + o_init);
            h->w.prev_d = reinterpret_cast<double *>(b + o_prev);
        }
    }
    const int rc = launch_items(h, mode == UAVX_POS_F64 ? widen_state_kernel : narrow_state_kernel, agent_slots(h), st, h->p, h->w);
    if (rc == UAVX_OK) h->wide = (mode == UAVX_POS_F64);
    return rc;
}

int uavx_set_state_f64(uavx_handle *h, const uavx_state_view_f64 *src, void *stream) {
    if (!h || !src) return UAVX_ERR_INVALID_ARG;
    const int rc = uavx_set_position_mode(h, UAVX_POS_F64, stream);  // assigning float64 arrays makes the episode float64
    if (rc != UAVX_OK) return rc;
    UAVX_ENTER(h);
    uavx_state_view none;
    std::memset(&none, 0, sizeof none);
    return wide_exchange(h, none, *src, 1, static_cast<hipStream_t>(stream));
}

int uavx_get_state_f64(uavx_handle *h, const uavx_state_view_f64 *dst, void *stream) {
    if (!h || !dst) return UAVX_ERR_INVALID_ARG;
    if (!h->wide) return fail(h, UAVX_ERR_UNSUPPORTED, "uavx_get_state_f64: the handle is in float32-position mode");
    UAVX_ENTER(h);
    uavx_state_view none;
    std::memset(&none, 0, sizeof none);
    return wide_exchange(h, none, *dst, 0, static_cast<hipStream_t>(stream));
}
int uavx_get_metrics(uavx_handle *h, uint32_t *counters, void *stream) {
    if (!h || !counters) return UAVX_ERR_INVALID_ARG;
    uavx_state_view v;
    std::memset(&v, 0, sizeof v);
    v.counters = counters;
    return uavx_get_state(h, &v, stream);
}

}  // extern "C"

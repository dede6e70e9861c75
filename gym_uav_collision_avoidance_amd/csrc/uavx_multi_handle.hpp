// uavx_multi_handle.hpp -- the handle of the C ABI and everything of it that follows from the world parameters (exact comparison
// limits, kernel-form curriculum levels, body rule).  Included by uavx_multi.hip at file scope (the handle and the three functions
// shared with uavx_uw.hip) and in an anonymous namespace (the rest), behind `using namespace uavx` and uavx_host_util.hpp.

struct uavx_handle {
    uavx_config cfg;
    MultiParams p;
    int device;
    void *slab;  // one allocation holding every state array
    size_t slab_bytes = 0;
    uint32_t off_vel = 0, off_goal = 0, off_rec = 0, off_wsteps = 0;   // byte offsets of vel / goal / env_rec / wave_steps in it (pos: 0)
    // float64-position mode (uavx_set_position_mode): arrays allocated on first use
    bool wide = false;
    WideState w = {};
    WideLimits wl = {};
    void *wide_slab = nullptr;
    // configs[4] extension: scripted bodies and / or an installed curriculum select the EXT kernel variants
    int gw = 1;  // wavefronts per workgroup of the step / reset / observe launches (pick_group_waves)
    int tiles = 1;  // one-wavefront tiles per workgroup of the step launches (tiles_for)
    // layouts drawn ahead (stage_ahead): every auto-resetting uavx_step_ex launch carries ceil(G / prefetch_every) staging
    // workgroups beside its G env-workgroups
    int prefetch_every = 16;   // 0: off
    uint2 *hints = nullptr;    // [env-workgroups + 1][kHintJobs] what each staging workgroup's last scan found (in the slab)
    int wave_slots = 8192;     // wavefronts the device holds at once (compute units x 32)
    int stage_behind = -1;     // staging workgroups behind (1) / in front of (0) the env-workgroups; -1: by launch shape.  A/B
                               // knob, read once from UAVX_STAGE_BEHIND when the handle is made; results do not depend on it
    bool ext = false;
    uavx_body_rule rule = {5.0, 128, 0, 0};
    LevelTable levels = {};
    LevelParams *levels_dev = nullptr;
    std::string err;
};

// div_tau() on the device replaces x/tau by a reciprocal + two fma; confirm on this tau that the
// form returns the IEEE quotient (differences a - v of the magnitudes the kinematics produce, plus
// the band |x| < amax*tau where the quotient is not clipped away).
bool uavx_recip_division_exact(double tau) {
    const double r = 1.0 / tau;
    uint64_t s0 = 0x9E3779B97F4A7C15ull, s1 = 0xD1B54A32D192ED03ull;
    for (int i = 0; i < 100000; i++) {
        uint64_t a = s0, b = s1;
        s0 = b; a ^= a << 23; s1 = a ^ b ^ (a >> 17) ^ (b >> 26);
        const uint64_t u = s1 + b;
        double x = ((double)(u >> 11) / 9007199254740992.0) * 2.0 - 1.0;  // (-1, 1)
        x = std::ldexp(x, (i % 3 == 0) ? 5 : ((i % 3 == 1) ? -3 : -(int)(u % 60)));
        const double q0 = x * r;
        const double q = std::fma(std::fma(-q0, tau, x), r, q0);
        if (q != x / tau) return false;
    }
    return true;
}

// float32 forms of a float64 bound b, exact for every float32 x:  (double)x >= b <=> x >= uavx_f32_at_or_above(b),
// (double)x <= b <=> x <= uavx_f32_at_or_below(b)
float uavx_f32_at_or_above(double b) {   // shared with uavx_uw.hip
    float f = (float)b;
    if ((double)f < b) f = std::nextafterf(f, INFINITY);
    return f;
}
float uavx_f32_at_or_below(double b) {
    float f = (float)b;
    if ((double)f > b) f = std::nextafterf(f, -INFINITY);
    return f;
}

namespace {

// smallest double s with sqrt(s) >= lim, so that  sqrt(s) < lim  <=>  s < result  (sqrt is
// correctly rounded and monotone): lets the device test MUW:218's speed without a float64 sqrt.
double sq_threshold(double lim) {
    double s = lim * lim;
    while (std::sqrt(s) >= lim) s = std::nextafter(s, 0.0);
    while (std::sqrt(s) < lim) s = std::nextafter(s, INFINITY);
    return s;
}

// float32 limits for threshold tests on squared distances (host sqrtf is correctly rounded):
// smallest s with sqrtf(s) >= lim   ->   sqrtf(s) <  lim  <=>  s <  result
float sq_limit_lt(float lim) {
    float s = lim * lim;
    while (s > 0.f && std::sqrt(s) >= lim) s = std::nextafterf(s, 0.f);
    while (std::sqrt(s) < lim) s = std::nextafterf(s, INFINITY);
    return s;
}
// largest s with sqrtf(s) <= lim    ->   sqrtf(s) <= lim  <=>  s <= result
float sq_limit_le(float lim) {
    float s = lim * lim;
    while (std::sqrt(s) <= lim) s = std::nextafterf(s, INFINITY);
    while (s > 0.f && std::sqrt(s) > lim) s = std::nextafterf(s, 0.f);
    return s;
}

// Everything of MultiParams that follows from the world's scalar parameters (MUW:13-58), shared by uavx_create and
// uavx_set_config.
void derive_world_params(const uavx_config &c, MultiParams &p) {
    const uavx_config *cfg = &c;
    p.tau = cfg->tau; p.amax = cfg->max_acceleration; p.vmax = cfg->max_speed;
    p.rtau = 1.0 / cfg->tau;
    p.recip_ok = uavx_recip_division_exact(cfg->tau) ? 1 : 0;
    p.lox = -cfg->x_size / 2.0; p.loy = -cfg->y_size / 2.0;  // MUW:19
    p.hix = cfg->x_size / 2.0; p.hiy = cfg->y_size / 2.0;    // MUW:20
    p.lo_x = uavx_f32_at_or_above(p.lox); p.lo_y = uavx_f32_at_or_above(p.loy);
    p.hi_x = uavx_f32_at_or_below(p.hix); p.hi_y = uavx_f32_at_or_below(p.hiy);
    p.speed_sq_lim = sq_threshold(0.2);
    p.two_r_reset = (float)(2 * cfg->collider_radius);
    p.sq_sense = sq_limit_lt((float)cfg->d_sense);
    p.sq_two_r = sq_limit_le(p.two_r_reset);
    p.sq_hard = sq_limit_le(1.0f);  // 2 * HARD_COLLISION_RADIUS, MUW:8,207
    p.inv_sense = 1.0f / (float)cfg->d_sense;
    p.vmax_norm = (float)std::sqrt(std::fma(cfg->max_speed, cfg->max_speed, cfg->max_speed * cfg->max_speed));
    p.inv_vmax_norm = 1.0f / p.vmax_norm;
    p.inv_diag = (float)(1.0 / std::sqrt(std::fma(cfg->y_size, cfg->y_size, cfg->x_size * cfg->x_size)));
}

// One curriculum level in kernel form: the handle's config with the level's four world parameters swapped in.
LevelParams make_level(const uavx_config &base, const uavx_level *lv, int L, int B) {
    uavx_config c = base;
    int nl = L, nb = B;
    if (lv) {
        c.x_size = lv->x_size; c.y_size = lv->y_size; c.collider_radius = lv->collider_radius; c.d_sense = lv->d_sense;
        nl = lv->n_active; nb = lv->b_active;
    }
    MultiParams t;
    std::memset(&t, 0, sizeof t);
    derive_world_params(c, t);
    LevelParams o;
    std::memset(&o, 0, sizeof o);
    o.lo_x = t.lo_x; o.lo_y = t.lo_y; o.hi_x = t.hi_x; o.hi_y = t.hi_y;
    o.sq_sense = t.sq_sense; o.sq_two_r = t.sq_two_r; o.inv_sense = t.inv_sense; o.inv_diag = t.inv_diag;
    o.lox = t.lox; o.loy = t.loy; o.hix = t.hix; o.hiy = t.hiy;
    o.n_active = nl; o.b_active = nb;
    return o;
}

void apply_body_rule(uavx_handle *h) {
    MultiParams &p = h->p;
    p.body_step = (float)(h->rule.speed * h->cfg.tau);
    p.body_pmask = h->rule.period - 1;
    p.body_pshift = 0;
    while ((1 << p.body_pshift) < h->rule.period) p.body_pshift++;
    p.body_k0 = (uint32_t)h->rule.seed; p.body_k1 = (uint32_t)(h->rule.seed >> 32);
}

WideLimits derive_wide_limits(const uavx_config &c) {  // the python-float comparands of the float64 episodes
    WideLimits l;
    l.d_sense = c.d_sense;                       // AG:52
    l.two_r = 2 * c.collider_radius;             // MUW:203
    l.two_hard = 2 * 0.5;                        // MUW:8,207
    l.vmax_norm = std::sqrt(std::fma(c.max_speed, c.max_speed, c.max_speed * c.max_speed));  // MUW:62,183
    l.diag = std::sqrt(std::fma(c.y_size, c.y_size, c.x_size * c.x_size));                   // MUW:17
    return l;
}

bool config_valid(const uavx_config *cfg) {
    return cfg->tau > 0 && cfg->max_speed > 0 && cfg->max_acceleration > 0 && cfg->x_size > 0 && cfg->y_size > 0 &&
           cfg->d_sense > 0 && cfg->collider_radius >= 0;
}

}  // namespace

// uavx_step64.hpp -- the float64-position step kernel, included by uavx_multi_f64.hpp once per action-mode family, like
// uavx_step_ex.hpp (no include guard): step64_kernel (UAVX_EX_REF false) and step64_ref_kernel (UAVX_ACTION_POLAR_REFERENCE).
// MUW:177-241 for one env per thread.  action_mode / track_returns as in uavx_step_ex (no auto-reset in this mode).
template <bool ACT64>
__global__ __launch_bounds__(kBlock) void UAVX_EX_KERNEL(MultiParams p, WideState w, WideLimits L, const void *actions,
                                                        int action_mode, int track_returns, int evaluate, float *obs,
                                                        float *rew_out, uint8_t *done_out) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= p.E) return;
    const int n = p.N;
    const int64_t a0 = e * n;
    double2 *pos = w.pos + a0, *vel = p.vel + a0;
    const double2 *tgt = w.tgt + a0;
    uint32_t reach = 0, coll = 0;
    float run0 = 0.f, score = 0.f;
    for (int i = 0; i < n; i++) {                                                    // MUW:181
        double ax, ay;
        load_action<ACT64>(actions, (uint32_t)(a0 + i), ax, ay);
        if constexpr (UAVX_EX_REF) polar_to_command_ref<ACT64>(p.vmax_norm, ax, ay);
        else if (action_mode == UAVX_ACTION_POLAR) polar_to_command(p, (float)ax, (float)ay, ax, ay);
        uint32_t flags = p.goal[a0 + i].flags & kFlagPublic;
        const uint32_t flags_in = flags;
        const bool was_done = (flags & UAVX_FLAG_DONE) != 0;
        double2 v = vel[i], x = pos[i];
        const double2 t = tgt[i];
        const double init_d = w.init_d[a0 + i];
        double pd = 0.0, d = 0.0;                                                    // AG:24-25
        if (!was_done) {                                                             // AG:26-36
            const double dvx = clip64_np((ax - v.x) / p.tau, -p.amax, p.amax), dvy = clip64_np((ay - v.y) / p.tau, -p.amax, p.amax);
            v.x = clip64_np(v.x + dvx * p.tau, -p.vmax, p.vmax);
            v.y = clip64_np(v.y + dvy * p.tau, -p.vmax, p.vmax);
            x.x = x.x + v.x * p.tau;                                                 // AG:28-29, float64 array
            x.y = x.y + v.y * p.tau;
            pos[i] = x;
            pd = w.prev_d[a0 + i];                                                   // AG:32
            d = nrm64(t.x - x.x, t.y - x.y);                                         // AG:33
        }
        // reward shaping, MUW:183-195
        const double dth = wrap64(atan2(t.y - x.y, t.x - x.x) - atan2(v.y, v.x));    // MUW:184-186
        const double q = L.vmax_norm / init_d;
        double r = 0.0 - 0.01 * ((1.0 < q) ? 1.0 : q);                               // MUW:188-189
        r += 50.0 * ((pd - d) / L.vmax_norm);                                        // MUW:190
        const double frac = d / (1.5 * init_d);
        r *= (r > 0) ? (1 - frac) : (1 + frac);                                      // MUW:191-194
        r -= 0.01 * fabs(dth);                                                       // MUW:195
        // collisions with the <= 2 nearest in-range agents at the CURRENT array (j<i moved, j>i not), MUW:197-210
        bool collision = false;
        int idx[2]; double dist[2];
        const int nn = nearest_two64(pos, n, i, L.d_sense, idx, dist);
        for (int k = 0; k < nn; k++) {
            if (dist[k] <= L.two_r) { r = -2.0; collision = true; }                  // MUW:203-205
            if (dist[k] <= L.two_hard && !(flags & (UAVX_FLAG_DONE | UAVX_FLAG_COLLIDED))) {
                coll += 1; flags |= UAVX_FLAG_COLLIDED;                              // MUW:207-210
            }
        }
        // termination, MUW:213-227
        const bool oob = !(x.x >= p.lox && x.x <= p.hix && x.y >= p.loy && x.y <= p.hiy);
        uint32_t dn = 0;
        if (d < 0.5 && !collision && nrm64(v.x, v.y) < 0.2) {                        // MUW:218
            dn = 1;
            if (!(flags & UAVX_FLAG_DONE)) reach += 1;                               // MUW:220-221
            flags |= UAVX_FLAG_DONE;                                                 // AG:38-42
            const double nv = nrm64(v.x, v.y);
            double fx = v.x / nv * 0.001, fy = v.y / nv * 0.001;
            if (fx != fx || fy != fy) { fx = 0.0; fy = 0.0; }
            v = make_double2(fx, fy);
            r += 10;                                                                 // MUW:223
        } else if (oob) {
            dn = evaluate ? 0u : 1u;                                                 // MUW:224-225
        }
        vel[i] = v;
        w.prev_d[a0 + i] = d;                                                        // MUW:229
        if (flags != flags_in) p.goal[a0 + i].flags = flags;
        const float rf = (float)r;
        rew_out[a0 + i] = rf;
        done_out[a0 + i] = (uint8_t)dn;
        if (i == 0) run0 = rf;
        score += rf * (1.0f - (float)dn);                                            // test_sac_multi.py:157
    }
    for (int i = 0; i < n; i++) observe_agent64(p, L, pos, tgt, vel, n, i, obs + (a0 + i) * 10);  // MUW:233-235
    if (reach) p.reach[e] += reach;
    if (coll) p.coll[e] += coll;
    uint4 rec = p.env_rec[e];
    rec.x -= 1u;                                                                     // MUW:238: steps = wave_steps - rec.x
    if (track_returns) {
        rec.z = __float_as_uint(__uint_as_float(rec.z) + run0);                      // test_sac_multi.py:106
        rec.w = __float_as_uint(__uint_as_float(rec.w) + score);
    }
    p.env_rec[e] = rec;
}

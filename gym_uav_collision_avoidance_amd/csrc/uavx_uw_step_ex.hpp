// uavx_uw_step_ex.hpp -- the UAVWorld2D step_ex kernel, included by uavx_uw.hip once per action-mode family, like
// uavx_step_ex.hpp (no include guard): uw_step_ex_kernel (UAVX_EX_REF false) and uw_step_ex_ref_kernel
// (UAVX_ACTION_POLAR_REFERENCE: act_f32 stays !ACT64, the command has the action's dtype).
// uavx_uw_step_ex: step + polar conversion + next-step auto-reset + episode statistics.
template <bool ACT64>
__global__ __launch_bounds__(kBlock) void UAVX_EX_KERNEL(UwParams p, UwExtra x, const void *__restrict__ actions,
                                                            float4 *__restrict__ obs_out, float *__restrict__ rew_out,
                                                            uint8_t *__restrict__ done_out, float *__restrict__ info_out) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = e < p.E;
    const uint32_t wave_count = p.wave_steps[blockIdx.x];
    if (live) {
        const uint4 rec = p.rec[e];
        uint32_t steps = wave_count - rec.x;
        UwRegs s;
        if (rec.y & kUwPending) {  // the env starts a new episode instead of stepping
            const uint32_t episode = rec.y & ~kUwPending;
            uw_fold(p, e, steps, (p.goal[e].flags & kUwReached) != 0, __uint_as_float(rec.z));
            uw_draw_episode(p, e, episode, x.seed_lo, x.seed_hi, s);
            uw_store_fresh(p, e, s);
            p.rec[e] = make_uint4(wave_count + 1u, episode + 1u, 0u, 0u);   // UW:131 steps = 0 after this launch
            const float tdx = s.tx - s.x, tdy = s.ty - s.y;
            const float theta = atan2_fast((float)s.vy, (float)s.vx);
            obs_out[e] = uw_obs(p, norm32((float)s.vx, (float)s.vy), theta, s.init_d, wrap_pi(atan2_fast(tdy, tdx) - theta));
            rew_out[e] = 0.f;
            done_out[e] = 0;
            if (info_out) info_out[e] = s.init_d;
            if (x.reset_mask) x.reset_mask[e] = 1;
            if (x.ended) x.ended[e] = 0;
            if (x.truncated) x.truncated[e] = 0;
        } else {
            double ax, ay;
            uw_load_action<ACT64>(actions, e, ax, ay);
            uw_load(p, e, s);
            const uint32_t flags_in = s.flags;
            bool act_f32 = !ACT64;
            if constexpr (UAVX_EX_REF) {   // test_sac.py:77-80 with the trainer's dtypes: a float32 action gives a float32 command
                polar_to_command_ref<ACT64>(p.high0, ax, ay);
            } else if (x.action_mode == UAVX_ACTION_POLAR) {  // test_sac.py:77-80 in float32
                const float v = fmaf((float)ax, 0.5f, 0.5f) * p.high0;
                float sn, cs;
                sincospi32((float)ay, sn, cs);
                ax = (double)(v * cs); ay = (double)(v * sn);
                act_f32 = true;
            }
            float4 obs; float rew, dist; uint32_t dn;
            uw_step_env(p, s, ax, ay, act_f32, obs, rew, dn, dist);
            obs_out[e] = obs;
            rew_out[e] = rew;
            done_out[e] = (uint8_t)dn;
            if (info_out) info_out[e] = dist;
            uw_store(p, e, s, flags_in);
            steps += 1;                                                      // UW:170
            const bool terminal = x.auto_reset && dn;                                 // test_sac.py:106-109
            const bool ended = terminal || (x.step_cap != 0 && steps >= x.step_cap);   // :17
            if (x.ended) x.ended[e] = ended ? 1 : 0;
            if (x.truncated) x.truncated[e] = (ended && !terminal) ? 1 : 0;
            uint4 out = rec;
            out.y = (rec.y & ~kUwPending) | (ended ? kUwPending : 0u);
            if (x.track_returns) out.z = __float_as_uint(__uint_as_float(rec.z) + rew);   // test_sac.py:98
            if (out.y != rec.y || out.z != rec.z) p.rec[e] = out;
            if (x.reset_mask) x.reset_mask[e] = 0;
        }
    }
    if (threadIdx.x == 0) p.wave_steps[blockIdx.x] = wave_count + 1u;   // single writer: this wavefront
}

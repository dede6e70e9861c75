// uavx_multi_params.hpp -- what the kernels of MultiUAVWorld2D are handed: the kernel-argument structs (MultiParams, StepExtra,
// the curriculum level table) and the LATE* macros that fetch single members of them late.  Included by uavx_multi.hip inside
// namespace uavx, first of its parts.

// LATE(on, p, member): p.member -- with `on` (a compile-time flag of the kernel variant) fetched where it is used instead of
// at the top of the kernel (late_karg(), uavx_device.hpp): for members that only a rare branch or the last instructions of a
// wavefront need, in the variants whose scalar registers are tight (8 wavefronts per SIMD = 80 SGPRs).  `p` must be the kernel's
// FIRST argument -- or, in step_ex_kernel, sit kExLead bytes into the segment (the macros add that).  NOT a free lunch, hence per variant: the headline kernel (4 UAVs, 66
// SGPRs, nothing to gain) lost 0.34 us of 5.85 with its `prev_ovr` / counter pointers fetched late -- the scalar loads at the top
// regroup (one dwordx8 became a dwordx2 + a dwordx4) and that launch is latency-shaped (profiles/r04_ab_notes.md).
// -DUAVX_LATE=0 turns every site off (A/B).
#ifndef UAVX_LATE
#define UAVX_LATE 1
#endif
template <bool ON>
__device__ __forceinline__ karg_ptr kargs_if() {
    if constexpr (ON && UAVX_LATE) return late_kargs();
    else return nullptr;
}
template <bool ON, class T>
__device__ __forceinline__ T karg_if(T plain, uint32_t byte_off) {   // (by value: an unused read of a kernel argument folds away)
    if constexpr (ON && UAVX_LATE) return late_karg<T>(byte_off);
    else return plain;
}
template <bool ON, class T>
__device__ __forceinline__ T karg_if(T plain, uint32_t byte_off, karg_ptr ka) {
    if constexpr (ON && UAVX_LATE) return late_karg<T>(byte_off, ka);
    else return plain;
}
// (every site that is switched on lives in step_ex_kernel, whose MultiParams sits behind kExLead bytes of leading scalar arguments)
constexpr uint32_t kExLead = 56;
#define LATE(on, p, member) karg_if<(on)>((p).member, kExLead + (uint32_t)offsetof(MultiParams, member))
// several members at one place: `LATE_BASE(on, ka);` once, then LATE_AT(on, ka, p, member) (one laundering point for all of them)
#define LATE_BASE(on, ka) const karg_ptr ka = kargs_if<(on)>()
#define LATE_AT(on, ka, p, member) karg_if<(on)>((p).member, kExLead + (uint32_t)offsetof(MultiParams, member), ka)
// members of uavx_step_ex's options block: the SECOND argument of step_ex_kernel, directly behind the first (static_assert below)
#define LATE_X(on, x, member) karg_if<(on)>((x).member, kExLead + (uint32_t)(sizeof(MultiParams) + offsetof(StepExtra, member)))
#define LATE_X_AT(on, ka, x, member) karg_if<(on)>((x).member, kExLead + (uint32_t)(sizeof(MultiParams) + offsetof(StepExtra, member)), ka)
// which sites a variant of step_ex_kernel switches on (bit mask, -DUAVX_LATE_EX=... for A/B): 1 the counter atomics at the end of a step,
// 2 a body's new waypoint (stage_bodies), 4 the episode fold, 8 step_ex's re-initialisation block, its tail pointers and flag arrays
#ifndef UAVX_LATE_EX
#define UAVX_LATE_EX 15       // step_ex_kernel with bodies / levels, and its 8-UAV specialisation
#endif

struct Goal { float tx, ty, init_d; uint32_t flags; };  // 16 B, one dwordx4 load; flags word stored only on change

// flag bits kept in Goal::flags (bits 0,1 are the public UAVX_FLAG_DONE / UAVX_FLAG_COLLIDED)
constexpr uint32_t kFlagPublic = UAVX_FLAG_DONE | UAVX_FLAG_COLLIDED | UAVX_FLAG_INACTIVE;
constexpr uint32_t kFlagPrevOvr = 8u;    // prev_distance is the value in prev_ovr[a], not ||target - location||
constexpr uint32_t kFlagJustDone = 16u;  // finished during the last step: prev_distance is still the distance then
                                         // (MUW:229 stores it once more; from the next step on it is 0, AG:24-25)

// One curriculum level as the kernels use it (uavx_level with the exact comparison limits precomputed on the host).
struct alignas(16) LevelParams {
    float lo_x, lo_y, hi_x, hi_y;                    // x inside [lox, hix] (MUW:213,224) <=> lo_x <= x <= hi_x in float32
    float sq_sense, sq_two_r, inv_sense, inv_diag;   // as the MultiParams fields of the same names
    double lox, loy, hix, hiy;                       // reset box (MUW:19-20); reset path only
    int32_t n_active, b_active, pad0, pad1;
};
// The world limits one lane works with: the handle's (kernel arguments, scalar registers) or its env's level's.
struct WorldLims {
    float lo_x, lo_y, hi_x, hi_y;
    float sq_sense, sq_two_r, inv_sense, inv_diag;
};

// The kernels take this struct BY VALUE: it is (most of) their kernel-argument segment, fetched by scalar loads, and a
// 65 536 x 4 step launch is latency-shaped -- so the ORDER of the members is a tuning parameter, and not an
// intuitive one.  (Since round 4 the arguments the first instructions need travel in front of it as preloaded leading scalars.)  Measured on one box (profiles/r03_ab_notes.md): a new pointer inserted after `coll`
// cost the headline launch 0.35 us of 5.72 with NO other change to the kernel (the members behind it moved across the
// scalar-load groups the compiler forms, nine loads instead of six sat in front of the first wait); the same pointer appended
// at the end costs nothing beyond its own use (5.78 with the tripwire it serves); a deliberate "hot members first, one
// 64-byte line per phase" order was WORSE at 4 UAVs (5.93) and better with scripted bodies (16.9 vs 17.4); parameters read
// from a device-resident block instead (one pointer in the kernel arguments) gave 5.78 / 17.7.  New members go at the END.
// What those figures measured is WHERE the compiler's scalar loads of the struct landed relative to the wait for the state
// loads, not the order as such.  The plain step_kernel variants no longer leave that to the compiler: they read three fixed
// runs of the struct by offset in front of that wait (fetch_step_args, uavx_multi_step.hpp; the static_asserts below HotParams
// pin the runs), so for them the order has stopped being a tuning parameter -- and moving a member of those runs breaks the
// build.  Every other kernel (the variants with bodies / levels, step_ex_kernel, step_k_kernel, reset, observe) still reads the
// struct through compiler-placed loads, and for those the note above stands.
struct MultiParams {
    double tau, rtau, amax, vmax;  // rtau = RN(1/tau), see div_tau()
    double lox, loy, hix, hiy;
    float lo_x, lo_y, hi_x, hi_y;  // float32 forms of the box test: (double)x >= lox  <=>  x >= lo_x  (smallest float32 >= lox) etc.
    double speed_sq_lim;  // ‖v‖ < 0.2 (MUW:218)  <=>  fma(vy,vy,vx*vx) < speed_sq_lim
    // exact float32 limits on the SQUARED distance s = fl(dx*dx)+fl(dy*dy) (sqrtf is monotone):
    float sq_sense;       // sqrtf(s) <  float32(d_sense)   <=>  s <  sq_sense   (AG:52)
    float sq_two_r;       // sqrtf(s) <= float32(2R)        <=>  s <= sq_two_r   (MUW:203)
    float sq_hard;        // sqrtf(s) <= 1.0                <=>  s <= sq_hard    (MUW:207)
    float inv_sense;      // 1/float32(d_sense)             MUW:77
    float vmax_norm;      // ‖(max_speed,max_speed)‖        MUW:62,183
    float inv_vmax_norm;
    float inv_diag;       // 1/‖(x_size,y_size)‖            MUW:17,68
    float two_r_reset;    // float32(2R), reset rejection (MUW:135,146,151)
    int recip_ok;         // div_tau() may use the reciprocal form for this tau
    int N, epw, magic;    // agents per env, envs per wave, 65536/N + 1 (lane / N == (lane * magic) >> 16 for lane < 64)
    int64_t E, env_offset;
    float2 *pos;
    float *prev_ovr;
    double2 *vel;
    Goal *goal;
    // env.steps (MUW:238) = wave_steps[wave of the env] - steps_base[env]: a step launch bumps ONE counter per
    // wavefront (every env of a wave is stepped by the same launches) instead of one word per env; reset and
    // set_state move the env's base (A/B at 65536x4: per-env counter updates cost 3 % of the launch).
    uint32_t *wave_steps;
    // per-env record, ONE 16-byte word (one load / one store per env in step_ex instead of four / three):
    //   .x steps_base   .y episode index (bits 0..30) | episode-ended flag (bit 31)   .z,.w running episode
    //   return of agent 0 and evaluation score sum_i r_i*(1-done_i) (float bits)
    uint4 *env_rec;
    uint32_t *reach, *coll;
    // episode bookkeeping (uavx_step_ex / uavx_reset)
    uint4 *fin_counts;  // [E] over ended episodes: {episodes, steps, target_reach_count, collision_count}
    float2 *fin_returns;  // [E] over ended episodes: {agent-0 return sum, evaluation score sum}
    // ---- configs[4] extension (scripted bodies + curriculum levels; EXT kernel variants only, see include/uavx.h) ----
    // Lanes stay one per LEARNER (N = L above); the B bodies of an env are slots L..L+B-1 of its LDS neighbour rows and
    // are moved by the env's learner lanes, body b by lane b % L in trip b / L.
    int B, nslots, kb;            // bodies per env, L + B, ceil(B / L)
    int body_pmask, body_pshift;  // period - 1, log2(period) (period is a power of two)
    float body_step;              // float32(speed * tau): metres per env step
    uint32_t body_k0, body_k1;    // Philox key of the waypoint streams
    int n_levels, level_lo, level_hi;
    float2 *body_pos;             // [E*B] {x, y}; +inf for a body its env's level switches off
    float4 *body_leg;             // [E*B] {dx, dy, heading, legs}: displacement per env step, direction of travel, steps of the leg that move
    uint8_t *lvl_cur, *lvl_next;  // [E] level in force / level assigned for the next reset
    const LevelParams *levels;    // [UAVX_MAX_LEVELS] device table, read only while a curriculum is installed (n_levels > 0)
    // ---- pre-drawn layouts (uavx_step_ex auto-reset; see stage_ahead) ----
    // The layout of an env's NEXT episode is a pure function of (seed, global env, episode index, level rule), so it is
    // drawn ahead of time by staging workgroups at the front of an earlier step launch and parked here; the step launch that
    // re-initialises the env then copies 16 B per slot instead of running the serial accept / reject chain on one wavefront while the
    // rest of the chip waits for it.  stage_tag says exactly what a parked layout was drawn for; anything else is a miss
    // and falls back to drawing in the step launch.
    // TWO parked layouts per env, for its next episode and the one after (slot = episode index & 1, slot-major arrays): the
    // layout of episode y + 1 is already there when episode y's is consumed, so an env only ever draws in place when two of its
    // episodes end within the two or three launches it takes to park a layout again
    float4 *stage_agent;          // [2][E*L] {sx, sy, tx, ty}
    float2 *stage_bpos;           // [2][E*B] as body_pos
    float4 *stage_bleg;           // [2][E*B] as body_leg
    uint4 *stage_tag;             // [2][E] {episode index, seed lo, seed hi, level | world version << 8 | valid << 31}
    int magic_s;                  // 65536 / (L + B) + 1: thread / (L + B) of a staging workgroup by multiply-shift
    uint32_t world_version;       // bumped by every call that changes what a layout depends on (config, curriculum, body rule)
    // agent-steps of the running episode whose reward came out non-finite (uavx_get_nonfinite): a NaN command or state
    // poisons an agent for good (AG:26-27 lets it through), and at 65 536 envs nobody scans the observations for it.
    // (LAST on purpose, see the note above the struct.)
    uint32_t *nonfin;
};
// What one agent step reads on its straight-line path, as VALUES: step_agent() and its helpers take these instead of reading
// a fixed struct (template parameter H), so a kernel decides where they come from: MultiParams itself is the plain form (the
// compiler places the scalar loads of the argument segment, as for any other member); step_kernel fetches a HotParams itself in
// front of its first wait (fetch_step_args).  Same member names as MultiParams.
struct HotParams {
    double tau, rtau, amax, vmax, speed_sq_lim;
    float lo_x, lo_y, hi_x, hi_y;
    float sq_sense, sq_two_r, sq_hard, inv_sense, vmax_norm, inv_vmax_norm, inv_diag;
    int recip_ok;
};
// fetch_step_args reads MultiParams as three runs of dwords; the runs are pinned here, so a moved member fails the build
static_assert(offsetof(MultiParams, tau) == 0 && offsetof(MultiParams, rtau) == 8 && offsetof(MultiParams, amax) == 16 &&
              offsetof(MultiParams, vmax) == 24, "fetch_step_args: the kinematics run");
static_assert(offsetof(MultiParams, lo_x) == 64 && offsetof(MultiParams, lo_y) == 68 && offsetof(MultiParams, hi_x) == 72 &&
              offsetof(MultiParams, hi_y) == 76 && offsetof(MultiParams, speed_sq_lim) == 80 && offsetof(MultiParams, sq_sense) == 88 &&
              offsetof(MultiParams, sq_two_r) == 92 && offsetof(MultiParams, sq_hard) == 96 && offsetof(MultiParams, inv_sense) == 100 &&
              offsetof(MultiParams, vmax_norm) == 104 && offsetof(MultiParams, inv_vmax_norm) == 108 &&
              offsetof(MultiParams, inv_diag) == 112 && offsetof(MultiParams, recip_ok) == 120, "fetch_step_args: the limits run");
constexpr uint32_t kStageValid = 0x80000000u;
constexpr uint32_t kRecEnded = 0x80000000u;  // env_rec.y bit 31: episode ended, re-initialise at the next step_ex
constexpr uint32_t kFlagInactive = UAVX_FLAG_INACTIVE;
constexpr int kLevelShift = 8;       // Goal::flags bits 8..11: the env's curriculum level (same value in every agent of the env)
constexpr uint32_t kLevelMask = 0xFu << kLevelShift;
constexpr int kExtSlots = 192;       // LDS neighbour rows per wave of an EXT kernel: epw * (L + B) <= 192
constexpr int kHintJobs = 8;         // layouts a staging workgroup takes on per draw: its 8 hint slots are ONE 64-byte scalar load

// options of uavx_step_ex that the kernel needs (uavx_step_args minus the buffers)
struct StepExtra {
    int action_mode, reset_policy, track_returns;
    uint32_t step_cap;
    uint32_t seed_lo, seed_hi;
    uint8_t *reset_mask;
    uint8_t *ended, *truncated;
    int flags_in_done;   // UAVX_FLAGS_IN_DONE: the three per-env flags travel in bits 1..3 of the env's first done byte
    int use_stage;   // consult the pre-drawn layouts
    // layouts drawn ahead: pf_blocks workgroups of the launch do not step anything -- they look for, and draw, the layouts of
    // the NEXT episodes (see stage_ahead); env-workgroup w is workgroup step_first + w
    uint32_t pf_blocks, pf_groups;   // staging workgroups, env-workgroups of the launch
    uint32_t stage_first, step_first;   // block id of the first staging / first env-workgroup: (0, pf_blocks) or (pf_groups, 0)
    uint2 *hints;                    // [pf_blocks][kHintJobs] {env + 1 (0: none), episode}: what a staging workgroup's last scan found
};

static_assert(sizeof(MultiParams) % alignof(StepExtra) == 0, "LATE_X: StepExtra must follow MultiParams without padding in the kernel-argument segment");

// The caller's buffers follow StepExtra in step_ex_kernel's argument list as plain parameters (`__restrict__`: they do not
// alias, and the compiler orders loads against stores on that knowledge -- handing them over in a struct cost the 4-UAV fused
// launch 0.2 us of 7.0).  Their places in the kernel-argument segment, for the variants that fetch the two output pointers
// again at their end (LATE_IO): each parameter sits at the next multiple of its alignment.
constexpr uint32_t kIoBase = kExLead + (uint32_t)(sizeof(MultiParams) + sizeof(StepExtra));   // int evaluate
constexpr uint32_t kIoRew = kIoBase + 16, kIoDone = kIoBase + 24;                    // (float *obs_out +8,) rew_out, done_out
static_assert(sizeof(StepExtra) % 8 == 0, "the pointer parameters behind StepExtra start on its end");

struct LevelTable { LevelParams l[UAVX_MAX_LEVELS]; };

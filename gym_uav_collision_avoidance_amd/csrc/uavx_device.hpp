// uavx_device.hpp — device-side building blocks shared by the MultiUAVWorld2D and UAVWorld2D
// kernels (gfx950 / CDNA4, wave64).  Compiled with -ffp-contract=off: the reference's float32
// norms and float64 kinematics are plain IEEE mul/add/div/sqrt chains with no FMA, and positions,
// distances and every mask must come out bit-identical to them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace uavx {

constexpr int kWave = 64;
#ifndef UAVX_BLOCK
#define UAVX_BLOCK 64  // A/B 64..1024 on MI355X: within 2 %, 64 marginally best (single-wave workgroups)
#endif
constexpr int kBlock = UAVX_BLOCK;        // waves per workgroup = kBlock / 64
constexpr int kWavesPerBlock = kBlock / kWave;
constexpr float kPi = 3.14159265358979323846f;
constexpr float kInvPi = 0.318309886183790671538f;
constexpr float kTwoPi = 6.28318530717958647692f;
constexpr float kInvTwoPi = 0.159154943091895335769f;

// LDS traffic below is wave-private (an env never spans two waves), so a compiler-level ordering
// point is all that is needed: DS instructions of one wave execute in issue order.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Write-through (sc1) vector stores.  A kernel boundary writes back whatever the launch left dirty
// in the XCD L2s (MI355X_MICROARCH.md price list, row "boundary": + B / 6 TB/s); the step kernel
// dirties ~20 MB per launch, so its bulk outputs are stored write-through and drain while the other
// waves still compute instead of serialising behind the last wave.  Out-of-range offsets are dropped
// by the buffer bounds check.
using rsrc_t = __amdgpu_buffer_rsrc_t;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
constexpr int kAuxSc1 = 16;  // gfx940+ cache-policy bit SC1 (write-through to memory)

__device__ __forceinline__ rsrc_t make_rsrc(const void *base, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), /*stride*/ 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ void store16_wt(rsrc_t r, uint32_t byte_off, float4 v) {
    u32x4 d = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
    __builtin_amdgcn_raw_buffer_store_b128(d, r, (int)byte_off, 0, kAuxSc1);
}
__device__ __forceinline__ void store16_wt(rsrc_t r, uint32_t byte_off, double2 v) {
    const unsigned long long a = __double_as_longlong(v.x), b = __double_as_longlong(v.y);
    u32x4 d = {(unsigned)a, (unsigned)(a >> 32), (unsigned)b, (unsigned)(b >> 32)};
    __builtin_amdgcn_raw_buffer_store_b128(d, r, (int)byte_off, 0, kAuxSc1);
}
__device__ __forceinline__ void store8_wt(rsrc_t r, uint32_t byte_off, float2 v) {
    u32x2 d = {__float_as_uint(v.x), __float_as_uint(v.y)};
    __builtin_amdgcn_raw_buffer_store_b64(d, r, (int)byte_off, 0, kAuxSc1);
}

// Lane L of a quad (four consecutive lanes) receives `v` of lane (L & ~3) + P<L & 3>: one DPP register move (v_mov_b32
// quad_perm), no LDS.  The source lane has to be enabled in EXEC: call it where the whole quad is live.
template <int P0, int P1, int P2, int P3>
__device__ __forceinline__ uint32_t quad_perm(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, P0 | (P1 << 2) | (P2 << 4) | (P3 << 6), 0xf, 0xf, true);
}
__device__ __forceinline__ float quad_perm_lane(float v, int k) {   // lane 4g of every quad: v of lane 4g + k (k = 1, 2, 3)
    const uint32_t u = __float_as_uint(v);
    return __uint_as_float(k == 1 ? quad_perm<1, 1, 1, 1>(u) : k == 2 ? quad_perm<2, 2, 2, 2>(u) : quad_perm<3, 3, 3, 3>(u));
}

// A kernel argument fetched WHERE IT IS USED.  The compiler treats the kernel-argument segment as invariant, dereferenceable
// memory and hoists every scalar load from it to the top of the kernel, where the value then occupies scalar registers for the
// whole life of the wavefront -- also the pointers that only a rare branch (an atomic on a goal arrival, a body's new waypoint)
// or the last few instructions need.  At 8 wavefronts per SIMD a wavefront has 80 scalar registers (800 per SIMD, 16 of each
// wavefront's share set aside for the trap handler, blocks of 16): the step kernels with scripted bodies went over and spilled
// such pointers into VGPR lanes (v_writelane / v_readlane).  Here the segment's address goes through an empty asm, which hides
// what it points at, so the load stays where it is written: one s_load through the scalar cache at the use (every wavefront of
// the launch reads the same line) instead of registers held from the first instruction on.
// `byte_off` is the argument's offset in the segment: offsetof() into the FIRST by-value argument of the kernel.  (Taking the
// address of a member of the argument itself will not do: an escaping address pins the kernel's private copy of the whole
// struct into scratch memory.)
typedef const __attribute__((address_space(4))) char *karg_ptr;
__device__ __forceinline__ karg_ptr late_kargs() {   // the segment, laundered: loads through it stay behind this point
    karg_ptr ka = (karg_ptr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(ka));
    return ka;
}
template <class T>
__device__ __forceinline__ T late_karg(uint32_t byte_off, karg_ptr ka = late_kargs()) {
    return *(const __attribute__((address_space(4))) T *)(ka + byte_off);
}

// Correctly rounded sqrtf in 9 instructions instead of the compiler's 17: v_sqrt_f32 (<= 1 ulp) followed by the
// same +-1 ulp residual test the compiler's IEEE expansion uses (e = s - c*r for the two neighbours c of r), but
// WITHOUT its input scaling by 2^32 / output scaling by 2^-16, which only serves s < 2^-96 (v_sqrt_f32 flushes
// denormal inputs and the residuals would underflow).  Squared distances of float32 world coordinates are either
// 0 or far above that (two distinct points closer than 1.1e-14 m would need coordinates of that size), so the
// scaled sequence sits behind a wave-uniform branch that is never taken in practice.  s = 0, +inf and NaN fall
// through the residual tests unchanged (every compare is false).  The step kernel spends a fifth of its VALU
// issue slots on square roots (prev / new target distance, N-1 neighbour distances); uavx_selftest() compares
// this function with sqrtf on every float32 bit pattern.
__device__ __forceinline__ float sqrt_rn(float s) {
    if (__builtin_expect(__any((__float_as_uint(s) - 1u) < 0x0F7FFFFFu), 0)) return sqrtf(s);  // 0 < s < 2^-96
    const float r = __builtin_amdgcn_sqrtf(s);
    const float lo = __uint_as_float(__float_as_uint(r) - 1u), hi = __uint_as_float(__float_as_uint(r) + 1u);
    const float e_lo = fmaf(-lo, r, s), e_hi = fmaf(-hi, r, s);
    float out = (e_lo <= 0.f) ? lo : r;
    out = (e_hi > 0.f) ? hi : out;
    return out;
}

// np.linalg.norm on a float32 pair: fl(fl(x*x) + fl(y*y)) then correctly rounded sqrt (AG:33,51).
__device__ __forceinline__ float norm32(float x, float y) {
    float a = x * x;
    float b = y * y;
    return sqrt_rn(a + b);
}

// np.clip on float64 scalars (AG:26-27): minimum(maximum(x, lo), hi)
__device__ __forceinline__ double clip64(double x, double lo, double hi) {
    double m = (x < lo) ? lo : x;
    return (m > hi) ? hi : m;
}

// atan2(sin x, cos x) for x in [-2pi, 2pi] (difference of two atan2 results), float32.  Equal to
// the reference's wrap on the circle; at the +-pi seam the sign may differ.
__device__ __forceinline__ float wrap_pi(float x) {
    float k = rintf(x * kInvTwoPi);
    return fmaf(-k, kTwoPi, x);
}

// wrap_pi(x) / pi for x in [-2pi, 2pi]: 2 fract(x / 2pi + 1/2) - 1, in [-1, 1) -- three instructions for the four of
// wrap_pi and the scaling (observation features, compared on the circle; |error| < 2.4e-7).
__device__ __forceinline__ float wrap_unit(float x) {
    return fmaf(__builtin_amdgcn_fractf(fmaf(x, kInvTwoPi, 0.5f)), 2.0f, -1.0f);
}

// atan2f for finite inputs, |error| < 7e-7 rad: t = min(|x|,|y|) / max(|x|,|y|) in [0, 1] and one odd minimax polynomial
// t * P(t^2) of degree 11 over the whole interval (fitted to atan on [0, 1]; 3.4e-7 there, 3.9e-7 evaluated in float32),
// then the quadrant.  No octant fold: the fold t -> (t-1)/(t+1) past tan(pi/8) cost eight instructions (compare, two selects,
// sub, add, the pi/4 add and select) against two more polynomial terms.  atan2(+-0, +0) = +-0: mx = 0 gives t = 0 / FLT_MIN.
// The quadrant is picked by the SIGN BIT of x, as atan2 does: atan2(+-0, -0) = +-pi (a compare x < 0 took -0 for +0 and gave
// 0 there, half a turn off math.atan2 for a poked -0.0 velocity or target offset).
// (Results only feed float32 observation/reward features that are compared at 1e-5.)
__device__ __forceinline__ float atan2_fast(float y, float x) {
    const float ax = fabsf(x), ay = fabsf(y);
    const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
    const float t = mn * __builtin_amdgcn_rcpf(fmaxf(mx, 1.17549435e-38f));
    const float z = t * t;
    float pl = fmaf(7.37447338e-3f, z, -3.55211943e-2f);
    pl = fmaf(pl, z, 8.21691155e-2f);
    pl = fmaf(pl, z, -1.33988619e-1f);
    pl = fmaf(pl, z, 1.98618680e-1f);
    pl = fmaf(pl, z, -3.33253950e-1f);
    float r = fmaf(pl * z, t, t);
    r = (ay > ax) ? 1.57079632679489661923f - r : r;
    r = (__float_as_int(x) < 0) ? kPi - r : r;
    return copysignf(r, y);
}

// The octant reduction and Cephes atanf polynomial on |t| <= tan(pi/8), with an IEEE division: every operation is correctly rounded, so
// the CPU test oracle restates it bit for bit (its atan2_leg).  Used where an angle becomes STATE (the heading
// a scripted body keeps for a whole leg); off the per-step path, so its cost does not matter.
__device__ __forceinline__ float atan2_exact(float y, float x) {
    const float ax = fabsf(x), ay = fabsf(y);
    const float mx = fmaxf(ax, ay), mn = fminf(ax, ay);
    const bool big = mn > 0.41421356237f * mx;
    const float num = big ? mn - mx : mn;
    float den = big ? mn + mx : mx;
    den = (mx == 0.f) ? 1.f : den;
    const float t = num / den;
    const float z = t * t;
    float pl = fmaf(8.05374449538e-2f, z, -1.38776856032e-1f);
    pl = fmaf(pl, z, 1.99777106478e-1f);
    pl = fmaf(pl, z, -3.33329491539e-1f);
    float r = fmaf(pl * z, t, t);
    r = big ? r + 0.78539816339744830962f : r;
    r = (ay > ax) ? 1.57079632679489661923f - r : r;
    r = (x < 0.f) ? kPi - r : r;
    return copysignf(r, y);
}

// v_max_f64 / v_min_f64 against a wave-uniform limit, as ONE instruction each.  fmax() / fmin() make hipcc canonicalise
// every operand first (v_max_f64 x, x, x -- also the limits held in scalar registers, again at every use): 20 float64
// instructions for the 12 clamps of one agent step, and a float64 instruction costs two float32 issue slots.  For
// non-NaN operands the result is the same; a NaN operand gives the other one back (what the callers count on: they
// re-poison NaN inputs afterwards).  `lim` must be uniform (kernel argument / literal): it is passed in scalar registers.
__device__ __forceinline__ double max64u(double x, double lim) {
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(x), "s"(lim));
    return r;
}
__device__ __forceinline__ double min64u(double x, double lim) {
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(x), "s"(lim));
    return r;
}

// x / tau, correctly rounded, without the hardware division sequence: with r = RN(1/tau) the
// Markstein form q0 = RN(x*r), rem = fma(-q0, tau, x) (exact), q = fma(rem, r, q0) returns the IEEE
// quotient (checked against x/tau on 2.1e9 samples for tau = 0.02 and six other steps; uavx_create
// re-checks the handle's tau on 1e5 samples and falls back to '/' if a single one differs).
// |x| is capped at 1e300 first so an infinite action still ends at the clip limit like np.clip does
// (a NaN turns into a finite value here; axis_update() poisons the result afterwards).
__device__ __forceinline__ double div_tau(double x, double tau, double rtau, bool recip_ok) {
    if (!recip_ok) return x / tau;
    x = min64u(max64u(x, -1e300), 1e300);
    const double q0 = x * rtau;
    const double rem = fma(-q0, tau, x);
    return fma(rem, rtau, q0);
}

// One double-integrator axis update, AG:26-29, float64 with a float32 position accumulate.  np.clip is
// done with v_max_f64 / v_min_f64 (one instruction each instead of compare + two selects); those return the
// non-NaN operand, so a NaN action or velocity is detected once (unordered compare) and put back, which
// is what np.clip / the reference would propagate.
__device__ __forceinline__ void axis_update(double a, double tau, double rtau, bool recip_ok, double amax, double vmax,
                                            double &v, float &x) {
    const bool poisoned = __builtin_isunordered(a, v);
    const double dv = min64u(max64u(div_tau(a - v, tau, rtau, recip_ok), -amax), amax);  // AG:26
    double nv = min64u(max64u(v + dv * tau, -vmax), vmax);                               // AG:27
    nv = poisoned ? __builtin_nan("") : nv;
    v = nv;
    x = (float)((double)x + v * tau);                                                // AG:28-29 (float32 array += float64 array)
}

// sin(pi*t), cos(pi*t) in float32: quarter-turn reduction + Taylor polynomials on |r| <= 1/4
// (|error| < 1e-7).  Fixed fmaf sequence so the CPU oracle can restate it bit for bit.
__device__ __forceinline__ void sincospi32(float t, float &sn, float &cs) {
    const float k = rintf(2.0f * t);
    const float r = fmaf(-0.5f, k, t);
    const float z = r * r;
    float ps = fmaf(z, 0.0821458866f, -0.599264529f);    //  pi^9/9!, -pi^7/7!
    ps = fmaf(ps, z, 2.55016404f);                       //  pi^5/5!
    ps = fmaf(ps, z, -5.16771278f);                      // -pi^3/3!
    ps = fmaf(ps, z, 3.14159265f);
    ps = ps * r;
    float pc = fmaf(z, -0.0258068913f, 0.235330630f);    // -pi^10/10!, pi^8/8!
    pc = fmaf(pc, z, -1.33526277f);                      // -pi^6/6!
    pc = fmaf(pc, z, 4.05871213f);                       //  pi^4/4!
    pc = fmaf(pc, z, -4.93480220f);                      // -pi^2/2!
    pc = fmaf(pc, z, 1.0f);
    const int q = (int)k & 3;
    sn = (q == 0) ? ps : (q == 1) ? pc : (q == 2) ? -ps : -pc;
    cs = (q == 0) ? pc : (q == 1) ? -ps : (q == 2) ? -pc : ps;
}

// sin and cos in double for the reference polar conversion (below): fdlibm's algorithm (e_rem_pio2 medium-size Cody-Waite
// reduction by pi/2 in three 33-bit parts, k_sin / k_cos polynomials on [-pi/4, pi/4] with the reduced argument as a
// double-double), error below 1 ulp -- what glibc's sin / cos promise, with neither a table nor a call.  |x| < 2^-27 returns
// (x, 1) as fdlibm does (keeps the sign of a zero).  Past |x| = 2^19 pi/2 (|a1| > 2.6e5, far outside the action box) the
// reduction would lose bits: those lanes take the library's sincos in a branch no action in [-1, 1] reaches.  NaN / +-inf give NaN.
__device__ __forceinline__ void sincos_ref(double x, double &sn, double &cs) {
    const double ax = fabs(x);
    if (__builtin_expect(__any(ax > 823549.6561538912), 0)) {   // 2^19 * pi/2 (cold: every action in [-1, 1] has |x| <= pi)
        if (ax > 823549.6561538912) { sincos(x, &sn, &cs); return; }
    }
    const double fn = rint(x * 6.36619772367581382433e-01);     // invpio2
    const int n = (int)fn;
    // e_rem_pio2 with the second and third iteration always taken (fdlibm skips them when they change nothing)
    double r = x - fn * 1.57079632673412561417e+00;              // pio2_1: 33 bits, fn * pio2_1 exact
    double t = r;                                                // (the first iteration's tail pio2_1t = pio2_2 + pio2_2t)
    double w = fn * 6.07710050630396597660e-11;                  // pio2_2
    r = t - w;
    w = fn * 2.02226624879595063154e-21 - ((t - r) - w);         // pio2_2t
    t = r;
    w = fn * 2.02226624871116645580e-21;                         // pio2_3
    r = t - w;
    w = fn * 8.47842766036889956997e-32 - ((t - r) - w);         // pio2_3t
    const double y0 = r - w;
    const double y1 = (r - y0) - w;
    // k_sin(y0, y1)
    const double z = y0 * y0, zz = z * z, v = z * y0;
    const double rs = 8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04 + z * 2.75573137070700676789e-06) +
                      z * zz * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10);
    const double ks = y0 - ((z * (0.5 * y1 - v * rs) - y1) - v * -1.66666666666666324348e-01);
    // k_cos(y0, y1)
    const double rc = z * (4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * 2.48015872894767294178e-05)) +
                      zz * zz * (-2.75573143513906633035e-07 + z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11));
    const double hz = 0.5 * z, wc = 1.0 - hz;
    const double kc = wc + (((1.0 - wc) - hz) + (z * rc - y0 * y1));
    const int q = n & 3;
    double s_ = (q == 0) ? ks : (q == 1) ? kc : (q == 2) ? -ks : -kc;
    double c_ = (q == 0) ? kc : (q == 1) ? -ks : (q == 2) ? -kc : ks;
    const bool tiny = ax < 7.450580596923828125e-9;              // 2^-27
    s_ = tiny ? x : s_;
    c_ = tiny ? 1.0 : c_;
    const bool fin = ax <= 1.7976931348623157e308;               // NaN / inf: NaN
    sn = fin ? s_ : __builtin_nan("");
    cs = fin ? c_ : __builtin_nan("");
}

// UAVX_ACTION_POLAR_REFERENCE: the trainers' own expression (test_sac_multi.py:77-80, test_sac.py:77-78) with the dtypes it
// has under NumPy 2 (NEP 50).  `h` is the float32 speed scale: ||action_space.high|| (MUW) or action_space.high[0] (UW).
// float32 action (the policy branch): v = fl32(fl32(a0/2 + 0.5f) * h), theta = fl32(a1 * fl32(pi)), the Python float
// math.cos / math.sin of the widened theta rounded to float32 (np.float32 * Python float), and a FLOAT32 command
// (fl32(v*c), fl32(v*s)).  Every step is one correctly rounded operation (compiled without contraction), so the result is the
// reference's bit for bit whenever the double cos / sin round to the same float32 as glibc's -- all but values within
// ~2^-52 of a float32 rounding midpoint.  a0/2 is computed as a0*0.5f: the same correctly rounded value, subnormals included.
// A NaN or infinite theta gives a NaN command (the reference returns NaN for NaN and raises for +-inf).
__device__ __forceinline__ void polar_to_command_ref32(float a0, float a1, float h, double &ax, double &ay) {
    const float u = a0 * 0.5f + 0.5f;
    const float v = u * h;
    const float theta = a1 * 3.14159265358979323846f;
    double s, c;
    sincos_ref((double)theta, s, c);
    ax = (double)(v * (float)c);
    ay = (double)(v * (float)s);
}
// float64 action (the warm-up branch, np.random.uniform): every step in double, a FLOAT64 command.  sincos_ref and glibc are
// both within 1 ulp of the true value, so the command may differ from the reference's by an ulp (rate).
__device__ __forceinline__ void polar_to_command_ref64(double a0, double a1, float h, double &ax, double &ay) {
    const double v = (a0 * 0.5 + 0.5) * (double)h;
    const double theta = a1 * 3.14159265358979323846;
    double s, c;
    sincos_ref(theta, s, c);
    ax = v * c;
    ay = v * s;
}
template <bool ACT64>
__device__ __forceinline__ void polar_to_command_ref(float h, double &ax, double &ay) {
    if (ACT64) polar_to_command_ref64(ax, ay, h, ax, ay);
    else polar_to_command_ref32((float)ax, (float)ay, h, ax, ay);   // ax, ay hold a widened float32 action: exact
}

// Philox4x32-10, counter-based: one call yields the two 53-bit uniforms of one
// np.random.uniform(lo, hi, (2,)) draw (MUW:126,131,144; UW:121-126).
__device__ __forceinline__ void philox4x32(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                           uint32_t k1, uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        uint32_t n1 = (uint32_t)p1;
        uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        uint32_t n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
__device__ __forceinline__ double bits53(uint32_t a, uint32_t b) {
    return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) / 9007199254740992.0;
}
// Candidates of the multi-agent reset.  Agent i of an env owns the Philox sequence with counter
// (global env [31:0], global env [47:32] | i << 16, attempt k, episode); call k yields the k-th START
// candidate from words 0,1 and the k-th TARGET candidate from words 2,3 (32-bit uniforms: 1e-8 m
// granularity over a 50 m box, far below float32 resolution).  Independent per-agent sequences let
// the lanes of an env draw in parallel while the accept/reject chain (MUW:127-153) keeps agent order.
// The reset path runs in a few waves per launch only, so its instructions are never warm in the
// instruction cache: code SIZE is what it costs (measured: an unrolled, 3x-inlined version added 3.6 us
// of tail to a 7 us step launch with 0.2 % of the envs resetting).  Hence rolled rounds; and inlined, because a
// real call makes the callee wait for vmcnt(0), i.e. for every load the wave still has in flight.
struct ResetCandidates {
    float sx, sy, tx, ty;
};
// the four Philox4x32-10 output words of counter (env[31:0], env[47:32] | agent << 16, attempt, episode); rolled rounds
__device__ __forceinline__ void reset_words(uint64_t global_env, uint32_t agent, uint32_t attempt, uint32_t episode,
                                            uint32_t k0, uint32_t k1, uint32_t o[4]) {
    uint32_t c0 = (uint32_t)global_env, c1 = ((uint32_t)(global_env >> 32) & 0xFFFFu) | (agent << 16);
    uint32_t c2 = attempt, c3 = episode;
#pragma unroll 1
    for (int r = 0; r < 10; r++) {  // Philox4x32-10, same rounds as philox4x32() above
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}
__device__ __forceinline__ ResetCandidates reset_candidates(uint64_t global_env, uint32_t agent, uint32_t attempt,
                                                            uint32_t episode, uint32_t k0, uint32_t k1, double lox,
                                                            double loy, double hix, double hiy) {
    uint32_t o[4];
    reset_words(global_env, agent, attempt, episode, k0, k1, o);
    const double sx = hix - lox, sy = hiy - loy, inv = 1.0 / 4294967296.0;
    ResetCandidates c;  // lo + (hi-lo)*U cast to float32 like np.random.uniform(lo, hi).astype(np.float32)
    c.sx = (float)(lox + sx * ((double)o[0] * inv));
    c.sy = (float)(loy + sy * ((double)o[1] * inv));
    c.tx = (float)(lox + sx * ((double)o[2] * inv));
    c.ty = (float)(loy + sy * ((double)o[3] * inv));
    return c;
}

struct PhiloxDraws {
    uint32_t env_lo, env_hi, episode, k0, k1, draw;
    // lo + (hi-lo)*U cast to float32, per axis, like np.random.uniform(...).astype(np.float32)
    __device__ __forceinline__ void point32(double lox, double loy, double hix, double hiy, float &px, float &py) {
        uint32_t o[4];
        philox4x32(env_lo, env_hi, draw++, episode, k0, k1, o);
        px = (float)(lox + (hix - lox) * bits53(o[0], o[1]));
        py = (float)(loy + (hiy - loy) * bits53(o[2], o[3]));
    }
};

}  // namespace uavx

// The n-step walk over the replay ring, once: uavx_replay.hip's sample_small and sample_gather run it with the
// start row, uavx_keywalk.hip's walk_rows (§25) without.  Prioritized n-step replay is the uniform sampler's n-step only
// because the two are this one function.
//
// Once (s, e, i) is chosen every address of the walk is known: step t lies in slot s + min(t, top), minus slots past the wrap
// (one compare, no division), so that every load is inside the window whatever the flags will say.  The rew, done and flag
// loads of ALL steps are issued together and unconditionally, with the start row's observation and action where they are
// wanted, and the stop is resolved in registers afterwards (a load under a run-time condition is branched around and waited
// for one by one: uavx_grad_impl.hpp).  Only next_state, whose slot is s + len, waits for that resolution.  §22 says what the
// compiler makes of other shapes of this function: it is one body on purpose, and not a set of helpers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace uavx_common {

// Row j's walk from slot s of env e, agent i.  top: the last step the walk can reach, min(n_step − 1, steps to the newest of
// the ring), the caller's to compute; NMAX >= n_step (the launches pick NMAX == n_step).  I: the type of the slot arithmetic,
// int32_t or uint32_t, s + NMAX < 2·slots either way.  START: the start row's observation and action go to a.state and
// a.action.  A: the kernel's arguments -- the ring's arrays and L, E, N, gamma, and the outputs reward, next_state, mask,
// length (or NULL), truncated and ended_out (both or neither).
template <int NMAX, bool PACKED, bool START, class I, class A>
__device__ inline void nstep_walk(const A &a, int64_t j, I s, I e, I i, I top) {
    constexpr int OBS = 10;
    const I L = (I)a.L;
    const int64_t se0 = (int64_t)s * a.E + e, cell0 = se0 * a.N + i;
    const bool flags = a.truncated != nullptr;
    float rew[NMAX];
    uint8_t dn[NMAX], sk[NMAX], en[NMAX], tr[NMAX];      // PACKED: sk holds agent 0's done byte, en and tr are not used
#pragma unroll
    for (int t = 0; t < NMAX; ++t) {
        I st = s + ((I)t < top ? (I)t : top);            // st < 2·slots: top <= span − 1 <= slots − 2
        if (st >= L) st -= L;
        const int64_t se = (int64_t)st * a.E + e, cell = se * a.N + i;
        rew[t] = a.rew[cell];
        dn[t] = a.done[cell];
        if (NMAX == 1) {
            // a single step stops by itself: its flags are only outputs, loaded below when they are asked for
            sk[t] = en[t] = tr[t] = 0;
        } else if (PACKED) {
            sk[t] = a.done[se * a.N];
        } else {
            sk[t] = a.skip[se];
            en[t] = a.ended[se];
            tr[t] = a.trunc[se];                         // wanted or not: a load under `flags` would be waited for by itself
        }
    }
    float2 xs[OBS / 2], ys[OBS / 2], act;
    if constexpr (START) {
        const float2 *__restrict__ x = (const float2 *)(a.obs + cell0 * OBS);
#pragma unroll
        for (int k = 0; k < OBS / 2; ++k) xs[k] = x[k];
        act = *(const float2 *)(a.act + cell0 * 2);
    }
    // every load above is issued before the first of them is waited for: left to itself the scheduler starts resolving
    // step 0 after half the loads, which puts a wait for memory between the two halves.  (A single step resolves nothing,
    // and its next_state load belongs with the others.)
    if (NMAX > 1) __builtin_amdgcn_sched_barrier(0);

    // the stop, in registers: nothing below loads, and every step is computed and then selected, so that there is no
    // conditional block for the compiler to sink a step's loads into
    double R = -0.0, g = 1.0;                            // −0 + x is x for every x, a reward of −0 included
    I len = 1;
    bool run = true;
    uint8_t d_last = 0, tr_last = 0, en_last = 0;
#pragma unroll
    for (int t = 0; t < NMAX; ++t) {
        const bool ended = PACKED ? (sk[t] & 4) != 0 : en[t] != 0;
        const bool trunc = PACKED ? (sk[t] & 8) != 0 : tr[t] != 0;
        bool stop = t == NMAX - 1 || (I)t >= top || (dn[t] & 1) || ended;
        if (t + 1 < NMAX) stop = stop || (PACKED ? (sk[t + 1] & 2) != 0 : sk[t + 1] != 0);
        const double Rt = R + g * (double)rew[t], gt = g * a.gamma;
        R = run ? Rt : R;
        d_last = run ? (uint8_t)(dn[t] & 1) : d_last;
        tr_last = run ? (uint8_t)trunc : tr_last;
        en_last = run ? (uint8_t)ended : en_last;
        run = run && !stop;
        g = run ? gt : g;
        len = run ? (I)t + 2 : len;
    }

    I s1 = s + len;                                      // len <= top + 1 <= span <= slots − 1
    if (s1 >= L) s1 -= L;
    const float2 *__restrict__ y = (const float2 *)(a.obs + (((int64_t)s1 * a.E + e) * a.N + i) * OBS);
#pragma unroll
    for (int k = 0; k < OBS / 2; ++k) ys[k] = y[k];
    if (NMAX == 1 && flags) {                            // behind the row's other loads, as the one-step sampler has them
        if (PACKED) {
            const uint8_t b = a.done[se0 * a.N];
            tr_last = (b >> 3) & 1;
            en_last = (b >> 2) & 1;
        } else {
            tr_last = a.trunc[se0] != 0;
            en_last = a.ended[se0] != 0;
        }
    }
    float2 *__restrict__ yo = (float2 *)(a.next_state + j * OBS);
    if constexpr (START) {
        float2 *__restrict__ xo = (float2 *)(a.state + j * OBS);
#pragma unroll
        for (int k = 0; k < OBS / 2; ++k) {
            xo[k] = xs[k];
            yo[k] = ys[k];
        }
        *(float2 *)(a.action + j * 2) = act;
    } else {
#pragma unroll
        for (int k = 0; k < OBS / 2; ++k) yo[k] = ys[k];
    }
    a.reward[j] = (float)R;
    a.mask[j] = (float)((1.0 - (double)d_last) * g);
    if (a.length) a.length[j] = (uint8_t)len;
    if (flags) {
        a.truncated[j] = tr_last;
        a.ended_out[j] = en_last;
    }
}

}  // namespace uavx_common

// Critic action-gradient (include/uavx_action_grad.h): q_t(s, a) and ∂q_t/∂a of the learners' actor update in ONE launch,
// from the module's live parameters, with no weight gradients and no workspace.  DESIGN.md §17.
//
// All products run on v_mfma_f32_16x16x4_f32 (exact f32, a k-ordered fmaf chain).  Lane l = 16·g + c of a wave holds
// A[m = c][k = g] and B[k = g][n = c]; the accumulator element ii holds C[m = 4g + ii][n = c].
//
//   action_grad   one workgroup of 8 waves per 16-row block and selected tower; rows are MFMA columns, units MFMA rows.
//                 Layer 1 (f64, rounded once) into LDS.  Then ONE sweep over W2, wave w taking the 16-unit blocks
//                 j ≡ w (mod 8): z2ᵀ = W2·h1ᵀ of the block (each 16-wide k block's MFMA chain added up in f64),
//                 w3·act(z2) folded into q (f64), and, because the upstream gradient of q is 1, δ2 = w3 ⊙ act′(z2)
//                 formed in the same registers and fed straight into δ1ᵀ += W2ᵀ·δ2ᵀ as its B operand (the k order of the
//                 accumulator is the unit order of the block).  z2 never leaves registers.  The eight waves' δ1ᵀ are
//                 summed through LDS in a fixed order, (w + (w+4)) for w = 0..3 in f32 and then those four in wave
//                 order in f64; δ1 = sum ⊙ act′(z1) and its product with the two action columns of W1 stay in f64 and
//                 are rounded once.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/uavx_action_grad.h"
#include "uavx_actor_impl.hpp"

namespace uavx_action_grad_k {

using uavx_actor_k::act;
using uavx_actor_k::f32x4;

constexpr int OBS = 10, IN = 12, WG = 512, WAVES = WG / 64, HALF = WAVES / 2;

__device__ inline f32x4 mma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// torch's backward of the activation, given the pre-activation z (or the activation: the sign is the same) and the
// incoming gradient d: relu: threshold_backward (z <= 0 gives 0; NaN passes), leaky_relu(0.01): z > 0 ? d : d·0.01
template <bool LEAKY>
__device__ inline float act_bwd(float z, float d) {
    if constexpr (LEAKY) return z > 0.f ? d : d * 0.01f;
    else return z <= 0.f ? 0.f : d;
}
template <bool LEAKY>
__device__ inline double act_bwd(float z, double d) {
    if constexpr (LEAKY) return z > 0.f ? d : d * 0.01;
    else return z <= 0.f ? 0.0 : d;
}

struct Args {
    const float *W1[2], *b1[2], *W2[2], *b2[2], *W3[2], *b3[2];
    const float *state, *action;
    float *q, *dqda;                   // tower t at + t * rows (* 2)
    int64_t rows, s_stride, a_stride;
    int h1, h2, nb2, t0;               // t0: the tower of blockIdx.y == 0
};

template <bool LEAKY, int NB1>
__global__ __launch_bounds__(WG) void action_grad(Args a) {
    constexpr int N1 = 16 * NB1, HP = N1 + 4;
    __shared__ float xs[16][IN];
    __shared__ __attribute__((aligned(16))) float h1s[16][HP];   // h1 of the block's rows (read as f32x4)
    __shared__ f32x4 red[HALF][NB1][64];       // δ1ᵀ accumulators: waves 4..7, then (w + (w+4)) of waves 0..3
    __shared__ double qs[WAVES][16];
    __shared__ double js[WAVES][16][2];
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c = lane & 15, wave = tid >> 6;
    const int t = a.t0 + blockIdx.y, h1 = a.h1, h2 = a.h2;
    const int64_t row0 = (int64_t)blockIdx.x * 16;
    // tower t's parameters, selected without indexing the argument arrays by a run-time value (that goes to scratch)
    const float *__restrict__ W1 = t ? a.W1[1] : a.W1[0], *__restrict__ b1 = t ? a.b1[1] : a.b1[0];
    const float *__restrict__ W2 = t ? a.W2[1] : a.W2[0], *__restrict__ b2 = t ? a.b2[1] : a.b2[0];
    const float *__restrict__ W3 = t ? a.W3[1] : a.W3[0], *__restrict__ b3 = t ? a.b3[1] : a.b3[0];
    const bool rin = row0 + c < a.rows;        // row c of the block is a real row

    // ---- [state, action] of the block's rows (0 past the last row: nothing there is read)
    if (tid < 16 * IN) {
        const int r = tid / IN, k = tid % IN;
        const int64_t row = row0 + r;
        float v = 0.f;
        if (row < a.rows) v = k < OBS ? a.state[row * a.s_stride + k] : a.action[row * a.a_stride + (k - OBS)];
        xs[r][k] = v;
    }
    __syncthreads();

    // ---- layer 1: h1 into LDS; 0 for padded units and padded rows
    for (int e = tid; e < 16 * N1; e += WG) {
        const int r = e / N1, i = e % N1;
        float h = 0.f;
        if (i < h1 && row0 + r < a.rows) {
            double z = b1[i];                  // in f64, rounded once
#pragma unroll
            for (int k = 0; k < IN; ++k) z += (double)W1[i * IN + k] * (double)xs[r][k];
            h = act<LEAKY>((float)z);
        }
        h1s[r][i] = h;
    }
    __syncthreads();

    // ---- the one sweep over W2: per unit block z2, q and δ2 in registers, then δ1ᵀ += W2ᵀ·δ2ᵀ
    double qp = 0.0;
    f32x4 dacc[NB1];
#pragma unroll
    for (int ib = 0; ib < NB1; ++ib) dacc[ib] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int jb = wave; jb < a.nb2; jb += WAVES) {
        const int j = 16 * jb + c;             // this lane's A row
        const bool jin = j < h2;
        const float *w2 = W2 + (int64_t)(jin ? j : 0) * h1;
        // each 16-wide k block is a 4-step fmaf chain of its own (rotating over four accumulators so that the MFMAs of
        // neighbouring blocks overlap), added into f64: z2, and with it q, is rounded once, not once per k step
        f32x4 acc4[4];
        double zd[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kb = 0; kb < NB1; ++kb) {
            const f32x4 hv = *(const f32x4 *)&h1s[c][16 * kb + 4 * g];
            f32x4 &acc = acc4[kb & 3];
            acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ii = 0; ii < 4; ++ii) {
                // every load is unconditional, from a clamped address, and the value is selected afterwards: a load under
                // a run-time condition is branched around and waited for one by one
                const int k = 16 * kb + 4 * g + ii;
                const bool kin = kb < NB1 - 1 || k < h1;                                  // h1 > 16·(NB1 − 1)
                const float wv = w2[kin ? k : h1 - 1];
                acc = mma(jin && kin ? wv : 0.f, hv[ii], acc);
            }
#pragma unroll
            for (int ii = 0; ii < 4; ++ii) zd[ii] += (double)acc[ii];
        }
        f32x4 d2;
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) {
            const int jj = 16 * jb + 4 * g + ii;
            const bool in = jj < h2;
            const float z = in ? (float)(zd[ii] + (double)b2[jj]) : 0.f;
            const float w3 = in ? W3[jj] : 0.f;
            qp += (double)w3 * (double)act<LEAKY>(z);
            d2[ii] = rin && in ? act_bwd<LEAKY>(z, w3) : 0.f;   // dq/dq = 1: δ2 does not wait for q
        }
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) {
            const int jj = 16 * jb + 4 * g + ii;
            const float *w2r = W2 + (int64_t)(jj < h2 ? jj : 0) * h1;
#pragma unroll
            for (int ib = 0; ib < NB1; ++ib) {
                const int i = 16 * ib + c;
                const bool iin = ib < NB1 - 1 || i < h1;
                const float wv = w2r[iin ? i : h1 - 1];
                dacc[ib] = mma(jj < h2 && iin ? wv : 0.f, d2[ii], dacc[ib]);
            }
            // the 25-block tile: keep the scheduler from hoisting all 100 loads of the four steps at once, which spills
            // (8 waves of 512 threads leave 256 registers a lane)
            if constexpr (NB1 > 16) __builtin_amdgcn_sched_barrier(0);
        }
    }
    qp += __shfl_xor(qp, 16);
    qp += __shfl_xor(qp, 32);
    if (g == 0) qs[wave][c] = qp;

    // ---- δ1ᵀ over the waves, in a fixed order: waves 4..7 park theirs, waves 0..3 add their own to it in place
    if (wave >= HALF) {
#pragma unroll
        for (int ib = 0; ib < NB1; ++ib) red[wave - HALF][ib][lane] = dacc[ib];
    }
    __syncthreads();
    if (wave < HALF) {
#pragma unroll
        for (int ib = 0; ib < NB1; ++ib) red[wave][ib][lane] = dacc[ib] + red[wave][ib][lane];
    }
    __syncthreads();
    // δ1 = (the four sums in wave order, f64) ⊙ act′(z1), over h1 in LDS (h1 > 0 exactly when z1 > 0; a NaN stays a NaN),
    // times the action columns of W1, summed over the units in f64
    double pj0 = 0.0, pj1 = 0.0;
    for (int ib = wave; ib < NB1; ib += WAVES) {
        const f32x4 r0 = red[0][ib][lane], r1 = red[1][ib][lane], r2 = red[2][ib][lane], r3 = red[3][ib][lane];
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) {
            const int i = 16 * ib + 4 * g + ii;
            if (i < h1) {
                const double s = (((double)r0[ii] + (double)r1[ii]) + (double)r2[ii]) + (double)r3[ii];
                const double d1 = act_bwd<LEAKY>(h1s[c][i], s);
                pj0 += d1 * (double)W1[i * IN + OBS];
                pj1 += d1 * (double)W1[i * IN + OBS + 1];
            }
        }
    }
    pj0 += __shfl_xor(pj0, 16);
    pj0 += __shfl_xor(pj0, 32);
    pj1 += __shfl_xor(pj1, 16);
    pj1 += __shfl_xor(pj1, 32);
    if (g == 0) {
        js[wave][c][0] = pj0;
        js[wave][c][1] = pj1;
    }
    __syncthreads();
    // ---- the waves' partial sums in wave order, rounded once; only real rows of the selected tower are written
    if (tid < 16) {
        const int64_t row = row0 + tid;
        if (a.q && row < a.rows) {
            double q = qs[0][tid];
#pragma unroll
            for (int w = 1; w < WAVES; ++w) q += qs[w][tid];
            a.q[t * a.rows + row] = (float)(q + (double)b3[0]);
        }
    } else if (tid >= 64 && tid < 96) {
        const int r = (tid - 64) >> 1, jx = tid & 1;
        const int64_t row = row0 + r;
        if (row < a.rows) {
            double s = js[0][r][jx];
#pragma unroll
            for (int w = 1; w < WAVES; ++w) s += js[w][r][jx];
            a.dqda[(t * a.rows + row) * 2 + jx] = (float)s;
        }
    }
}

}  // namespace uavx_action_grad_k

using namespace uavx_action_grad_k;

extern "C" {

int uavx_action_grad_version(void) { return UAVX_ACTION_GRAD_VERSION; }

int uavx_action_grad(const uavx_critic *h, int towers_mask, const float *const *params, const float *state, int64_t rows,
                     int64_t s_stride, const float *action, int64_t a_stride, float *q, float *dqda, void *stream) {
    if (!h || !params || !state || !action || !dqda) return UAVX_CRITIC_ERR_INVALID_ARG;
    if (rows < 1 || rows > UAVX_ACTION_GRAD_MAX_ROWS || s_stride < OBS || a_stride < 2) return UAVX_CRITIC_ERR_INVALID_ARG;
    if (towers_mask < 1 || towers_mask > 3) return UAVX_CRITIC_ERR_INVALID_ARG;
    if (h->prec != UAVX_CRITIC_F32) return UAVX_CRITIC_ERR_UNSUPPORTED;
    if (h->L.nb1 != (h->kind == UAVX_CRITIC_DDPG ? 25 : 16)) return UAVX_CRITIC_ERR_UNSUPPORTED;
    if (towers_mask >> h->towers) return UAVX_CRITIC_ERR_INVALID_ARG;   // a tower the handle does not have
    Args ka{};
    for (int t = 0; t < h->towers; ++t) {
        if (!(towers_mask >> t & 1)) continue;
        for (int i = 0; i < 6; ++i)
            if (!params[6 * t + i]) return UAVX_CRITIC_ERR_INVALID_ARG;
        ka.W1[t] = params[6 * t + 0];
        ka.b1[t] = params[6 * t + 1];
        ka.W2[t] = params[6 * t + 2];
        ka.b2[t] = params[6 * t + 3];
        ka.W3[t] = params[6 * t + 4];
        ka.b3[t] = params[6 * t + 5];
    }
    ka.state = state;
    ka.action = action;
    ka.q = q;
    ka.dqda = dqda;
    ka.rows = rows;
    ka.s_stride = s_stride;
    ka.a_stride = a_stride;
    ka.h1 = h->h1;
    ka.h2 = h->h2;
    ka.nb2 = (h->h2 + 15) / 16;
    ka.t0 = towers_mask == 2 ? 1 : 0;
    const unsigned blocks = (unsigned)((rows + 15) / 16), sel = towers_mask == 3 ? 2u : 1u;
    void (*fn)(Args) = h->kind == UAVX_CRITIC_DDPG ? action_grad<true, 25> : action_grad<false, 16>;
    hipLaunchKernelGGL(fn, dim3(blocks, sel), dim3(WG), 0, (hipStream_t)stream, ka);
    return hipGetLastError() == hipSuccess ? UAVX_CRITIC_OK : UAVX_CRITIC_ERR_HIP;
}

}  // extern "C"

// Critic action-gradient (include/uavx_action_grad.h): q_t(s, a) and ∂q_t/∂a of the learners' actor update in ONE launch,
// from the module's live parameters, with no weight gradients and no workspace.  DESIGN.md §17.
//
// The lane layout of the MFMA products, layer 1, the z2 chain of a unit block and the eight-wave fold are shared with the
// other gradient units: uavx_grad_impl.hpp.  The δ1 step is that header's too, but written out here (see the kernel).
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
#include "uavx_grad_impl.hpp"

namespace uavx_action_grad_k {

using namespace uavx_grad_k;

constexpr int OBS = 10, IN = 12, WG = 512, WAVES = WG / 64;

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
    __shared__ f32x4 red[4][NB1][64];          // δ1ᵀ accumulators: waves 4..7, then (w + (w+4)) of waves 0..3
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

    // ---- layer 1: h1 into LDS only
    layer1<LEAKY, NB1, IN, WG>(W1, b1, xs, h1s, nullptr, h1, row0, a.rows, tid);
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
        double zd[4];
        z2_block<NB1, false>(w2, jin, h1, h1s, g, c, zd);
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
        // uavx_grad_impl.hpp's delta1_block, written out: through the helper the compiler orders action_grad<true, 25>
        // differently (same registers) and the launch measured 0.4 % slower at 65 536 rows
        // (profiles/r17_grad_share_bench.jsonl); policy_bwd compiles the same either way and uses the helper
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
            if constexpr (NB1 > 16) __builtin_amdgcn_sched_barrier(0);   // see delta1_block
        }
    }
    qp += __shfl_xor(qp, 16);
    qp += __shfl_xor(qp, 32);
    if (g == 0) qs[wave][c] = qp;

    // ---- δ1ᵀ over the waves: (w + (w+4)) for w = 0..3 in LDS, then
    // δ1 = (the four sums in wave order, f64) ⊙ act′(z1), over h1 in LDS (h1 > 0 exactly when z1 > 0; a NaN stays a NaN),
    // times the action columns of W1, summed over the units in f64
    fold8<NB1>(red, dacc, wave, lane);
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

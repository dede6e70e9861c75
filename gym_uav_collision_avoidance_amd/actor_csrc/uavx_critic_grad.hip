// Critic-loss gradients (include/uavx_critic_grad.h): the forward with saved activations, the MSE / L1 loss and the
// backward of the learners' critic update, in three launches.  DESIGN.md §14.  The weighted call
// (include/uavx_wcritic_grad.h) is the same three launches: a per-row importance-sampling weight enters dq
// and the loss term once, in the row pass's 16-thread dq step, and q(s, a) is an output; every summation order is shared,
// so a weight of 1 gives the unweighted gradients and losses bit for bit.
//
// The lane layout of the MFMA products, layer 1, the W1 / b1 tail, the small helpers and the weights launch are shared with
// the other gradient units: uavx_grad_impl.hpp.
//
//   1. grad_rows     one workgroup (4 waves) per 16-row block and tower; rows are MFMA columns, units MFMA rows.
//                    Layer 1 (f64, rounded once) into LDS and to the workspace, for dW2; z2ᵀ = W2·h1ᵀ with wave w
//                    taking the 16-unit blocks j ≡ w (mod 4), each 16-wide k block's MFMA chain added up in f64, z2
//                    written to the workspace; q summed over units and waves in a fixed order;
//                    dq per row (W: times the row's weight, and q written out);
//                    then per unit block again: δ2 = dq·w3 ⊙ act′(z2) over z2 in the workspace, and
//                    δ1ᵀ += W2ᵀ·δ2ᵀ straight from the δ2 accumulator (its k order is the unit order of the block).  The
//                    four waves' δ1 are summed through LDS in wave order.  The block's sums over its 16 rows of the
//                    small gradients (W1, b1, b2, W3, b3) and of the loss go to a per-block partial row (f64).
//   2. uavx_grad_k::grad_weights (uavx_grad_common.hip)  dW2 per split-K slice of rows and the partial rows per slice.
//   3. grad_combine  one thread per output element: the split-K slices summed in slice order (f64), rounded once to f32
//                    and written in torch layout; the loss divided by the row count.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/uavx_critic_grad.h"
#include "../../include/uavx_wcritic_grad.h"
#include "uavx_grad_impl.hpp"

namespace uavx_critic_grad_k {

using namespace uavx_grad_k;

constexpr int OBS = 10, IN = 12, WG = 256, WAVES = WG / 64;

// offsets inside a per-block partial row (and inside the small-gradient slices): W1 [h1][12], b1, b2, W3, b3, loss
struct Small {
    int w1, b1, b2, w3, b3, loss, n;
};
__host__ __device__ inline Small small_layout(int h1, int h2) {
    Small s;
    s.w1 = 0;
    s.b1 = 12 * h1;
    s.b2 = 13 * h1;
    s.w3 = s.b2 + h2;
    s.b3 = s.w3 + h2;
    s.loss = s.b3 + 1;
    s.n = s.loss + 1;
    return s;
}

struct RowArgs {
    const float *W1[2], *b1[2], *W2[2], *b2[2], *W3[2], *b3[2];
    const float *state, *action, *y;
    int64_t rows, s_stride, a_stride, y_stride;
    float *h1ws, *d2ws;                // tower t at + t * *_tower
    double *pws;
    int64_t h1_tower, d2_tower, p_tower;
    int h1, h2, nb2, lp, loss;
    double mse_scale;                  // 2.0 / rows
    float dq_scale;                    // L1: 1.f / rows
    // read by the weighted instantiations alone, and last, so that every member above keeps its offset
    const float *weight;               // nullptr: every weight is 1
    float *q_out;                      // [towers][rows], or nullptr
    int64_t w_stride;
};

// W: the weighted call.  The dq step is the only place the two forms differ.
template <bool LEAKY, int NB1, bool W>
__global__ __launch_bounds__(WG) void grad_rows(RowArgs a) {
    constexpr int N1 = 16 * NB1, HP = N1 + 4;
    __shared__ float xs[16][IN];
    __shared__ float h1s[16][HP];              // h1 of the block's rows; δ1 at the end
    __shared__ f32x4 red[WAVES][NB1][64];      // each wave's δ1ᵀ accumulators
    __shared__ double qs[WAVES][16];
    __shared__ float ls[16];
    __shared__ float dqs[16];
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c = lane & 15, wave = tid >> 6;
    const int t = blockIdx.y, h1 = a.h1, h2 = a.h2, ld2 = 16 * a.nb2;
    const int64_t row0 = (int64_t)blockIdx.x * 16;
    // tower t's parameters, selected without indexing the argument arrays by a run-time value (that goes to scratch)
    const float *__restrict__ W1 = t ? a.W1[1] : a.W1[0], *__restrict__ b1 = t ? a.b1[1] : a.b1[0];
    const float *__restrict__ W2 = t ? a.W2[1] : a.W2[0], *__restrict__ b2 = t ? a.b2[1] : a.b2[0];
    const float *__restrict__ W3 = t ? a.W3[1] : a.W3[0], *__restrict__ b3 = t ? a.b3[1] : a.b3[0];
    float *H1w = a.h1ws + t * a.h1_tower + row0 * N1;
    float *D2w = a.d2ws + t * a.d2_tower + row0 * ld2;
    double *P = a.pws + t * a.p_tower + (int64_t)blockIdx.x * a.lp;
    const Small sl = small_layout(h1, h2);
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

    // ---- layer 1: h1 into LDS and the workspace, for dW2
    layer1<LEAKY, NB1, IN, WG>(W1, b1, xs, h1s, H1w, h1, row0, a.rows, tid);
    __syncthreads();

    // ---- pass 1: z2 of the wave's unit blocks into the workspace, q folded per lane (in f64: dq is the only per-row value
    // every gradient scales with).  This loop and pass 2's δ1 step are NOT uavx_grad_impl.hpp's z2_block / delta1_block /
    // fold8: they load under a condition, not from a clamped address, run 4 waves and sum the waves' δ1 in f32, and
    // grad_rows<true, 25> sits at 360 VGPRs.  Moving them to the clamped form is an optimisation with a measurement of its
    // own, so the two forms stay apart, with no template switch between them.
    double qp = 0.0;
    for (int jb = wave; jb < a.nb2; jb += WAVES) {
        const int j = 16 * jb + c;             // this lane's A row
        const bool jin = j < h2;
        const float *w2 = W2 + (int64_t)(jin ? j : 0) * h1;
        // each 16-wide k block is a 4-step fmaf chain of its own (rotating over four accumulators so that the MFMAs of
        // neighbouring blocks overlap), added into f64: z2, and with it dq, is rounded once, not once per k step
        f32x4 acc4[4];
        double zd[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kb = 0; kb < NB1; ++kb) {
            const f32x4 hv = *(const f32x4 *)&h1s[c][16 * kb + 4 * g];
            f32x4 &acc = acc4[kb & 3];
            acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ii = 0; ii < 4; ++ii) {
                const int k = 16 * kb + 4 * g + ii;
                acc = mma(jin && (kb < NB1 - 1 || k < h1) ? w2[k] : 0.f, hv[ii], acc);   // h1 > 16·(NB1 − 1)
            }
#pragma unroll
            for (int ii = 0; ii < 4; ++ii) zd[ii] += (double)acc[ii];
        }
        f32x4 z;
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) {
            const int jj = 16 * jb + 4 * g + ii;
            z[ii] = jj < h2 ? (float)(zd[ii] + (double)b2[jj]) : 0.f;
            qp += (double)(jj < h2 ? W3[jj] : 0.f) * (double)act<LEAKY>(z[ii]);
        }
        *(f32x4 *)&D2w[(int64_t)c * ld2 + 16 * jb + 4 * g] = z;
    }
    qp += __shfl_xor(qp, 16);
    qp += __shfl_xor(qp, 32);
    if (g == 0) qs[wave][c] = qp;
    __syncthreads();
    if (tid < 16) {
        const int64_t row = row0 + tid;
        double q = qs[0][tid];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) q += qs[w][tid];
        q += (double)b3[0];
        float dq = 0.f, l = 0.f;
        if constexpr (W) {
            if (row < a.rows) {
                // the weight enters here, once: dq and the loss term are linear in it, everything downstream is in dq
                const float w = a.weight ? a.weight[row * a.w_stride] : 1.f;
                const double dd = q - (double)a.y[row * a.y_stride];
                const float d = (float)dd;
                if (a.loss == UAVX_WCRITIC_MSE) {
                    dq = (float)(((double)w * dd) * a.mse_scale);   // w · (q − y) · (2 / B), rounded once
                    l = (float)((double)w * dd * dd);
                } else {
                    const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);   // torch.sign (0 for 0 and NaN)
                    dq = sg * (w * a.dq_scale);   // w · sign(q − y) · (1 / B)
                    l = w * fabsf(d);
                }
                if (a.q_out) a.q_out[t * a.rows + row] = (float)q;
            }
        } else {
            if (row < a.rows) {
                const double dd = q - (double)a.y[row * a.y_stride];
                const float d = (float)dd;
                if (a.loss == UAVX_CRITIC_GRAD_MSE) {
                    dq = (float)(dd * a.mse_scale);   // mse_loss_backward: (q − y) · (2 / B), rounded once
                    l = (float)(dd * dd);
                } else {
                    const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);   // torch.sign (0 for 0 and NaN)
                    dq = sg * a.dq_scale;         // mean then abs backward: sign(q − y) · (1 / B)
                    l = fabsf(d);
                }
            }
        }
        dqs[tid] = dq;
        ls[tid] = l;
    }
    __syncthreads();
    if (tid == 0) {
        double sd = 0.0, sl2 = 0.0;
        for (int r = 0; r < 16; ++r) {
            sd += dqs[r];
            sl2 += ls[r];
        }
        P[sl.b3] = sd;
        P[sl.loss] = sl2;
    }

    // ---- pass 2: δ2 over the workspace's z2, its column sums (b2) and those of dq·h2 (W3); δ1ᵀ += W2ᵀ·δ2ᵀ
    const float dq = dqs[c];
    f32x4 dacc[NB1];
#pragma unroll
    for (int ib = 0; ib < NB1; ++ib) dacc[ib] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int jb = wave; jb < a.nb2; jb += WAVES) {
        f32x4 *zp = (f32x4 *)&D2w[(int64_t)c * ld2 + 16 * jb + 4 * g];
        const f32x4 z = *zp;
        f32x4 d2;
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) {
            const int jj = 16 * jb + 4 * g + ii;
            const float w3 = jj < h2 ? W3[jj] : 0.f;
            d2[ii] = rin && jj < h2 ? act_bwd<LEAKY>(z[ii], dq * w3) : 0.f;
            const double s2 = sum16(d2[ii]);
            const double s3 = sum16(rin && jj < h2 ? (double)dq * (double)act<LEAKY>(z[ii]) : 0.0);
            if (c == 0 && jj < h2) {
                P[sl.b2 + jj] = s2;
                P[sl.w3 + jj] = s3;
            }
        }
        *zp = d2;
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) {
            const int j = 16 * jb + 4 * g + ii;
            const float *w2 = W2 + (int64_t)(j < h2 ? j : 0) * h1;
#pragma unroll
            for (int ib = 0; ib < NB1; ++ib) {
                const int i = 16 * ib + c;
                dacc[ib] = mma(j < h2 && (ib < NB1 - 1 || i < h1) ? w2[i] : 0.f, d2[ii], dacc[ib]);
            }
        }
    }
#pragma unroll
    for (int ib = 0; ib < NB1; ++ib) red[wave][ib][lane] = dacc[ib];
    __syncthreads();
    // δ1 = (Σ_waves, in wave order) ⊙ act′(z1), over h1 in LDS (h1 > 0 exactly when z1 > 0; a NaN stays a NaN)
    for (int ib = wave; ib < NB1; ib += WAVES) {
        f32x4 s = red[0][ib][lane];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) s += red[w][ib][lane];
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) {
            const int i = 16 * ib + 4 * g + ii;
            const float hv = h1s[c][i];
            h1s[c][i] = rin && i < h1 ? act_bwd<LEAKY>(hv, s[ii]) : 0.f;
        }
    }
    __syncthreads();
    // W1, b1 over the block's 16 rows
    w1b1_tail<WG>(h1s, xs, P, sl.w1, sl.b1, h1, tid);
}

struct CombineArgs {
    const float *part2;
    const double *partp;
    float *grads[12];
    float *loss;
    int64_t rows;
    int h1, h2, lp, towers, S;
};

__global__ __launch_bounds__(WG) void grad_combine(CombineArgs a) {
    const Small sl = small_layout(a.h1, a.h2);
    const int64_t n2 = (int64_t)a.h2 * a.h1, per = n2 + sl.n;
    const int64_t e = (int64_t)blockIdx.x * WG + threadIdx.x;
    if (e >= a.towers * per) return;
    const int t = (int)(e / per);
    int64_t f = e % per;
    double s = 0.0;
    if (f < n2) {
        for (int k = 0; k < a.S; ++k) s += (double)a.part2[((int64_t)k * a.towers + t) * n2 + f];
        a.grads[6 * t + 2][f] = (float)s;
        return;
    }
    f -= n2;
    for (int k = 0; k < a.S; ++k) s += a.partp[((int64_t)k * a.towers + t) * a.lp + f];
    if (f < sl.b1) a.grads[6 * t + 0][f] = (float)s;
    else if (f < sl.b2) a.grads[6 * t + 1][f - sl.b1] = (float)s;
    else if (f < sl.w3) a.grads[6 * t + 3][f - sl.b2] = (float)s;
    else if (f < sl.b3) a.grads[6 * t + 4][f - sl.w3] = (float)s;
    else if (f == sl.b3) a.grads[6 * t + 5][0] = (float)s;
    else a.loss[t] = (float)(s / (double)a.rows);
}

}  // namespace uavx_critic_grad_k

using namespace uavx_critic_grad_k;

namespace {

struct Plan {
    int n1, nb2, lp, tj, ti, pchunks, S;
    int64_t b16, kc, h1_tower, d2_tower, p_tower, off_d2, off_p, off_part2, off_partp, bytes;
};

Plan plan(int nb1, int h1, int h2, int T, int64_t rows) {
    Plan p;
    p.n1 = 16 * nb1;
    p.nb2 = (h2 + 15) / 16;
    p.lp = (small_layout(h1, h2).n + 3) & ~3;
    p.tj = (h2 + 63) / 64;
    p.ti = (h1 + 63) / 64;
    p.pchunks = (p.lp + 255) / 256;
    p.b16 = (rows + 15) / 16 * 16;
    split_k((int64_t)T * p.tj * p.ti, p.b16, &p.kc, &p.S);
    p.h1_tower = p.b16 * p.n1;
    p.d2_tower = p.b16 * 16 * p.nb2;
    p.p_tower = p.b16 / 16 * p.lp;
    p.off_d2 = align256(T * p.h1_tower * 4);
    p.off_p = p.off_d2 + align256(T * p.d2_tower * 4);
    p.off_part2 = p.off_p + align256(T * p.p_tower * 8);
    p.off_partp = p.off_part2 + align256((int64_t)p.S * T * h2 * h1 * 4);
    p.bytes = p.off_partp + align256((int64_t)p.S * T * p.lp * 8);
    return p;
}

typedef void (*rows_fn)(RowArgs);

int check_handle(const uavx_critic *h, int64_t rows) {
    if (!h || rows < 1 || rows > UAVX_CRITIC_GRAD_MAX_ROWS) return UAVX_CRITIC_ERR_INVALID_ARG;
    if (h->prec != UAVX_CRITIC_F32) return UAVX_CRITIC_ERR_UNSUPPORTED;
    if (h->L.nb1 != (h->kind == UAVX_CRITIC_DDPG ? 25 : 16)) return UAVX_CRITIC_ERR_UNSUPPORTED;
    return UAVX_CRITIC_OK;
}

constexpr int MAX_H2 = 1 << 20;    // keeps every int offset of a partial row (13·h1 + 2·h2 + 2) far from overflow

// the weighted call takes no handle: check_handle's limits (the tiles uavx_critic_create accepts) on the dimensions
// themselves -> nb1 through *nb1
int check_dims(int kind, int h1, int h2, int towers, int64_t rows, int *nb1) {
    if (kind != UAVX_WCRITIC_SAC && kind != UAVX_WCRITIC_TD3 && kind != UAVX_WCRITIC_DDPG) return UAVX_WCRITIC_ERR_INVALID_ARG;
    if (rows < 1 || rows > UAVX_WCRITIC_GRAD_MAX_ROWS || towers < 1 || towers > 2 || h2 < 1 || h2 > MAX_H2)
        return UAVX_WCRITIC_ERR_INVALID_ARG;
    *nb1 = kind == UAVX_WCRITIC_DDPG ? 25 : 16;
    if (h1 <= 16 * (*nb1 - 1) || h1 > 16 * *nb1) return UAVX_WCRITIC_ERR_UNSUPPORTED;
    return UAVX_WCRITIC_OK;
}

// the two headers' status codes are uavx_critic.h's values, so launch() serves both entry points
static_assert(UAVX_WCRITIC_OK == UAVX_CRITIC_OK && UAVX_WCRITIC_ERR_INVALID_ARG == UAVX_CRITIC_ERR_INVALID_ARG &&
              UAVX_WCRITIC_ERR_HIP == UAVX_CRITIC_ERR_HIP && UAVX_WCRITIC_ERR_UNSUPPORTED == UAVX_CRITIC_ERR_UNSUPPORTED, "");
static_assert((int)UAVX_WCRITIC_MSE == (int)UAVX_CRITIC_GRAD_MSE && (int)UAVX_WCRITIC_L1 == (int)UAVX_CRITIC_GRAD_L1, "");

// The three launches of both entry points, behind their argument checks.  weighted: the W instantiation of the row pass
// (weight and q_out may each be NULL there); nb1: 25 for the leaky (DDPG) tile, 16 for the relu one.
int launch(bool weighted, int nb1, int h1, int h2, int T, int loss, const float *const *params, const float *state,
           int64_t rows, int64_t s_stride, const float *action, int64_t a_stride, const float *y, int64_t y_stride,
           const float *weight, int64_t w_stride, float *const *grads, float *loss_out, float *q_out, void *workspace,
           int64_t workspace_bytes, void *stream) {
    for (int i = 0; i < 6 * T; ++i)
        if (!params[i] || !grads[i]) return UAVX_CRITIC_ERR_INVALID_ARG;
    const Plan p = plan(nb1, h1, h2, T, rows);
    if (workspace_bytes < p.bytes) return UAVX_CRITIC_ERR_INVALID_ARG;
    char *ws = (char *)workspace;
    const hipStream_t st = (hipStream_t)stream;

    RowArgs ra{};
    for (int t = 0; t < T; ++t) {
        ra.W1[t] = params[6 * t + 0];
        ra.b1[t] = params[6 * t + 1];
        ra.W2[t] = params[6 * t + 2];
        ra.b2[t] = params[6 * t + 3];
        ra.W3[t] = params[6 * t + 4];
        ra.b3[t] = params[6 * t + 5];
    }
    ra.state = state;
    ra.action = action;
    ra.y = y;
    ra.rows = rows;
    ra.s_stride = s_stride;
    ra.a_stride = a_stride;
    ra.y_stride = y_stride;
    ra.h1ws = (float *)ws;
    ra.d2ws = (float *)(ws + p.off_d2);
    ra.pws = (double *)(ws + p.off_p);
    ra.h1_tower = p.h1_tower;
    ra.d2_tower = p.d2_tower;
    ra.p_tower = p.p_tower;
    ra.h1 = h1;
    ra.h2 = h2;
    ra.nb2 = p.nb2;
    ra.lp = p.lp;
    ra.loss = loss;
    ra.mse_scale = 2.0 / (double)rows;
    ra.dq_scale = 1.f / (float)rows;
    ra.weight = weight;
    ra.q_out = q_out;
    ra.w_stride = weight ? w_stride : 0;
    const rows_fn fr = nb1 == 25 ? (weighted ? grad_rows<true, 25, true> : grad_rows<true, 25, false>)
                                 : (weighted ? grad_rows<false, 16, true> : grad_rows<false, 16, false>);
    hipLaunchKernelGGL(fr, dim3((unsigned)(p.b16 / 16), (unsigned)T), dim3(WG), 0, st, ra);
    if (hipGetLastError() != hipSuccess) return UAVX_CRITIC_ERR_HIP;

    WeightArgs wa{};
    wa.h1ws = ra.h1ws;
    wa.d2ws = ra.d2ws;
    wa.pws = ra.pws;
    wa.h1_tower = p.h1_tower;
    wa.d2_tower = p.d2_tower;
    wa.p_tower = p.p_tower;
    wa.part2 = (float *)(ws + p.off_part2);
    wa.partp = (double *)(ws + p.off_partp);
    wa.b16 = p.b16;
    wa.kc = p.kc;
    wa.h1 = h1;
    wa.n1 = p.n1;
    wa.h2 = h2;
    wa.nb2 = p.nb2;
    wa.lp = p.lp;
    wa.towers = T;
    wa.S = p.S;
    wa.tj = p.tj;
    wa.ti = p.ti;
    wa.pchunks = p.pchunks;
    if (!launch_grad_weights(wa, st)) return UAVX_CRITIC_ERR_HIP;

    CombineArgs ca{};
    ca.part2 = wa.part2;
    ca.partp = wa.partp;
    for (int i = 0; i < 6 * T; ++i) ca.grads[i] = grads[i];
    ca.loss = loss_out;
    ca.rows = rows;
    ca.h1 = h1;
    ca.h2 = h2;
    ca.lp = p.lp;
    ca.towers = T;
    ca.S = p.S;
    const int64_t n = (int64_t)T * ((int64_t)h2 * h1 + small_layout(h1, h2).n);
    hipLaunchKernelGGL(grad_combine, dim3((unsigned)((n + WG - 1) / WG)), dim3(WG), 0, st, ca);
    return hipGetLastError() == hipSuccess ? UAVX_CRITIC_OK : UAVX_CRITIC_ERR_HIP;
}

}  // namespace

extern "C" {

int uavx_critic_grad_version(void) { return UAVX_CRITIC_GRAD_VERSION; }

int uavx_critic_grad_workspace_bytes(const uavx_critic *h, int64_t rows, int64_t *bytes) {
    if (!bytes) return UAVX_CRITIC_ERR_INVALID_ARG;
    *bytes = 0;
    const int rc = check_handle(h, rows);
    if (rc != UAVX_CRITIC_OK) return rc;
    *bytes = plan(h->L.nb1, h->h1, h->h2, h->towers, rows).bytes;
    return UAVX_CRITIC_OK;
}

int uavx_critic_grad(const uavx_critic *h, int loss, const float *const *params, const float *state, int64_t rows,
                     int64_t s_stride, const float *action, int64_t a_stride, const float *y, int64_t y_stride,
                     float *const *grads, float *loss_out, void *workspace, int64_t workspace_bytes, void *stream) {
    if (!h || !params || !grads || rows < 1 || s_stride < OBS || a_stride < 2 || y_stride < 1)
        return UAVX_CRITIC_ERR_INVALID_ARG;
    if (loss != UAVX_CRITIC_GRAD_MSE && loss != UAVX_CRITIC_GRAD_L1) return UAVX_CRITIC_ERR_INVALID_ARG;
    if (!state || !action || !y || !loss_out || !workspace || ((uintptr_t)workspace & 15)) return UAVX_CRITIC_ERR_INVALID_ARG;
    const int rc = check_handle(h, rows);
    if (rc != UAVX_CRITIC_OK) return rc;
    return launch(false, h->L.nb1, h->h1, h->h2, h->towers, loss, params, state, rows, s_stride, action, a_stride, y, y_stride,
                  nullptr, 0, grads, loss_out, nullptr, workspace, workspace_bytes, stream);
}

int uavx_wcritic_grad_version(void) { return UAVX_WCRITIC_GRAD_VERSION; }

int uavx_wcritic_grad_workspace_bytes(int kind, int h1, int h2, int towers, int64_t rows, int64_t *bytes) {
    if (!bytes) return UAVX_WCRITIC_ERR_INVALID_ARG;
    *bytes = 0;
    int nb1 = 0;
    const int rc = check_dims(kind, h1, h2, towers, rows, &nb1);
    if (rc != UAVX_WCRITIC_OK) return rc;
    *bytes = plan(nb1, h1, h2, towers, rows).bytes;
    return UAVX_WCRITIC_OK;
}

int uavx_wcritic_grad(int kind, int h1, int h2, int towers, int loss, const float *const *params, const float *state,
                      int64_t rows, int64_t s_stride, const float *action, int64_t a_stride, const float *y,
                      int64_t y_stride, const float *weight, int64_t w_stride, float *const *grads, float *loss_out,
                      float *q_out, void *workspace, int64_t workspace_bytes, void *stream) {
    if (!params || !grads || rows < 1 || s_stride < OBS || a_stride < 2 || y_stride < 1) return UAVX_WCRITIC_ERR_INVALID_ARG;
    if (weight && w_stride < 1) return UAVX_WCRITIC_ERR_INVALID_ARG;
    if (loss != UAVX_WCRITIC_MSE && loss != UAVX_WCRITIC_L1) return UAVX_WCRITIC_ERR_INVALID_ARG;
    if (!state || !action || !y || !loss_out || !workspace || ((uintptr_t)workspace & 15)) return UAVX_WCRITIC_ERR_INVALID_ARG;
    int nb1 = 0;
    const int rc = check_dims(kind, h1, h2, towers, rows, &nb1);
    if (rc != UAVX_WCRITIC_OK) return rc;
    return launch(true, nb1, h1, h2, towers, loss, params, state, rows, s_stride, action, a_stride, y, y_stride, weight,
                  w_stride, grads, loss_out, q_out, workspace, workspace_bytes, stream);
}

}  // extern "C"

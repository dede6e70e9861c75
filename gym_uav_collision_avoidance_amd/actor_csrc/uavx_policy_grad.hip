// Actor forward and backward of the learners' actor update (include/uavx_policy_grad.h): the action (and SAC's logπ)
// from the actor's live parameters, and, once the critic's q and ∂q/∂a are known, every actor parameter's gradient, the
// loss and SAC's mean logπ.  Four launches of this unit around the one of uavx_action_grad.  DESIGN.md §18.
//
// The lane layout of the MFMA products, layer 1, the z2 chain and the δ1 step of a unit block, the eight-wave fold, the
// W1 / b1 tail, the small helpers and the weights launch are shared with the other gradient units: uavx_grad_impl.hpp.
//
//   1. policy_fwd      one workgroup of 8 waves per 16-row block; rows are MFMA columns, units MFMA rows.  Layer 1 (f64,
//                      rounded once) into LDS and to the workspace, for dW2; z2ᵀ = W2·h1ᵀ with wave w taking the 16-unit
//                      blocks j ≡ w (mod 8), each 16-wide k block's MFMA chain added up in f64, z2 written to the
//                      workspace; the O head rows folded over act(z2) per lane in f64 and summed over the waves in wave
//                      order; the epilogue (f64 exp / tanh / log on two values a row) writes the action, SAC's logπ and
//                      the row's head record: 2y(1−y²)/(1−y²+1e-6), 1−y², σε, the clamp mask and logπ.
//   3. policy_bwd      the same grid.  δ3 per row (f64) from the head record, q, ∂q/∂a and α; per unit block
//                      δ2 = (W3ᵀδ3) ⊙ act′(z2) over z2 in the workspace (overwritten by δ2), and δ1ᵀ += W2ᵀ·δ2ᵀ straight
//                      from the δ2 accumulator (its k order is the unit order of the block).  The eight waves' δ1ᵀ are
//                      summed through LDS in a fixed order, (w + (w+4)) for w = 0..3 in f32 and those four in wave order
//                      in f64.  The block's sums over its 16 rows of the small gradients (W1, b1, b2, W3, b3), of the
//                      loss and of logπ go to a per-block partial row (f64).
//   4. uavx_grad_k::grad_weights (uavx_grad_common.hip), one tower  dW2 per split-K slice of rows and the partial rows
//                      per slice.
//   5. policy_combine  one thread per output element: the split-K slices summed in slice order (f64), rounded once to f32
//                      and written in torch layout; the loss and logπ sums divided by the row count.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/uavx_policy_grad.h"
#include "uavx_grad_impl.hpp"

namespace uavx_policy_grad_k {

using namespace uavx_grad_k;

constexpr int OBS = 10, WG = 512, WAVES = WG / 64, REC = 8, CWG = 256;   // CWG: the combine kernel's workgroup
// a row's head record in the workspace
constexpr int R_T = 0, R_U = 2, R_SE = 4, R_MASK = 6, R_LOGPI = 7;

// offsets inside a per-block partial row (and inside the small-gradient slices): W1 [h1][10], b1, b2, W3 [O][h2], b3 [O],
// loss, Σ logπ
struct Small {
    int w1, b1, b2, w3, b3, loss, logpi, n;
};
__host__ __device__ inline Small small_layout(int h1, int h2, int O) {
    Small s;
    s.w1 = 0;
    s.b1 = OBS * h1;
    s.b2 = s.b1 + h1;
    s.w3 = s.b2 + h2;
    s.b3 = s.w3 + O * h2;
    s.loss = s.b3 + O;
    s.logpi = s.loss + 1;
    s.n = s.logpi + 1;
    return s;
}

struct FwdArgs {
    const float *W1, *b1, *W2, *b2, *W3, *b3, *W3b, *b3b;
    const float *state, *eps;
    float *action, *log_pi;
    float *h1ws, *z2ws, *rec;
    int64_t rows, s_stride;
    int h1, h2, nb2, sac;
};

template <bool LEAKY, int NB1>
__global__ __launch_bounds__(WG) void policy_fwd(FwdArgs a) {
    constexpr int N1 = 16 * NB1, HP = N1 + 4;
    __shared__ float xs[16][OBS];
    __shared__ __attribute__((aligned(16))) float h1s[16][HP];   // h1 of the block's rows (read as f32x4)
    __shared__ double hs[WAVES][16][4];
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c = lane & 15, wave = tid >> 6;
    const int h1 = a.h1, h2 = a.h2, ld2 = 16 * a.nb2;
    const bool sac = a.sac != 0;
    const int64_t row0 = (int64_t)blockIdx.x * 16;
    const float *__restrict__ W1 = a.W1, *__restrict__ b1 = a.b1, *__restrict__ W2 = a.W2, *__restrict__ b2 = a.b2;
    // the four head rows; TD3 / DDPG have two, and rows 2 and 3 then alias row 0 so that every load stays unconditional
    const float *__restrict__ Wh0 = a.W3, *__restrict__ Wh1 = a.W3 + h2;
    const float *__restrict__ Wh2 = sac ? a.W3b : a.W3, *__restrict__ Wh3 = sac ? a.W3b + h2 : a.W3;
    float *H1w = a.h1ws + row0 * N1;
    float *Z2w = a.z2ws + row0 * ld2;

    // ---- state of the block's rows (0 past the last row: nothing there is read)
    if (tid < 16 * OBS) {
        const int r = tid / OBS, k = tid % OBS;
        const int64_t row = row0 + r;
        xs[r][k] = row < a.rows ? a.state[row * a.s_stride + k] : 0.f;
    }
    __syncthreads();

    // ---- layer 1: h1 into LDS and the workspace, for dW2
    layer1<LEAKY, NB1, OBS, WG>(W1, b1, xs, h1s, H1w, h1, row0, a.rows, tid);
    __syncthreads();

    // ---- the sweep over W2: z2 of the wave's unit blocks into the workspace, the head rows folded per lane in f64
    double hp0 = 0.0, hp1 = 0.0, hp2 = 0.0, hp3 = 0.0;
    for (int jb = wave; jb < a.nb2; jb += WAVES) {
        const int j = 16 * jb + c;             // this lane's A row
        const bool jin = j < h2;
        const float *w2 = W2 + (int64_t)(jin ? j : 0) * h1;
        double zd[4];
        z2_block<NB1, (NB1 > 16)>(w2, jin, h1, h1s, g, c, zd);   // the 25-block tile spills without the barrier
        f32x4 z;
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) {
            const int jj = 16 * jb + 4 * g + ii;
            const bool in = jj < h2;
            const int jc = in ? jj : 0;
            z[ii] = in ? (float)(zd[ii] + (double)b2[jc]) : 0.f;
            const double hv2 = in ? (double)act<LEAKY>(z[ii]) : 0.0;
            const float w0 = Wh0[jc], w1 = Wh1[jc], w2h = Wh2[jc], w3h = Wh3[jc];
            hp0 += (double)(in ? w0 : 0.f) * hv2;
            hp1 += (double)(in ? w1 : 0.f) * hv2;
            hp2 += (double)(in ? w2h : 0.f) * hv2;
            hp3 += (double)(in ? w3h : 0.f) * hv2;
        }
        *(f32x4 *)&Z2w[(int64_t)c * ld2 + 16 * jb + 4 * g] = z;
    }
    hp0 += __shfl_xor(hp0, 16);
    hp0 += __shfl_xor(hp0, 32);
    hp1 += __shfl_xor(hp1, 16);
    hp1 += __shfl_xor(hp1, 32);
    hp2 += __shfl_xor(hp2, 16);
    hp2 += __shfl_xor(hp2, 32);
    hp3 += __shfl_xor(hp3, 16);
    hp3 += __shfl_xor(hp3, 32);
    if (g == 0) {
        hs[wave][c][0] = hp0;
        hs[wave][c][1] = hp1;
        hs[wave][c][2] = hp2;
        hs[wave][c][3] = hp3;
    }
    __syncthreads();

    // ---- the head of one row per thread: the waves' partial sums in wave order, then the epilogue in f64
    if (tid < 16) {
        const int64_t row = row0 + tid;
        float *rec = a.rec + row * REC;
        float rv[REC] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (row < a.rows) {
            double p[4];
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                double s = hs[0][tid][o];
#pragma unroll
                for (int w = 1; w < WAVES; ++w) s += hs[w][tid][o];
                p[o] = s;
            }
            if (!sac) {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const double y = tanh(p[j] + (double)a.b3[j]);
                    a.action[row * 2 + j] = (float)y;
                    rv[R_U + j] = (float)(1.0 - y * y);
                }
            } else {
                double lp = 0.0;
                int mask = 0;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const double mu = p[j] + (double)a.b3[j], raw = p[2 + j] + (double)a.b3b[j];
                    const float rf = (float)raw;                      // the clamp's gradient passes at equality
                    if (rf >= -20.f && rf <= 2.f) mask |= 1 << j;
                    const double l = raw < -20.0 ? -20.0 : (raw > 2.0 ? 2.0 : raw);   // NaN stays NaN
                    const double e = (double)a.eps[row * 2 + j];
                    const double se = exp(l) * e;
                    const double y = tanh(mu + se), u = 1.0 - y * y;
                    lp += ((-0.5 * e * e - l) - 0.91893853320467274178) - log(u + 1e-6);
                    a.action[row * 2 + j] = (float)y;
                    rv[R_T + j] = (float)(2.0 * y * u / (u + 1e-6));
                    rv[R_U + j] = (float)u;
                    rv[R_SE + j] = (float)se;
                }
                rv[R_MASK] = (float)mask;
                rv[R_LOGPI] = (float)lp;
                a.log_pi[row] = (float)lp;
            }
        }
#pragma unroll
        for (int k = 0; k < REC; ++k) rec[k] = rv[k];
    }
}

struct BwdArgs {
    const float *W2, *W3, *W3b;
    const float *state, *q, *dqda, *alpha_dev;
    const float *h1ws, *rec;
    float *d2ws;
    double *pws;
    int64_t rows, s_stride, qts;
    int h1, h2, nb2, lp, sac;
    float alpha;
};

template <bool LEAKY, int NB1>
__global__ __launch_bounds__(WG) void policy_bwd(BwdArgs a) {
    constexpr int N1 = 16 * NB1, HP = N1 + 4;
    __shared__ float xs[16][OBS];
    __shared__ float h1s[16][HP];              // h1 of the block's rows; δ1 at the end
    __shared__ f32x4 red[4][NB1][64];          // δ1ᵀ accumulators: waves 4..7, then (w + (w+4)) of waves 0..3
    __shared__ double d3s[16][4];
    __shared__ double ls[16], lps[16];
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c = lane & 15, wave = tid >> 6;
    const int h1 = a.h1, h2 = a.h2, ld2 = 16 * a.nb2;
    const bool sac = a.sac != 0;
    const int O = sac ? 4 : 2;
    const int64_t row0 = (int64_t)blockIdx.x * 16;
    const float *__restrict__ W2 = a.W2;
    const float *__restrict__ Wh0 = a.W3, *__restrict__ Wh1 = a.W3 + h2;
    const float *__restrict__ Wh2 = sac ? a.W3b : a.W3, *__restrict__ Wh3 = sac ? a.W3b + h2 : a.W3;
    const float *H1w = a.h1ws + row0 * N1;
    float *D2w = a.d2ws + row0 * ld2;
    double *P = a.pws + (int64_t)blockIdx.x * a.lp;
    const Small sl = small_layout(h1, h2, O);
    const bool rin = row0 + c < a.rows;        // row c of the block is a real row

    // ---- state and h1 of the block's rows, and δ3 of one row per thread of the last wave
    if (tid < 16 * OBS) {
        const int r = tid / OBS, k = tid % OBS;
        const int64_t row = row0 + r;
        xs[r][k] = row < a.rows ? a.state[row * a.s_stride + k] : 0.f;
    }
    for (int e = tid; e < 16 * N1; e += WG) h1s[e / N1][e % N1] = H1w[e];
    if (tid >= WG - 16) {
        const int r = tid - (WG - 16);
        const int64_t row = row0 + r;
        double d[4] = {0.0, 0.0, 0.0, 0.0}, l = 0.0, lp = 0.0;
        if (row < a.rows) {
            const float *rec = a.rec + row * REC;
            const double B = (double)a.rows;
            if (!sac) {
#pragma unroll
                for (int j = 0; j < 2; ++j) d[j] = -(double)a.dqda[row * 2 + j] * (double)rec[R_U + j] / B;
                l = -(double)a.q[row];
            } else {
                const double al = a.alpha_dev ? (double)*a.alpha_dev : (double)a.alpha;
                const float q1 = a.q[row], q2 = a.q[a.qts + row];
                const double w = q1 < q2 ? 1.0 : (q1 > q2 ? 0.0 : 0.5);     // torch.minimum's backward
                const int mask = (int)rec[R_MASK];
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const double J = w * (double)a.dqda[row * 2 + j] + (1.0 - w) * (double)a.dqda[(a.qts + row) * 2 + j];
                    const double gx = (al * (double)rec[R_T + j] - J * (double)rec[R_U + j]) / B;
                    d[j] = gx;
                    d[2 + j] = mask >> j & 1 ? -al / B + gx * (double)rec[R_SE + j] : 0.0;
                }
                lp = (double)rec[R_LOGPI];
                l = al * lp - (double)(q1 < q2 || q1 != q1 ? q1 : q2);      // a NaN passes like torch.min
            }
        }
#pragma unroll
        for (int o = 0; o < 4; ++o) d3s[r][o] = d[o];
        ls[r] = l;
        lps[r] = lp;
    }
    __syncthreads();
    if (tid < 6) {                             // b3 [O], the loss and logπ over the block's rows, in row order
        double s = 0.0;
        for (int r = 0; r < 16; ++r) s += tid < 4 ? d3s[r][tid] : (tid == 4 ? ls[r] : lps[r]);
        if (tid < O) P[sl.b3 + tid] = s;
        else if (tid == 4) P[sl.loss] = s;
        else if (tid == 5) P[sl.logpi] = s;
    }

    // ---- δ2 over the workspace's z2, its column sums (b2) and those of δ3·h2 (W3); δ1ᵀ += W2ᵀ·δ2ᵀ
    const double d30 = d3s[c][0], d31 = d3s[c][1], d32 = d3s[c][2], d33 = d3s[c][3];
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
            const bool in = jj < h2, on = rin && in;
            const int jc = in ? jj : 0;
            const float w0 = Wh0[jc], w1 = Wh1[jc], w2h = Wh2[jc], w3h = Wh3[jc];
            double up = (double)w0 * d30 + (double)w1 * d31;
            if (sac) up = (up + (double)w2h * d32) + (double)w3h * d33;
            d2[ii] = on ? (float)act_bwd<LEAKY>(z[ii], up) : 0.f;
            const double hv2 = on ? (double)act<LEAKY>(z[ii]) : 0.0;
            const double s2 = sum16((double)d2[ii]);
            const double s30 = sum16(d30 * hv2), s31 = sum16(d31 * hv2);
            if (c == 0 && in) {
                P[sl.b2 + jj] = s2;
                P[sl.w3 + jj] = s30;
                P[sl.w3 + h2 + jj] = s31;
            }
            if (sac) {
                const double s32 = sum16(d32 * hv2), s33 = sum16(d33 * hv2);
                if (c == 0 && in) {
                    P[sl.w3 + 2 * h2 + jj] = s32;
                    P[sl.w3 + 3 * h2 + jj] = s33;
                }
            }
        }
        *zp = d2;
        delta1_block<NB1>(W2, jb, h1, h2, d2, g, c, dacc);
    }

    // ---- δ1ᵀ over the waves: (w + (w+4)) for w = 0..3 in LDS, then
    // δ1 = (the four sums in wave order, f64) ⊙ act′(z1), over h1 in LDS (h1 > 0 exactly when z1 > 0; a NaN stays a NaN)
    fold8<NB1>(red, dacc, wave, lane);
    for (int ib = wave; ib < NB1; ib += WAVES) {
        const f32x4 r0 = red[0][ib][lane], r1 = red[1][ib][lane], r2 = red[2][ib][lane], r3 = red[3][ib][lane];
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) {
            const int i = 16 * ib + 4 * g + ii;
            const double s = (((double)r0[ii] + (double)r1[ii]) + (double)r2[ii]) + (double)r3[ii];
            const float hv = h1s[c][i];
            h1s[c][i] = rin && i < h1 ? (float)act_bwd<LEAKY>(hv, s) : 0.f;
        }
    }
    __syncthreads();
    // W1, b1 over the block's 16 rows
    w1b1_tail<WG>(h1s, xs, P, sl.w1, sl.b1, h1, tid);
}

struct CombineArgs {
    const float *part2;
    const double *partp;
    float *gW1, *gb1, *gW2, *gb2, *gW3, *gb3, *gW3b, *gb3b;
    float *loss, *log_pi_mean;
    int64_t rows;
    int h1, h2, lp, S, O;
};

__global__ __launch_bounds__(CWG) void policy_combine(CombineArgs a) {
    const Small sl = small_layout(a.h1, a.h2, a.O);
    const int64_t n2 = (int64_t)a.h2 * a.h1;
    const int64_t e = (int64_t)blockIdx.x * CWG + threadIdx.x;
    if (e >= n2 + sl.n) return;
    double s = 0.0;
    if (e < n2) {
        for (int k = 0; k < a.S; ++k) s += (double)a.part2[(int64_t)k * n2 + e];
        a.gW2[e] = (float)s;
        return;
    }
    const int f = (int)(e - n2);
    for (int k = 0; k < a.S; ++k) s += a.partp[(int64_t)k * a.lp + f];
    if (f < sl.b1) a.gW1[f] = (float)s;
    else if (f < sl.b2) a.gb1[f - sl.b1] = (float)s;
    else if (f < sl.w3) a.gb2[f - sl.b2] = (float)s;
    else if (f < sl.b3) {
        const int k = f - sl.w3;
        if (k < 2 * a.h2) a.gW3[k] = (float)s;
        else a.gW3b[k - 2 * a.h2] = (float)s;
    } else if (f < sl.loss) {
        const int o = f - sl.b3;
        if (o < 2) a.gb3[o] = (float)s;
        else a.gb3b[o - 2] = (float)s;
    } else if (f == sl.loss) a.loss[0] = (float)(s / (double)a.rows);
    else if (a.O == 4) a.log_pi_mean[0] = (float)(s / (double)a.rows);
}

}  // namespace uavx_policy_grad_k

using namespace uavx_policy_grad_k;

namespace {

struct Plan {
    int n1, nb2, O, lp, tj, ti, pchunks, S;
    int64_t b16, kc, off_z2, off_rec, off_p, off_part2, off_partp, bytes;
};

Plan plan(int kind, int h1, int h2, int64_t rows) {
    Plan p;
    p.n1 = (h1 + 15) / 16 * 16;
    p.nb2 = (h2 + 15) / 16;
    p.O = kind == UAVX_ACTOR_SAC ? 4 : 2;
    p.lp = (small_layout(h1, h2, p.O).n + 3) & ~3;
    p.tj = (h2 + 63) / 64;
    p.ti = (h1 + 63) / 64;
    p.pchunks = (p.lp + 255) / 256;
    p.b16 = (rows + 15) / 16 * 16;
    split_k((int64_t)p.tj * p.ti, p.b16, &p.kc, &p.S);
    p.off_z2 = align256(p.b16 * p.n1 * 4);
    p.off_rec = p.off_z2 + align256(p.b16 * 16 * p.nb2 * 4);
    p.off_p = p.off_rec + align256(p.b16 * REC * 4);
    p.off_part2 = p.off_p + align256(p.b16 / 16 * p.lp * 8);
    p.off_partp = p.off_part2 + align256((int64_t)p.S * h2 * h1 * 4);
    p.bytes = p.off_partp + align256((int64_t)p.S * p.lp * 8);
    return p;
}

int check_dims(int kind, int h1, int h2, int64_t rows) {
    if (kind < UAVX_ACTOR_SAC || kind > UAVX_ACTOR_DDPG || h1 < 1 || h2 < 1) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (rows < 1 || rows > UAVX_POLICY_GRAD_MAX_ROWS) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (!uavx_actor_k::hidden_supported(kind, h1, h2)) return UAVX_ACTOR_ERR_UNSUPPORTED;
    return UAVX_ACTOR_OK;
}

// the pointers of `list` the learner uses: six, and SAC's two more
bool all_set(const void *const *list, int kind) {
    const int n = kind == UAVX_ACTOR_SAC ? 8 : 6;
    for (int i = 0; i < n; ++i)
        if (!list[i]) return false;
    return true;
}

}  // namespace

extern "C" {

int uavx_policy_grad_version(void) { return UAVX_POLICY_GRAD_VERSION; }

int uavx_policy_grad_workspace_bytes(int kind, int hidden1, int hidden2, int64_t rows, int64_t *bytes) {
    if (!bytes) return UAVX_ACTOR_ERR_INVALID_ARG;
    *bytes = 0;
    const int rc = check_dims(kind, hidden1, hidden2, rows);
    if (rc != UAVX_ACTOR_OK) return rc;
    *bytes = plan(kind, hidden1, hidden2, rows).bytes;
    return UAVX_ACTOR_OK;
}

int uavx_policy_grad_forward(int kind, int hidden1, int hidden2, const float *const *params, const float *state,
                             int64_t rows, int64_t s_stride, const float *eps, float *action, float *log_pi,
                             void *workspace, int64_t workspace_bytes, void *stream) {
    if (!params || !state || !action || !workspace || ((uintptr_t)workspace & 15) || s_stride < OBS)
        return UAVX_ACTOR_ERR_INVALID_ARG;
    const int rc = check_dims(kind, hidden1, hidden2, rows);
    if (rc != UAVX_ACTOR_OK) return rc;
    if (!all_set((const void *const *)params, kind)) return UAVX_ACTOR_ERR_INVALID_ARG;
    const bool sac = kind == UAVX_ACTOR_SAC;
    if (sac && (!eps || !log_pi)) return UAVX_ACTOR_ERR_INVALID_ARG;
    const Plan p = plan(kind, hidden1, hidden2, rows);
    if (workspace_bytes < p.bytes) return UAVX_ACTOR_ERR_INVALID_ARG;
    char *ws = (char *)workspace;

    FwdArgs fa{};
    fa.W1 = params[0];
    fa.b1 = params[1];
    fa.W2 = params[2];
    fa.b2 = params[3];
    fa.W3 = params[4];
    fa.b3 = params[5];
    fa.W3b = sac ? params[6] : nullptr;
    fa.b3b = sac ? params[7] : nullptr;
    fa.state = state;
    fa.eps = sac ? eps : nullptr;
    fa.action = action;
    fa.log_pi = sac ? log_pi : nullptr;
    fa.h1ws = (float *)ws;
    fa.z2ws = (float *)(ws + p.off_z2);
    fa.rec = (float *)(ws + p.off_rec);
    fa.rows = rows;
    fa.s_stride = s_stride;
    fa.h1 = hidden1;
    fa.h2 = hidden2;
    fa.nb2 = p.nb2;
    fa.sac = sac;
    void (*fn)(FwdArgs) = kind == UAVX_ACTOR_DDPG ? policy_fwd<true, 25> : policy_fwd<false, 16>;
    hipLaunchKernelGGL(fn, dim3((unsigned)(p.b16 / 16)), dim3(WG), 0, (hipStream_t)stream, fa);
    return hipGetLastError() == hipSuccess ? UAVX_ACTOR_OK : UAVX_ACTOR_ERR_HIP;
}

int uavx_policy_grad_backward(int kind, int hidden1, int hidden2, const float *const *params, const float *state,
                              int64_t rows, int64_t s_stride, const float *q, const float *dqda, int64_t q_tower_stride,
                              float alpha, const float *alpha_dev, float *const *grads, float *loss_out,
                              float *log_pi_mean_out, void *workspace, int64_t workspace_bytes, void *stream) {
    if (!params || !grads || !state || !q || !dqda || !loss_out || !workspace || ((uintptr_t)workspace & 15) ||
        s_stride < OBS)
        return UAVX_ACTOR_ERR_INVALID_ARG;
    const int rc = check_dims(kind, hidden1, hidden2, rows);
    if (rc != UAVX_ACTOR_OK) return rc;
    if (q_tower_stride < rows) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (!all_set((const void *const *)params, kind) || !all_set((const void *const *)grads, kind))
        return UAVX_ACTOR_ERR_INVALID_ARG;
    const bool sac = kind == UAVX_ACTOR_SAC;
    if (sac && !log_pi_mean_out) return UAVX_ACTOR_ERR_INVALID_ARG;
    const Plan p = plan(kind, hidden1, hidden2, rows);
    if (workspace_bytes < p.bytes) return UAVX_ACTOR_ERR_INVALID_ARG;
    char *ws = (char *)workspace;
    const hipStream_t st = (hipStream_t)stream;

    BwdArgs ba{};
    ba.W2 = params[2];
    ba.W3 = params[4];
    ba.W3b = sac ? params[6] : nullptr;
    ba.state = state;
    ba.q = q;
    ba.dqda = dqda;
    ba.alpha_dev = sac ? alpha_dev : nullptr;
    ba.h1ws = (const float *)ws;
    ba.d2ws = (float *)(ws + p.off_z2);
    ba.rec = (const float *)(ws + p.off_rec);
    ba.pws = (double *)(ws + p.off_p);
    ba.rows = rows;
    ba.s_stride = s_stride;
    ba.qts = q_tower_stride;
    ba.h1 = hidden1;
    ba.h2 = hidden2;
    ba.nb2 = p.nb2;
    ba.lp = p.lp;
    ba.sac = sac;
    ba.alpha = alpha;
    void (*fb)(BwdArgs) = kind == UAVX_ACTOR_DDPG ? policy_bwd<true, 25> : policy_bwd<false, 16>;
    hipLaunchKernelGGL(fb, dim3((unsigned)(p.b16 / 16)), dim3(WG), 0, st, ba);
    if (hipGetLastError() != hipSuccess) return UAVX_ACTOR_ERR_HIP;

    WeightArgs wa{};                           // one tower: the tower strides stay 0
    wa.h1ws = ba.h1ws;
    wa.d2ws = ba.d2ws;
    wa.pws = ba.pws;
    wa.part2 = (float *)(ws + p.off_part2);
    wa.partp = (double *)(ws + p.off_partp);
    wa.b16 = p.b16;
    wa.kc = p.kc;
    wa.h1 = hidden1;
    wa.n1 = p.n1;
    wa.h2 = hidden2;
    wa.nb2 = p.nb2;
    wa.lp = p.lp;
    wa.towers = 1;
    wa.S = p.S;
    wa.tj = p.tj;
    wa.ti = p.ti;
    wa.pchunks = p.pchunks;
    if (!launch_grad_weights(wa, st)) return UAVX_ACTOR_ERR_HIP;

    CombineArgs ca{};
    ca.part2 = wa.part2;
    ca.partp = wa.partp;
    ca.gW1 = grads[0];
    ca.gb1 = grads[1];
    ca.gW2 = grads[2];
    ca.gb2 = grads[3];
    ca.gW3 = grads[4];
    ca.gb3 = grads[5];
    ca.gW3b = sac ? grads[6] : nullptr;
    ca.gb3b = sac ? grads[7] : nullptr;
    ca.loss = loss_out;
    ca.log_pi_mean = sac ? log_pi_mean_out : nullptr;
    ca.rows = rows;
    ca.h1 = hidden1;
    ca.h2 = hidden2;
    ca.lp = p.lp;
    ca.S = p.S;
    ca.O = p.O;
    const int64_t n = (int64_t)hidden2 * hidden1 + small_layout(hidden1, hidden2, p.O).n;
    hipLaunchKernelGGL(policy_combine, dim3((unsigned)((n + CWG - 1) / CWG)), dim3(CWG), 0, st, ca);
    return hipGetLastError() == hipSuccess ? UAVX_ACTOR_OK : UAVX_ACTOR_ERR_HIP;
}

}  // extern "C"

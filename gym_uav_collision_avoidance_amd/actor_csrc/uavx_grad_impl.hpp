// Pieces shared by the gradient translation units of libuavx_actor.so: uavx_critic_grad.hip,
// uavx_action_grad.hip (§17), uavx_policy_grad.hip (§18) and uavx_grad_common.hip, which holds the one dW2 weights kernel.
// Every piece here is the only definition of a summation order the units' bit-level contracts rest on.
//
// All products run on v_mfma_f32_16x16x4_f32 (exact f32, a k-ordered fmaf chain).  Lane l = 16·g + c of a wave holds
// A[m = c][k = g] and B[k = g][n = c]; the accumulator element ii holds C[m = 4g + ii][n = c].  A row kernel takes one
// 16-row block: rows are MFMA columns, units MFMA rows, and h1 of the block's rows lies in LDS as h1s[16][16·NB1 + 4].
//
// What is NOT here: the z2 and δ1 loops of grad_rows (uavx_critic_grad.hip), which load under a condition instead of from
// a clamped address, run 4 waves and sum the waves' δ1 in f32.  See the comment there.
#pragma once
#include <type_traits>
#include "uavx_actor_impl.hpp"

namespace uavx_grad_k {

using uavx_actor_k::act;
using uavx_actor_k::f32x4;

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

// sum over the 16 lanes of a lane group (c = lane & 15) by butterfly: every lane ends with the same bits
__device__ inline double sum16(double v) {
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

// layer 1 of the block's 16 rows over the inputs xs (IN wide): h1 into LDS and, when there is one, the workspace H1w (a
// float *, or nullptr itself: known when compiling, not tested when running); 0 for padded units and padded rows
template <bool LEAKY, int NB1, int IN, int WG, typename WS>
__device__ __forceinline__ void layer1(const float *W1, const float *b1, const float (&xs)[16][IN],
                                       float (&h1s)[16][16 * NB1 + 4], WS H1w, int h1, int64_t row0, int64_t rows, int tid) {
    constexpr int N1 = 16 * NB1;
    for (int e = tid; e < 16 * N1; e += WG) {
        const int r = e / N1, i = e % N1;
        float h = 0.f;
        if (i < h1 && row0 + r < rows) {
            double z = b1[i];                  // in f64, rounded once
#pragma unroll
            for (int k = 0; k < IN; ++k) z += (double)W1[i * IN + k] * (double)xs[r][k];
            h = act<LEAKY>((float)z);
        }
        h1s[r][i] = h;
        if constexpr (!std::is_null_pointer_v<WS>) H1w[(int64_t)r * N1 + i] = h;
    }
}

// z2ᵀ = W2·h1ᵀ of one 16-unit block, before the bias: w2 is the lane's A row of W2 (row 0 when jin is false).  Each
// 16-wide k block is a 4-step fmaf chain of its own (rotating over four accumulators so that the MFMAs of neighbouring
// blocks overlap), added into f64: z2 is rounded once, not once per k step.  Every load is unconditional, from a clamped
// address, and the value is selected afterwards: a load under a run-time condition is branched around and waited for one
// by one.  BARRIER keeps the scheduler from hoisting all 100 loads of a 25-block row at once where that spills.
template <int NB1, bool BARRIER>
__device__ __forceinline__ void z2_block(const float *w2, bool jin, int h1, const float (&h1s)[16][16 * NB1 + 4], int g,
                                         int c, double (&zd)[4]) {
    f32x4 acc4[4];
#pragma unroll
    for (int ii = 0; ii < 4; ++ii) zd[ii] = 0.0;
#pragma unroll
    for (int kb = 0; kb < NB1; ++kb) {
        const f32x4 hv = *(const f32x4 *)&h1s[c][16 * kb + 4 * g];
        f32x4 &acc = acc4[kb & 3];
        acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) {
            const int k = 16 * kb + 4 * g + ii;
            const bool kin = kb < NB1 - 1 || k < h1;                                  // h1 > 16·(NB1 − 1)
            const float wv = w2[kin ? k : h1 - 1];
            acc = mma(jin && kin ? wv : 0.f, hv[ii], acc);
        }
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) zd[ii] += (double)acc[ii];
        if constexpr (BARRIER) {
            if ((kb & 7) == 7) __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// δ1ᵀ += W2ᵀ·δ2ᵀ of unit block jb, straight from the δ2 accumulator (its k order is the unit order of the block), with
// the same clamped loads.  policy_bwd's; action_grad keeps the same lines written out (see there: its code came out
// slower through this helper)
template <int NB1>
__device__ __forceinline__ void delta1_block(const float *W2, int jb, int h1, int h2, f32x4 d2, int g, int c,
                                             f32x4 (&dacc)[NB1]) {
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

// δ1ᵀ over eight waves, in a fixed order: waves 4..7 park theirs, waves 0..3 add their own to it in place (f32).  The
// caller then adds red[0..3] in wave order in f64.
template <int NB1>
__device__ __forceinline__ void fold8(f32x4 (&red)[4][NB1][64], const f32x4 (&dacc)[NB1], int wave, int lane) {
    if (wave >= 4) {
#pragma unroll
        for (int ib = 0; ib < NB1; ++ib) red[wave - 4][ib][lane] = dacc[ib];
    }
    __syncthreads();
    if (wave < 4) {
#pragma unroll
        for (int ib = 0; ib < NB1; ++ib) red[wave][ib][lane] = dacc[ib] + red[wave][ib][lane];
    }
    __syncthreads();
}

// W1 [h1][IN] to P[w1..) and b1 to P[b1..) of the block's partial row, over the block's 16 rows of δ1 (in h1s): one
// (unit, input) pair per thread step, rows in order
template <int WG, int IN, int HP>
__device__ __forceinline__ void w1b1_tail(const float (&h1s)[16][HP], const float (&xs)[16][IN], double *P, int w1, int b1,
                                          int h1, int tid) {
    for (int e = tid; e < h1 * (IN + 1); e += WG) {
        const int i = e / (IN + 1), k = e % (IN + 1);
        double s = 0.0;
        if (k < IN) {
#pragma unroll
            for (int r = 0; r < 16; ++r) s += (double)h1s[r][i] * (double)xs[r][k];
            P[w1 + i * IN + k] = s;
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) s += h1s[r][i];
            P[b1 + i] = s;
        }
    }
}

// ---- the dW2 weights launch (uavx_grad_common.hip): one wave per job and tower (the grid's y), a 64 x 64 tile of
// dW2 = Σ_rows δ2ᵀ·h1 over one split-K slice of rows, or a 256-column slice of the per-block partial rows summed over the
// slice's blocks (f64)
struct WeightArgs {
    const float *h1ws, *d2ws;          // [b16][n1], [b16][16·nb2]; tower t at + t * *_tower
    const double *pws;                 // [b16 / 16][lp]
    int64_t h1_tower, d2_tower, p_tower;
    float *part2;                      // [S][towers][h2][h1]
    double *partp;                     // [S][towers][lp]
    int64_t b16, kc;
    int h1, n1, h2, nb2, lp, towers, S, tj, ti, pchunks;
};

bool launch_grad_weights(const WeightArgs &a, hipStream_t stream);   // false: the launch failed

inline int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }

// split-K over b16 rows for `tiles` 64 x 64 tiles of dW2: about 8192 tile jobs, slices of at least 64 rows (a multiple of
// 16: whole row blocks).  S slices of kc rows, the last one possibly short.
inline void split_k(int64_t tiles, int64_t b16, int64_t *kc, int *S) {
    const int64_t by_rows = (b16 + 63) / 64;
    int64_t s = 8192 / tiles;
    if (s < 1) s = 1;
    if (s > by_rows) s = by_rows;
    *kc = ((b16 + s - 1) / s + 15) / 16 * 16;
    *S = (int)((b16 + *kc - 1) / *kc);
}

}  // namespace uavx_grad_k

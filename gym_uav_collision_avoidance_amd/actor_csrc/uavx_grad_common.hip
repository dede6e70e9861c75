// The dW2 weights kernel of the critic-loss gradient and of the actor backward (§18, one tower), and its
// launch.  The lane layout and WeightArgs are in uavx_grad_impl.hpp.
#include "uavx_grad_impl.hpp"

namespace uavx_grad_k {

constexpr int WG = 256, WAVES = WG / 64;

__global__ __launch_bounds__(WG) void grad_weights(WeightArgs a) {
    const int lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
    // the tower is the grid's y: decoding it from the job number would cost the one-tower caller a 64-bit division a wave
    const int t = blockIdx.y;
    int64_t job = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    const int64_t tiles = (int64_t)a.tj * a.ti;
    if (job < tiles * a.S) {
        // ---- a 64 x 64 tile of dW2 over rows [s·kc, (s+1)·kc): A = δ2ᵀ (units x rows), B = h1 (rows x inputs)
        const int s = (int)(job / tiles), tile = (int)(job % tiles);
        const int j0 = 64 * (tile / a.ti), i0 = 64 * (tile % a.ti), ld2 = 16 * a.nb2;
        const float *D = a.d2ws + t * a.d2_tower, *H = a.h1ws + t * a.h1_tower;
        const int64_t r_lo = s * a.kc, r_hi = r_lo + a.kc < a.b16 ? r_lo + a.kc : a.b16;
        int jm[4], in_[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            jm[m] = j0 + 16 * m + c;
            in_[m] = i0 + 16 * m + c;
        }
        f32x4 acc[4][4];
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int64_t r = r_lo; r < r_hi; r += 4) {
            const float *dr = D + (r + g) * ld2, *hr = H + (r + g) * a.n1;
            float av[4], bv[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                av[m] = jm[m] < a.h2 ? dr[jm[m]] : 0.f;
                bv[m] = in_[m] < a.h1 ? hr[in_[m]] : 0.f;
            }
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int n = 0; n < 4; ++n) acc[m][n] = mma(av[m], bv[n], acc[m][n]);
        }
        float *out = a.part2 + ((int64_t)s * a.towers + t) * a.h2 * a.h1;
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int ii = 0; ii < 4; ++ii) {
                const int j = j0 + 16 * m + 4 * g + ii;
                if (j >= a.h2) continue;
#pragma unroll
                for (int n = 0; n < 4; ++n)
                    if (in_[n] < a.h1) out[(int64_t)j * a.h1 + in_[n]] = acc[m][n][ii];
            }
        return;
    }
    job -= tiles * a.S;
    if (job >= (int64_t)a.pchunks * a.S) return;
    // ---- 256 columns of the per-block partial rows summed over the blocks of slice s, in block order, in f64
    const int s = (int)(job / a.pchunks), chunk = (int)(job % a.pchunks);
    const int e0 = 256 * chunk + 4 * lane;
    if (e0 >= a.lp) return;
    const int64_t w_lo = s * (a.kc / 16), w_end = (s + 1) * (a.kc / 16), nblk = a.b16 / 16;
    const int64_t w_hi = w_end < nblk ? w_end : nblk;
    const double *P = a.pws + t * a.p_tower + e0;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t w = w_lo; w < w_hi; ++w) {
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] += P[w * a.lp + q];
    }
    double *out = a.partp + ((int64_t)s * a.towers + t) * a.lp + e0;
#pragma unroll
    for (int q = 0; q < 4; ++q) out[q] = acc[q];
}

bool launch_grad_weights(const WeightArgs &a, hipStream_t stream) {
    const int64_t jobs = ((int64_t)a.tj * a.ti + a.pchunks) * a.S;   // of one tower
    const dim3 grid((unsigned)((jobs + WAVES - 1) / WAVES), (unsigned)a.towers);
    hipLaunchKernelGGL(grad_weights, grid, dim3(WG), 0, stream, a);
    return hipGetLastError() == hipSuccess;
}

}  // namespace uavx_grad_k

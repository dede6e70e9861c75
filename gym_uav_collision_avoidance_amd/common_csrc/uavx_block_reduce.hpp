// The workgroup reductions of libuavx_clip.so, libuavx_gae.so, libuavx_ppo.so and libuavx_norm.so.  Their
// headers promise results that do not depend on the launch: "same order, same bits".  The order is the one written here, for
// all four: an edit to it changes the bits of every one of them, and their GPU tests say so.
#pragma once

namespace uavx_common {

constexpr int WAVE = 64;

// the sum of a workgroup's WG values, in every thread: lanes by a halving tree, wavefronts through LDS left to right.  `part`
// (WG / WAVE elements) is this call's own: a second call may not reuse it without a barrier in between.
template <int WG, typename T>
__device__ inline T block_sum(T s, T *part) {
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) s += __shfl_down(s, off, WAVE);
    if ((threadIdx.x & (WAVE - 1)) == 0) part[threadIdx.x / WAVE] = s;
    __syncthreads();
    T r = part[0];
#pragma unroll
    for (int w = 1; w < WG / WAVE; ++w) r += part[w];
    return r;
}

// the total of `count` per-workgroup partials, in every thread of the calling workgroup
template <int WG, typename T>
__device__ inline T total(const T *__restrict__ partial, int count, T *part) {
    T s = 0;
    for (int i = threadIdx.x; i < count; i += WG) s += partial[i];
    return block_sum<WG>(s, part);
}

}  // namespace uavx_common

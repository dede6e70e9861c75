// Definitions shared by the translation units of libuavx_actor.so that work on the actor or the critic: uavx_actor.hip,
// uavx_critic.hip, uavx_explore.hip (clampf) and, through uavx_grad_impl.hpp, the gradient units uavx_critic_grad.hip,
// uavx_action_grad.hip, uavx_policy_grad.hip and uavx_grad_common.hip.  The packed-weight layout of one 3-layer MLP, the
// MFMA k order, the activations and the actor and critic handles themselves.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/uavx_actor.h"
#include "../../include/uavx_critic.h"

namespace uavx_actor_k {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int OBS = 10, ACT = 2, WG = 256, WAVES = WG / 64;

// packed layout of the weights of one 3-layer MLP, an actor or one critic tower (element counts; fragments are 64 lanes x
// EPL elements, lane-major)
struct Layout {
    int prec, nb1, nb2, ks1, ks2, ks3, epl;
    int64_t b1, b2, b3;           // float offsets of the biases (zero padded to whole blocks)
    int64_t w1, w2, w3;           // element offsets of the fragments, in units of the precision's element
    int64_t bias_floats, frag_elems;
};

__host__ __device__ inline Layout layout(int prec, int h1, int h2) {
    Layout L;
    L.prec = prec;
    L.epl = prec == UAVX_ACTOR_F32 ? 1 : 8;
    L.nb1 = (h1 + 15) / 16;
    L.nb2 = (h2 + 15) / 16;
    if (prec == UAVX_ACTOR_BF16) {           // a bf16 step consumes two 16-unit blocks of the previous layer
        L.nb1 += L.nb1 & 1;
        L.nb2 += L.nb2 & 1;
    }
    L.ks1 = prec == UAVX_ACTOR_F32 ? 3 : 1;                       // K 10 -> 12 (f32) / 32 (bf16)
    L.ks2 = prec == UAVX_ACTOR_F32 ? 4 * L.nb1 : L.nb1 / 2;
    L.ks3 = prec == UAVX_ACTOR_F32 ? 4 * L.nb2 : L.nb2 / 2;
    L.b1 = 0;
    L.b2 = 16 * L.nb1;
    L.b3 = L.b2 + 16 * L.nb2;
    L.bias_floats = L.b3 + 16;
    L.w1 = 0;
    L.w2 = L.w1 + (int64_t)L.nb1 * L.ks1 * 64 * L.epl;
    L.w3 = L.w2 + (int64_t)L.nb2 * L.ks2 * 64 * L.epl;
    L.frag_elems = L.w3 + (int64_t)L.ks3 * 64 * L.epl;
    return L;
}

// The hidden sizes uavx_actor_create and uavx_critic_create accept, for both precisions (include/uavx_actor.h,
// include/uavx_critic.h): hidden1 within the last 16-unit block of a compiled register tile (SAC / TD3 241..256, DDPG
// 385..400), hidden2 1..4096.  bf16 rounds nb1 up to an even block count, so a lookup by nb1 alone would also accept
// 225..240 and 401..416 there.
inline bool hidden_supported(int kind, int h1, int h2) {
    const int top = kind == UAVX_ACTOR_DDPG ? 400 : 256;
    return h1 > top - 16 && h1 <= top && h2 >= 1 && h2 <= 4096;
}

// row k of the input that element e of lane `lane` in MFMA step ks multiplies (see the header comment)
__device__ inline int k_of(int prec, bool first, int ks, int lane, int e) {
    const int g = lane >> 4;
    if (prec == UAVX_ACTOR_F32)
        return first ? 4 * ks + g : 16 * (ks >> 2) + 4 * g + (ks & 3);
    return first ? 8 * g + e : 16 * (2 * ks + (e >> 2)) + 4 * g + (e & 3);
}

template <bool LEAKY>
__device__ inline float act(float x) {
    return LEAKY ? (x > 0.f ? x : 0.01f * x) : (x > 0.f ? x : (x != x ? x : 0.f));   // NaN passes like torch's relu
}

__device__ inline float clampf(float x, float lo, float hi) {   // torch.clamp: NaN stays NaN
    return x < lo ? lo : (x > hi ? hi : x);
}

}  // namespace uavx_actor_k

struct uavx_actor {
    int kind, prec, h1, h2;
    uavx_actor_k::Layout L;
    float *bias;        // device: L.bias_floats floats, then the fragments
    void *frags;
    bool packed;
};

struct uavx_critic {
    int kind, prec, h1, h2, towers;
    uavx_actor_k::Layout L;   // of one tower
    float *bias;        // device: towers x L.bias_floats floats, then towers x L.frag_elems fragment elements
    void *frags;
    int64_t split_rows;
    bool packed;
};

// Fused critic forwards and TD targets (include/uavx_critic.h): [state, action] -> the critic's towers on the matrix cores,
// and, for the target, the actor forward and its sample / smoothing epilogue before them, in one launch.  DESIGN.md §13.
//
// Every tower is an MLP with the actor's tiling and packing (uavx_actor.hip's header comment): Hᵀ = W·Xᵀ, the accumulator of
// one layer is the B operand of the next, layer 2 is folded block by block into the output accumulator.  Layer 1 reads
// K = 12: the state in k 0..9, the action in k 10..11.  f32: k = 4*ks + g, so k 10 / 11 sit in step 2 of lanes 32..47 /
// 48..63; bf16: k = 8*g + e, so they are elements 2 / 3 of lanes 16..31.  The target kernel computes a' in accumulator rows
// 0..1 of lanes 0..15 (row c = lane & 15 of the batch) and moves it there with one ds_bpermute per value.
// Twin critics share one output accumulator: tower t's output weights are packed into row t, so Q1 / Q2 land in rows 0 / 1.
//
// Two variants of each kernel (S = waves per 16-row block):
//   S == 1  the actor's tile: 4 independent waves per workgroup, each carrying JB row blocks through every layer.
//   S  > 1  small batches: one row block per workgroup of S waves; every wave computes layer 1 whole and the layer-2 groups
//           p ≡ wave (mod S), then the S partial output accumulators are summed through LDS in wave order.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "../../include/uavx_critic.h"
#include "uavx_actor_impl.hpp"

namespace uavx_critic_k {

using uavx_actor_k::act;
using uavx_actor_k::bf16x8;
using uavx_actor_k::clampf;
using uavx_actor_k::f32x4;
using uavx_actor_k::Layout;

constexpr int OBS = 10, IN = 12, WG = 256, WAVES = WG / 64, SPLIT = 8;

struct PackArgs {
    const float *W1[2], *b1[2], *W2[2], *b2[2], *W3[2], *b3[2];
    int h1, h2, towers;
};

// one thread per packed element: every tower's biases (float), then every tower's fragments (float or bf16); tower t's
// output layer goes into row t of its 16-row block
__global__ __launch_bounds__(256) void critic_pack_kernel(PackArgs a, Layout L, float *bias, void *frags) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < a.towers * L.bias_floats) {
        const int t = (int)(i / L.bias_floats);
        const int64_t j = i % L.bias_floats;
        float v = 0.f;
        if (j < L.b2) v = j < a.h1 ? a.b1[t][j] : 0.f;
        else if (j < L.b3) v = j - L.b2 < a.h2 ? a.b2[t][j - L.b2] : 0.f;
        else v = j - L.b3 == t ? a.b3[t][0] : 0.f;
        bias[i] = v;
        return;
    }
    const int64_t f = i - a.towers * L.bias_floats;
    if (f >= a.towers * L.frag_elems) return;
    const int t = (int)(f / L.frag_elems);
    const int64_t fe = f % L.frag_elems;
    const int e = (int)(fe % L.epl), lane = (int)((fe / L.epl) & 63);
    const int64_t frag = fe / (64 * L.epl);
    int layer, nb, ks;
    if (fe < L.w2) { layer = 1; nb = (int)(frag / L.ks1); ks = (int)(frag % L.ks1); }
    else if (fe < L.w3) { const int64_t q = frag - L.w2 / (64 * L.epl); layer = 2; nb = (int)(q / L.ks2); ks = (int)(q % L.ks2); }
    else { layer = 3; nb = 0; ks = (int)(frag - L.w3 / (64 * L.epl)); }
    const int n = 16 * nb + (lane & 15), k = uavx_actor_k::k_of(L.prec, layer == 1, ks, lane, e);
    float v = 0.f;
    if (layer == 1) v = (n < a.h1 && k < IN) ? a.W1[t][(int64_t)n * IN + k] : 0.f;
    else if (layer == 2) v = (n < a.h2 && k < a.h1) ? a.W2[t][(int64_t)n * a.h1 + k] : 0.f;
    else v = (n == t && k < a.h2) ? a.W3[t][k] : 0.f;
    if (L.prec == UAVX_CRITIC_F32) ((float *)frags)[f] = v;
    else ((__bf16 *)frags)[f] = (__bf16)v;        // round to nearest even (v_cvt_pk_bf16_f32)
}

template <int PREC>
struct Tile {
    static constexpr bool F32 = PREC == UAVX_CRITIC_F32;
    using frag_t = typename std::conditional<F32, float, bf16x8>::type;
    static constexpr int KS1 = F32 ? 3 : 1;
    __device__ static f32x4 mma(frag_t x, frag_t y, f32x4 acc) {
        if constexpr (F32) return __builtin_amdgcn_mfma_f32_16x16x4f32(x, y, acc, 0, 0, 0);
        else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(x, y, acc, 0, 0, 0);
    }
};

// One MLP (an actor or one critic tower) on the layer-1 operands x, its layer-2 groups p = part, part + step, ...
// folded into o (bias of the output layer NOT added).  bias / F: the MLP's packed biases and fragments (Layout).
template <int PREC, bool LEAKY, int NB1, int JB>
__device__ inline void mlp(const typename Tile<PREC>::frag_t (&x)[JB][Tile<PREC>::KS1], const float *__restrict__ bias,
                           const typename Tile<PREC>::frag_t *__restrict__ F, int nb2, int part, int step, f32x4 (&o)[JB]) {
    using T = Tile<PREC>;
    using frag_t = typename T::frag_t;
    constexpr bool F32 = T::F32;
    constexpr int KS1 = T::KS1, KS2 = F32 ? 4 * NB1 : NB1 / 2, HS = F32 ? NB1 : NB1 / 2, GB = F32 ? 1 : 2;
    using h_t = typename std::conditional<F32, f32x4, bf16x8>::type;
    const int lane = threadIdx.x & 63, g = lane >> 4;
    const frag_t *W1 = F, *W2 = F + (int64_t)NB1 * KS1 * 64;
    const frag_t *W3 = W2 + (int64_t)nb2 * KS2 * 64;

    h_t h[JB][HS];
#pragma unroll
    for (int nb = 0; nb < NB1; ++nb) {
        f32x4 acc[JB];
#pragma unroll
        for (int jb = 0; jb < JB; ++jb) acc[jb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS1; ++ks) {
            const frag_t w = W1[(nb * KS1 + ks) * 64 + lane];
#pragma unroll
            for (int jb = 0; jb < JB; ++jb) acc[jb] = T::mma(w, x[jb][ks], acc[jb]);
        }
        const f32x4 b = *(const f32x4 *)(bias + 16 * nb + 4 * g);
#pragma unroll
        for (int jb = 0; jb < JB; ++jb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = act<LEAKY>(acc[jb][r] + b[r]);
                if constexpr (F32) h[jb][nb][r] = v;
                else h[jb][nb >> 1][4 * (nb & 1) + r] = (__bf16)v;
            }
    }

    const float *b2 = bias + 16 * NB1;
    for (int p = part; p < nb2 / GB; p += step) {
        f32x4 acc[JB][GB];
#pragma unroll
        for (int jb = 0; jb < JB; ++jb)
#pragma unroll
            for (int q = 0; q < GB; ++q) acc[jb][q] = f32x4{0.f, 0.f, 0.f, 0.f};
        const frag_t *w = W2 + (int64_t)(GB * p) * KS2 * 64 + lane;
#pragma unroll
        for (int ks = 0; ks < KS2; ++ks) {
#pragma unroll
            for (int q = 0; q < GB; ++q) {
                const frag_t wk = w[(q * KS2 + ks) * 64];
#pragma unroll
                for (int jb = 0; jb < JB; ++jb) {
                    if constexpr (F32) acc[jb][q] = T::mma(wk, h[jb][ks >> 2][ks & 3], acc[jb][q]);
                    else acc[jb][q] = T::mma(wk, h[jb][ks], acc[jb][q]);
                }
            }
        }
        if constexpr (F32) {
            const f32x4 b = *(const f32x4 *)(b2 + 16 * p + 4 * g);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float w3 = W3[(4 * p + r) * 64 + lane];
#pragma unroll
                for (int jb = 0; jb < JB; ++jb) o[jb] = T::mma(w3, act<LEAKY>(acc[jb][0][r] + b[r]), o[jb]);
            }
        } else {
            const f32x4 b0 = *(const f32x4 *)(b2 + 32 * p + 4 * g), b1 = *(const f32x4 *)(b2 + 32 * p + 16 + 4 * g);
            const frag_t w3 = W3[p * 64 + lane];
#pragma unroll
            for (int jb = 0; jb < JB; ++jb) {
                bf16x8 v;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    v[r] = (__bf16)act<LEAKY>(acc[jb][0][r] + b0[r]);
                    v[4 + r] = (__bf16)act<LEAKY>(acc[jb][1][r] + b1[r]);
                }
                o[jb] = T::mma(w3, v, o[jb]);
            }
        }
    }
}

struct Args {
    const float *state, *action;               // action: critic_q only
    const float *reward, *mask, *eps, *alpha;  // target only
    float *out, *aux;
    int64_t rows, s_stride, a_stride, r_stride, m_stride, out_stride, aux_stride;
    float gamma, noise_std, noise_clip;
    int kind;
    const float *cbias;                        // critic: towers' biases, tower t at cbias + t * c_tb
    const void *cfrags;                        // critic: towers' fragments, tower t at element t * c_tf
    int64_t c_tb, c_tf;
    int cnb2;
    const float *abias;                        // actor (target only)
    const void *afrags;
    int anb2;
};

// torch.min: a NaN in either argument gives NaN
__device__ inline float tmin(float a, float b) { return (a != a || a < b) ? a : b; }

// The S partial accumulators of a row block summed in wave order (S > 1): every wave gets the same bits.
template <int S>
__device__ inline f32x4 reduce(f32x4 (*red)[64], f32x4 v, int wave, int lane) {
    red[wave][lane] = v;
    __syncthreads();
    f32x4 s = red[0][lane];
#pragma unroll
    for (int w = 1; w < S; ++w) s += red[w][lane];
    return s;
}

// TARGET = false: critic_q; true: critic_target.  S: waves per row block (1 = the actor's tile); JB: row blocks per wave
// (1 when S > 1); WPS: waves per SIMD the register allocation must allow.
template <int PREC, bool LEAKY, int NB1, int JB, int S, int WPS, bool TARGET>
__global__ __launch_bounds__(S == 1 ? WG : 64 * S, WPS) void critic_fwd(Args a) {
    using T = Tile<PREC>;
    using frag_t = typename T::frag_t;
    constexpr bool F32 = T::F32;
    constexpr int KS1 = T::KS1, TOWERS = LEAKY ? 1 : 2;
    static_assert(S == 1 || JB == 1, "the small-batch variant carries one row block per workgroup");
    const int lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15, wave = threadIdx.x >> 6;
    const int64_t row0 = S == 1 ? ((int64_t)blockIdx.x * WAVES + wave) * (16 * JB) : (int64_t)blockIdx.x * 16;
    if (row0 >= a.rows) return;                       // S > 1: the same for the whole workgroup, before any barrier
    const int part = S == 1 ? 0 : wave;
    __shared__ f32x4 red[S > 1 ? 2 : 1][S][64];

    // ---- layer-1 operands: state in k 0..9; the action in k 10..11 (critic_q: from memory; target: a', set below)
    frag_t x[JB][KS1];
#pragma unroll
    for (int jb = 0; jb < JB; ++jb) {
        const int64_t r = row0 + 16 * jb + c;
        const bool in = r < a.rows;
        const float *s = a.state + r * a.s_stride;
        const float *u = TARGET ? nullptr : a.action + r * a.a_stride;
#pragma unroll
        for (int ks = 0; ks < KS1; ++ks) {
            if constexpr (F32) {
                const int k = 4 * ks + g;
                x[jb][ks] = !in ? 0.f : k < OBS ? s[k] : (!TARGET && k < IN) ? u[k - OBS] : 0.f;
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int k = 8 * g + e;
                    x[jb][ks][e] = (__bf16)(!in ? 0.f : k < OBS ? s[k] : (!TARGET && k < IN) ? u[k - OBS] : 0.f);
                }
            }
        }
    }

    f32x4 o[JB];
    float ap0[JB], ap1[JB], lp[JB];                   // target: a' and logπ of row c (lanes 0..15)
    if constexpr (TARGET) {
        // ---- the actor on s'
#pragma unroll
        for (int jb = 0; jb < JB; ++jb) o[jb] = f32x4{0.f, 0.f, 0.f, 0.f};
        mlp<PREC, LEAKY, NB1, JB>(x, a.abias, (const frag_t *)a.afrags, a.anb2, part, S, o);
        if constexpr (S > 1) o[0] = reduce<S>(red[0], o[0], wave, lane);
        const float *b3 = a.abias + 16 * NB1 + 16 * a.anb2;
#pragma unroll
        for (int jb = 0; jb < JB; ++jb) {
            const int64_t r = row0 + 16 * jb + c;
            const float y0 = o[jb][0] + b3[0], y1 = o[jb][1] + b3[1];
            const float e0 = r < a.rows && a.kind != UAVX_CRITIC_DDPG ? a.eps[2 * r] : 0.f;
            const float e1 = r < a.rows && a.kind != UAVX_CRITIC_DDPG ? a.eps[2 * r + 1] : 0.f;
            float a0, a1, l = 0.f;
            if (a.kind == UAVX_CRITIC_SAC) {
                // GaussianPolicy.sample (model.py:88-101): x_t = mean + std * eps, a = tanh(x_t), summed
                // Normal(mean, std).log_prob(x_t) - log(1 * (1 - a^2) + 1e-6), in torch-f32's operation order
                const float y[2] = {y0, y1}, e[2] = {e0, e1}, lr[2] = {o[jb][2] + b3[2], o[jb][3] + b3[3]};
                float av[2], lv[2];
#pragma unroll
                for (int d = 0; d < 2; ++d) {
                    const float sd = expf(clampf(lr[d], -20.f, 2.f));
                    const float xt = y[d] + e[d] * sd;
                    av[d] = tanhf(xt);
                    const float z = xt - y[d];
                    const float lpd = -(z * z) / (2.f * (sd * sd)) - logf(sd) - 0.918938533204672742f;
                    lv[d] = lpd - logf(1.f * (1.f - av[d] * av[d]) + 1e-6f);   // tanh = ±1 gives log(1e-6)
                }
                a0 = av[0];
                a1 = av[1];
                l = lv[0] + lv[1];
            } else if (a.kind == UAVX_CRITIC_TD3) {
                a0 = clampf(tanhf(y0) + clampf(e0 * a.noise_std, -a.noise_clip, a.noise_clip), -1.f, 1.f);
                a1 = clampf(tanhf(y1) + clampf(e1 * a.noise_std, -a.noise_clip, a.noise_clip), -1.f, 1.f);
            } else {
                a0 = tanhf(y0);
                a1 = tanhf(y1);
            }
            ap0[jb] = a0;
            ap1[jb] = a1;
            lp[jb] = l;
            // a' of row c (lanes 0..15) into the critic's layer-1 operand
            const float v0 = __shfl(a0, c), v1 = __shfl(a1, c);
            if constexpr (F32) {
                if (g == 2) x[jb][2] = v0;
                else if (g == 3) x[jb][2] = v1;
            } else if (g == 1) {
                x[jb][0][2] = (__bf16)v0;
                x[jb][0][3] = (__bf16)v1;
            }
        }
    }

    // ---- the critic tower(s), folded into one accumulator (tower t in row t)
#pragma unroll
    for (int jb = 0; jb < JB; ++jb) o[jb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < TOWERS; ++t)
        mlp<PREC, LEAKY, NB1, JB>(x, a.cbias + t * a.c_tb, (const frag_t *)a.cfrags + t * a.c_tf / (F32 ? 1 : 8), a.cnb2, part, S,
                                  o);
    if constexpr (S > 1) {
        o[0] = reduce<S>(red[1], o[0], wave, lane);
        if (wave != 0) return;
    }

    // ---- epilogue: lanes 0..15 hold the towers' outputs in rows 0 (and 1) of row c of each row block
    if (g != 0) return;
    const int64_t ob = 16 * NB1 + 16 * a.cnb2;        // output bias of a tower, tower t's in element t
#pragma unroll
    for (int jb = 0; jb < JB; ++jb) {
        const int64_t r = row0 + 16 * jb + c;
        if (r >= a.rows) continue;
        const float q1 = o[jb][0] + a.cbias[ob];
        const float q2 = TOWERS == 2 ? o[jb][1] + a.cbias[a.c_tb + ob + 1] : q1;
        if constexpr (!TARGET) {
            float *dst = a.out + r * a.out_stride;
            dst[0] = q1;
            if (TOWERS == 2) dst[1] = q2;
        } else {
            const float m = tmin(q1, q2);
            const float rw = a.reward[r * a.r_stride], mk = a.mask[r * a.m_stride];
            float y;
            if (a.kind == UAVX_CRITIC_SAC) y = rw + (mk * a.gamma) * (m - a.alpha[0] * lp[jb]);   // sac.py:59-60
            else y = rw + (mk * a.gamma) * m;   // td3.py:126 not_done * discount; ddpg.py:62 gamma * mask (the same product)
            a.out[r * a.out_stride] = y;
            if (a.aux) {
                float *x4 = a.aux + r * a.aux_stride;
                x4[0] = ap0[jb];
                x4[1] = ap1[jb];
                x4[2] = lp[jb];
                x4[3] = m;
            }
        }
    }
}

}  // namespace uavx_critic_k

using namespace uavx_critic_k;

namespace {

typedef void (*fwd_fn)(Args);
struct Entry {
    int prec;
    bool leaky;
    int nb1, jb;
    fwd_fn q, target, q_small, target_small;
};
// the actor's register tiles for the large-batch variant; the small-batch variant runs SPLIT waves per row
// block at 2 waves per SIMD
#define UAVX_CRITIC_ENTRY(P, LK, NB1, JB, WPS)                                                                             \
    {P, LK, NB1, JB, critic_fwd<P, LK, NB1, JB, 1, WPS, false>, critic_fwd<P, LK, NB1, JB, 1, WPS, true>,                \
     critic_fwd<P, LK, NB1, 1, SPLIT, 2, false>, critic_fwd<P, LK, NB1, 1, SPLIT, 2, true>}
const Entry ENTRIES[] = {
    UAVX_CRITIC_ENTRY(UAVX_CRITIC_F32, false, 16, 2, 2),
    UAVX_CRITIC_ENTRY(UAVX_CRITIC_BF16, false, 16, 2, 2),
    UAVX_CRITIC_ENTRY(UAVX_CRITIC_F32, true, 25, 2, 1),
    UAVX_CRITIC_ENTRY(UAVX_CRITIC_BF16, true, 26, 1, 2),
};
#undef UAVX_CRITIC_ENTRY

const Entry *find(int prec, bool leaky, int nb1) {
    for (const Entry &e : ENTRIES)
        if (e.prec == prec && e.leaky == leaky && e.nb1 == nb1) return &e;
    return nullptr;
}

int launch(const uavx_critic *h, bool target, Args &a, hipStream_t stream) {
    const Entry *e = find(h->prec, h->kind == UAVX_CRITIC_DDPG, h->L.nb1);
    const bool small = a.rows < h->split_rows;
    const int64_t per = small ? 16 : (int64_t)WAVES * 16 * e->jb, blocks = (a.rows + per - 1) / per;
    if (blocks > 0x7fffffff) return UAVX_CRITIC_ERR_INVALID_ARG;
    a.cbias = h->bias;
    a.cfrags = h->frags;
    a.c_tb = h->L.bias_floats;
    a.c_tf = h->L.frag_elems;
    a.cnb2 = h->L.nb2;
    const fwd_fn fn = small ? (target ? e->target_small : e->q_small) : (target ? e->target : e->q);
    hipLaunchKernelGGL(fn, dim3((unsigned)blocks), dim3(small ? 64 * SPLIT : WG), 0, stream, a);
    return hipGetLastError() == hipSuccess ? UAVX_CRITIC_OK : UAVX_CRITIC_ERR_HIP;
}

}  // namespace

extern "C" {

int uavx_critic_version(void) { return UAVX_CRITIC_VERSION; }

const char *uavx_critic_strerror(int s) {
    switch (s) {
        case UAVX_CRITIC_OK: return "ok";
        case UAVX_CRITIC_ERR_INVALID_ARG: return "invalid argument";
        case UAVX_CRITIC_ERR_HIP: return "HIP runtime error";
        case UAVX_CRITIC_ERR_UNSUPPORTED: return "no kernel compiled for these dimensions";
        case UAVX_CRITIC_ERR_NOT_PACKED: return "q / target before pack";
        default: return "unknown status";
    }
}

int uavx_critic_create(int kind, int precision, int obs_dim, int hidden1, int hidden2, int act_dim, uavx_critic **out) {
    if (!out) return UAVX_CRITIC_ERR_INVALID_ARG;
    *out = nullptr;
    if (kind < UAVX_CRITIC_SAC || kind > UAVX_CRITIC_DDPG || (precision != UAVX_CRITIC_F32 && precision != UAVX_CRITIC_BF16) ||
        hidden1 < 1 || hidden2 < 1)
        return UAVX_CRITIC_ERR_INVALID_ARG;
    if (obs_dim != OBS || act_dim != 2 || hidden2 > 4096) return UAVX_CRITIC_ERR_UNSUPPORTED;
    const Layout L = uavx_actor_k::layout(precision, hidden1, hidden2);
    if (!uavx_actor_k::hidden_supported(kind, hidden1, hidden2) || !find(precision, kind == UAVX_CRITIC_DDPG, L.nb1))
        return UAVX_CRITIC_ERR_UNSUPPORTED;
    const int towers = kind == UAVX_CRITIC_DDPG ? 1 : 2;
    const size_t esz = precision == UAVX_CRITIC_F32 ? 4 : 2;
    void *mem = nullptr;
    if (hipMalloc(&mem, towers * (L.bias_floats * 4 + L.frag_elems * esz)) != hipSuccess) {
        (void)hipGetLastError();
        return UAVX_CRITIC_ERR_HIP;
    }
    *out = new uavx_critic{kind, precision, hidden1, hidden2, towers, L, (float *)mem,
                           (char *)mem + towers * L.bias_floats * 4, UAVX_CRITIC_SPLIT_ROWS, false};
    return UAVX_CRITIC_OK;
}

int uavx_critic_destroy(uavx_critic *h) {
    if (!h) return UAVX_CRITIC_ERR_INVALID_ARG;
    const hipError_t e = hipFree(h->bias);
    delete h;
    return e == hipSuccess ? UAVX_CRITIC_OK : UAVX_CRITIC_ERR_HIP;
}

int uavx_critic_set_split_rows(uavx_critic *h, int64_t rows) {
    if (!h || rows < 0) return UAVX_CRITIC_ERR_INVALID_ARG;
    h->split_rows = rows;
    return UAVX_CRITIC_OK;
}

int uavx_critic_pack(uavx_critic *h, const float *W1, const float *b1, const float *W2, const float *b2, const float *W3,
                     const float *b3, const float *W4, const float *b4, const float *W5, const float *b5, const float *W6,
                     const float *b6, void *stream) {
    if (!h || !W1 || !b1 || !W2 || !b2 || !W3 || !b3) return UAVX_CRITIC_ERR_INVALID_ARG;
    const bool second = W4 || b4 || W5 || b5 || W6 || b6;
    if (h->towers == 2 && !(W4 && b4 && W5 && b5 && W6 && b6)) return UAVX_CRITIC_ERR_INVALID_ARG;
    if (h->towers == 1 && second) return UAVX_CRITIC_ERR_INVALID_ARG;
    PackArgs a{{W1, W4}, {b1, b4}, {W2, W5}, {b2, b5}, {W3, W6}, {b3, b6}, h->h1, h->h2, h->towers};
    const int64_t n = h->towers * (h->L.bias_floats + h->L.frag_elems);
    hipLaunchKernelGGL(critic_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, h->L,
                       h->bias, h->frags);
    if (hipGetLastError() != hipSuccess) return UAVX_CRITIC_ERR_HIP;
    h->packed = true;
    return UAVX_CRITIC_OK;
}

int uavx_critic_q(uavx_critic *h, const float *state, int64_t rows, int64_t state_stride, const float *action,
                  int64_t action_stride, float *out, int64_t out_stride, void *stream) {
    if (!h || rows < 0 || state_stride < OBS || action_stride < 2 || out_stride < h->towers) return UAVX_CRITIC_ERR_INVALID_ARG;
    if (rows > 0 && (!state || !action || !out)) return UAVX_CRITIC_ERR_INVALID_ARG;
    if (!h->packed) return UAVX_CRITIC_ERR_NOT_PACKED;
    if (rows == 0) return UAVX_CRITIC_OK;
    Args a{};
    a.state = state;
    a.action = action;
    a.out = out;
    a.rows = rows;
    a.s_stride = state_stride;
    a.a_stride = action_stride;
    a.out_stride = out_stride;
    a.kind = h->kind;
    return launch(h, false, a, (hipStream_t)stream);
}

int uavx_critic_target(uavx_critic *h, const uavx_actor *actor, const float *next_state, int64_t rows, int64_t state_stride,
                       const float *reward, int64_t reward_stride, const float *mask, int64_t mask_stride, const float *eps,
                       const float *alpha, float gamma, float noise_std, float noise_clip, float *out, int64_t out_stride,
                       float *aux, int64_t aux_stride, void *stream) {
    if (!h || !actor || rows < 0) return UAVX_CRITIC_ERR_INVALID_ARG;
    if (actor->kind != h->kind || actor->prec != h->prec || actor->L.nb1 != h->L.nb1) return UAVX_CRITIC_ERR_INVALID_ARG;
    if (state_stride < OBS || reward_stride < 1 || mask_stride < 1 || out_stride < 1 || (aux && aux_stride < 4))
        return UAVX_CRITIC_ERR_INVALID_ARG;
    if (rows > 0 && (!next_state || !reward || !mask || !out)) return UAVX_CRITIC_ERR_INVALID_ARG;
    if (rows > 0 && h->kind != UAVX_CRITIC_DDPG && !eps) return UAVX_CRITIC_ERR_INVALID_ARG;
    if (h->kind == UAVX_CRITIC_SAC && !alpha) return UAVX_CRITIC_ERR_INVALID_ARG;
    if (!h->packed || !actor->packed) return UAVX_CRITIC_ERR_NOT_PACKED;
    if (rows == 0) return UAVX_CRITIC_OK;
    Args a{};
    a.state = next_state;
    a.reward = reward;
    a.mask = mask;
    a.eps = eps;
    a.alpha = alpha;
    a.out = out;
    a.aux = aux;
    a.rows = rows;
    a.s_stride = state_stride;
    a.r_stride = reward_stride;
    a.m_stride = mask_stride;
    a.out_stride = out_stride;
    a.aux_stride = aux_stride;
    a.gamma = gamma;
    a.noise_std = noise_std;
    a.noise_clip = noise_clip;
    a.kind = h->kind;
    a.abias = actor->bias;
    a.afrags = actor->frags;
    a.anb2 = actor->L.nb2;
    return launch(h, true, a, (hipStream_t)stream);
}

}  // extern "C"

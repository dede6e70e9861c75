// Fused actor inference (include/uavx_actor.h): obs [rows, 10] -> 3 linear layers on the matrix cores -> action epilogue,
// one launch, hidden activations kept in registers.  DESIGN.md "Fused actor kernel" has the tiling and its reasoning.
//
// Orientation: every layer computes Hᵀ = W·Xᵀ, so a wave's 16 batch rows sit on the MFMA column (lane & 15) and the
// layer's output units on the accumulator rows (4 * (lane >> 4) + reg).  That accumulator is already the B operand of the
// next layer's MFMA, which sums over the same row index: no LDS, no lane movement.  The k order inside one MFMA step
// therefore follows the accumulator map, and the pack kernel writes the A operand (the weights) in that same order:
//   f32  v_mfma_f32_16x16x4_f32,  step ks of a layer fed by an accumulator: k = 16*(ks>>2) + 4*g + (ks&3)
//   bf16 v_mfma_f32_16x16x32_bf16, element e of step ks:                    k = 16*(2*ks + (e>>2)) + 4*g + (e&3)
// (g = lane >> 4); layer 1 reads the observation in natural order (f32: k = 4*ks + g, bf16: k = 8*g + e).
// Layer 2 is produced one 16-unit block (bf16: two) at a time and folded into the layer-3 accumulator at once, so only
// layer 1's activations are held whole.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include "../../include/uavx_actor.h"
#include "uavx_actor_impl.hpp"

namespace uavx_actor_k {

struct PackArgs {
    const float *W1, *b1, *W2, *b2, *W3, *b3, *W3b, *b3b;
    int h1, h2, nout;             // nout: 2, or 4 with SAC's log_std head in rows 2..3
};

// one thread per packed element: biases (float) first, then the fragments (float or bf16)
__global__ __launch_bounds__(256) void pack_kernel(PackArgs a, Layout L, float *bias, void *frags) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < L.bias_floats) {
        float v = 0.f;
        if (i < L.b2) v = i < a.h1 ? a.b1[i] : 0.f;
        else if (i < L.b3) v = i - L.b2 < a.h2 ? a.b2[i - L.b2] : 0.f;
        else {
            const int n = (int)(i - L.b3);
            v = n < 2 ? a.b3[n] : n < a.nout ? a.b3b[n - 2] : 0.f;
        }
        bias[i] = v;
        return;
    }
    const int64_t f = i - L.bias_floats;
    if (f >= L.frag_elems) return;
    const int e = (int)(f % L.epl), lane = (int)((f / L.epl) & 63);
    const int64_t frag = f / (64 * L.epl);
    int layer, nb, ks;
    if (f < L.w2) { layer = 1; nb = (int)(frag / L.ks1); ks = (int)(frag % L.ks1); }
    else if (f < L.w3) { const int64_t q = frag - L.w2 / (64 * L.epl); layer = 2; nb = (int)(q / L.ks2); ks = (int)(q % L.ks2); }
    else { layer = 3; nb = 0; ks = (int)(frag - L.w3 / (64 * L.epl)); }
    const int n = 16 * nb + (lane & 15), k = k_of(L.prec, layer == 1, ks, lane, e);
    float v = 0.f;
    if (layer == 1) v = (n < a.h1 && k < OBS) ? a.W1[(int64_t)n * OBS + k] : 0.f;
    else if (layer == 2) v = (n < a.h2 && k < a.h1) ? a.W2[(int64_t)n * a.h1 + k] : 0.f;
    else if (k < a.h2) v = n < 2 ? a.W3[(int64_t)n * a.h2 + k] : n < a.nout ? a.W3b[(int64_t)(n - 2) * a.h2 + k] : 0.f;
    if (L.prec == UAVX_ACTOR_F32) ((float *)frags)[f] = v;
    else ((__bf16 *)frags)[f] = (__bf16)v;        // round to nearest even (v_cvt_pk_bf16_f32)
}

struct FwdArgs {
    const float *obs;
    const float *eps;
    float *out;
    int64_t rows, obs_stride, out_stride;
    float scale;
    int mode, sac, nb2;
};

// NB1: 16-unit blocks of layer 1 (compile time: its activations live in registers); JB: 16-row blocks per wave;
// WPS: waves per SIMD the register allocation must allow (__launch_bounds__)
template <int PREC, bool LEAKY, int NB1, int JB, int WPS>
__global__ __launch_bounds__(WG, WPS) void actor_fwd(FwdArgs a, const float *__restrict__ bias, const void *__restrict__ frags) {
    constexpr bool F32 = PREC == UAVX_ACTOR_F32;
    using frag_t = typename std::conditional<F32, float, bf16x8>::type;
    constexpr int KS1 = F32 ? 3 : 1, KS2 = F32 ? 4 * NB1 : NB1 / 2;
    constexpr int HS = F32 ? NB1 : NB1 / 2;           // held layer-1 operands per row block
    using h_t = typename std::conditional<F32, f32x4, bf16x8>::type;
    const int lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
    const int64_t row0 = ((int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6)) * (16 * JB);
    if (row0 >= a.rows) return;                       // (no barriers below: a wave may leave on its own)
    const frag_t *F = (const frag_t *)frags;
    const int nb2 = a.nb2;
    const frag_t *W1 = F, *W2 = F + (int64_t)NB1 * KS1 * 64;
    const frag_t *W3 = W2 + (int64_t)nb2 * KS2 * 64;

    auto mma = [](frag_t x, frag_t y, f32x4 acc) -> f32x4 {
        if constexpr (F32) return __builtin_amdgcn_mfma_f32_16x16x4f32(x, y, acc, 0, 0, 0);
        else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(x, y, acc, 0, 0, 0);
    };

    // ---- layer 1: observations (B operand straight from global memory; rows past the end and k >= 10 read as 0)
    frag_t x[JB][KS1];
#pragma unroll
    for (int jb = 0; jb < JB; ++jb) {
        const int64_t r = row0 + 16 * jb + c;
        const float *o = a.obs + r * a.obs_stride;
#pragma unroll
        for (int ks = 0; ks < KS1; ++ks) {
            if constexpr (F32) {
                const int k = 4 * ks + g;
                x[jb][ks] = (r < a.rows && k < OBS) ? o[k] : 0.f;
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int k = 8 * g + e;
                    x[jb][ks][e] = (__bf16)((r < a.rows && k < OBS) ? o[k] : 0.f);
                }
            }
        }
    }
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
            for (int jb = 0; jb < JB; ++jb) acc[jb] = mma(w, x[jb][ks], acc[jb]);
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

    // ---- layers 2 + 3: one group of layer-2 blocks (f32: 1, bf16: 2) at a time, folded straight into the output
    constexpr int GB = F32 ? 1 : 2;
    const float *b2 = bias + 16 * NB1;
    f32x4 o[JB];
#pragma unroll
    for (int jb = 0; jb < JB; ++jb) o[jb] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int p = 0; p < nb2 / GB; ++p) {
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
                    if constexpr (F32) acc[jb][q] = mma(wk, h[jb][ks >> 2][ks & 3], acc[jb][q]);
                    else acc[jb][q] = mma(wk, h[jb][ks], acc[jb][q]);
                }
            }
        }
        if constexpr (F32) {
            const f32x4 b = *(const f32x4 *)(b2 + 16 * p + 4 * g);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float w3 = W3[(4 * p + r) * 64 + lane];
#pragma unroll
                for (int jb = 0; jb < JB; ++jb) o[jb] = mma(w3, act<LEAKY>(acc[jb][0][r] + b[r]), o[jb]);
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
                o[jb] = mma(w3, v, o[jb]);
            }
        }
    }

    // ---- epilogue: lanes 0..15 hold output units 0..3 of row c of each row block
    if (g != 0) return;
    const float *b3 = b2 + 16 * nb2;
#pragma unroll
    for (int jb = 0; jb < JB; ++jb) {
        const int64_t r = row0 + 16 * jb + c;
        if (r >= a.rows) continue;
        float *dst = a.out + r * a.out_stride;
        const float y0 = o[jb][0] + b3[0], y1 = o[jb][1] + b3[1];
        if (a.mode == UAVX_ACTOR_RAW) {
            dst[0] = y0;
            dst[1] = y1;
            if (a.sac) {
                dst[2] = clampf(o[jb][2] + b3[2], -20.f, 2.f);
                dst[3] = clampf(o[jb][3] + b3[3], -20.f, 2.f);
            }
        } else if (a.mode == UAVX_ACTOR_DETERMINISTIC) {
            dst[0] = tanhf(y0);
            dst[1] = tanhf(y1);
        } else if (a.mode == UAVX_ACTOR_SAC_SAMPLE) {
            const float l0 = clampf(o[jb][2] + b3[2], -20.f, 2.f), l1 = clampf(o[jb][3] + b3[3], -20.f, 2.f);
            dst[0] = tanhf(y0 + expf(l0) * a.eps[2 * r]);
            dst[1] = tanhf(y1 + expf(l1) * a.eps[2 * r + 1]);
        } else {
            dst[0] = clampf(tanhf(y0) + a.scale * a.eps[2 * r], -1.f, 1.f);
            dst[1] = clampf(tanhf(y1) + a.scale * a.eps[2 * r + 1], -1.f, 1.f);
        }
    }
}

}  // namespace uavx_actor_k

using namespace uavx_actor_k;

namespace {

typedef void (*fwd_fn)(FwdArgs, const float *, const void *);
struct Entry {
    int prec;
    bool leaky;
    int nb1, jb;
    fwd_fn fn;
};
// the compiled register tiles: SAC / TD3 (256 hidden units) and DDPG (400); JB and waves per SIMD measured
const Entry ENTRIES[] = {
    {UAVX_ACTOR_F32, false, 16, 2, actor_fwd<UAVX_ACTOR_F32, false, 16, 2, 2>},
    {UAVX_ACTOR_BF16, false, 16, 2, actor_fwd<UAVX_ACTOR_BF16, false, 16, 2, 2>},
    {UAVX_ACTOR_F32, true, 25, 2, actor_fwd<UAVX_ACTOR_F32, true, 25, 2, 1>},
    {UAVX_ACTOR_BF16, true, 26, 1, actor_fwd<UAVX_ACTOR_BF16, true, 26, 1, 2>},
};

const Entry *find(int prec, bool leaky, int nb1) {
    for (const Entry &e : ENTRIES)
        if (e.prec == prec && e.leaky == leaky && e.nb1 == nb1) return &e;
    return nullptr;
}

}  // namespace

extern "C" {

int uavx_actor_version(void) { return UAVX_ACTOR_VERSION; }

const char *uavx_actor_strerror(int s) {
    switch (s) {
        case UAVX_ACTOR_OK: return "ok";
        case UAVX_ACTOR_ERR_INVALID_ARG: return "invalid argument";
        case UAVX_ACTOR_ERR_HIP: return "HIP runtime error";
        case UAVX_ACTOR_ERR_UNSUPPORTED: return "no kernel compiled for these dimensions";
        case UAVX_ACTOR_ERR_NOT_PACKED: return "forward before pack";
        default: return "unknown status";
    }
}

int uavx_actor_create(int kind, int precision, int obs_dim, int hidden1, int hidden2, int act_dim, uavx_actor **out) {
    if (!out) return UAVX_ACTOR_ERR_INVALID_ARG;
    *out = nullptr;
    if (kind < UAVX_ACTOR_SAC || kind > UAVX_ACTOR_DDPG || (precision != UAVX_ACTOR_F32 && precision != UAVX_ACTOR_BF16) ||
        hidden1 < 1 || hidden2 < 1)
        return UAVX_ACTOR_ERR_INVALID_ARG;
    if (obs_dim != OBS || act_dim != ACT || hidden2 > 4096) return UAVX_ACTOR_ERR_UNSUPPORTED;
    const Layout L = layout(precision, hidden1, hidden2);
    if (!hidden_supported(kind, hidden1, hidden2) || !find(precision, kind == UAVX_ACTOR_DDPG, L.nb1))
        return UAVX_ACTOR_ERR_UNSUPPORTED;
    const size_t esz = precision == UAVX_ACTOR_F32 ? 4 : 2;
    void *mem = nullptr;
    if (hipMalloc(&mem, L.bias_floats * 4 + L.frag_elems * esz) != hipSuccess) {
        (void)hipGetLastError();
        return UAVX_ACTOR_ERR_HIP;
    }
    uavx_actor *h = new uavx_actor{kind, precision, hidden1, hidden2, L, (float *)mem,
                                   (char *)mem + L.bias_floats * 4, false};
    *out = h;
    return UAVX_ACTOR_OK;
}

int uavx_actor_destroy(uavx_actor *h) {
    if (!h) return UAVX_ACTOR_ERR_INVALID_ARG;
    const hipError_t e = hipFree(h->bias);
    delete h;
    return e == hipSuccess ? UAVX_ACTOR_OK : UAVX_ACTOR_ERR_HIP;
}

int uavx_actor_pack(uavx_actor *h, const float *W1, const float *b1, const float *W2, const float *b2, const float *W3,
                    const float *b3, const float *W3b, const float *b3b, void *stream) {
    if (!h || !W1 || !b1 || !W2 || !b2 || !W3 || !b3) return UAVX_ACTOR_ERR_INVALID_ARG;
    const bool sac = h->kind == UAVX_ACTOR_SAC;
    if (sac != (W3b != nullptr && b3b != nullptr) || (!sac && (W3b || b3b))) return UAVX_ACTOR_ERR_INVALID_ARG;
    PackArgs a{W1, b1, W2, b2, W3, b3, W3b, b3b, h->h1, h->h2, sac ? 4 : 2};
    const int64_t n = h->L.bias_floats + h->L.frag_elems;
    hipLaunchKernelGGL(pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, h->L, h->bias,
                       h->frags);
    if (hipGetLastError() != hipSuccess) return UAVX_ACTOR_ERR_HIP;
    h->packed = true;
    return UAVX_ACTOR_OK;
}

int uavx_actor_forward(uavx_actor *h, const float *obs, int64_t rows, int64_t obs_stride, const float *eps, float scale,
                       int mode, float *out, int64_t out_stride, void *stream) {
    if (!h || rows < 0 || mode < UAVX_ACTOR_RAW || mode > UAVX_ACTOR_ADD_CLAMP) return UAVX_ACTOR_ERR_INVALID_ARG;
    const bool sac = h->kind == UAVX_ACTOR_SAC;
    if (mode == UAVX_ACTOR_SAC_SAMPLE && !sac) return UAVX_ACTOR_ERR_INVALID_ARG;
    const int cols = (mode == UAVX_ACTOR_RAW && sac) ? 4 : 2;
    if (obs_stride < OBS || out_stride < cols) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (rows > 0 && (!obs || !out)) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (rows > 0 && !eps && (mode == UAVX_ACTOR_SAC_SAMPLE || mode == UAVX_ACTOR_ADD_CLAMP)) return UAVX_ACTOR_ERR_INVALID_ARG;
    if (!h->packed) return UAVX_ACTOR_ERR_NOT_PACKED;
    if (rows == 0) return UAVX_ACTOR_OK;
    const Entry *e = find(h->prec, h->kind == UAVX_ACTOR_DDPG, h->L.nb1);
    const int64_t per = (int64_t)WAVES * 16 * e->jb, blocks = (rows + per - 1) / per;
    if (blocks > 0x7fffffff) return UAVX_ACTOR_ERR_INVALID_ARG;
    FwdArgs a{obs, eps, out, rows, obs_stride, out_stride, scale, mode, sac ? 1 : 0, h->L.nb2};
    hipLaunchKernelGGL(e->fn, dim3((unsigned)blocks), dim3(WG), 0, (hipStream_t)stream, a, h->bias, h->frags);
    return hipGetLastError() == hipSuccess ? UAVX_ACTOR_OK : UAVX_ACTOR_ERR_HIP;
}

#ifndef UAVX_ACTOR_SRC_HASH
#define UAVX_ACTOR_SRC_HASH ""
#endif
// the loader (_actor_lib.py) finds this marker in the file without mapping it
__attribute__((used)) static const char kBuildInfo[] = "UAVX_ACTOR_SRC_HASH=" UAVX_ACTOR_SRC_HASH;

}  // extern "C"

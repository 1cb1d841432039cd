// LayerNorm of the transformer blocks with the residual add in front of it folded in:
//     h = x + delta (rounded to the storage type),   y = LayerNorm(h)·γ + β,      rows [M, C], last dimension contiguous,
// and its backward with the residual gradient joined in:
//     x̂ = (h − mean)·rstd,  g = dy·γ,   dx = rstd·(g − mean_c(g) − x̂·mean_c(g·x̂)) + dh.
// Stock PyTorch writes the residual sum with one kernel and reads it back with the LayerNorm; in the backward it writes the
// LayerNorm's input gradient and reads it back with the add that joins the residual gradient.  Here each way is ONE streaming
// launch: every tensor is read once and written once.
//
// One wave owns a row (four rows per 256-thread workgroup, grid-stride over the rows).  A row of C ≤ 2048 16-bit channels is
// C/8 ≤ 256 16-byte chunks, at most R = 4 per lane (chunk i of the row belongs to lane i % 64, round i / 64), and stays in
// registers between the passes: the mean, then the CENTRED sum of squares about that mean (not E[x²] − E[x]²), then the
// output.  Lanes whose chunk lies past the row load nothing and add zeros.  The reductions are the xor butterfly of
// `wave_sum`: a fixed order, the same on every lane, no LDS, no barrier, no atomics, no workspace — two runs are
// bit-identical and the launches record into a graph as they are.  γ (and β) stay packed in registers across a wave's rows.
// The statistics are computed from the ROUNDED h, which is what the stock composite normalises, what makes h bit-equal to
// the stock `x + delta`, and what lets the backward recompute x̂ from the saved h.  All arithmetic is fp32 up to the one
// rounding of h, y and dx.
#include "common.h"

namespace {

constexpr int kLnMaxC = 2048;    // 4 rounds × 64 lanes × 8 channels
constexpr int kLnThreads = 256;  // 4 waves = 4 rows per workgroup
constexpr int kLnMaxGrid = 1 << 16;

template <typename T> __device__ __forceinline__ Chunk<T> ln_load(const T* p) { return *reinterpret_cast<const Chunk<T>*>(p); }
template <typename T> __device__ __forceinline__ void ln_store(T* p, const Chunk<T>& c) { *reinterpret_cast<Chunk<T>*>(p) = c; }

// R: rounds of 64 chunks that cover the row (C ≤ 512·R).  ADD: delta is given and h is written.
template <typename T, int R, bool ADD>
__global__ __launch_bounds__(kLnThreads) void add_layer_norm_fwd_kernel(const T* x, const T* delta, const T* gamma, const T* beta,
                                                                       T* h, T* y, float* mean_out, float* rstd_out, int64_t M,
                                                                       int C, float eps) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, chunks = C >> 3;
    const float fc = (float)C;  // the means are true divisions: a constant row's mean is that constant exactly
    Chunk<T> gm[R], bt[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = lane + 64 * r;
        if (i < chunks) {
            gm[r] = ln_load(gamma + i * 8);
            bt[r] = ln_load(beta + i * 8);
        }
    }
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < M; row += (int64_t)gridDim.x * 4) {  // wave-uniform
        const int64_t base = row * C;
        float v[R][8];
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = lane + 64 * r;
            if (i < chunks) {
                Chunk<T> a = ln_load(x + base + i * 8);
                if (ADD) {
                    const Chunk<T> d = ln_load(delta + base + i * 8);
#pragma unroll
                    for (int e = 0; e < 8; ++e) a.v[e] = from_f32<T>(to_f32<T>(a.v[e]) + to_f32<T>(d.v[e]));
                    ln_store(h + base + i * 8, a);
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    v[r][e] = to_f32<T>(a.v[e]);
                    s += v[r][e];
                }
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[r][e] = 0.f;
            }
        }
        const float mean = wave_sum(s) / fc;
        float ss = 0.f;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (lane + 64 * r < chunks) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    v[r][e] -= mean;
                    ss = fmaf(v[r][e], v[r][e], ss);
                }
            }
        }
        const float rstd = rsqrtf(wave_sum(ss) / fc + eps);
        if (lane == 0) {
            mean_out[row] = mean;
            rstd_out[row] = rstd;
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = lane + 64 * r;
            if (i < chunks) {
                Chunk<T> o;
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    o.v[e] = from_f32<T>(fmaf(v[r][e] * rstd, to_f32<T>(gm[r].v[e]), to_f32<T>(bt[r].v[e])));
                ln_store(y + base + i * 8, o);
            }
        }
    }
}

// DH: the residual gradient dh is given and joins dx before its one rounding.
template <typename T, int R, bool DH>
__global__ __launch_bounds__(kLnThreads) void add_layer_norm_bwd_kernel(const T* dy, const T* dh, const T* h, const T* gamma,
                                                                       const float* mean_in, const float* rstd_in, T* dx,
                                                                       int64_t M, int C) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, chunks = C >> 3;
    const float fc = (float)C;
    Chunk<T> gm[R];
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (lane + 64 * r < chunks) gm[r] = ln_load(gamma + (lane + 64 * r) * 8);
    for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < M; row += (int64_t)gridDim.x * 4) {  // wave-uniform
        const int64_t base = row * C;
        const float mean = mean_in[row], rstd = rstd_in[row];
        float g[R][8], xh[R][8];
        Chunk<T> res[R];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = lane + 64 * r;
            if (i < chunks) {
                const Chunk<T> a = ln_load(h + base + i * 8), w = ln_load(dy + base + i * 8);
                if (DH) res[r] = ln_load(dh + base + i * 8);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    xh[r][e] = (to_f32<T>(a.v[e]) - mean) * rstd;
                    g[r][e] = to_f32<T>(w.v[e]) * to_f32<T>(gm[r].v[e]);
                    s1 += g[r][e];
                    s2 = fmaf(g[r][e], xh[r][e], s2);
                }
            }
        }
        const float k2 = wave_sum(s1) / fc, k1 = wave_sum(s2) / fc;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = lane + 64 * r;
            if (i < chunks) {
                Chunk<T> o;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float d = rstd * (g[r][e] - k2 - xh[r][e] * k1);
                    o.v[e] = from_f32<T>(DH ? d + to_f32<T>(res[r].v[e]) : d);
                }
                ln_store(dx + base + i * 8, o);
            }
        }
    }
}

int ln_grid(int64_t M) {
    const int64_t blocks = (M + 3) / 4;
    return (int)(blocks < kLnMaxGrid ? blocks : kLnMaxGrid);
}

int ln_check(int64_t M, int C, int dtype) {
    if (M < 1 || C < 1) return LORA_E_BADARG;
    if (dtype != LORA_F32 && dtype != LORA_F16 && dtype != LORA_BF16) return LORA_E_BADARG;
    if (dtype == LORA_F32 || C % 8 != 0 || C > kLnMaxC) return LORA_E_UNSUPPORTED;
    return LORA_OK;
}

template <typename T, int R>
void launch_fwd(const void* x, const void* delta, const void* gamma, const void* beta, void* h, void* y, float* mean, float* rstd,
                int64_t M, int C, float eps, hipStream_t s) {
    const dim3 grid(ln_grid(M)), block(kLnThreads);
    if (delta)
        hipLaunchKernelGGL((add_layer_norm_fwd_kernel<T, R, true>), grid, block, 0, s, static_cast<const T*>(x),
                           static_cast<const T*>(delta), static_cast<const T*>(gamma), static_cast<const T*>(beta),
                           static_cast<T*>(h), static_cast<T*>(y), mean, rstd, M, C, eps);
    else
        hipLaunchKernelGGL((add_layer_norm_fwd_kernel<T, R, false>), grid, block, 0, s, static_cast<const T*>(x),
                           static_cast<const T*>(nullptr), static_cast<const T*>(gamma), static_cast<const T*>(beta),
                           static_cast<T*>(nullptr), static_cast<T*>(y), mean, rstd, M, C, eps);
}

template <typename T, int R>
void launch_bwd(const void* dy, const void* dh, const void* h, const void* gamma, const float* mean, const float* rstd, void* dx,
                int64_t M, int C, hipStream_t s) {
    const dim3 grid(ln_grid(M)), block(kLnThreads);
    if (dh)
        hipLaunchKernelGGL((add_layer_norm_bwd_kernel<T, R, true>), grid, block, 0, s, static_cast<const T*>(dy),
                           static_cast<const T*>(dh), static_cast<const T*>(h), static_cast<const T*>(gamma), mean, rstd,
                           static_cast<T*>(dx), M, C);
    else
        hipLaunchKernelGGL((add_layer_norm_bwd_kernel<T, R, false>), grid, block, 0, s, static_cast<const T*>(dy),
                           static_cast<const T*>(nullptr), static_cast<const T*>(h), static_cast<const T*>(gamma), mean, rstd,
                           static_cast<T*>(dx), M, C);
}

template <typename T, typename... A> void run_fwd(int C, A... a) {
    switch ((C + 511) / 512) {
        case 1: return launch_fwd<T, 1>(a...);
        case 2: return launch_fwd<T, 2>(a...);
        case 3: return launch_fwd<T, 3>(a...);
        default: return launch_fwd<T, 4>(a...);
    }
}

template <typename T, typename... A> void run_bwd(int C, A... a) {
    switch ((C + 511) / 512) {
        case 1: return launch_bwd<T, 1>(a...);
        case 2: return launch_bwd<T, 2>(a...);
        case 3: return launch_bwd<T, 3>(a...);
        default: return launch_bwd<T, 4>(a...);
    }
}

}  // namespace

extern "C" int add_layer_norm_max_channels(void) { return kLnMaxC; }

extern "C" int add_layer_norm_fwd(const void* x, const void* delta, const void* gamma, const void* beta, void* h, void* y,
                                  float* mean, float* rstd, int64_t M, int C, float eps, int dtype, void* stream) {
    if (!x || !gamma || !beta || !y || !mean || !rstd || (delta == nullptr) != (h == nullptr)) return LORA_E_BADARG;
    if (const int st = ln_check(M, C, dtype)) return st;
    if (!aligned16(x) || !aligned16(delta) || !aligned16(gamma) || !aligned16(beta) || !aligned16(h) || !aligned16(y) ||
        (reinterpret_cast<uintptr_t>(mean) & 3u) || (reinterpret_cast<uintptr_t>(rstd) & 3u))
        return LORA_E_ALIGN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == LORA_F16)
        run_fwd<half_t>(C, x, delta, gamma, beta, h, y, mean, rstd, M, C, eps, s);
    else
        run_fwd<bf16_t>(C, x, delta, gamma, beta, h, y, mean, rstd, M, C, eps, s);
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}

extern "C" int add_layer_norm_bwd(const void* dy, const void* dh, const void* h, const void* gamma, const float* mean,
                                  const float* rstd, void* dx, int64_t M, int C, int dtype, void* stream) {
    if (!dy || !h || !gamma || !mean || !rstd || !dx) return LORA_E_BADARG;
    if (const int st = ln_check(M, C, dtype)) return st;
    if (!aligned16(dy) || !aligned16(dh) || !aligned16(h) || !aligned16(gamma) || !aligned16(dx) ||
        (reinterpret_cast<uintptr_t>(mean) & 3u) || (reinterpret_cast<uintptr_t>(rstd) & 3u))
        return LORA_E_ALIGN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == LORA_F16)
        run_bwd<half_t>(C, dy, dh, h, gamma, mean, rstd, dx, M, C, s);
    else
        run_bwd<bf16_t>(C, dy, dh, h, gamma, mean, rstd, dx, M, C, s);
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}

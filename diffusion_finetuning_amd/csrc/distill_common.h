// Device helpers shared by the two svd_distill kernel sets (distill.hip: block width 32, ranks 1–16; distill_wide.hip: block
// widths 48/64/80, ranks up to 64): the difference on load, the start block, the fixed-order workgroup sum and the
// torch.quantile + clamp by radix select.  Everything here is width-agnostic; workgroups are 256 threads.
#pragma once
#include "common.h"

namespace {

constexpr int kTile = 64;            // rows of a diff-GEMM tile
constexpr double kMaskEps = 1e-12;   // λ ≤ ε·λ_max: a dropped direction (σ below 1e-6·σ_1: fp32 noise)

// D = T(w1 − w0) as fp32: the reference subtracts in the weights' dtype (cli_svd.py:59-63), then .float() (:69).  The fp32
// difference of two 16-bit values rounded once to the 16-bit type is the correctly rounded 16-bit difference (24 ≥ 2·11 + 2).
template <typename T> __device__ __forceinline__ float diff_of(const T* w1, const T* w0, int64_t i) {
    const float d = to_f32(w1[i]) - to_f32(w0[i]);
    if constexpr (sizeof(T) == 4) return d;
    else return to_f32(from_f32<T>(d));
}

// Workgroup helpers (256 threads).  Reductions are fixed-order LDS trees: the results do not depend on timing.
__device__ double block_sum(double v, double* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

__device__ __forceinline__ float start_value(uint64_t seed, int64_t layer, int64_t e) {
    uint64_t x = seed ^ (uint64_t)(layer + 1) * 0x9E3779B97F4A7C15ull ^ (uint64_t)e * 0xD1B54A32D192ED03ull;
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return (float)(x >> 40) * (2.0f / 16777216.0f) - 1.0f;  // uniform in [-1, 1)
}

// ---------------------------------------------------------------------------------------------------------------------
// torch.quantile (linear interpolation) + torch.clamp(−hi, hi) over x[0..n) in place, by one workgroup.
// Radix select on order-preserving uint32 keys (−0 counted as +0), 4 passes of 8 bits per order statistic.
__device__ __forceinline__ uint32_t fkey(float f) {
    uint32_t u = __float_as_uint(f);
    if (f == 0.f) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float fkey_inv(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

__device__ float radix_select(const float* x, int64_t n, int64_t k, int* hist, int64_t* sh) {
    const int tid = threadIdx.x;
    uint32_t prefix = 0, pmask = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        hist[tid] = 0;
        __syncthreads();
        for (int64_t e = tid; e < n; e += 256) {
            const uint32_t key = fkey(x[e]);
            if ((key & pmask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1);
        }
        __syncthreads();
        if (tid == 0) {
            int64_t cum = 0;
            int b = 0;
            for (; b < 255; ++b) {
                if (cum + hist[b] > k) break;
                cum += hist[b];
            }
            sh[0] = prefix | ((uint32_t)b << shift);
            sh[1] = k - cum;
        }
        __syncthreads();
        prefix = (uint32_t)sh[0];
        k = sh[1];
        pmask |= 0xFFu << shift;
        __syncthreads();
    }
    return fkey_inv(prefix);
}

// returns hi (the clamp bound); x is clamped in place when `clamp`
__device__ float quantile_clamp(float* x, int64_t n, float q, bool clamp, int* hist, int64_t* sh) {
    // torch: ranks = q·(n−1) in the input's dtype (fp32), below = trunc, above = ceil, w = ranks − below,
    // lerp(a, b, w) = |w| < 0.5 ? a + w·(b − a) : b − (b − a)·(1 − w), each product-sum one fused multiply-add
    const float rank = __fmul_rn(q, (float)(n - 1));
    const int64_t lo = (int64_t)rank;
    const int64_t hi = (int64_t)ceilf(rank);
    const float w = __fsub_rn(rank, (float)lo);
    const float a = radix_select(x, n, lo, hist, sh);
    const float b = hi == lo ? a : radix_select(x, n, hi, hist, sh);
    const float d = __fsub_rn(b, a);
    const float v = fabsf(w) < 0.5f ? __fmaf_rn(w, d, a) : __fmaf_rn(-d, __fsub_rn(1.f, w), b);
    if (clamp) {
        const float lo_v = -v;
        for (int64_t e = threadIdx.x; e < n; e += 256) x[e] = fminf(fmaxf(x[e], lo_v), v);  // torch.clamp(min, max)
        __syncthreads();
    }
    return v;
}

// Final factors of one layer into up[0 ..]: up [N,r] = U_r·diag(σ_r), then down [r,K] = V_rᵀ; the sign of each pair makes the
// largest-magnitude entry of the down row positive (ties: lowest index); then the quantile clamp.  U and V are the layer's
// blocks with row stride W, lam its λ, flag its state word (set to 3 on a non-finite factor); r ≤ MAXR.
template <int MAXR>
__device__ __forceinline__ void finalize_layer(const float* U, const float* V, const double* lam, int* flag, int64_t N,
                                               int64_t K, int W, int r, float q, int clamp, float* up) {
    const int tid = threadIdx.x;
    __shared__ float redv[256];
    __shared__ int64_t redi[256];
    __shared__ float sgn[MAXR];
    __shared__ int hist[256];
    __shared__ int64_t sh[2];
    __shared__ int bad;
    for (int i = 0; i < r; ++i) {
        float best = -1.f;
        int64_t bi = 0;
        for (int64_t k = tid; k < K; k += 256) {
            const float a = fabsf(V[k * W + i]);
            if (a > best) {
                best = a;
                bi = k;
            }
        }
        redv[tid] = best;
        redi[tid] = bi;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s) {
                const float o = redv[tid + s];
                const int64_t oi = redi[tid + s];
                if (o > redv[tid] || (o == redv[tid] && oi < redi[tid])) {
                    redv[tid] = o;
                    redi[tid] = oi;
                }
            }
            __syncthreads();
        }
        if (tid == 0) sgn[i] = V[redi[0] * W + i] < 0.f ? -1.f : 1.f;
        __syncthreads();
    }
    if (tid == 0) bad = 0;
    __syncthreads();
    float* down = up + N * r;
    int my_bad = 0;
    for (int64_t e = tid; e < N * r; e += 256) {
        const int i = (int)(e % r);
        float v = (float)((double)U[(e / r) * W + i] * sqrt(lam[i]));
        if (sgn[i] < 0.f) v = -v;
        my_bad |= !isfinite(v);
        up[e] = v;
    }
    for (int64_t e = tid; e < (int64_t)r * K; e += 256) {
        const int i = (int)(e / K);
        float v = V[(e % K) * W + i];
        if (sgn[i] < 0.f) v = -v;
        my_bad |= !isfinite(v);
        down[e] = v;
    }
    if (my_bad) atomicOr(&bad, 1);
    __syncthreads();
    if (bad) {
        if (tid == 0) *flag = 3;
        return;
    }
    if (clamp) quantile_clamp(up, (N + K) * r, q, true, hist, sh);
}

}  // namespace

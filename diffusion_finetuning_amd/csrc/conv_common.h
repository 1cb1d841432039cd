// What the two packed-weight 3x3 convolution families (conv_small.hip, conv_large.hip) share: the MFMA wrapper, the padded
// image coordinates of the LDS staging area and the constants of the pack layout (documented in conv_small.hip).
#pragma once
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 32;      // input channels per staged chunk = one MFMA K-step
constexpr int kPitch = 80;      // bytes per LDS position: 32 channels + 16 bytes (16 consecutive positions hit 16 distinct slots)
constexpr int kCUs = 256;

template <typename T> struct Mfma;
template <> struct Mfma<half_t> {
    using Frag = f16x8;
    static __device__ __forceinline__ f32x4 run(Frag a, Frag b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
    }
};
template <> struct Mfma<bf16_t> {
    using Frag = bf16x8;
    static __device__ __forceinline__ f32x4 run(Frag a, Frag b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
};

// padded-coordinate position of pixel m (both host and device)
__host__ __device__ __forceinline__ int padded_pos(int m, int H, int W) {
    const int HW = H * W, img = m / HW, r = m - img * HW, h = r / W, w = r - h * W;
    return img * (H + 2) * (W + 2) + (h + 1) * (W + 2) + (w + 1);
}
// positions a tile of pixels [m0, m0 + MT) ∩ [0, M) stages: from its first pixel's tap (0,0) to its last pixel's tap (2,2)
__host__ __device__ __forceinline__ int tile_positions(int m0, int MT, int M, int H, int W) {
    const int mlast = (m0 + MT < M ? m0 + MT : M) - 1;
    return padded_pos(mlast, H, W) - padded_pos(m0, H, W) + 2 * (W + 3) + 1;
}

// n / d for 0 <= n < 2^22 (the geometry functions bound the padded positions) through the float reciprocal, corrected by one
// either way
__device__ __forceinline__ int fast_div(int n, int d, float inv) {
    int q = (int)((float)n * inv);
    int r = n - q * d;
    q += r >= d ? 1 : 0;
    q -= r < 0 ? 1 : 0;
    return q;
}

// the 32-bit indexing envelope both families share: every element offset and every padded position fits an int
inline bool conv_shape_in_range(int N, int Cin, int Cout, int H, int W) {
    if (N < 1 || H < 1 || W < 1 || Cin < 32 || Cout < 32 || Cin % 32 || Cout % 32) return false;
    const int64_t M64 = (int64_t)N * H * W;
    return !(M64 > (1 << 22) || M64 * Cin >= (1ll << 31) || M64 * Cout >= (1ll << 31) || (int64_t)(H + 2) * (W + 2) * N >= (1ll << 22));
}

}  // namespace

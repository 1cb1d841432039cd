// Max-norm constraint on the learned update of every LoRA layer of the flat fp32 slab, in ONE launch: the Frobenius norm of
// ΔW = scale·up·down per layer, and — above the bound — both factors scaled back onto it.  No line of the reference does this;
// the rule is restated from its published definition ("Max-norm constraint"; include/lora_hip.h: lora_max_norm).
//   ‖up·down‖_F² = Σ_ij (down·downᵀ)_ij · (upᵀ·up)_ij
// needs the two r×r Gram matrices only, so a layer costs one read of its own factors (and, when it is scaled, one more read and
// one write of them, from L2) and never forms the [N,K] product.
// One workgroup per layer, 1024 threads (DESIGN.md says what else was measured).  The reduction dimension (the N rows of up, the
// K columns of down) is staged through LDS in chunks as [row][r4] (r4 = r rounded up to 4, the pad zero), whatever the layer's
// alignment in the slab; a thread owns one 4×4 tile of the Gram's upper triangle and one of S = 1024 / tiles row slots,
// accumulates its rows in increasing order in fp32 registers, and the S slots are summed by a binary tree in LDS.  Every sum has
// an order that follows from (rows, r) alone: no atomics on floating-point values, the same bits on every run and for every grid.
#include "common.h"

namespace {

constexpr int NT = 1024;       // threads of a workgroup
constexpr int kStage = 16384;  // floats of staging LDS: a chunk of the factors, then the tree's 4 × NT float4 (and NT doubles)
constexpr int kMaxRank = 64;

static_assert(kStage >= 16 * NT, "the slot tree keeps 16 floats per thread in the staging buffer");

// G (r4 × r4, LDS) = Σ_ρ x_ρ·x_ρᵀ over `rows` vectors x_ρ of r elements: element i of vector ρ is src[ρ·r + i] (row_major: up) or
// src[i·ld + ρ] (down).  Ends with the workgroup synchronised and G complete.
__device__ __forceinline__ void gram(const float* __restrict__ src, int rows, int r, int r4, bool row_major, int64_t ld, float* G,
                                     float* stage) {
    const int t = threadIdx.x;
    const int nt = r4 >> 2, ntiles = nt * (nt + 1) / 2;
    const int S = NT / ntiles;  // >= 7 (r = 64: 136 tiles)
    const int q = t % ntiles, s = t / ntiles;
    const bool active = s < S;
    int ti = 0, rem = q;  // tile q of the upper triangle, row by row: (ti, tj >= ti)
    while (rem >= nt - ti) {
        rem -= nt - ti;
        ++ti;
    }
    const int tj = ti + rem;
    float acc[4][4];
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) acc[x][y] = 0.f;
    const int chunk_rows = kStage / r4;
    for (int r0 = 0; r0 < rows; r0 += chunk_rows) {
        const int R = rows - r0 < chunk_rows ? rows - r0 : chunk_rows;
        if (row_major && r == r4) {  // a contiguous piece of the slab, copied as it lies
            const float* p = src + (int64_t)r0 * r;
#pragma unroll 4
            for (int idx = t; idx < R * r4; idx += NT) stage[idx] = p[idx];
        } else if (row_major) {
#pragma unroll 4
            for (int idx = t; idx < R * r4; idx += NT) {
                const int rho = idx / r4, i = idx - rho * r4;
                stage[idx] = i < r ? src[(int64_t)(r0 + rho) * r + i] : 0.f;
            }
        } else {  // lanes along the contiguous dimension of down; transposed on the way into LDS
#pragma unroll 4
            for (int idx = t; idx < R * r4; idx += NT) {
                const int i = idx / R, rho = idx - i * R;
                stage[rho * r4 + i] = i < r ? src[(int64_t)i * ld + r0 + rho] : 0.f;
            }
        }
        __syncthreads();
        if (active) {
            for (int rho = s; rho < R; rho += S) {
                const float4 a = *reinterpret_cast<const float4*>(stage + rho * r4 + 4 * ti);
                const float4 b = *reinterpret_cast<const float4*>(stage + rho * r4 + 4 * tj);
                const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
                for (int x = 0; x < 4; ++x)
#pragma unroll
                    for (int y = 0; y < 4; ++y) acc[x][y] = fmaf(av[x], bv[y], acc[x][y]);
            }
        }
        __syncthreads();
    }
    // the S row slots of a tile, summed by a binary tree over the slot index (slot s takes slot s + half): [e4][thread] float4
    float4* sc = reinterpret_cast<float4*>(stage);
#pragma unroll
    for (int x = 0; x < 4; ++x) sc[x * NT + t] = make_float4(acc[x][0], acc[x][1], acc[x][2], acc[x][3]);
    __syncthreads();
    for (int cur = S; cur > 1;) {
        const int half = (cur + 1) >> 1;
        if (active && s + half < cur) {
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                float4 mine = sc[x * NT + t];
                const float4 other = sc[x * NT + t + half * ntiles];
                mine.x += other.x;
                mine.y += other.y;
                mine.z += other.z;
                mine.w += other.w;
                sc[x * NT + t] = mine;
            }
        }
        __syncthreads();
        cur = half;
    }
    if (t < ntiles) {  // slot 0 holds the tile; its mirror image fills the lower triangle
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            const float4 v4 = sc[x * NT + t];
            const float v[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
            for (int y = 0; y < 4; ++y) {
                G[(4 * ti + x) * r4 + 4 * tj + y] = v[y];
                G[(4 * tj + y) * r4 + 4 * ti + x] = v[y];
            }
        }
    }
    __syncthreads();
}

// p[0..n) *= f, one fp32 multiply per element: 16 bytes per lane between a scalar head and tail (a layer starts anywhere)
__device__ __forceinline__ void scale_range(float* p, int64_t n, float f) {
    const int t = threadIdx.x;
    int64_t head = (int64_t)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) >> 2);
    if (head > n) head = n;
    for (int64_t i = t; i < head; i += NT) p[i] = p[i] * f;
    float4* p4 = reinterpret_cast<float4*>(p + head);
    const int64_t nvec = (n - head) >> 2;
    for (int64_t i = t; i < nvec; i += NT) {
        float4 v = p4[i];
        v.x *= f;
        v.y *= f;
        v.z *= f;
        v.w *= f;
        p4[i] = v;
    }
    for (int64_t i = head + (nvec << 2) + t; i < n; i += NT) p[i] = p[i] * f;
}

__global__ __launch_bounds__(NT) void max_norm_kernel(float* params, const int64_t* __restrict__ table, int max_r, float max_norm,
                                                      float* stats, int* counters) {
    extern __shared__ __attribute__((aligned(16))) float smem_f[];
    const int l = blockIdx.x, t = threadIdx.x;
    const int64_t* e = table + (int64_t)l * 8;
    const int64_t up_off = e[0], down_off = e[1];
    const int64_t K64 = e[2], N64 = e[3], r64 = e[4];
    if (up_off < 0 || down_off < 0 || K64 < 1 || N64 < 1 || K64 > 0x7fffffff || N64 > 0x7fffffff || r64 < 1 || r64 > max_r) {
        if (t == 0) {  // a row the kernel cannot run (workgroup-uniform): nothing touched, norm −1
            stats[2 * (int64_t)l] = -1.f;
            stats[2 * (int64_t)l + 1] = 1.f;
        }
        return;
    }
    const int K = (int)K64, N = (int)N64, r = (int)r64;
    const float scale = __int_as_float((int)e[5]);
    const int r4 = (r + 3) & ~3;
    const int max_r4 = (max_r + 3) & ~3;
    float* stage = smem_f;
    float* GA = smem_f + kStage;         // down·downᵀ
    float* GB = GA + max_r4 * max_r4;    // upᵀ·up
    float* s_factor = GB + max_r4 * max_r4;
    float* up = params + up_off;
    float* down = params + down_off;
    gram(up, N, r, r4, true, 0, GB, stage);
    gram(down, K, r, r4, false, K, GA, stage);
    // n² = scale²·Σ_ij GA_ij·GB_ij in double: a strided partial per thread, then a binary tree over the threads
    double part = 0.0;
    for (int i = t; i < r4 * r4; i += NT) part += (double)GA[i] * (double)GB[i];
    double* sd = reinterpret_cast<double*>(stage);
    sd[t] = part;
    __syncthreads();
    for (int off = NT >> 1; off > 0; off >>= 1) {
        if (t < off) sd[t] += sd[t + off];
        __syncthreads();
    }
    if (t == 0) {
        const double n2 = (double)scale * (double)scale * sd[0];
        const double norm = sqrt(n2 > 0.0 ? n2 : 0.0);
        const float factor = norm > (double)max_norm ? (float)sqrt((double)max_norm / norm) : 1.f;
        stats[2 * (int64_t)l] = (float)norm;
        stats[2 * (int64_t)l + 1] = factor;
        if (factor != 1.f && counters) atomicAdd(counters, 1);  // (an integer count: any order of arrival gives the same value)
        *s_factor = factor;
    }
    __syncthreads();
    const float factor = *s_factor;
    if (factor == 1.f) return;  // (workgroup-uniform) a layer inside the bound is not written at all
    scale_range(up, (int64_t)N * r, factor);
    scale_range(down, (int64_t)r * K, factor);
}

int lds_bytes(int max_r) {
    const int r4 = (max_r + 3) & ~3;
    return (kStage + 2 * r4 * r4 + 4) * 4;
}

}  // namespace

extern "C" int lora_max_norm(float* params, const int64_t* table, int n_layers, int max_r, float max_norm, float* stats,
                             int* counters, void* stream) {
    if (!params || !table || !stats || n_layers < 1 || !(max_norm > 0.f)) return LORA_E_BADARG;  // (NaN fails the comparison)
    if (max_r < 1 || max_r > kMaxRank) return LORA_E_RANK;
    const int lds = lds_bytes(max_r);
    static const bool ok = hipFuncSetAttribute(reinterpret_cast<const void*>(max_norm_kernel),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes(kMaxRank)) == hipSuccess;
    if (!ok) return LORA_E_LAUNCH;
    hipLaunchKernelGGL(max_norm_kernel, dim3((unsigned)n_layers), dim3(NT), lds, static_cast<hipStream_t>(stream), params, table,
                       max_r, max_norm, stats, counters);
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}

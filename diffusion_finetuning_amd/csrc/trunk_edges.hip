// The passes at the edges of the UNet trunk's blocks that move or add activations and compute nothing else, each as one
// streaming kernel with 16-byte global accesses, fp32 sums and one rounding at the store:
//   * residual_bias_add: out = res + h + b1[c] (+ b2[c]) on NCHW tensors, the tail of a ResNet block.  The biases of conv2 and
//     conv_shortcut, which the convolution library adds in a pass of its own over each output, and the residual sum: one pass
//     instead of up to three.
//   * tokens_to_nchw_add / nchw_to_tokens: the [N, H·W, C] ↔ [N, C, H·W] re-layouts at a transformer's exit and entry, the first
//     with the residual added on the way (out[n,c,p] = res[n,c,p] + tok[n,p,c]).  Both are ONE kernel, a batched transpose of
//     16-bit [R, Q] matrices with an optional addend in the destination's layout: R = H·W, Q = C one way, R = C, Q = H·W back.
// No reductions, no atomics, no workspace: every output element is written once by one thread and two runs are bit-identical.
//
// The transposing tile is 64 × 64 elements in LDS, [64][66] halves (8448 bytes per workgroup of 256 threads).  A thread loads
// two 16-byte chunks of source rows (8 lanes cover 128 contiguous bytes of a row) and scatters each chunk's 8 elements down a
// tile column with 2-byte stores: at the 33-dword row stride the 32 lanes of a store group fall on 16 banks, two addresses
// each, which a store's own issue time covers.  It then reads 16-byte runs of tile rows as four dwords (lane groups of 32 on
// 32 distinct banks: dword j·33 + 4·i + w, j = 0..3, i = 0..7) and writes them as whole chunks, again 128 contiguous bytes per
// 8 lanes.  Ragged edges are cut in whole chunks (R % 8 == 0 and Q % 8 == 0), so a tile cell is read only if it was loaded.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): no scratch in any kernel; transpose_add_kernel 8448 bytes
// of LDS and at most 24 VGPRs, so the 8 waves per SIMD (8 workgroups per CU) are limited by the wave slots, not by LDS (19
// workgroups would fit) or registers; residual_bias_add_kernel no LDS, occupancy 8.
#include "common.h"

namespace {

constexpr int kTile = 64;              // tile edge in elements
constexpr int kTileStride = kTile + 2;  // halves per tile row: 33 dwords

template <typename T> __device__ __forceinline__ Chunk<T> load_chunk(const T* p) { return *reinterpret_cast<const Chunk<T>*>(p); }

// out[row, :] = res[row, :] + h[row, :] + b1[c] (+ b2[c]), row = n·C + c of HW elements; one chunk per thread
template <typename T>
__global__ __launch_bounds__(256) void residual_bias_add_kernel(const T* h, const T* res, const T* b1, const T* b2, T* out,
                                                                int64_t chunks, int cpr, int C) {
    constexpr int VEC = ElemTraits<T>::kVec;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= chunks) return;
    const int c = (int)((i / cpr) % C);
    float b = to_f32<T>(b1[c]);
    if (b2) b += to_f32<T>(b2[c]);
    const Chunk<T> u = load_chunk(h + i * VEC), v = load_chunk(res + i * VEC);
    Chunk<T> o;
#pragma unroll
    for (int e = 0; e < VEC; ++e) o.v[e] = from_f32<T>(to_f32<T>(v.v[e]) + to_f32<T>(u.v[e]) + b);
    *reinterpret_cast<Chunk<T>*>(out + i * VEC) = o;
}

// dst[n, q, r] = src[n, r, q] (+ add[n, q, r]) for src [N, R, Q]; grid (⌈Q/64⌉, ⌈R/64⌉, N)
template <typename T, bool ADD>
__global__ __launch_bounds__(256) void transpose_add_kernel(const T* src, const T* add, T* dst, int R, int Q) {
    static_assert(sizeof(T) == 2, "16-bit elements");
    __shared__ uint32_t tile32[kTile * kTileStride / 2];
    T* tile = reinterpret_cast<T*>(tile32);
    const int64_t base = (int64_t)blockIdx.z * R * Q;
    const int r0 = blockIdx.y * kTile, q0 = blockIdx.x * kTile;
#pragma unroll
    for (int k = 0; k < 2; ++k) {  // source rows r0 + r, chunk qc of the row → tile[q][r]
        const int id = threadIdx.x + k * 256, r = id >> 3, qc = id & 7;
        if (r0 + r < R && q0 + qc * 8 < Q) {
            const Chunk<T> v = load_chunk(src + base + (int64_t)(r0 + r) * Q + q0 + qc * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) tile[(qc * 8 + e) * kTileStride + r] = v.v[e];
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2; ++k) {  // destination rows q0 + q, chunk rc of the row ← tile[q][8·rc .. 8·rc + 8)
        const int id = threadIdx.x + k * 256, q = id >> 3, rc = id & 7;
        if (q0 + q < Q && r0 + rc * 8 < R) {
            union {
                uint32_t w[4];
                Chunk<T> c;
            } t;
#pragma unroll
            for (int w = 0; w < 4; ++w) t.w[w] = tile32[q * (kTileStride / 2) + rc * 4 + w];
            const int64_t off = base + (int64_t)(q0 + q) * R + r0 + rc * 8;
            if (ADD) {
                const Chunk<T> a = load_chunk(add + off);
#pragma unroll
                for (int e = 0; e < 8; ++e) t.c.v[e] = from_f32<T>(to_f32<T>(t.c.v[e]) + to_f32<T>(a.v[e]));
            }
            *reinterpret_cast<Chunk<T>*>(dst + off) = t.c;
        }
    }
}

// what the transposing kernel takes: 16-bit elements, whole chunks both ways, a grid the launch can express
int check_transpose(int N, int R, int Q, int dtype) {
    if (N < 1 || R < 1 || Q < 1) return LORA_E_BADARG;
    if (dtype == LORA_F32) return LORA_E_UNSUPPORTED;
    if (dtype != LORA_F16 && dtype != LORA_BF16) return LORA_E_BADARG;
    if (R % 8 || Q % 8 || N > 65535 || (R + kTile - 1) / kTile > 65535) return LORA_E_UNSUPPORTED;
    return LORA_OK;
}

template <typename T>
int run_transpose(const void* src, const void* add, void* dst, int N, int R, int Q, hipStream_t s) {
    const dim3 grid((Q + kTile - 1) / kTile, (R + kTile - 1) / kTile, N);
    if (add)
        hipLaunchKernelGGL((transpose_add_kernel<T, true>), grid, dim3(256), 0, s, static_cast<const T*>(src),
                           static_cast<const T*>(add), static_cast<T*>(dst), R, Q);
    else
        hipLaunchKernelGGL((transpose_add_kernel<T, false>), grid, dim3(256), 0, s, static_cast<const T*>(src),
                           static_cast<const T*>(nullptr), static_cast<T*>(dst), R, Q);
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}

int transpose_entry(const void* src, const void* add, void* dst, int N, int R, int Q, int dtype, void* stream) {
    if (!src || !dst) return LORA_E_BADARG;
    if (const int st = check_transpose(N, R, Q, dtype)) return st;
    if (!aligned16(src) || !aligned16(add) || !aligned16(dst)) return LORA_E_ALIGN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return dtype == LORA_F16 ? run_transpose<half_t>(src, add, dst, N, R, Q, s) : run_transpose<bf16_t>(src, add, dst, N, R, Q, s);
}

template <typename T>
int run_residual(const void* h, const void* res, const void* b1, const void* b2, void* out, int N, int C, int HW, hipStream_t s) {
    const int64_t chunks = (int64_t)N * C * HW / 8;
    hipLaunchKernelGGL(residual_bias_add_kernel<T>, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, s,
                       static_cast<const T*>(h), static_cast<const T*>(res), static_cast<const T*>(b1), static_cast<const T*>(b2),
                       static_cast<T*>(out), chunks, HW / 8, C);
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}

int check_residual(int N, int C, int HW, int dtype) {
    if (N < 1 || C < 1 || HW < 1) return LORA_E_BADARG;
    if (dtype == LORA_F32) return LORA_E_UNSUPPORTED;
    if (dtype != LORA_F16 && dtype != LORA_BF16) return LORA_E_BADARG;
    if (HW % 8 || (int64_t)N * C * HW / 8 > (int64_t)256 * 0x7fffffff) return LORA_E_UNSUPPORTED;
    return LORA_OK;
}

}  // namespace

extern "C" int residual_bias_add_supported(int N, int C, int HW, int dtype) { return check_residual(N, C, HW, dtype) == LORA_OK; }

extern "C" int residual_bias_add(const void* h, const void* res, const void* b1, const void* b2, void* out, int N, int C, int HW,
                                 int dtype, void* stream) {
    if (!h || !res || !b1 || !out) return LORA_E_BADARG;
    if (const int st = check_residual(N, C, HW, dtype)) return st;
    if (!aligned16(h) || !aligned16(res) || !aligned16(out)) return LORA_E_ALIGN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return dtype == LORA_F16 ? run_residual<half_t>(h, res, b1, b2, out, N, C, HW, s)
                             : run_residual<bf16_t>(h, res, b1, b2, out, N, C, HW, s);
}

extern "C" int tokens_nchw_supported(int N, int C, int HW, int dtype) { return check_transpose(N, HW, C, dtype) == LORA_OK; }

extern "C" int tokens_to_nchw_add(const void* tok, const void* res, void* out, int N, int C, int HW, int dtype, void* stream) {
    return transpose_entry(tok, res, out, N, HW, C, dtype, stream);
}

extern "C" int nchw_to_tokens(const void* x, void* tok, int N, int C, int HW, int dtype, void* stream) {
    return transpose_entry(x, nullptr, tok, N, C, HW, dtype, stream);
}

// Packing of the fp32 LoRA factors into the rank-padded tiles that the fused GEMM (lora_gemm.hip) and the grouped launches
// (groups.py) stage like operand tiles: lora_pack_factors, lora_pack_factors_batched, lora_pack_items.
#include "common.h"

namespace {

// Packed factors, both orientations per factor (dtype T, rank padded to 16 with zeros):
//   Apack = [ A16 [16,K] : A16[j,k] = A[j,k] | At16 [K,16] : At16[k,j] = A[j,k] ]      (32·K elements)
//   Bpack = [ Bt16[16,N] : Bt16[j,n] = B[n,j] | B16 [N,16] : B16[n,j] = B[n,j] ]       (32·N elements)
// The [16,len] halves are the main-loop factor tiles (F), the [len,16] halves the epilogue factors (Q).
template <typename T>
__device__ __forceinline__ void pack_one(const float* A, const float* B, T* Apack, T* Bpack, int K, int N, int r,
                                         int which, int start, int step) {
    const int len = which == 0 ? K : N;
    T* dst = which == 0 ? Apack : Bpack;
    for (int idx = start; idx < kRP * len; idx += step) {
        const int j = idx / len, c = idx - j * len;
        const int jj = j < r ? j : r - 1;
        const float v = which == 0 ? A[(int64_t)jj * K + c] : B[(int64_t)c * r + jj];
        const T t = from_f32<T>(j < r ? v : 0.f);
        dst[idx] = t;                                   // [16, len]
        dst[(int64_t)kRP * len + (int64_t)c * kRP + j] = t;  // [len, 16]
    }
}
template <typename T>
__global__ __launch_bounds__(256) void pack_factor_kernel(const float* A, const float* B, T* Apack, T* Bpack, int K,
                                                          int N, int r) {
    pack_one<T>(A, B, Apack, Bpack, K, N, r, blockIdx.y, blockIdx.x * 256 + threadIdx.x, gridDim.x * 256);
}

// All layers of a slab in one launch.  table[l] = {a_off, b_off, K, N, r, apack_off, bpack_off, 0}: element
// offsets of A[r,K] / B[N,r] inside `params` (fp32) and of Apack / Bpack inside `packed` (T).
template <typename T>
__global__ __launch_bounds__(256) void pack_factors_batched_kernel(const int64_t* table, const float* params,
                                                                   T* packed) {
    const int64_t* e = table + (int64_t)(blockIdx.y >> 1) * 8;
    const int K = (int)e[2], N = (int)e[3], r = (int)e[4];
    if (r > kRP) return;
    pack_one<T>(params + e[0], params + e[1], packed + e[5], packed + e[6], K, N, r, blockIdx.y & 1,
                blockIdx.x * 256 + threadIdx.x, gridDim.x * 256);
}

// Generalised packing for grouped layers: one table row per FACTOR,
//   {src_off, which (0: A [r,len] / 1: B [len,r]), len, r, d16_off, d16_ld, dT_off, rows}
// writes rows j < `rows` of the [16,len] form at packed[d16_off + j·d16_ld + c] and/or columns j < `rows` of the [len,16]
// form at packed[dT_off + c·16 + j] (an offset of -1 skips that form).  rows = 16 zero-fills the unused rank rows; a
// block-diagonal group passes rows = r and pre-offset destinations so that every member fills only its own rank slots of
// a buffer that was zeroed once.
template <typename T>
__global__ __launch_bounds__(256) void pack_items_kernel(const int64_t* table, const float* params, T* packed) {
    const int64_t* e = table + (int64_t)blockIdx.y * 8;
    const float* src = params + e[0];
    const int which = (int)e[1], len = (int)e[2], r = (int)e[3], rows = (int)e[7];
    const int64_t d16 = e[4], ld16 = e[5], dT = e[6];
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < rows * len; idx += gridDim.x * 256) {
        const int j = idx / len, c = idx - j * len;
        const int jj = j < r ? j : r - 1;
        const float v = which == 0 ? src[(int64_t)jj * len + c] : src[(int64_t)c * r + jj];
        const T t = from_f32<T>(j < r ? v : 0.f);
        if (d16 >= 0) packed[d16 + (int64_t)j * ld16 + c] = t;
        if (dT >= 0) packed[dT + (int64_t)c * kRP + j] = t;
    }
}

// Grid of the two table-driven kernels: up to 64 workgroups stride over the longest factor, one grid row per table entry.
dim3 table_grid(int max_len, int rows) {
    const int blocks = (kRP * max_len + 255) / 256;
    return dim3((unsigned)(blocks > 64 ? 64 : blocks), rows);
}

}  // namespace

extern "C" int lora_pack_factors(const float* A, const float* B, void* Apack, void* Bpack, int K, int N, int r,
                                 int dtype, void* stream) {
    if (!A || !B || !Apack || !Bpack || K < 1 || N < 1) return LORA_E_BADARG;
    if (r < 1 || r > (K < N ? K : N)) return LORA_E_RANK;
    if (r > kRP) return LORA_OK;  // large ranks run on the generic kernels, which read the fp32 masters
    const int len = K > N ? K : N;
    const dim3 grid((unsigned)((kRP * len + 255) / 256), 2);
    return by_dtype(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(pack_factor_kernel<T>, grid, dim3(256), 0, static_cast<hipStream_t>(stream), A, B,
                           static_cast<T*>(Apack), static_cast<T*>(Bpack), K, N, r);
    });
}

extern "C" int lora_pack_factors_batched(const int64_t* table, int n_layers, int max_len, const float* params,
                                         void* packed, int dtype, void* stream) {
    if (!table || !params || !packed || n_layers < 1 || max_len < 1) return LORA_E_BADARG;
    return by_dtype(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(pack_factors_batched_kernel<T>, table_grid(max_len, 2 * n_layers), dim3(256), 0,
                           static_cast<hipStream_t>(stream), table, params, static_cast<T*>(packed));
    });
}

extern "C" int lora_pack_items(const int64_t* table, int n_items, int max_len, const float* params, void* packed,
                               int dtype, void* stream) {
    if (!table || !params || !packed || n_items < 1 || max_len < 1) return LORA_E_BADARG;
    return by_dtype(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(pack_items_kernel<T>, table_grid(max_len, n_items), dim3(256), 0, static_cast<hipStream_t>(stream),
                           table, params, static_cast<T*>(packed));
    });
}

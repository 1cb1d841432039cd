// The fused LoRA GEMM without shape conditions: one thread per output element.  Included by lora_gemm.hip alone
// (launch_typed() falls back to these kernels).
#pragma once
#include "common.h"

namespace {

// Shape-agnostic path (unaligned sizes or r > 16): correct, not fast.  F/Q read as fp32 masters.
struct GenericParams {
    const void* Am;
    const void* Bm;
    const void* bias;
    const float* F;
    int64_t f_sr, f_sk;
    const float* Q;
    int64_t q_sn, q_sj;
    void* C;
    float* P;
    int64_t M;
    int Kc, Nc, r;
    float scale;
    const float* row_scale;  // RS kernel: per-sample gates (GemmParams::row_scale)
    int64_t rs_rps;
    int rs_ld;
};
template <typename T>
__global__ void lora_skinny_generic_kernel(GenericParams p) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= p.M * p.r) return;
    const int64_t m = idx / p.r;
    const int j = (int)(idx - m * p.r);
    const T* a = static_cast<const T*>(p.Am) + m * p.Kc;
    float s = 0.f;
    for (int k = 0; k < p.Kc; ++k) s += to_f32<T>(a[k]) * to_f32<T>(from_f32<T>(p.F[j * p.f_sr + k * p.f_sk]));
    p.P[idx] = s;
}
// f − f0 with f = scale·g rounded on its own: contracted into one fma the difference of two EQUAL factors would be the product's
// rounding error instead of zero
__device__ __forceinline__ float gate_deviation(float scale, float g, float f0) {
#pragma clang fp contract(off)
    const float f = scale * g;
    return f - f0;
}
template <typename T, bool RS = false>
__global__ void lora_gemm_generic_kernel(GenericParams p) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= p.M * p.Nc) return;
    const int64_t m = idx / p.Nc;
    const int n = (int)(idx - m * p.Nc);
    const T* a = static_cast<const T*>(p.Am) + m * p.Kc;
    const T* b = static_cast<const T*>(p.Bm) + (int64_t)n * p.Kc;
    float s = 0.f;
    for (int k = 0; k < p.Kc; ++k) s += to_f32<T>(a[k]) * to_f32<T>(b[k]);
    float l = 0.f;
    if constexpr (RS) {
        // This kernel's ungated form scales the SUM, s·(Σ_j P_j·Q_j) — there is no per-row s·P to put a factor into, as the MFMA
        // epilogues have.  With f_j = scale·G[sample][j] (formed first, in fp32) the gated form is that same arithmetic at the
        // factor of slot 0 plus the other slots' deviations from it,
        //     Σ_j f_j·P_j·Q_j = f_0·(Σ_j P_j·Q_j) + Σ_j ((f_j − f_0)·P_j)·Q_j ,
        // so a row whose gates are all equal — a uniform table, a table of ones under any scale, a closed sample — is the
        // ungated launch at that factor bit for bit (every deviation is an exact zero), as it is on the MFMA forms.
        const float* g = p.row_scale + (m / p.rs_rps) * p.rs_ld;
        const float f0 = p.scale * g[0];
        float dev = 0.f;
        for (int j = 0; j < p.r; ++j) {
            const float q = to_f32<T>(from_f32<T>(p.Q[(int64_t)n * p.q_sn + j * p.q_sj]));
            l += p.P[m * p.r + j] * q;
            dev += (gate_deviation(p.scale, g[j], f0) * p.P[m * p.r + j]) * q;
        }
        s += f0 * l;
        s += dev;
    } else {
    for (int j = 0; j < p.r; ++j)
        l += p.P[m * p.r + j] * to_f32<T>(from_f32<T>(p.Q[(int64_t)n * p.q_sn + j * p.q_sj]));
    s += p.scale * l;
    }
    if (p.bias) s += to_f32<T>(static_cast<const T*>(p.bias)[n]);
    static_cast<T*>(p.C)[idx] = from_f32<T>(s);
}

}  // namespace

// Guidance rescale of the latent sampler (S. Lin, B. Liu, J. Li, X. Yang, "Common Diffusion Noise Schedules and Sample Steps are
// Flawed", WACV 2024, arXiv:2305.08891, §3.4, in the model-output form the pipelines run: `rescale_noise_cfg`).  Restated from
// the paper and the published behaviour; no line of the reference, which has no such step.
// A pre-pass IN FRONT of the step launch of an iteration: per sample b of model_out [2B, per_row] = unconditional rows | conditional
// rows, all fp32,
//     o_e = u_e + g·(c_e − u_e)                       the guided output as the step kernels form it (product rounded on its own)
//     σ_c, σ_o                                        standard deviations of c and o over the row, CENTRED: means first, then the
//                                                     sums of squared deviations (E[x²] − E[x]² loses the digits when |mean| ≫ σ)
//     k_b = φ·(σ_c/σ_o) + (1 − φ)                     one fma; exactly 1 where the two deviations agree
//     c_e ← dtype(k_b·c_e),  u_e ← dtype(k_b·u_e)     in place, one fp32 product each, rounded to nearest even
// so that the step launch behind it forms u' + g·(c' − u') = k_b·o.  k_b = 1 — and nothing is written — where σ_o == 0, per_row == 1
// or the value is not finite (the published function writes NaN there).
// One workgroup of 1024 threads per sample, whatever B: a row's result does not depend on the other rows.  A thread keeps its first
// kHeld packs of both halves in registers (16 elements each at per_row = 16384, SD at 512²) and re-reads the rest through L2.
// Sums in a fixed order — a thread's packs in ascending order, a 64-lane butterfly, a tree over the 16 wave sums — without atomics:
// equal input gives equal bits.
#include "common.h"

namespace {

constexpr int kThreads = 1024, kWaves = kThreads / 64, kHeld = 4;

template <typename T, int V> struct alignas(V * sizeof(T)) Pack {
    T v[V];
};

// the guided output, as `guided` of ddpm_sample.hip: the difference, the product and the sum each rounded to fp32
__device__ __forceinline__ float guided(float u, float c, float g) {
#pragma clang fp contract(off)
    const float d = c - u;
    return u + g * d;
}

// (a, b) summed over the workgroup, the same bits in every thread
__device__ __forceinline__ void block_sum2(float& a, float& b, float (*s_part)[kWaves]) {
    a = wave_sum(a);
    b = wave_sum(b);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) {
        s_part[0][w] = a;
        s_part[1][w] = b;
    }
    __syncthreads();
    float t[2][kWaves];
#pragma unroll
    for (int i = 0; i < kWaves; ++i) {
        t[0][i] = s_part[0][i];
        t[1][i] = s_part[1][i];
    }
#pragma unroll
    for (int n = kWaves / 2; n > 0; n >>= 1)
#pragma unroll
        for (int i = 0; i < n; ++i) {
            t[0][i] = t[0][2 * i] + t[0][2 * i + 1];
            t[1][i] = t[1][2 * i] + t[1][2 * i + 1];
        }
    a = t[0][0];
    b = t[1][0];
    __syncthreads();  // s_part is written again by the next pass
}

template <typename T, int V>
__device__ __forceinline__ void add_sums(const Pack<T, V>& U, const Pack<T, V>& C, float g, float& sc, float& so) {
#pragma unroll
    for (int e = 0; e < V; ++e) {
        const float c = to_f32<T>(C.v[e]);
        sc += c;
        so += guided(to_f32<T>(U.v[e]), c, g);
    }
}

template <typename T, int V>
__device__ __forceinline__ void add_deviations(const Pack<T, V>& U, const Pack<T, V>& C, float g, float mc, float mo, float& qc,
                                               float& qo) {
#pragma unroll
    for (int e = 0; e < V; ++e) {
        const float c = to_f32<T>(C.v[e]);
        const float dc = c - mc, d_o = guided(to_f32<T>(U.v[e]), c, g) - mo;
        qc = fmaf(dc, dc, qc);
        qo = fmaf(d_o, d_o, qo);
    }
}

template <typename T, int V> __device__ __forceinline__ Pack<T, V> scaled(const Pack<T, V>& P, float k) {
    Pack<T, V> r;
#pragma unroll
    for (int e = 0; e < V; ++e) r.v[e] = from_f32<T>(rounded_f32(k * to_f32<T>(P.v[e])));
    return r;
}

// V = 4: per_row % 4 == 0 and model_out aligned to 4 elements, so every row of both halves is; V = 1 otherwise
template <typename T, int V>
__global__ __launch_bounds__(kThreads) void cfg_rescale_kernel(T* model_out, float* k_out, int B, int64_t per_row, float g,
                                                               float phi) {
    __shared__ float s_part[2][kWaves];
    using P = Pack<T, V>;
    const int64_t b = blockIdx.x;
    P* u = reinterpret_cast<P*>(model_out + b * per_row);
    P* c = reinterpret_cast<P*>(model_out + ((int64_t)B + b) * per_row);
    const int64_t n = per_row / V;
    const int64_t tid = threadIdx.x, rest = tid + (int64_t)kHeld * kThreads;
    P hu[kHeld], hc[kHeld];
    float sc = 0.f, so = 0.f;
#pragma unroll
    for (int j = 0; j < kHeld; ++j) {
        const int64_t i = tid + (int64_t)j * kThreads;
        if (i < n) {
            hu[j] = u[i];
            hc[j] = c[i];
            add_sums<T, V>(hu[j], hc[j], g, sc, so);
        }
    }
    for (int64_t i = rest; i < n; i += kThreads) add_sums<T, V>(u[i], c[i], g, sc, so);
    block_sum2(sc, so, s_part);
    const float mc = sc / (float)per_row, mo = so / (float)per_row;
    float qc = 0.f, qo = 0.f;
#pragma unroll
    for (int j = 0; j < kHeld; ++j)
        if (tid + (int64_t)j * kThreads < n) add_deviations<T, V>(hu[j], hc[j], g, mc, mo, qc, qo);
    for (int64_t i = rest; i < n; i += kThreads) add_deviations<T, V>(u[i], c[i], g, mc, mo, qc, qo);
    block_sum2(qc, qo, s_part);
    // the ratio of the population deviations: their common 1/n cancels
    const float ratio = sqrtf(qc) / sqrtf(qo);
    float k = fmaf(phi, ratio, 1.f - phi);
    // (equal deviations — c == u — give exactly 1, also for a φ whose 1 − φ is not an fp32 number)
    if (ratio == 1.f || qo == 0.f || per_row == 1 || !__builtin_isfinite(k)) k = 1.f;
    if (k_out && tid == 0) k_out[b] = k;
    if (k == 1.f) return;  // (every thread holds the same k)
#pragma unroll
    for (int j = 0; j < kHeld; ++j) {
        const int64_t i = tid + (int64_t)j * kThreads;
        if (i < n) {
            u[i] = scaled<T, V>(hu[j], k);
            c[i] = scaled<T, V>(hc[j], k);
        }
    }
    for (int64_t i = rest; i < n; i += kThreads) {
        u[i] = scaled<T, V>(u[i], k);
        c[i] = scaled<T, V>(c[i], k);
    }
}

template <typename T>
int launch_cfg_rescale(void* model_out, float* k_out, int B, int64_t per_row, float g, float phi, hipStream_t s) {
    T* out = static_cast<T*>(model_out);
    const bool quad = (per_row % 4) == 0 && (reinterpret_cast<uintptr_t>(model_out) & (4 * sizeof(T) - 1)) == 0;
    ProfWork work(4.0 * (double)B * (double)per_row * sizeof(T), 12.0 * (double)B * (double)per_row);
    if (quad)
        LORA_LAUNCH(PK_OTHER, (cfg_rescale_kernel<T, 4>), dim3((unsigned)B), dim3(kThreads), 0, s, out, k_out, B, per_row, g, phi);
    else
        LORA_LAUNCH(PK_OTHER, (cfg_rescale_kernel<T, 1>), dim3((unsigned)B), dim3(kThreads), 0, s, out, k_out, B, per_row, g, phi);
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}

}  // namespace

extern "C" int ddpm_cfg_rescale(void* model_out, float* k_out, int B, int64_t per_row, float guidance_scale, float rescale,
                                int dtype, void* stream) {
    if (!model_out || B < 1 || per_row < 1 || !(rescale >= 0.f && rescale <= 1.f) || !__builtin_isfinite(guidance_scale))
        return LORA_E_BADARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (dtype) {
        case LORA_F32: return launch_cfg_rescale<float>(model_out, k_out, B, per_row, guidance_scale, rescale, s);
        case LORA_F16: return launch_cfg_rescale<half_t>(model_out, k_out, B, per_row, guidance_scale, rescale, s);
        case LORA_BF16: return launch_cfg_rescale<bf16_t>(model_out, k_out, B, per_row, guidance_scale, rescale, s);
        default: return LORA_E_BADARG;
    }
}

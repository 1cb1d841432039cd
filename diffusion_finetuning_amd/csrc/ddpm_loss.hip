// DDPM noise-prediction loss (forward value + gradient in one pass), the PTI mask preparation and
// the add_noise / target prologue, with and without the draw of the latents from the VAE's moments.
//   loss      : training_scripts/train_lora_dreambooth.py:855-875, lora_diffusion/cli_lora_pti.py:243-247
//   mask prep : lora_diffusion/cli_lora_pti.py:222-241
//   prologue  : training_scripts/train_lora_dreambooth.py:824-853 (DDPM add_noise / get_velocity)
//   posterior : training_scripts/train_lora_dreambooth.py:818-821, lora_diffusion/cli_lora_pti.py:180-184
// All HBM-bound elementwise/reduction work: 16-byte vector loads, wave-shuffle → LDS → one partial
// per workgroup, and a deterministic "last workgroup sums the partials in index order" finish
// (agent-scope release/acquire around an arrival ticket, so the result does not depend on which
// XCD a workgroup ran on).
#include "common.h"

namespace {

constexpr int kMaxBlocks = 1024;
constexpr int64_t kWsBytes = 16 + kMaxBlocks * 4;

// Block-level sum in a fixed order; result valid in thread 0.
__device__ __forceinline__ float block_sum_256(float v, float* s_wave) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) s_wave[w] = v;
    __syncthreads();
    float t = 0.f;
    if (threadIdx.x == 0) t = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
    __syncthreads();
    return t;
}

// Publishes this workgroup's partial, returns true in the workgroup that arrived last, after an
// agent-scope acquire (so plain loads of every partial are fresh for all its waves).
__device__ __forceinline__ bool publish_partial_and_check_last(float partial, float* partials,
                                                               unsigned* ticket, bool* s_last) {
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = partial;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool last = (t == gridDim.x - 1);
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        *s_last = last;
    }
    __syncthreads();
    return *s_last;
}

struct MseParams {
    const void* pred;
    const void* target;
    const float* mask;
    void* dpred;
    float* loss_out;
    float* partials;
    unsigned* ticket;
    int64_t n_total;   // rows * per_row
    int64_t per_row;
    int64_t hw;
    int64_t inst_elems;  // n_inst * per_row
    float coef_inst;     // 1 / (n_inst * per_row)
    float coef_prior;    // prior_weight / (n_prior * per_row)
    float grad_scale;
};

template <typename T, int VEC>
__global__ __launch_bounds__(256) void ddpm_mse_kernel(MseParams p) {
    __shared__ float s_wave[4];
    __shared__ bool s_last;
    const T* pred = static_cast<const T*>(p.pred);
    const T* target = static_cast<const T*>(p.target);
    T* dpred = static_cast<T*>(p.dpred);
    float local = 0.f;
    const int64_t nvec = p.n_total / VEC;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < nvec; v += (int64_t)gridDim.x * 256) {
        const int64_t i0 = v * VEC;
        T pv[VEC], tv[VEC], gv[VEC];
        if constexpr (VEC > 1) {
            *reinterpret_cast<Chunk<T>*>(pv) = *reinterpret_cast<const Chunk<T>*>(pred + i0);
            *reinterpret_cast<Chunk<T>*>(tv) = *reinterpret_cast<const Chunk<T>*>(target + i0);
        } else {
            pv[0] = pred[i0];
            tv[0] = target[i0];
        }
        // a vector never straddles a row: per_row % VEC == 0 on this path
        const float coef = i0 < p.inst_elems ? p.coef_inst : p.coef_prior;
        const int64_t row = i0 / p.per_row;
        const int64_t in_row = i0 - row * p.per_row;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            float mk = 1.f;
            if (p.mask) mk = p.mask[row * p.hw + (in_row + e) % p.hw];
            // pred·mask and target·mask promote to fp32 in the reference (fp32 mask tensor)
            const float a = to_f32<T>(pv[e]) * mk;
            const float b = to_f32<T>(tv[e]) * mk;
            const float d = a - b;
            local = fmaf(coef * d, d, local);
            gv[e] = from_f32<T>(p.grad_scale * 2.f * coef * d * mk);
        }
        if (dpred) {
            if constexpr (VEC > 1) {
                *reinterpret_cast<Chunk<T>*>(dpred + i0) = *reinterpret_cast<const Chunk<T>*>(gv);
            } else {
                dpred[i0] = gv[0];
            }
        }
    }
    const float bsum = block_sum_256(local, s_wave);
    if (publish_partial_and_check_last(bsum, p.partials, p.ticket, &s_last)) {
        float t = 0.f;
        for (int i = threadIdx.x; i < (int)gridDim.x; i += 256) t += p.partials[i];
        t = block_sum_256(t, s_wave);
        if (threadIdx.x == 0) p.loss_out[0] = t;
    }
}

__global__ __launch_bounds__(1024) void mask_prepare_kernel(const float* in, float* out, int B, int Hin,
                                                            int Win, int H, int W) {
    __shared__ float s_part[16];
    __shared__ float s_mean;
    const int64_t n = (int64_t)B * H * W;
    const float sh = (float)Hin / (float)H, sw = (float)Win / (float)W;
    float local = 0.f;
    for (int64_t i = threadIdx.x; i < n; i += 1024) {
        const int x = (int)(i % W);
        const int y = (int)((i / W) % H);
        const int b = (int)(i / ((int64_t)W * H));
        int sy = (int)floorf(y * sh), sx = (int)floorf(x * sw);
        if (sy > Hin - 1) sy = Hin - 1;
        if (sx > Win - 1) sx = Win - 1;
        const float v = in[((int64_t)b * Hin + sy) * Win + sx] + 0.05f;
        out[i] = v;
        local += v;
    }
    local = wave_sum(local);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = local;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int i = 0; i < 16; ++i) t += s_part[i];
        s_mean = t / (float)n;
    }
    __syncthreads();
    const float mean = s_mean;
    for (int64_t i = threadIdx.x; i < n; i += 1024) out[i] = out[i] / mean;
}

template <typename T>
__global__ __launch_bounds__(256) void add_noise_kernel(const float* x0, const float* eps, const int64_t* t,
                                                        const float* sa, const float* sb, T* noisy, T* target,
                                                        int64_t per_row, int64_t n_total, int v_pred) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_total; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / per_row;
        const int64_t ti = t[b];
        const float a = sa[ti], s = sb[ti];
        const float x = x0[i], e = eps[i];
        noisy[i] = from_f32<T>(a * x + s * e);
        if (target) target[i] = from_f32<T>(v_pred ? a * e - s * x : e);
    }
}

template <typename T>
int launch_mse(MseParams p, hipStream_t s) {
    constexpr int V = ElemTraits<T>::kVec;
    const bool vec = (p.per_row % V) == 0 && aligned16(p.pred) && aligned16(p.target) &&
                     (!p.dpred || aligned16(p.dpred));
    const int64_t work = vec ? p.n_total / V : p.n_total;
    int64_t blocks = (work + 255) / 256;
    if (blocks > kMaxBlocks) blocks = kMaxBlocks;
    if (blocks < 1) blocks = 1;
    if (vec)
        LORA_LAUNCH(PK_MSE, (ddpm_mse_kernel<T, V>), dim3((unsigned)blocks), dim3(256), 0, s, p);
    else
        LORA_LAUNCH(PK_MSE, (ddpm_mse_kernel<T, 1>), dim3((unsigned)blocks), dim3(256), 0, s, p);
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}

// The same loss with one weight per row, looked up on the device by the row's timestep: w_b = weights[t[b]] — Min-SNR-γ
// (Hang et al. 2023, "Efficient Diffusion Training via Min-SNR Weighting Strategy": min(SNR(t), γ)/SNR(t), divided by SNR + 1
// instead of SNR for v-prediction) or any table of the caller's.  The reference has no counterpart (its objective is the plain
// mean); the timesteps of a replayed step exist on the device only, so the lookup cannot be the host's.  The weight is folded
// into the row's coefficient, coef_row = coef·w_b, read once per 16-byte chunk (a chunk lies inside one row), and everything
// else is ddpm_mse_kernel's arithmetic word for word: a table of ones leaves its bits.  A timestep outside [0, n_weights) is
// never used as an index: the row's weight is NaN, so the loss is NaN and the step is skipped like any overflow (the
// convention for token ids outside the embedding table).  Kernels of their own: ddpm_mse_kernel is not touched.
struct MseWeightedParams {
    MseParams m;
    const int64_t* t;      // [rows]
    const float* weights;  // [n_weights]
    int n_weights;
};

template <typename T, int VEC>
__global__ __launch_bounds__(256) void ddpm_mse_weighted_kernel(MseWeightedParams q) {
    __shared__ float s_wave[4];
    __shared__ bool s_last;
    const MseParams& p = q.m;
    const T* pred = static_cast<const T*>(p.pred);
    const T* target = static_cast<const T*>(p.target);
    T* dpred = static_cast<T*>(p.dpred);
    float local = 0.f;
    const int64_t nvec = p.n_total / VEC;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < nvec; v += (int64_t)gridDim.x * 256) {
        const int64_t i0 = v * VEC;
        T pv[VEC], tv[VEC], gv[VEC];
        if constexpr (VEC > 1) {
            *reinterpret_cast<Chunk<T>*>(pv) = *reinterpret_cast<const Chunk<T>*>(pred + i0);
            *reinterpret_cast<Chunk<T>*>(tv) = *reinterpret_cast<const Chunk<T>*>(target + i0);
        } else {
            pv[0] = pred[i0];
            tv[0] = target[i0];
        }
        // a vector never straddles a row: per_row % VEC == 0 on this path
        const int64_t row = i0 / p.per_row;
        const int64_t in_row = i0 - row * p.per_row;
        const int64_t ti = q.t[row];
        const float w = (ti >= 0 && ti < (int64_t)q.n_weights) ? q.weights[ti] : __builtin_nanf("");
        const float coef = (i0 < p.inst_elems ? p.coef_inst : p.coef_prior) * w;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            float mk = 1.f;
            if (p.mask) mk = p.mask[row * p.hw + (in_row + e) % p.hw];
            const float a = to_f32<T>(pv[e]) * mk;
            const float b = to_f32<T>(tv[e]) * mk;
            const float d = a - b;
            local = fmaf(coef * d, d, local);
            gv[e] = from_f32<T>(p.grad_scale * 2.f * coef * d * mk);
        }
        if (dpred) {
            if constexpr (VEC > 1) {
                *reinterpret_cast<Chunk<T>*>(dpred + i0) = *reinterpret_cast<const Chunk<T>*>(gv);
            } else {
                dpred[i0] = gv[0];
            }
        }
    }
    const float bsum = block_sum_256(local, s_wave);
    if (publish_partial_and_check_last(bsum, p.partials, p.ticket, &s_last)) {
        float t = 0.f;
        for (int i = threadIdx.x; i < (int)gridDim.x; i += 256) t += p.partials[i];
        t = block_sum_256(t, s_wave);
        if (threadIdx.x == 0) p.loss_out[0] = t;
    }
}

template <typename T>
int launch_mse_weighted(MseWeightedParams q, hipStream_t s) {
    constexpr int V = ElemTraits<T>::kVec;
    const MseParams& p = q.m;
    const bool vec = (p.per_row % V) == 0 && aligned16(p.pred) && aligned16(p.target) &&
                     (!p.dpred || aligned16(p.dpred));
    const int64_t work = vec ? p.n_total / V : p.n_total;
    int64_t blocks = (work + 255) / 256;
    if (blocks > kMaxBlocks) blocks = kMaxBlocks;
    if (blocks < 1) blocks = 1;
    if (vec)
        LORA_LAUNCH(PK_MSE, (ddpm_mse_weighted_kernel<T, V>), dim3((unsigned)blocks), dim3(256), 0, s, q);
    else
        LORA_LAUNCH(PK_MSE, (ddpm_mse_weighted_kernel<T, 1>), dim3((unsigned)blocks), dim3(256), 0, s, q);
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}

// What both loss entries check and fill in before their launch; LORA_OK with the ticket zeroed on `s`.
int mse_params(MseParams& p, const void* pred, const void* target, const float* mask, int n_inst, int n_prior,
               int64_t per_row, int64_t hw, float prior_weight, float grad_scale, float* loss_out, void* dpred,
               void* workspace, hipStream_t s) {
    if (!pred || !target || !loss_out || !workspace) return LORA_E_BADARG;
    if (n_inst < 1 || n_prior < 0 || per_row < 1 || hw < 1 || (per_row % hw) != 0) return LORA_E_BADARG;
    if (!aligned16(workspace)) return LORA_E_ALIGN;
    if (!lora_zero_ticket(workspace, s)) return LORA_E_LAUNCH;
    p.pred = pred; p.target = target; p.mask = mask; p.dpred = dpred; p.loss_out = loss_out;
    p.ticket = static_cast<unsigned*>(workspace);
    p.partials = reinterpret_cast<float*>(static_cast<char*>(workspace) + 16);
    p.n_total = (int64_t)(n_inst + n_prior) * per_row;
    p.per_row = per_row; p.hw = hw;
    p.inst_elems = (int64_t)n_inst * per_row;
    p.coef_inst = 1.0f / ((float)n_inst * (float)per_row);
    p.coef_prior = n_prior > 0 ? prior_weight / ((float)n_prior * (float)per_row) : 0.f;
    p.grad_scale = grad_scale;
    return LORA_OK;
}

}  // namespace

extern "C" int64_t lora_mse_workspace_bytes(void) { return kWsBytes; }

extern "C" int ddpm_mse_fwd_bwd(const void* pred, const void* target, const float* mask, int n_inst,
                                int n_prior, int64_t per_row, int64_t hw, float prior_weight, float grad_scale,
                                float* loss_out, void* dpred, void* workspace, int dtype, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    MseParams p{};
    int rc = mse_params(p, pred, target, mask, n_inst, n_prior, per_row, hw, prior_weight, grad_scale, loss_out, dpred,
                        workspace, s);
    if (rc != LORA_OK) return rc;
    const double e = dtype == LORA_F32 ? 4.0 : 2.0;
    ProfWork work(e * (double)p.n_total * (dpred ? 3.0 : 2.0), 4.0 * (double)p.n_total);
    switch (dtype) {
        case LORA_F32: rc = launch_mse<float>(p, s); break;
        case LORA_F16: rc = launch_mse<half_t>(p, s); break;
        case LORA_BF16: rc = launch_mse<bf16_t>(p, s); break;
        default: rc = LORA_E_BADARG;
    }
    return rc;
}

extern "C" int ddpm_mse_weighted_fwd_bwd(const void* pred, const void* target, const float* mask, const int64_t* t,
                                         const float* weights, int n_weights, int n_inst, int n_prior, int64_t per_row,
                                         int64_t hw, float prior_weight, float grad_scale, float* loss_out, void* dpred,
                                         void* workspace, int dtype, void* stream) {
    if (!t || !weights || n_weights < 1) return LORA_E_BADARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    MseWeightedParams q{};
    int rc = mse_params(q.m, pred, target, mask, n_inst, n_prior, per_row, hw, prior_weight, grad_scale, loss_out, dpred,
                        workspace, s);
    if (rc != LORA_OK) return rc;
    q.t = t; q.weights = weights; q.n_weights = n_weights;
    const double e = dtype == LORA_F32 ? 4.0 : 2.0;
    ProfWork work(e * (double)q.m.n_total * (dpred ? 3.0 : 2.0), 5.0 * (double)q.m.n_total);
    switch (dtype) {
        case LORA_F32: rc = launch_mse_weighted<float>(q, s); break;
        case LORA_F16: rc = launch_mse_weighted<half_t>(q, s); break;
        case LORA_BF16: rc = launch_mse_weighted<bf16_t>(q, s); break;
        default: rc = LORA_E_BADARG;
    }
    return rc;
}

extern "C" int lora_mask_prepare(const float* mask_in, float* mask_out, int B, int Hin, int Win, int H, int W,
                                 void* stream) {
    if (!mask_in || !mask_out || B < 1 || Hin < 1 || Win < 1 || H < 1 || W < 1) return LORA_E_BADARG;
    hipLaunchKernelGGL(mask_prepare_kernel, dim3(1), dim3(1024), 0, static_cast<hipStream_t>(stream), mask_in,
                       mask_out, B, Hin, Win, H, W);
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}

extern "C" int ddpm_add_noise(const float* x0, const float* eps, const int64_t* t, const float* sqrt_acp,
                              const float* sqrt_1macp, void* noisy, void* target, int B, int64_t per_row,
                              int v_prediction, int dtype, void* stream) {
    if (!x0 || !eps || !t || !sqrt_acp || !sqrt_1macp || !noisy || B < 1 || per_row < 1) return LORA_E_BADARG;
    const int64_t n = (int64_t)B * per_row;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (dtype) {
        case LORA_F32:
            hipLaunchKernelGGL(add_noise_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, s, x0, eps, t, sqrt_acp,
                               sqrt_1macp, static_cast<float*>(noisy), static_cast<float*>(target), per_row, n,
                               v_prediction);
            break;
        case LORA_F16:
            hipLaunchKernelGGL(add_noise_kernel<half_t>, dim3((unsigned)blocks), dim3(256), 0, s, x0, eps, t, sqrt_acp,
                               sqrt_1macp, static_cast<half_t*>(noisy), static_cast<half_t*>(target), per_row, n,
                               v_prediction);
            break;
        case LORA_BF16:
            hipLaunchKernelGGL(add_noise_kernel<bf16_t>, dim3((unsigned)blocks), dim3(256), 0, s, x0, eps, t, sqrt_acp,
                               sqrt_1macp, static_cast<bf16_t*>(noisy), static_cast<bf16_t*>(target), per_row, n,
                               v_prediction);
            break;
        default: return LORA_E_BADARG;
    }
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Step prologue with build-owned, counter-based randomness:
//   t_b  ~ U{0..T-1},  eps ~ N(0,1)  from Philox4x32-10 keyed by (seed, step) — the same stream on every rank
//   (set_seed semantics of train_lora_dreambooth.py:509-510) and on the CPU oracle (oracle/philox.py) —
//   then noisy = sqrt_acp[t]·x0 + sqrt_1macp[t]·eps and target = eps | velocity, in ONE elementwise launch that
//   replaces randn_like + randint + add_noise (+ get_velocity) of train_lora_dreambooth.py:824-853.
// Counter layout: element group g (4 consecutive elements) uses counter (g, 0, stream, 0) with stream 0 for
// eps and 1 for the timesteps (row b uses counter (b, 0, 1, 0), first word).  Normals: Box–Muller on the two
// word pairs, u = (x + 0.5)·2^-32 ∈ (0,1).
namespace {

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1, uint32_t out[4]) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        const uint32_t n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

__device__ __forceinline__ float u01(uint32_t x) { return ((float)x + 0.5f) * 2.3283064365386963e-10f; }

template <typename T>
__global__ __launch_bounds__(256) void noise_prologue_kernel(const float* x0, const float* sa, const float* sb,
                                                             T* noisy, T* target, float* eps_out, int64_t* t_out,
                                                             int B, int64_t per_row, int n_timesteps, uint32_t seed,
                                                             uint32_t step, int v_pred) {
    const int64_t n_total = (int64_t)B * per_row;
    const int64_t groups = (n_total + 3) >> 2;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
        uint32_t r[4];
        philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), 0u, 0u, seed, step, r);
        float z[4];
        {
            const float r0 = sqrtf(-2.f * logf(u01(r[0]))), r1 = sqrtf(-2.f * logf(u01(r[2])));
            float s0, c0, s1, c1;
            sincosf(6.283185307179586f * u01(r[1]), &s0, &c0);
            sincosf(6.283185307179586f * u01(r[3]), &s1, &c1);
            z[0] = r0 * c0; z[1] = r0 * s0; z[2] = r1 * c1; z[3] = r1 * s1;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t i = g * 4 + e;
            if (i >= n_total) break;
            const int64_t b = i / per_row;
            uint32_t tr[4];
            philox4x32_10((uint32_t)b, 0u, 1u, 0u, seed, step, tr);
            const int64_t ti = (int64_t)(((uint64_t)tr[0] * (uint64_t)n_timesteps) >> 32);
            if (i == b * per_row && t_out) t_out[b] = ti;
            const float a = sa[ti], s = sb[ti];
            const float x = x0[i];
            noisy[i] = from_f32<T>(a * x + s * z[e]);
            if (target) target[i] = from_f32<T>(v_pred ? a * z[e] - s * x : z[e]);
            if (eps_out) eps_out[i] = z[e];
        }
    }
}

}  // namespace

extern "C" int ddpm_noise_prologue(const float* x0, const float* sqrt_acp, const float* sqrt_1macp, void* noisy,
                                   void* target, float* eps_out, int64_t* t_out, int B, int64_t per_row,
                                   int n_timesteps, uint64_t seed, uint64_t step, int v_prediction, int dtype,
                                   void* stream) {
    if (!x0 || !sqrt_acp || !sqrt_1macp || !noisy || B < 1 || per_row < 1 || n_timesteps < 1) return LORA_E_BADARG;
    const int64_t groups = ((int64_t)B * per_row + 3) / 4;
    int64_t blocks = (groups + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint32_t sd = (uint32_t)seed, st = (uint32_t)step;
    switch (dtype) {
        case LORA_F32:
            hipLaunchKernelGGL(noise_prologue_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, s, x0, sqrt_acp,
                               sqrt_1macp, static_cast<float*>(noisy), static_cast<float*>(target), eps_out, t_out, B,
                               per_row, n_timesteps, sd, st, v_prediction);
            break;
        case LORA_F16:
            hipLaunchKernelGGL(noise_prologue_kernel<half_t>, dim3((unsigned)blocks), dim3(256), 0, s, x0, sqrt_acp,
                               sqrt_1macp, static_cast<half_t*>(noisy), static_cast<half_t*>(target), eps_out, t_out, B,
                               per_row, n_timesteps, sd, st, v_prediction);
            break;
        case LORA_BF16:
            hipLaunchKernelGGL(noise_prologue_kernel<bf16_t>, dim3((unsigned)blocks), dim3(256), 0, s, x0, sqrt_acp,
                               sqrt_1macp, static_cast<bf16_t*>(noisy), static_cast<bf16_t*>(target), eps_out, t_out, B,
                               per_row, n_timesteps, sd, st, v_prediction);
            break;
        default: return LORA_E_BADARG;
    }
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}

// ---------------------------------------------------------------------------------------------------------
// The same prologue one step earlier: the latents themselves are drawn from the VAE encoder's moments,
//   x0 = (mean + exp(0.5·clamp(logvar, −30, 20))·z)·scale        (`latent_dist.sample() * 0.18215`,
//   train_lora_dreambooth.py:818-821, cli_lora_pti.py:180-184; DiagonalGaussianDistribution is diffusers', restated from its
//   published definition)
// with z ~ N(0,1) from Philox stream 2 — counter (g, g>>32, 2, 0) — next to eps (stream 0) and t (stream 1), which keep the
// counters and the arithmetic of noise_prologue_kernel: for equal (seed, step) they come out bit-identical to its draw.
// One thread per Philox group of 4 consecutive elements.  QUAD: per_row % 4 == 0 and every pointer aligned to its 4-element
// access, so a group lies inside one row and mean / logvar / every output move as one 16-byte (fp32) or 8-byte (16-bit)
// access; otherwise element by element, a group may straddle rows and the last one may be ragged.
namespace {

template <typename T> struct alignas(4 * sizeof(T)) Quad {
    T v[4];
};

__device__ __forceinline__ void philox_normals4(uint64_t g, uint32_t stream, uint32_t seed, uint32_t step, float z[4]) {
    uint32_t r[4];
    philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), stream, 0u, seed, step, r);
    const float r0 = sqrtf(-2.f * logf(u01(r[0]))), r1 = sqrtf(-2.f * logf(u01(r[2])));
    float s0, c0, s1, c1;
    sincosf(6.283185307179586f * u01(r[1]), &s0, &c0);
    sincosf(6.283185307179586f * u01(r[3]), &s1, &c1);
    z[0] = r0 * c0; z[1] = r0 * s0; z[2] = r1 * c1; z[3] = r1 * s1;
}

__device__ __forceinline__ int64_t philox_timestep(uint32_t b, uint32_t seed, uint32_t step, int n_timesteps) {
    uint32_t tr[4];
    philox4x32_10(b, 0u, 1u, 0u, seed, step, tr);
    return (int64_t)(((uint64_t)tr[0] * (uint64_t)n_timesteps) >> 32);
}

// torch.clamp's semantics (a NaN stays a NaN), then diffusers' std = exp(0.5·logvar)
__device__ __forceinline__ float posterior_x0(float mean, float logvar, float z, float scale) {
    const float lv = logvar < -30.f ? -30.f : (logvar > 20.f ? 20.f : logvar);
    return fmaf(expf(0.5f * lv), z, mean) * scale;
}

// noisy and target with every product rounded on its own — what add_noise_kernel and noise_prologue_kernel compile to — and
// said so here, where the compiler would otherwise fuse them: a step fed with moments then leaves the very bits of the step
// fed with this launch's x0_out / eps_out / t_out.
__device__ __forceinline__ float ddpm_noisy(float a, float s, float x, float e) {
#pragma clang fp contract(off)
    const float ax = a * x, se = s * e;
    return ax + se;
}
__device__ __forceinline__ float ddpm_target(float a, float s, float x, float e, int v_pred) {
#pragma clang fp contract(off)
    const float ae = a * e, sx = s * x;
    return v_pred ? ae - sx : e;
}

struct PosteriorParams {
    const void* moments;  // [B, 2·per_row]: row b = mean | logvar
    const float* sa;
    const float* sb;
    void* noisy;
    void* target;   // nullable
    float* x0_out;  // nullable, like z_out / eps_out / t_out
    float* z_out;
    float* eps_out;
    int64_t* t_out;
    int64_t per_row;
    int64_t n_total;  // B · per_row
    int n_timesteps;
    uint32_t seed, step;
    float scale;
    int v_pred;
};

template <typename TM, typename TO, bool QUAD>
__global__ __launch_bounds__(256) void posterior_prologue_kernel(PosteriorParams p) {
    const TM* moments = static_cast<const TM*>(p.moments);
    TO* noisy = static_cast<TO*>(p.noisy);
    TO* target = static_cast<TO*>(p.target);
    const int64_t groups = (p.n_total + 3) >> 2;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
        Quad<float> eps_q, z_q;
        philox_normals4((uint64_t)g, 0u, p.seed, p.step, eps_q.v);
        philox_normals4((uint64_t)g, 2u, p.seed, p.step, z_q.v);
        const float* eps = eps_q.v;
        const float* z = z_q.v;
        const int64_t i0 = g * 4;
        int64_t b = i0 / p.per_row;  // row of the group's first element (B is an int: b fits 32 bits)
        // The timestep is a property of the row.  All 64 groups of a wave mostly lie in one row: its Philox call then has
        // wave-uniform inputs and runs once per wave on the scalar unit; only the lanes of a wave that straddles a row
        // boundary make a call of their own.
        const uint32_t b_wave = __builtin_amdgcn_readfirstlane((uint32_t)b);
        int64_t ti = philox_timestep(b_wave, p.seed, p.step, p.n_timesteps);
        if ((uint32_t)b != b_wave) ti = philox_timestep((uint32_t)b, p.seed, p.step, p.n_timesteps);
        if constexpr (QUAD) {
            const int64_t col = i0 - b * p.per_row;
            const TM* row = moments + b * 2 * p.per_row + col;
            const Quad<TM> mean = *reinterpret_cast<const Quad<TM>*>(row);
            const Quad<TM> logvar = *reinterpret_cast<const Quad<TM>*>(row + p.per_row);
            if (col == 0 && p.t_out) p.t_out[b] = ti;
            const float a = p.sa[ti], s = p.sb[ti];
            Quad<float> x;
            Quad<TO> nv, tv;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                x.v[e] = posterior_x0(to_f32<TM>(mean.v[e]), to_f32<TM>(logvar.v[e]), z[e], p.scale);
                nv.v[e] = from_f32<TO>(ddpm_noisy(a, s, x.v[e], eps[e]));
                tv.v[e] = from_f32<TO>(ddpm_target(a, s, x.v[e], eps[e], p.v_pred));
            }
            *reinterpret_cast<Quad<TO>*>(noisy + i0) = nv;
            if (target) *reinterpret_cast<Quad<TO>*>(target + i0) = tv;
            if (p.x0_out) *reinterpret_cast<Quad<float>*>(p.x0_out + i0) = x;
            if (p.z_out) *reinterpret_cast<Quad<float>*>(p.z_out + i0) = z_q;
            if (p.eps_out) *reinterpret_cast<Quad<float>*>(p.eps_out + i0) = eps_q;
        } else {
            int64_t row_end = (b + 1) * p.per_row;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int64_t i = i0 + e;
                if (i >= p.n_total) break;
                if (i >= row_end) {  // the group runs on into the next row(s): per_row may be below 4
                    b = i / p.per_row;
                    row_end = (b + 1) * p.per_row;
                    ti = philox_timestep((uint32_t)b, p.seed, p.step, p.n_timesteps);
                }
                const int64_t col = i - b * p.per_row;
                if (col == 0 && p.t_out) p.t_out[b] = ti;
                const float a = p.sa[ti], s = p.sb[ti];
                const TM* row = moments + b * 2 * p.per_row + col;
                const float x = posterior_x0(to_f32<TM>(row[0]), to_f32<TM>(row[p.per_row]), z[e], p.scale);
                noisy[i] = from_f32<TO>(ddpm_noisy(a, s, x, eps[e]));
                if (target) target[i] = from_f32<TO>(ddpm_target(a, s, x, eps[e], p.v_pred));
                if (p.x0_out) p.x0_out[i] = x;
                if (p.z_out) p.z_out[i] = z[e];
                if (p.eps_out) p.eps_out[i] = eps[e];
            }
        }
    }
}

template <typename TM, bool QUAD>
__global__ __launch_bounds__(256) void posterior_sample_kernel(const TM* moments, const float* z, float* x0, int64_t per_row,
                                                               int64_t n_total, float scale) {
    const int64_t groups = (n_total + 3) >> 2;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
        const int64_t i0 = g * 4;
        if constexpr (QUAD) {
            const int64_t b = i0 / per_row;
            const TM* row = moments + b * 2 * per_row + (i0 - b * per_row);
            const Quad<TM> mean = *reinterpret_cast<const Quad<TM>*>(row);
            const Quad<TM> logvar = *reinterpret_cast<const Quad<TM>*>(row + per_row);
            const Quad<float> zv = *reinterpret_cast<const Quad<float>*>(z + i0);
            Quad<float> x;
#pragma unroll
            for (int e = 0; e < 4; ++e)
                x.v[e] = posterior_x0(to_f32<TM>(mean.v[e]), to_f32<TM>(logvar.v[e]), zv.v[e], scale);
            *reinterpret_cast<Quad<float>*>(x0 + i0) = x;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int64_t i = i0 + e;
                if (i >= n_total) break;
                const int64_t b = i / per_row;
                const TM* row = moments + b * 2 * per_row + (i - b * per_row);
                x0[i] = posterior_x0(to_f32<TM>(row[0]), to_f32<TM>(row[per_row]), z[i], scale);
            }
        }
    }
}

template <typename T> bool quad_aligned(const void* p) {  // null: nothing to access
    return (reinterpret_cast<uintptr_t>(p) & (4 * sizeof(T) - 1)) == 0;
}

unsigned posterior_blocks(int64_t n_total) {
    int64_t blocks = ((n_total + 3) / 4 + 255) / 256;
    return (unsigned)(blocks > 2048 ? 2048 : blocks);
}

template <typename TM, typename TO>
void launch_posterior_prologue(const PosteriorParams& p, hipStream_t s) {
    const bool quad = (p.per_row % 4) == 0 && quad_aligned<TM>(p.moments) && quad_aligned<TO>(p.noisy) &&
                      quad_aligned<TO>(p.target) && quad_aligned<float>(p.x0_out) && quad_aligned<float>(p.z_out) &&
                      quad_aligned<float>(p.eps_out);
    const dim3 grid(posterior_blocks(p.n_total));
    if (quad)
        hipLaunchKernelGGL((posterior_prologue_kernel<TM, TO, true>), grid, dim3(256), 0, s, p);
    else
        hipLaunchKernelGGL((posterior_prologue_kernel<TM, TO, false>), grid, dim3(256), 0, s, p);
}

template <typename TM>
void launch_posterior_prologue_out(const PosteriorParams& p, int dtype, hipStream_t s) {
    switch (dtype) {
        case LORA_F32: launch_posterior_prologue<TM, float>(p, s); break;
        case LORA_F16: launch_posterior_prologue<TM, half_t>(p, s); break;
        default: launch_posterior_prologue<TM, bf16_t>(p, s); break;
    }
}

template <typename TM>
void launch_posterior_sample(const void* moments, const float* z, float* x0, int64_t per_row, int64_t n_total, float scale,
                             hipStream_t s) {
    const bool quad = (per_row % 4) == 0 && quad_aligned<TM>(moments) && quad_aligned<float>(z) && quad_aligned<float>(x0);
    const dim3 grid(posterior_blocks(n_total));
    const TM* m = static_cast<const TM*>(moments);
    if (quad)
        hipLaunchKernelGGL((posterior_sample_kernel<TM, true>), grid, dim3(256), 0, s, m, z, x0, per_row, n_total, scale);
    else
        hipLaunchKernelGGL((posterior_sample_kernel<TM, false>), grid, dim3(256), 0, s, m, z, x0, per_row, n_total, scale);
}

bool known_dtype(int dtype) { return dtype == LORA_F32 || dtype == LORA_F16 || dtype == LORA_BF16; }

}  // namespace

extern "C" int ddpm_posterior_prologue(const void* moments, int moments_dtype, const float* sqrt_acp, const float* sqrt_1macp,
                                       void* noisy, void* target, float* x0_out, float* z_out, float* eps_out, int64_t* t_out,
                                       int B, int64_t per_row, int n_timesteps, float scale, uint64_t seed, uint64_t step,
                                       int v_prediction, int dtype, void* stream) {
    if (!moments || !sqrt_acp || !sqrt_1macp || !noisy || B < 1 || per_row < 1 || n_timesteps < 1) return LORA_E_BADARG;
    if (!known_dtype(moments_dtype) || !known_dtype(dtype)) return LORA_E_BADARG;
    PosteriorParams p{};
    p.moments = moments; p.sa = sqrt_acp; p.sb = sqrt_1macp; p.noisy = noisy; p.target = target;
    p.x0_out = x0_out; p.z_out = z_out; p.eps_out = eps_out; p.t_out = t_out;
    p.per_row = per_row; p.n_total = (int64_t)B * per_row; p.n_timesteps = n_timesteps;
    p.seed = (uint32_t)seed; p.step = (uint32_t)step; p.scale = scale; p.v_pred = v_prediction;
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (moments_dtype) {
        case LORA_F32: launch_posterior_prologue_out<float>(p, dtype, s); break;
        case LORA_F16: launch_posterior_prologue_out<half_t>(p, dtype, s); break;
        default: launch_posterior_prologue_out<bf16_t>(p, dtype, s); break;
    }
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}

extern "C" int ddpm_posterior_sample(const void* moments, int moments_dtype, const float* z, float* x0, int B, int64_t per_row,
                                     float scale, void* stream) {
    if (!moments || !z || !x0 || B < 1 || per_row < 1 || !known_dtype(moments_dtype)) return LORA_E_BADARG;
    const int64_t n = (int64_t)B * per_row;
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (moments_dtype) {
        case LORA_F32: launch_posterior_sample<float>(moments, z, x0, per_row, n, scale, s); break;
        case LORA_F16: launch_posterior_sample<half_t>(moments, z, x0, per_row, n, scale, s); break;
        default: launch_posterior_sample<bf16_t>(moments, z, x0, per_row, n, scale, s); break;
    }
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Offset noise inside the two device-drawn prologues (N. Guttenberg, "Diffusion with Offset Noise", 2023 — `--noise_offset` of
// the diffusers and kohya trainers; the reference has no counterpart): one more normal ξ per (row, channel), added to every
// element of that channel's noise,
//     eps' = fmaf(noise_offset, ξ[b, c], eps)
// and eps' is the noise everywhere downstream (noisy, target, eps_out).  ξ is a FOURTH stream of the step's key (seed, step):
// with j = b·C + c and C = per_row / hw, counter (j, j>>32, 3, 0), first normal of the Box–Muller mapping above — next to eps
// (stream 0), t (1) and the posterior z (2), whose counters and arithmetic are unchanged: t and, before the offset is added,
// eps and z are the bits of the plain prologues.  (The sampler's streams 3 and 4 below belong to another key: (seed, denoising
// step) of a sampling run, never a training step's.)  noise_offset == 0 selects eps itself, not eps + 0·ξ: every output is
// then the plain entry's bit for bit, −0 included.
// One kernel serves both entries: MOMENTS draws the latents as posterior_prologue_kernel does, otherwise x0 is read.  One
// thread per Philox group; QUAD as above.  A group inside one row can still straddle CHANNELS (hw % 4 != 0 with
// per_row % 4 == 0), so the channel is tracked per element on both paths: one division per group, then a running channel end.
namespace {

constexpr uint32_t kStreamOffset = 3u;

struct OffsetParams {
    PosteriorParams p;  // MOMENTS: as for posterior_prologue_kernel; otherwise moments, x0_out, z_out and scale are unused
    const float* x0;    // !MOMENTS: the latents, fp32 [B, per_row]
    float* xi_out;      // nullable, [B, C]
    int64_t hw, C;
    float noise_offset;
};

__device__ __forceinline__ float offset_normal(int64_t j, uint32_t seed, uint32_t step) {
    uint32_t r[4];
    philox4x32_10((uint32_t)j, (uint32_t)((uint64_t)j >> 32), kStreamOffset, 0u, seed, step, r);
    float s0, c0;
    sincosf(6.283185307179586f * u01(r[1]), &s0, &c0);
    return sqrtf(-2.f * logf(u01(r[0]))) * c0;
}

template <typename TM, typename TO, bool QUAD, bool MOMENTS>
__global__ __launch_bounds__(256) void offset_prologue_kernel(OffsetParams q) {
    const PosteriorParams& p = q.p;
    const TM* moments = static_cast<const TM*>(p.moments);
    TO* noisy = static_cast<TO*>(p.noisy);
    TO* target = static_cast<TO*>(p.target);
    const bool shifted = q.noise_offset != 0.f;
    const int64_t groups = (p.n_total + 3) >> 2;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (int64_t)gridDim.x * 256) {
        Quad<float> eps_q, z_q = {};
        philox_normals4((uint64_t)g, 0u, p.seed, p.step, eps_q.v);
        if constexpr (MOMENTS) philox_normals4((uint64_t)g, 2u, p.seed, p.step, z_q.v);
        float* eps = eps_q.v;
        const float* z = z_q.v;
        const int64_t i0 = g * 4;
        int64_t b = i0 / p.per_row;  // row of the group's first element (B is an int: b fits 32 bits)
        const uint32_t b_wave = __builtin_amdgcn_readfirstlane((uint32_t)b);  // (see posterior_prologue_kernel)
        int64_t ti = philox_timestep(b_wave, p.seed, p.step, p.n_timesteps);
        if ((uint32_t)b != b_wave) ti = philox_timestep((uint32_t)b, p.seed, p.step, p.n_timesteps);
        // channel of the group's first element, and the element index at which that channel ends
        int64_t ch = (i0 - b * p.per_row) / q.hw;
        int64_t ch_end = b * p.per_row + (ch + 1) * q.hw;
        float xi = offset_normal(b * q.C + ch, p.seed, p.step);
        if constexpr (QUAD) {
            const int64_t col = i0 - b * p.per_row;
            Quad<TM> mean, logvar;
            Quad<float> x;
            if constexpr (MOMENTS) {
                const TM* row = moments + b * 2 * p.per_row + col;
                mean = *reinterpret_cast<const Quad<TM>*>(row);
                logvar = *reinterpret_cast<const Quad<TM>*>(row + p.per_row);
            } else {
                x = *reinterpret_cast<const Quad<float>*>(q.x0 + i0);
            }
            if (col == 0 && p.t_out) p.t_out[b] = ti;
            const float a = p.sa[ti], s = p.sb[ti];
            Quad<TO> nv, tv;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int64_t i = i0 + e;
                if (i >= ch_end) {  // the group runs on into the next channel of its row (a channel has at least one element)
                    ++ch;
                    ch_end += q.hw;
                    xi = offset_normal(b * q.C + ch, p.seed, p.step);
                }
                if (q.xi_out && i == ch_end - q.hw) q.xi_out[b * q.C + ch] = xi;
                if (shifted) eps[e] = fmaf(q.noise_offset, xi, eps[e]);
                if constexpr (MOMENTS) x.v[e] = posterior_x0(to_f32<TM>(mean.v[e]), to_f32<TM>(logvar.v[e]), z[e], p.scale);
                nv.v[e] = from_f32<TO>(ddpm_noisy(a, s, x.v[e], eps[e]));
                tv.v[e] = from_f32<TO>(ddpm_target(a, s, x.v[e], eps[e], p.v_pred));
            }
            *reinterpret_cast<Quad<TO>*>(noisy + i0) = nv;
            if (target) *reinterpret_cast<Quad<TO>*>(target + i0) = tv;
            if constexpr (MOMENTS) {
                if (p.x0_out) *reinterpret_cast<Quad<float>*>(p.x0_out + i0) = x;
                if (p.z_out) *reinterpret_cast<Quad<float>*>(p.z_out + i0) = z_q;
            }
            if (p.eps_out) *reinterpret_cast<Quad<float>*>(p.eps_out + i0) = eps_q;
        } else {
            int64_t row_end = (b + 1) * p.per_row;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int64_t i = i0 + e;
                if (i >= p.n_total) break;
                if (i >= row_end) {  // the group runs on into the next row(s): per_row may be below 4
                    b = i / p.per_row;
                    row_end = (b + 1) * p.per_row;
                    ti = philox_timestep((uint32_t)b, p.seed, p.step, p.n_timesteps);
                    ch = 0;  // (i advances by one: the first element of a row the group enters is its column 0)
                    ch_end = b * p.per_row + q.hw;
                    xi = offset_normal(b * q.C, p.seed, p.step);
                } else if (i >= ch_end) {
                    ++ch;
                    ch_end += q.hw;
                    xi = offset_normal(b * q.C + ch, p.seed, p.step);
                }
                const int64_t col = i - b * p.per_row;
                if (col == 0 && p.t_out) p.t_out[b] = ti;
                if (q.xi_out && i == ch_end - q.hw) q.xi_out[b * q.C + ch] = xi;
                const float en = shifted ? fmaf(q.noise_offset, xi, eps[e]) : eps[e];
                const float a = p.sa[ti], s = p.sb[ti];
                float x;
                if constexpr (MOMENTS) {
                    const TM* row = moments + b * 2 * p.per_row + col;
                    x = posterior_x0(to_f32<TM>(row[0]), to_f32<TM>(row[p.per_row]), z[e], p.scale);
                } else {
                    x = q.x0[i];
                }
                noisy[i] = from_f32<TO>(ddpm_noisy(a, s, x, en));
                if (target) target[i] = from_f32<TO>(ddpm_target(a, s, x, en, p.v_pred));
                if constexpr (MOMENTS) {
                    if (p.x0_out) p.x0_out[i] = x;
                    if (p.z_out) p.z_out[i] = z[e];
                }
                if (p.eps_out) p.eps_out[i] = en;
            }
        }
    }
}

template <typename TM, typename TO, bool MOMENTS>
void launch_offset_prologue(const OffsetParams& q, hipStream_t s) {
    const PosteriorParams& p = q.p;
    const bool quad = (p.per_row % 4) == 0 && quad_aligned<TM>(p.moments) && quad_aligned<float>(q.x0) &&
                      quad_aligned<TO>(p.noisy) && quad_aligned<TO>(p.target) && quad_aligned<float>(p.x0_out) &&
                      quad_aligned<float>(p.z_out) && quad_aligned<float>(p.eps_out);
    const dim3 grid(posterior_blocks(p.n_total));
    if (quad)
        hipLaunchKernelGGL((offset_prologue_kernel<TM, TO, true, MOMENTS>), grid, dim3(256), 0, s, q);
    else
        hipLaunchKernelGGL((offset_prologue_kernel<TM, TO, false, MOMENTS>), grid, dim3(256), 0, s, q);
}

template <typename TM, bool MOMENTS>
void launch_offset_prologue_out(const OffsetParams& q, int dtype, hipStream_t s) {
    switch (dtype) {
        case LORA_F32: launch_offset_prologue<TM, float, MOMENTS>(q, s); break;
        case LORA_F16: launch_offset_prologue<TM, half_t, MOMENTS>(q, s); break;
        default: launch_offset_prologue<TM, bf16_t, MOMENTS>(q, s); break;
    }
}

bool offset_args_ok(int64_t per_row, int64_t hw, float noise_offset) {
    return hw >= 1 && (per_row % hw) == 0 && noise_offset == noise_offset && noise_offset - noise_offset == 0.f;  // (finite)
}

}  // namespace

extern "C" int ddpm_noise_prologue_offset(const float* x0, const float* sqrt_acp, const float* sqrt_1macp, void* noisy,
                                          void* target, float* eps_out, int64_t* t_out, int B, int64_t per_row, int n_timesteps,
                                          uint64_t seed, uint64_t step, int v_prediction, int dtype, int64_t hw,
                                          float noise_offset, float* xi_out, void* stream) {
    if (!x0 || !sqrt_acp || !sqrt_1macp || !noisy || B < 1 || per_row < 1 || n_timesteps < 1) return LORA_E_BADARG;
    if (!known_dtype(dtype) || !offset_args_ok(per_row, hw, noise_offset)) return LORA_E_BADARG;
    OffsetParams q{};
    PosteriorParams& p = q.p;
    p.sa = sqrt_acp; p.sb = sqrt_1macp; p.noisy = noisy; p.target = target; p.eps_out = eps_out; p.t_out = t_out;
    p.per_row = per_row; p.n_total = (int64_t)B * per_row; p.n_timesteps = n_timesteps;
    p.seed = (uint32_t)seed; p.step = (uint32_t)step; p.v_pred = v_prediction;
    q.x0 = x0; q.xi_out = xi_out; q.hw = hw; q.C = per_row / hw; q.noise_offset = noise_offset;
    launch_offset_prologue_out<float, false>(q, dtype, static_cast<hipStream_t>(stream));
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}

extern "C" int ddpm_posterior_prologue_offset(const void* moments, int moments_dtype, const float* sqrt_acp,
                                              const float* sqrt_1macp, void* noisy, void* target, float* x0_out, float* z_out,
                                              float* eps_out, int64_t* t_out, int B, int64_t per_row, int n_timesteps,
                                              float scale, uint64_t seed, uint64_t step, int v_prediction, int dtype, int64_t hw,
                                              float noise_offset, float* xi_out, void* stream) {
    if (!moments || !sqrt_acp || !sqrt_1macp || !noisy || B < 1 || per_row < 1 || n_timesteps < 1) return LORA_E_BADARG;
    if (!known_dtype(moments_dtype) || !known_dtype(dtype) || !offset_args_ok(per_row, hw, noise_offset)) return LORA_E_BADARG;
    OffsetParams q{};
    PosteriorParams& p = q.p;
    p.moments = moments; p.sa = sqrt_acp; p.sb = sqrt_1macp; p.noisy = noisy; p.target = target;
    p.x0_out = x0_out; p.z_out = z_out; p.eps_out = eps_out; p.t_out = t_out;
    p.per_row = per_row; p.n_total = (int64_t)B * per_row; p.n_timesteps = n_timesteps;
    p.seed = (uint32_t)seed; p.step = (uint32_t)step; p.scale = scale; p.v_pred = v_prediction;
    q.xi_out = xi_out; q.hw = hw; q.C = per_row / hw; q.noise_offset = noise_offset;
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (moments_dtype) {
        case LORA_F32: launch_offset_prologue_out<float, true>(q, dtype, s); break;
        case LORA_F16: launch_offset_prologue_out<half_t, true>(q, dtype, s); break;
        default: launch_offset_prologue_out<bf16_t, true>(q, dtype, s); break;
    }
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Latent sampler: the loop around the UNet forward of lora_diffusion/utils.py:112-163 (evaluate_pipe, guidance 5.0, 50 steps of
// the training DDPMScheduler, cli_lora_pti.py:370-402), of the class-image generation of train_lora_dreambooth.py:512-558 and of
// utils.py:166-214 — classifier-free guidance, the scheduler step, the variance noise and the re-assembly of the doubled model
// input — as ONE launch per denoising step.  With SD's clip_sample=False every supported step (DDPM ancestral, DDIM with any η,
// ε- or v-prediction) is linear in the state x and the guided model output o:
//     o = u + g·(c − u)   (no guidance: o = out),      x ← a·x + b·o + σ·z,  z ~ N(0,1) only where σ ≠ 0
// with (a, b, σ) per step from the host (sampling.sampler_schedule, float64 rounded once).  The step index is read from DEVICE
// memory (`cursor[0]`, and the run's seed from `cursor[1]`), so a recorded launch serves every step and every seed of a replayed
// hipGraph; a one-thread launch BEHIND the step advances
// it — stream order puts it after every workgroup of the step, which have all read the cursor by then, and before the next
// step's first.  A cursor outside [0, S) makes the step a no-op: nothing is read from the tables, nothing written.
// Counter layout, key (seed, i) with i the denoising-step index (0 for the initial draw): element group g (4 consecutive
// elements of the [B, per_row] state) uses counter (g, g>>32, 3, 0) for x_T and (g, g>>32, 4, 0) for the variance noise z —
// streams of their own next to eps (0), the timesteps (1) and the posterior z (2); Box–Muller as above.  The draw depends on
// (seed, i, B·per_row) alone: not on the dtype, the access path or guidance.
// QUAD as in posterior_prologue_kernel: per_row % 4 == 0 and every pointer aligned to its 4-element access.
namespace {

constexpr uint32_t kStreamInit = 3u, kStreamStepNoise = 4u;

struct SampleParams {
    float* x;             // [B, per_row] fp32 state, updated in place
    const void* out;      // model output, [rows, per_row]; rows = 2B (uncond | cond) under guidance, else B
    void* in;             // next model input, [rows, per_row]: the new state cast, twice under guidance
    int64_t* t_model;     // [rows] timestep tensor of the next forward
    int* cursor;          // [2]: the denoising-step index, the seed (Philox key word) of the run
    const int64_t* timesteps;  // [S]
    const float* coef;         // [S, 3] = (a, b, σ)
    float* z_out;              // nullable
    int64_t n_total;           // B · per_row
    int rows;
    int S;
    int cfg;
    float guidance;
    uint32_t seed;
    int64_t shared_row;        // 0: the draws of the batch (counter = element group of the [B, per_row] state); per_row: every
                               // sample takes the draws of the B = 1 run (the *_shared entries, sample_normals4 below)
};

// The four normals of element group g (elements 4g .. 4g+3 of the [B, per_row] state) of `stream` under key (seed, step).
//   shared_row == 0:  counter g — one stream over the whole batch (what every entry without `_shared` draws);
//   shared_row == per_row ("equal seed" in the reference's loops: torch.manual_seed(seed) before every member of a sweep,
//       utils.py:191-211): element j of EVERY sample takes lane j mod 4 of counter j div 4 — exactly what the B = 1 run of the
//       same seed gives its element j.  With per_row % 4 == 0 a group lies inside one sample and maps to one counter; otherwise
//       a group straddles counters (and samples) and is assembled element by element, at most one Philox call per counter.
__device__ __forceinline__ void sample_normals4(int64_t g, int64_t shared_row, uint32_t stream, uint32_t seed, uint32_t step,
                                                float z[4]) {
    if (shared_row == 0) {
        philox_normals4((uint64_t)g, stream, seed, step, z);
        return;
    }
    const int64_t j0 = (g * 4) % shared_row;
    if ((j0 & 3) == 0 && j0 + 4 <= shared_row) {
        philox_normals4((uint64_t)(j0 >> 2), stream, seed, step, z);
        return;
    }
    float t[4] = {0.f, 0.f, 0.f, 0.f};
    int64_t have = -1;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int64_t j = (g * 4 + e) % shared_row;
        if ((j >> 2) != have) {
            have = j >> 2;
            philox_normals4((uint64_t)have, stream, seed, step, t);
        }
        z[e] = t[j & 3];
    }
}

__device__ __forceinline__ float sample_update(float a, float b, float sigma, float x, float o, float z) {
#pragma clang fp contract(off)
    const float ax = a * x, bo = b * o, sz = sigma * z;
    return (ax + bo) + sz;
}
__device__ __forceinline__ float guided(float u, float c, float g) {
#pragma clang fp contract(off)
    const float d = c - u;
    return u + g * d;
}

template <typename T, bool QUAD>
__device__ __forceinline__ void store_model_input(const SampleParams& p, int64_t i0, const float* v) {
    T* in = static_cast<T*>(p.in);
    if constexpr (QUAD) {
        Quad<T> q;
#pragma unroll
        for (int e = 0; e < 4; ++e) q.v[e] = from_f32<T>(v[e]);
        *reinterpret_cast<Quad<T>*>(in + i0) = q;
        if (p.cfg) *reinterpret_cast<Quad<T>*>(in + p.n_total + i0) = q;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (i0 + e >= p.n_total) break;
            const T c = from_f32<T>(v[e]);
            in[i0 + e] = c;
            if (p.cfg) in[p.n_total + i0 + e] = c;
        }
    }
}

// Keep mask (image-to-image with part of the latent held): after the method's own update x', the state becomes
//     x = m·y + (1 − m)·x',   y = k·init + n·ε       every product rounded on its own, each sum rounded once
// with m = mask[b, pixel] broadcast over channels, (k, n) = keep_coef[i] = (√ᾱ, √(1−ᾱ)) at the timestep of the NEXT evaluation
// ((1, 0) in the last row: sampling.keep_schedule) and ε the run's start draw, regenerated from (cursor[1], stream 3) — no noise
// buffer exists.  m == 1 leaves y, m == 0 leaves x', bit for bit.  The step kernels are templates over their parameter block: with
// SampleParams / MultistepParams they are the kernels they were, with the Keep* blocks below the blend is compiled in.
struct KeepParams {
    const float* mask;       // [B, hw]
    const float* init;       // [B, per_row] fp32, model space
    const float* keep_coef;  // [S, 2] = (k, n)
    int64_t per_row, hw;
};

struct KeepSampleParams : SampleParams {
    KeepParams k;
};
template <typename P> constexpr bool kHasKeep = false;
template <> constexpr bool kHasKeep<KeepSampleParams> = true;

__device__ __forceinline__ float keep_blend(float m, float y, float xn) {
#pragma clang fp contract(off)
    const float my = m * y, rest = (1.f - m) * xn;
    return my + rest;
}

// xn[0..3] of element group g (first element i0) blended in place.  QUAD: hw % 4 == 0 too, so the group lies inside one channel
// of one row and its four mask values are consecutive; otherwise the mask index is computed per element.
template <bool QUAD>
__device__ __forceinline__ void keep_apply(const KeepParams& k, int64_t n_total, int64_t shared_row, uint32_t seed, int step,
                                           int64_t g, float* xn) {
    const float kk = k.keep_coef[2 * step], kn = k.keep_coef[2 * step + 1];
    Quad<float> eps;
    sample_normals4(g, shared_row, kStreamInit, seed, 0u, eps.v);
    const int64_t i0 = g * 4;
    if constexpr (QUAD) {
        const int64_t b = i0 / k.per_row;
        const int64_t pix = (i0 - b * k.per_row) % k.hw;
        const Quad<float> init = *reinterpret_cast<const Quad<float>*>(k.init + i0);
        const Quad<float> m = *reinterpret_cast<const Quad<float>*>(k.mask + b * k.hw + pix);
#pragma unroll
        for (int e = 0; e < 4; ++e) xn[e] = keep_blend(m.v[e], ddpm_noisy(kk, kn, init.v[e], eps.v[e]), xn[e]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t i = i0 + e;
            if (i >= n_total) break;
            const int64_t b = i / k.per_row;
            const int64_t pix = (i - b * k.per_row) % k.hw;
            xn[e] = keep_blend(k.mask[b * k.hw + pix], ddpm_noisy(kk, kn, k.init[i], eps.v[e]), xn[e]);
        }
    }
}

template <typename T, bool QUAD>
__global__ __launch_bounds__(256) void sample_init_kernel(SampleParams p) {
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nthreads = (int64_t)gridDim.x * 256;
    const int64_t t0 = p.timesteps[0];
    for (int64_t r = tid; r < p.rows; r += nthreads) p.t_model[r] = t0;
    if (tid == 0) {
        p.cursor[0] = 0;
        p.cursor[1] = (int)p.seed;
    }
    const int64_t groups = (p.n_total + 3) >> 2;
    for (int64_t g = tid; g < groups; g += nthreads) {
        Quad<float> z;
        sample_normals4(g, p.shared_row, kStreamInit, p.seed, 0u, z.v);
        const int64_t i0 = g * 4;
        if constexpr (QUAD) {
            *reinterpret_cast<Quad<float>*>(p.x + i0) = z;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (i0 + e < p.n_total) p.x[i0 + e] = z.v[e];
        }
        store_model_input<T, QUAD>(p, i0, z.v);
    }
}

template <typename T, bool QUAD, typename P>
__global__ __launch_bounds__(256) void sample_step_kernel(P p) {
    constexpr bool KEEP = kHasKeep<P>;
    const int step = p.cursor[0];
    const uint32_t seed = (uint32_t)p.cursor[1];
    if (step < 0 || step >= p.S) return;  // (uniform over the whole launch: one replay too many touches nothing)
    const float a = p.coef[3 * step], b = p.coef[3 * step + 1], sigma = p.coef[3 * step + 2];
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nthreads = (int64_t)gridDim.x * 256;
    const int64_t t_next = p.timesteps[step + 1 < p.S ? step + 1 : step];  // (the last step leaves its own timestep)
    for (int64_t r = tid; r < p.rows; r += nthreads) p.t_model[r] = t_next;
    const T* out = static_cast<const T*>(p.out);
    const int64_t groups = (p.n_total + 3) >> 2;
    for (int64_t g = tid; g < groups; g += nthreads) {
        Quad<float> z;
        if (sigma != 0.f) {
            sample_normals4(g, p.shared_row, kStreamStepNoise, seed, (uint32_t)step, z.v);
        } else {
            z.v[0] = z.v[1] = z.v[2] = z.v[3] = 0.f;
        }
        const int64_t i0 = g * 4;
        Quad<float> xn = {};
        if constexpr (QUAD) {
            const Quad<float> x = *reinterpret_cast<const Quad<float>*>(p.x + i0);
            const Quad<T> u = *reinterpret_cast<const Quad<T>*>(out + i0);
            Quad<T> c = u;
            if (p.cfg) c = *reinterpret_cast<const Quad<T>*>(out + p.n_total + i0);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float uf = to_f32<T>(u.v[e]);
                const float o = p.cfg ? guided(uf, to_f32<T>(c.v[e]), p.guidance) : uf;
                xn.v[e] = sample_update(a, b, sigma, x.v[e], o, z.v[e]);
            }
            if constexpr (KEEP) keep_apply<true>(p.k, p.n_total, p.shared_row, seed, step, g, xn.v);
            *reinterpret_cast<Quad<float>*>(p.x + i0) = xn;
            if (p.z_out) *reinterpret_cast<Quad<float>*>(p.z_out + i0) = z;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int64_t i = i0 + e;
                if (i >= p.n_total) break;
                const float uf = to_f32<T>(out[i]);
                const float o = p.cfg ? guided(uf, to_f32<T>(out[p.n_total + i]), p.guidance) : uf;
                xn.v[e] = sample_update(a, b, sigma, p.x[i], o, z.v[e]);
                if constexpr (!KEEP) p.x[i] = xn.v[e];
                if (p.z_out) p.z_out[i] = z.v[e];
            }
            if constexpr (KEEP) {
                keep_apply<false>(p.k, p.n_total, p.shared_row, seed, step, g, xn.v);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (i0 + e < p.n_total) p.x[i0 + e] = xn.v[e];
            }
        }
        store_model_input<T, QUAD>(p, i0, xn.v);
    }
}

__global__ void sample_advance_kernel(int* cursor, int S) {
    const int c = *cursor;
    if (c >= 0 && c < S) *cursor = c + 1;  // (saturates at S: further replays stay no-ops)
}

template <typename T>
void launch_sample(const SampleParams& p, int64_t per_row, bool init, hipStream_t s) {
    const bool quad = (per_row % 4) == 0 && quad_aligned<float>(p.x) && quad_aligned<T>(p.out) && quad_aligned<T>(p.in) &&
                      quad_aligned<float>(p.z_out);
    const dim3 grid(posterior_blocks(p.n_total));
    if (init) {
        if (quad)
            hipLaunchKernelGGL((sample_init_kernel<T, true>), grid, dim3(256), 0, s, p);
        else
            hipLaunchKernelGGL((sample_init_kernel<T, false>), grid, dim3(256), 0, s, p);
    } else {
        if (quad)
            hipLaunchKernelGGL((sample_step_kernel<T, true, SampleParams>), grid, dim3(256), 0, s, p);
        else
            hipLaunchKernelGGL((sample_step_kernel<T, false, SampleParams>), grid, dim3(256), 0, s, p);
    }
}

int launch_sample_dtype(const SampleParams& p, int64_t per_row, bool init, int dtype, hipStream_t s) {
    switch (dtype) {
        case LORA_F32: launch_sample<float>(p, per_row, init, s); break;
        case LORA_F16: launch_sample<half_t>(p, per_row, init, s); break;
        default: launch_sample<bf16_t>(p, per_row, init, s); break;
    }
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}

// Linear multistep step (PLMS = PNDM with skip_prk_steps, the scheduler of the class-image pipeline of
// train_lora_dreambooth.py:512-558 and of visualize_progress, utils.py:191-211; DPM-Solver++(2M)).  Per iteration i = cursor[0]:
//     h    = p·x + q·o                          the quantity the method keeps history of (o guided as above)
//     base = USE_SAVED ? xs : x
//     x'   = a·base + c0·h + c1·H[s1] + c2·H[s2] + c3·H[s3]          summed left to right, every product rounded on its own
//     SAVE: xs ← x (the state before the update);   PUSH: H[w] ← h;   x ← x'
// (p, q, a, c0..c3) = coef[i] and (w, s1, s2, s3, flags) = plan[i] come from the host (sampling.multistep_schedule), which knows
// the ring's whole future: no ring arithmetic here.  A term whose coefficient is exactly 0 is neither loaded nor added — the
// history slots and xs are uninitialised memory during warm-up and 0·NaN must not reach the state; the branch is uniform over
// the launch.  Each thread reads and writes its own elements of x, xs and H[*] only, every read before the first write.
constexpr int kMultistepPush = 1, kMultistepSave = 2, kMultistepUseSaved = 4;

struct MultistepParams {
    SampleParams s;   // x, out, in, t_model, cursor, timesteps, coef = [I, 7], n_total, rows, S = I, cfg, guidance
    float* xs;        // [B, per_row] fp32: the saved state
    float* hist;      // [4, B·per_row] fp32: the history ring
    const int* plan;  // [I, 5]
};
struct KeepMultistepParams : MultistepParams {
    KeepParams k;
};
template <> constexpr bool kHasKeep<KeepMultistepParams> = true;

__device__ __forceinline__ float multistep_history(float p, float q, float x, float o) {
#pragma clang fp contract(off)
    const float px = p * x, qo = q * o;
    return px + qo;
}
__device__ __forceinline__ float multistep_update(float a, float c0, float c1, float c2, float c3, float base, float h, float h1,
                                                  float h2, float h3) {
#pragma clang fp contract(off)
    float acc = 0.f;
    if (a != 0.f) acc = a * base;
    if (c0 != 0.f) { const float t = c0 * h; acc = acc + t; }
    if (c1 != 0.f) { const float t = c1 * h1; acc = acc + t; }
    if (c2 != 0.f) { const float t = c2 * h2; acc = acc + t; }
    if (c3 != 0.f) { const float t = c3 * h3; acc = acc + t; }
    return acc;
}

template <typename T, bool QUAD, typename P>
__global__ __launch_bounds__(256) void sample_multistep_kernel(P m) {
    constexpr bool KEEP = kHasKeep<P>;
    const SampleParams& p = m.s;
    const int it = p.cursor[0];
    if (it < 0 || it >= p.S) return;  // (uniform over the whole launch: one replay too many touches nothing)
    const float* cf = p.coef + 7 * it;
    const float kp = cf[0], kq = cf[1], a = cf[2], c0 = cf[3], c1 = cf[4], c2 = cf[5], c3 = cf[6];
    const int* pl = m.plan + 5 * it;
    const int flags = pl[4];
    // (slot numbers masked to the ring: a wrong plan reads a wrong slot, never memory outside the ring)
    float* hw = m.hist + (int64_t)(pl[0] & 3) * p.n_total;
    const float* hs1 = m.hist + (int64_t)(pl[1] & 3) * p.n_total;
    const float* hs2 = m.hist + (int64_t)(pl[2] & 3) * p.n_total;
    const float* hs3 = m.hist + (int64_t)(pl[3] & 3) * p.n_total;
    const bool push = (flags & kMultistepPush) != 0, save = (flags & kMultistepSave) != 0;
    const bool saved_base = (flags & kMultistepUseSaved) != 0 && a != 0.f;
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nthreads = (int64_t)gridDim.x * 256;
    const int64_t t_next = p.timesteps[it + 1 < p.S ? it + 1 : it];
    for (int64_t r = tid; r < p.rows; r += nthreads) p.t_model[r] = t_next;
    const T* out = static_cast<const T*>(p.out);
    const int64_t groups = (p.n_total + 3) >> 2;
    for (int64_t g = tid; g < groups; g += nthreads) {
        const int64_t i0 = g * 4;
        Quad<float> xn = {};
        if constexpr (QUAD) {
            const Quad<float> x = *reinterpret_cast<const Quad<float>*>(p.x + i0);
            const Quad<T> u = *reinterpret_cast<const Quad<T>*>(out + i0);
            Quad<T> c = u;
            if (p.cfg) c = *reinterpret_cast<const Quad<T>*>(out + p.n_total + i0);
            Quad<float> base = x, h1 = {}, h2 = {}, h3 = {}, h;
            if (saved_base) base = *reinterpret_cast<const Quad<float>*>(m.xs + i0);
            if (c1 != 0.f) h1 = *reinterpret_cast<const Quad<float>*>(hs1 + i0);
            if (c2 != 0.f) h2 = *reinterpret_cast<const Quad<float>*>(hs2 + i0);
            if (c3 != 0.f) h3 = *reinterpret_cast<const Quad<float>*>(hs3 + i0);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float uf = to_f32<T>(u.v[e]);
                const float o = p.cfg ? guided(uf, to_f32<T>(c.v[e]), p.guidance) : uf;
                h.v[e] = multistep_history(kp, kq, x.v[e], o);
                xn.v[e] = multistep_update(a, c0, c1, c2, c3, base.v[e], h.v[e], h1.v[e], h2.v[e], h3.v[e]);
            }
            if constexpr (KEEP) keep_apply<true>(m.k, p.n_total, p.shared_row, (uint32_t)p.cursor[1], it, g, xn.v);
            if (save) *reinterpret_cast<Quad<float>*>(m.xs + i0) = x;
            if (push) *reinterpret_cast<Quad<float>*>(hw + i0) = h;
            *reinterpret_cast<Quad<float>*>(p.x + i0) = xn;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int64_t i = i0 + e;
                if (i >= p.n_total) break;
                const float x = p.x[i];
                const float uf = to_f32<T>(out[i]);
                const float o = p.cfg ? guided(uf, to_f32<T>(out[p.n_total + i]), p.guidance) : uf;
                const float base = saved_base ? m.xs[i] : x;
                const float h1 = c1 != 0.f ? hs1[i] : 0.f, h2 = c2 != 0.f ? hs2[i] : 0.f, h3 = c3 != 0.f ? hs3[i] : 0.f;
                const float h = multistep_history(kp, kq, x, o);
                xn.v[e] = multistep_update(a, c0, c1, c2, c3, base, h, h1, h2, h3);
                if (save) m.xs[i] = x;
                if (push) hw[i] = h;
                if constexpr (!KEEP) p.x[i] = xn.v[e];
            }
            if constexpr (KEEP) {
                keep_apply<false>(m.k, p.n_total, p.shared_row, (uint32_t)p.cursor[1], it, g, xn.v);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (i0 + e < p.n_total) p.x[i0 + e] = xn.v[e];
            }
        }
        store_model_input<T, QUAD>(p, i0, xn.v);
    }
}


template <typename T>
void launch_multistep(const MultistepParams& m, int64_t per_row, hipStream_t s) {
    const SampleParams& p = m.s;
    const bool quad = (per_row % 4) == 0 && quad_aligned<float>(p.x) && quad_aligned<T>(p.out) && quad_aligned<T>(p.in) &&
                      quad_aligned<float>(m.xs) && quad_aligned<float>(m.hist);  // (n_total % 4 == 0: every slot as hist)
    const dim3 grid(posterior_blocks(p.n_total));
    if (quad)
        hipLaunchKernelGGL((sample_multistep_kernel<T, true, MultistepParams>), grid, dim3(256), 0, s, m);
    else
        hipLaunchKernelGGL((sample_multistep_kernel<T, false, MultistepParams>), grid, dim3(256), 0, s, m);
}

}  // namespace

extern "C" int ddpm_sample_multistep(float* x, float* xs, float* hist, const void* model_out, void* model_in, int64_t* t_model,
                                     const int* cursor, const int64_t* timesteps, const float* coef, const int* plan, int B,
                                     int64_t per_row, int I, int cfg, float guidance_scale, int dtype, void* stream) {
    if (!x || !xs || !hist || !model_out || !model_in || !t_model || !cursor || !timesteps || !coef || !plan || B < 1 ||
        per_row < 1 || I < 1 || !known_dtype(dtype))
        return LORA_E_BADARG;
    MultistepParams m{};
    SampleParams& p = m.s;
    p.x = x; p.out = model_out; p.in = model_in; p.t_model = t_model; p.cursor = const_cast<int*>(cursor);
    p.timesteps = timesteps; p.coef = coef;
    p.n_total = (int64_t)B * per_row; p.rows = cfg ? 2 * B : B; p.S = I; p.cfg = cfg ? 1 : 0;
    p.guidance = guidance_scale;
    m.xs = xs; m.hist = hist; m.plan = plan;
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (dtype) {
        case LORA_F32: launch_multistep<float>(m, per_row, s); break;
        case LORA_F16: launch_multistep<half_t>(m, per_row, s); break;
        default: launch_multistep<bf16_t>(m, per_row, s); break;
    }
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}

namespace {
int ddpm_sample_init_impl(float* x, void* model_in, int64_t* t_model, int* cursor, const int64_t* timesteps, int B,
                                int64_t per_row, int S, int cfg, uint64_t seed, int dtype, void* stream, bool shared) {
    if (!x || !model_in || !t_model || !cursor || !timesteps || B < 1 || per_row < 1 || S < 1 || !known_dtype(dtype))
        return LORA_E_BADARG;
    SampleParams p{};
    p.x = x; p.in = model_in; p.t_model = t_model; p.cursor = cursor; p.timesteps = timesteps;
    p.n_total = (int64_t)B * per_row; p.rows = cfg ? 2 * B : B; p.S = S; p.cfg = cfg ? 1 : 0; p.seed = (uint32_t)seed;
    p.shared_row = shared ? per_row : 0;
    return launch_sample_dtype(p, per_row, true, dtype, static_cast<hipStream_t>(stream));
}
}  // namespace

extern "C" int ddpm_sample_init(float* x, void* model_in, int64_t* t_model, int* cursor, const int64_t* timesteps, int B,
                                int64_t per_row, int S, int cfg, uint64_t seed, int dtype, void* stream) {
    return ddpm_sample_init_impl(x, model_in, t_model, cursor, timesteps, B, per_row, S, cfg, seed, dtype, stream, false);
}
extern "C" int ddpm_sample_init_shared(float* x, void* model_in, int64_t* t_model, int* cursor, const int64_t* timesteps, int B,
                                int64_t per_row, int S, int cfg, uint64_t seed, int dtype, void* stream) {
    return ddpm_sample_init_impl(x, model_in, t_model, cursor, timesteps, B, per_row, S, cfg, seed, dtype, stream, true);
}

namespace {
int ddpm_sample_step_impl(float* x, const void* model_out, void* model_in, int64_t* t_model, const int* cursor,
                                const int64_t* timesteps, const float* coef, float* z_out, int B, int64_t per_row, int S,
                                int cfg, float guidance_scale, int dtype, void* stream, bool shared) {
    if (!x || !model_out || !model_in || !t_model || !cursor || !timesteps || !coef || B < 1 || per_row < 1 || S < 1 ||
        !known_dtype(dtype))
        return LORA_E_BADARG;
    SampleParams p{};
    p.x = x; p.out = model_out; p.in = model_in; p.t_model = t_model; p.cursor = const_cast<int*>(cursor);
    p.timesteps = timesteps; p.coef = coef; p.z_out = z_out;
    p.n_total = (int64_t)B * per_row; p.rows = cfg ? 2 * B : B; p.S = S; p.cfg = cfg ? 1 : 0;
    p.guidance = guidance_scale;
    p.shared_row = shared ? per_row : 0;
    return launch_sample_dtype(p, per_row, false, dtype, static_cast<hipStream_t>(stream));
}
}  // namespace

extern "C" int ddpm_sample_step(float* x, const void* model_out, void* model_in, int64_t* t_model, const int* cursor,
                                const int64_t* timesteps, const float* coef, float* z_out, int B, int64_t per_row, int S,
                                int cfg, float guidance_scale, int dtype, void* stream) {
    return ddpm_sample_step_impl(x, model_out, model_in, t_model, cursor, timesteps, coef, z_out, B, per_row, S, cfg,
                                 guidance_scale, dtype, stream, false);
}
extern "C" int ddpm_sample_step_shared(float* x, const void* model_out, void* model_in, int64_t* t_model, const int* cursor,
                                const int64_t* timesteps, const float* coef, float* z_out, int B, int64_t per_row, int S,
                                int cfg, float guidance_scale, int dtype, void* stream) {
    return ddpm_sample_step_impl(x, model_out, model_in, t_model, cursor, timesteps, coef, z_out, B, per_row, S, cfg,
                                 guidance_scale, dtype, stream, true);
}

extern "C" int ddpm_sample_advance(int* cursor, int S, void* stream) {
    if (!cursor || S < 1) return LORA_E_BADARG;
    hipLaunchKernelGGL(sample_advance_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), cursor, S);
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Image-to-image starts and keep-mask steps of the latent sampler ("Making Img2Img Inference with LoRA", README.md:287-289 and
// scripts/run_img2img.ipynb of the reference: `pipe(image=init_image, strength=0.75)`).  A run that starts part-way down the grid
// is the same recorded iteration with another cursor: ddpm_sample_init_from writes the noised start state
//     x = k·init + n·ε,   ε the x_T draw of ddpm_sample_init (stream 3, key (seed, 0)),   (k, n) = (√ᾱ, √(1−ᾱ)) at timesteps[start]
// and cursor = {start, seed}; the keep entries are the two step kernels with KEEP on (keep_apply above).
namespace {

struct InitFromParams {
    const float* init;  // [B, per_row] fp32
    float* eps_out;     // nullable
    int start;
    float k, n;
};

template <typename T, bool QUAD>
__global__ __launch_bounds__(256) void sample_init_from_kernel(SampleParams p, InitFromParams f) {
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nthreads = (int64_t)gridDim.x * 256;
    const int64_t t0 = p.timesteps[f.start];
    for (int64_t r = tid; r < p.rows; r += nthreads) p.t_model[r] = t0;
    if (tid == 0) {
        p.cursor[0] = f.start;
        p.cursor[1] = (int)p.seed;
    }
    const int64_t groups = (p.n_total + 3) >> 2;
    for (int64_t g = tid; g < groups; g += nthreads) {
        Quad<float> z, x = {};
        sample_normals4(g, p.shared_row, kStreamInit, p.seed, 0u, z.v);
        const int64_t i0 = g * 4;
        if constexpr (QUAD) {
            const Quad<float> init = *reinterpret_cast<const Quad<float>*>(f.init + i0);
#pragma unroll
            for (int e = 0; e < 4; ++e) x.v[e] = ddpm_noisy(f.k, f.n, init.v[e], z.v[e]);
            *reinterpret_cast<Quad<float>*>(p.x + i0) = x;
            if (f.eps_out) *reinterpret_cast<Quad<float>*>(f.eps_out + i0) = z;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int64_t i = i0 + e;
                if (i >= p.n_total) break;
                x.v[e] = ddpm_noisy(f.k, f.n, f.init[i], z.v[e]);
                p.x[i] = x.v[e];
                if (f.eps_out) f.eps_out[i] = z.v[e];
            }
        }
        store_model_input<T, QUAD>(p, i0, x.v);
    }
}

template <typename T>
void launch_init_from(const SampleParams& p, const InitFromParams& f, int64_t per_row, hipStream_t s) {
    const bool quad = (per_row % 4) == 0 && quad_aligned<float>(p.x) && quad_aligned<T>(p.in) && quad_aligned<float>(f.init) &&
                      quad_aligned<float>(f.eps_out);
    const dim3 grid(posterior_blocks(p.n_total));
    if (quad)
        hipLaunchKernelGGL((sample_init_from_kernel<T, true>), grid, dim3(256), 0, s, p, f);
    else
        hipLaunchKernelGGL((sample_init_from_kernel<T, false>), grid, dim3(256), 0, s, p, f);
}

// (hw % 4 == 0: a group of four then lies inside one channel and its mask values are four consecutive, aligned floats)
template <typename T>
bool keep_quad(const SampleParams& p, const KeepParams& k) {
    return (k.per_row % 4) == 0 && (k.hw % 4) == 0 && quad_aligned<float>(p.x) && quad_aligned<T>(p.out) && quad_aligned<T>(p.in) &&
           quad_aligned<float>(p.z_out) && quad_aligned<float>(k.init) && quad_aligned<float>(k.mask);
}

template <typename T>
void launch_step_keep(const KeepSampleParams& p, hipStream_t s) {
    const dim3 grid(posterior_blocks(p.n_total));
    if (keep_quad<T>(p, p.k))
        hipLaunchKernelGGL((sample_step_kernel<T, true, KeepSampleParams>), grid, dim3(256), 0, s, p);
    else
        hipLaunchKernelGGL((sample_step_kernel<T, false, KeepSampleParams>), grid, dim3(256), 0, s, p);
}

template <typename T>
void launch_multistep_keep(const KeepMultistepParams& m, hipStream_t s) {
    const dim3 grid(posterior_blocks(m.s.n_total));
    if (keep_quad<T>(m.s, m.k) && quad_aligned<float>(m.xs) && quad_aligned<float>(m.hist))
        hipLaunchKernelGGL((sample_multistep_kernel<T, true, KeepMultistepParams>), grid, dim3(256), 0, s, m);
    else
        hipLaunchKernelGGL((sample_multistep_kernel<T, false, KeepMultistepParams>), grid, dim3(256), 0, s, m);
}

bool keep_args_ok(const float* mask, const float* init, const float* keep_coef, int64_t per_row, int64_t hw) {
    return mask && init && keep_coef && per_row >= 1 && hw >= 1 && per_row % hw == 0;
}

}  // namespace

namespace {
int ddpm_sample_init_from_impl(float* x, void* model_in, int64_t* t_model, int* cursor, const int64_t* timesteps,
                                     const float* init, float* eps_out, int B, int64_t per_row, int S, int start, float k,
                                     float n, int cfg, uint64_t seed, int dtype, void* stream, bool shared) {
    if (!x || !model_in || !t_model || !cursor || !timesteps || !init || B < 1 || per_row < 1 || S < 1 || start < 0 ||
        start >= S || !known_dtype(dtype))
        return LORA_E_BADARG;
    SampleParams p{};
    p.x = x; p.in = model_in; p.t_model = t_model; p.cursor = cursor; p.timesteps = timesteps;
    p.n_total = (int64_t)B * per_row; p.rows = cfg ? 2 * B : B; p.S = S; p.cfg = cfg ? 1 : 0; p.seed = (uint32_t)seed;
    p.shared_row = shared ? per_row : 0;
    InitFromParams f{};
    f.init = init; f.eps_out = eps_out; f.start = start; f.k = k; f.n = n;
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (dtype) {
        case LORA_F32: launch_init_from<float>(p, f, per_row, s); break;
        case LORA_F16: launch_init_from<half_t>(p, f, per_row, s); break;
        default: launch_init_from<bf16_t>(p, f, per_row, s); break;
    }
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}
}  // namespace

extern "C" int ddpm_sample_init_from(float* x, void* model_in, int64_t* t_model, int* cursor, const int64_t* timesteps,
                                     const float* init, float* eps_out, int B, int64_t per_row, int S, int start, float k,
                                     float n, int cfg, uint64_t seed, int dtype, void* stream) {
    return ddpm_sample_init_from_impl(x, model_in, t_model, cursor, timesteps, init, eps_out, B, per_row, S, start, k, n,
                                      cfg, seed, dtype, stream, false);
}
extern "C" int ddpm_sample_init_from_shared(float* x, void* model_in, int64_t* t_model, int* cursor, const int64_t* timesteps,
                                     const float* init, float* eps_out, int B, int64_t per_row, int S, int start, float k,
                                     float n, int cfg, uint64_t seed, int dtype, void* stream) {
    return ddpm_sample_init_from_impl(x, model_in, t_model, cursor, timesteps, init, eps_out, B, per_row, S, start, k, n,
                                      cfg, seed, dtype, stream, true);
}

namespace {
int ddpm_sample_step_keep_impl(float* x, const void* model_out, void* model_in, int64_t* t_model, const int* cursor,
                                     const int64_t* timesteps, const float* coef, float* z_out, const float* mask,
                                     const float* init, const float* keep_coef, int B, int64_t per_row, int64_t hw, int S, int cfg,
                                     float guidance_scale, int dtype, void* stream, bool shared) {
    if (!x || !model_out || !model_in || !t_model || !cursor || !timesteps || !coef || B < 1 || S < 1 ||
        !keep_args_ok(mask, init, keep_coef, per_row, hw) || !known_dtype(dtype))
        return LORA_E_BADARG;
    KeepSampleParams p{};
    p.x = x; p.out = model_out; p.in = model_in; p.t_model = t_model; p.cursor = const_cast<int*>(cursor);
    p.timesteps = timesteps; p.coef = coef; p.z_out = z_out;
    p.n_total = (int64_t)B * per_row; p.rows = cfg ? 2 * B : B; p.S = S; p.cfg = cfg ? 1 : 0;
    p.guidance = guidance_scale;
    p.k = KeepParams{mask, init, keep_coef, per_row, hw};
    p.shared_row = shared ? per_row : 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (dtype) {
        case LORA_F32: launch_step_keep<float>(p, s); break;
        case LORA_F16: launch_step_keep<half_t>(p, s); break;
        default: launch_step_keep<bf16_t>(p, s); break;
    }
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}
}  // namespace

extern "C" int ddpm_sample_step_keep(float* x, const void* model_out, void* model_in, int64_t* t_model, const int* cursor,
                                     const int64_t* timesteps, const float* coef, float* z_out, const float* mask,
                                     const float* init, const float* keep_coef, int B, int64_t per_row, int64_t hw, int S, int cfg,
                                     float guidance_scale, int dtype, void* stream) {
    return ddpm_sample_step_keep_impl(x, model_out, model_in, t_model, cursor, timesteps, coef, z_out, mask, init, keep_coef,
                                      B, per_row, hw, S, cfg, guidance_scale, dtype, stream, false);
}
extern "C" int ddpm_sample_step_keep_shared(float* x, const void* model_out, void* model_in, int64_t* t_model, const int* cursor,
                                     const int64_t* timesteps, const float* coef, float* z_out, const float* mask,
                                     const float* init, const float* keep_coef, int B, int64_t per_row, int64_t hw, int S, int cfg,
                                     float guidance_scale, int dtype, void* stream) {
    return ddpm_sample_step_keep_impl(x, model_out, model_in, t_model, cursor, timesteps, coef, z_out, mask, init, keep_coef,
                                      B, per_row, hw, S, cfg, guidance_scale, dtype, stream, true);
}

namespace {
int ddpm_sample_multistep_keep_impl(float* x, float* xs, float* hist, const void* model_out, void* model_in,
                                          int64_t* t_model, const int* cursor, const int64_t* timesteps, const float* coef,
                                          const int* plan, const float* mask, const float* init, const float* keep_coef, int B,
                                          int64_t per_row, int64_t hw, int I, int cfg, float guidance_scale, int dtype,
                                          void* stream, bool shared) {
    if (!x || !xs || !hist || !model_out || !model_in || !t_model || !cursor || !timesteps || !coef || !plan || B < 1 || I < 1 ||
        !keep_args_ok(mask, init, keep_coef, per_row, hw) || !known_dtype(dtype))
        return LORA_E_BADARG;
    KeepMultistepParams m{};
    SampleParams& p = m.s;
    p.x = x; p.out = model_out; p.in = model_in; p.t_model = t_model; p.cursor = const_cast<int*>(cursor);
    p.timesteps = timesteps; p.coef = coef;
    p.n_total = (int64_t)B * per_row; p.rows = cfg ? 2 * B : B; p.S = I; p.cfg = cfg ? 1 : 0;
    p.guidance = guidance_scale;
    m.xs = xs; m.hist = hist; m.plan = plan;
    m.k = KeepParams{mask, init, keep_coef, per_row, hw};
    p.shared_row = shared ? per_row : 0;
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (dtype) {
        case LORA_F32: launch_multistep_keep<float>(m, s); break;
        case LORA_F16: launch_multistep_keep<half_t>(m, s); break;
        default: launch_multistep_keep<bf16_t>(m, s); break;
    }
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}
}  // namespace

extern "C" int ddpm_sample_multistep_keep(float* x, float* xs, float* hist, const void* model_out, void* model_in,
                                          int64_t* t_model, const int* cursor, const int64_t* timesteps, const float* coef,
                                          const int* plan, const float* mask, const float* init, const float* keep_coef, int B,
                                          int64_t per_row, int64_t hw, int I, int cfg, float guidance_scale, int dtype,
                                          void* stream) {
    return ddpm_sample_multistep_keep_impl(x, xs, hist, model_out, model_in, t_model, cursor, timesteps, coef, plan, mask,
                                           init, keep_coef, B, per_row, hw, I, cfg, guidance_scale, dtype, stream, false);
}
extern "C" int ddpm_sample_multistep_keep_shared(float* x, float* xs, float* hist, const void* model_out, void* model_in,
                                          int64_t* t_model, const int* cursor, const int64_t* timesteps, const float* coef,
                                          const int* plan, const float* mask, const float* init, const float* keep_coef, int B,
                                          int64_t per_row, int64_t hw, int I, int cfg, float guidance_scale, int dtype,
                                          void* stream) {
    return ddpm_sample_multistep_keep_impl(x, xs, hist, model_out, model_in, t_model, cursor, timesteps, coef, plan, mask,
                                           init, keep_coef, B, per_row, hw, I, cfg, guidance_scale, dtype, stream, true);
}

// ---------------------------------------------------------------------------------------------------------
// Sigma-space step (k-diffusion's Euler, Euler-ancestral and Heun: the `EulerAncestralDiscreteScheduler` cells of
// scripts/lora_training_process_visualized.ipynb:57 and scripts/merge_lora_with_lora.ipynb:74 of the reference, and the
// equal-seed comparison loop of utils.py:191-211 run under them).  The state lives in sigma space — x_T = σ₀·z — the model is
// fed c_in(σ)·x with the σ of the NEXT evaluation, and the timestep grid is fractional: `timesteps` and `t_model` are fp32.
// Per iteration i = cursor[0], (p, q, a, c0, c1, s, n, σ_eval) = coef[i] and flags = plan[i][4] (sampling.sigma_schedule):
//     h    = p·x + q·o                          d = (x − denoised)/σ of the method (o guided as above)
//     base = USE_SAVED ? xs : x
//     x'   = a·base + c0·h + c1·H + s·z         left to right, every product rounded on its own; z only where s ≠ 0
//     SAVE: xs ← x;   PUSH: H ← h               (one history slot: Heun's d₁)
//     x ← x' (after the keep blend, where compiled in);   model_in ← cast(fp32(n·x));   t_model ← timesteps[min(i+1, I−1)]
// It needs what neither kernel above has alone: the variance noise of sample_step_kernel (euler_a) and the saved state and
// history of sample_multistep_kernel (heun).  A term whose coefficient is exactly 0 is neither loaded nor added, so xs and H
// stay unread until a Heun stage B — they are uninitialised memory before.
namespace {

struct SigmaParams {
    SampleParams s;   // x, out, in, cursor, coef = [I, 8], z_out, n_total, rows, S = I, cfg, guidance, shared_row; t_model and
                      // timesteps unused (fp32 here: below)
    float* xs;        // [B, per_row] fp32: the saved state
    float* hist;      // [B, per_row] fp32: the one history slot
    const int* plan;  // [I, 5]
    float* t_model;           // [rows] fp32
    const float* timesteps;   // [I] fp32
};
struct KeepSigmaParams : SigmaParams {
    KeepParams k;
};
template <> constexpr bool kHasKeep<KeepSigmaParams> = true;

__device__ __forceinline__ float sigma_history(float p, float q, float x, float o) {
#pragma clang fp contract(off)
    const float qo = q * o;
    if (p == 0.f) return qo;
    const float px = p * x;
    return px + qo;
}
__device__ __forceinline__ float sigma_update(float a, float c0, float c1, float s, float base, float h, float h1, float z) {
#pragma clang fp contract(off)
    float acc = 0.f;
    if (a != 0.f) acc = a * base;
    if (c0 != 0.f) { const float t = c0 * h; acc = acc + t; }
    if (c1 != 0.f) { const float t = c1 * h1; acc = acc + t; }
    if (s != 0.f) { const float t = s * z; acc = acc + t; }
    return acc;
}
// fp32(n·x), an operation of its own: without `exceptions(strict)` hipcc folds the product into the f16 conversion that follows
// (v_fma_mixlo_f16 — ONE rounding, to f16), and the model input is then not the cast of the fp32 product: 1 f16 ulp off in about
// one element in a thousand, and differently on the 4-element path, which converts in pairs.
__device__ __forceinline__ float sigma_scaled(float n, float x) {
#pragma clang fp contract(off)
#pragma clang fp exceptions(strict)
    return n * x;
}

template <typename T, bool QUAD, typename P>
__global__ __launch_bounds__(256) void sample_sigma_kernel(P m) {
    constexpr bool KEEP = kHasKeep<P>;
    const SampleParams& p = m.s;
    const int it = p.cursor[0];
    const uint32_t seed = (uint32_t)p.cursor[1];
    if (it < 0 || it >= p.S) return;  // (uniform over the whole launch: one replay too many touches nothing)
    const float* cf = p.coef + 8 * it;
    const float kp = cf[0], kq = cf[1], a = cf[2], c0 = cf[3], c1 = cf[4], sn = cf[5], n_in = cf[6];
    const int flags = m.plan[5 * it + 4];
    const bool push = (flags & kMultistepPush) != 0, save = (flags & kMultistepSave) != 0;
    const bool saved_base = (flags & kMultistepUseSaved) != 0 && a != 0.f;
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nthreads = (int64_t)gridDim.x * 256;
    const float t_next = m.timesteps[it + 1 < p.S ? it + 1 : it];
    for (int64_t r = tid; r < p.rows; r += nthreads) m.t_model[r] = t_next;
    const T* out = static_cast<const T*>(p.out);
    const int64_t groups = (p.n_total + 3) >> 2;
    for (int64_t g = tid; g < groups; g += nthreads) {
        Quad<float> z;
        if (sn != 0.f) {
            sample_normals4(g, p.shared_row, kStreamStepNoise, seed, (uint32_t)it, z.v);
        } else {
            z.v[0] = z.v[1] = z.v[2] = z.v[3] = 0.f;
        }
        const int64_t i0 = g * 4;
        Quad<float> xn = {}, scaled;
        if constexpr (QUAD) {
            const Quad<float> x = *reinterpret_cast<const Quad<float>*>(p.x + i0);
            const Quad<T> u = *reinterpret_cast<const Quad<T>*>(out + i0);
            Quad<T> c = u;
            if (p.cfg) c = *reinterpret_cast<const Quad<T>*>(out + p.n_total + i0);
            Quad<float> base = x, h1 = {}, h;
            if (saved_base) base = *reinterpret_cast<const Quad<float>*>(m.xs + i0);
            if (c1 != 0.f) h1 = *reinterpret_cast<const Quad<float>*>(m.hist + i0);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float uf = to_f32<T>(u.v[e]);
                const float o = p.cfg ? guided(uf, to_f32<T>(c.v[e]), p.guidance) : uf;
                h.v[e] = sigma_history(kp, kq, x.v[e], o);
                xn.v[e] = sigma_update(a, c0, c1, sn, base.v[e], h.v[e], h1.v[e], z.v[e]);
            }
            if constexpr (KEEP) keep_apply<true>(m.k, p.n_total, p.shared_row, seed, it, g, xn.v);
            if (save) *reinterpret_cast<Quad<float>*>(m.xs + i0) = x;
            if (push) *reinterpret_cast<Quad<float>*>(m.hist + i0) = h;
            *reinterpret_cast<Quad<float>*>(p.x + i0) = xn;
            if (p.z_out) *reinterpret_cast<Quad<float>*>(p.z_out + i0) = z;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int64_t i = i0 + e;
                if (i >= p.n_total) break;
                const float x = p.x[i];
                const float uf = to_f32<T>(out[i]);
                const float o = p.cfg ? guided(uf, to_f32<T>(out[p.n_total + i]), p.guidance) : uf;
                const float base = saved_base ? m.xs[i] : x;
                const float h1 = c1 != 0.f ? m.hist[i] : 0.f;
                const float h = sigma_history(kp, kq, x, o);
                xn.v[e] = sigma_update(a, c0, c1, sn, base, h, h1, z.v[e]);
                if (save) m.xs[i] = x;
                if (push) m.hist[i] = h;
                if constexpr (!KEEP) p.x[i] = xn.v[e];
                if (p.z_out) p.z_out[i] = z.v[e];
            }
            if constexpr (KEEP) {
                keep_apply<false>(m.k, p.n_total, p.shared_row, seed, it, g, xn.v);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (i0 + e < p.n_total) p.x[i0 + e] = xn.v[e];
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) scaled.v[e] = sigma_scaled(n_in, xn.v[e]);
        store_model_input<T, QUAD>(p, i0, scaled.v);
    }
}

struct SigmaInitParams {
    const float* init;  // nullable: text-to-image, x = nn·ε
    float* eps_out;     // nullable
    float* t_model;           // [rows] fp32
    const float* timesteps;   // [I] fp32
    int start;
    float k, nn, c_in;
};

template <typename T, bool QUAD>
__global__ __launch_bounds__(256) void sample_sigma_init_kernel(SampleParams p, SigmaInitParams f) {
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nthreads = (int64_t)gridDim.x * 256;
    const float t0 = f.timesteps[f.start];
    for (int64_t r = tid; r < p.rows; r += nthreads) f.t_model[r] = t0;
    if (tid == 0) {
        p.cursor[0] = f.start;
        p.cursor[1] = (int)p.seed;
    }
    const int64_t groups = (p.n_total + 3) >> 2;
    for (int64_t g = tid; g < groups; g += nthreads) {
        Quad<float> z, x = {}, scaled;
        sample_normals4(g, p.shared_row, kStreamInit, p.seed, 0u, z.v);
        const int64_t i0 = g * 4;
        if constexpr (QUAD) {
            if (f.init) {
                const Quad<float> init = *reinterpret_cast<const Quad<float>*>(f.init + i0);
#pragma unroll
                for (int e = 0; e < 4; ++e) x.v[e] = ddpm_noisy(f.k, f.nn, init.v[e], z.v[e]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) x.v[e] = sigma_scaled(f.nn, z.v[e]);
            }
            *reinterpret_cast<Quad<float>*>(p.x + i0) = x;
            if (f.eps_out) *reinterpret_cast<Quad<float>*>(f.eps_out + i0) = z;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int64_t i = i0 + e;
                if (i >= p.n_total) break;
                x.v[e] = f.init ? ddpm_noisy(f.k, f.nn, f.init[i], z.v[e]) : sigma_scaled(f.nn, z.v[e]);
                p.x[i] = x.v[e];
                if (f.eps_out) f.eps_out[i] = z.v[e];
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) scaled.v[e] = sigma_scaled(f.c_in, x.v[e]);
        store_model_input<T, QUAD>(p, i0, scaled.v);
    }
}

template <typename T>
void launch_sigma(const KeepSigmaParams& m, int64_t per_row, bool keep, hipStream_t s) {
    const SampleParams& p = m.s;
    const dim3 grid(posterior_blocks(p.n_total));
    const bool own = quad_aligned<float>(m.xs) && quad_aligned<float>(m.hist);
    if (keep) {
        if (keep_quad<T>(p, m.k) && own)
            hipLaunchKernelGGL((sample_sigma_kernel<T, true, KeepSigmaParams>), grid, dim3(256), 0, s, m);
        else
            hipLaunchKernelGGL((sample_sigma_kernel<T, false, KeepSigmaParams>), grid, dim3(256), 0, s, m);
    } else {
        const SigmaParams& plain = m;  // (the instantiation without the blend: the keep block is sliced off)
        const bool quad = (per_row % 4) == 0 && quad_aligned<float>(p.x) && quad_aligned<T>(p.out) && quad_aligned<T>(p.in) &&
                          quad_aligned<float>(p.z_out) && own;
        if (quad)
            hipLaunchKernelGGL((sample_sigma_kernel<T, true, SigmaParams>), grid, dim3(256), 0, s, plain);
        else
            hipLaunchKernelGGL((sample_sigma_kernel<T, false, SigmaParams>), grid, dim3(256), 0, s, plain);
    }
}

template <typename T>
void launch_sigma_init(const SampleParams& p, const SigmaInitParams& f, int64_t per_row, hipStream_t s) {
    const bool quad = (per_row % 4) == 0 && quad_aligned<float>(p.x) && quad_aligned<T>(p.in) && quad_aligned<float>(f.init) &&
                      quad_aligned<float>(f.eps_out);
    const dim3 grid(posterior_blocks(p.n_total));
    if (quad)
        hipLaunchKernelGGL((sample_sigma_init_kernel<T, true>), grid, dim3(256), 0, s, p, f);
    else
        hipLaunchKernelGGL((sample_sigma_init_kernel<T, false>), grid, dim3(256), 0, s, p, f);
}

}  // namespace

extern "C" int ddpm_sample_sigma_init(float* x, void* model_in, float* t_model, int* cursor, const float* timesteps,
                                      const float* init, float* eps_out, int B, int64_t per_row, int I, int start, float k,
                                      float nn, float c_in, int cfg, int shared, uint64_t seed, int dtype, void* stream) {
    if (!x || !model_in || !t_model || !cursor || !timesteps || B < 1 || per_row < 1 || I < 1 || start < 0 || start >= I ||
        !known_dtype(dtype))
        return LORA_E_BADARG;
    SampleParams p{};
    p.x = x; p.in = model_in; p.cursor = cursor;
    p.n_total = (int64_t)B * per_row; p.rows = cfg ? 2 * B : B; p.S = I; p.cfg = cfg ? 1 : 0; p.seed = (uint32_t)seed;
    p.shared_row = shared ? per_row : 0;
    SigmaInitParams f{};
    f.init = init; f.eps_out = eps_out; f.t_model = t_model; f.timesteps = timesteps; f.start = start;
    f.k = k; f.nn = nn; f.c_in = c_in;
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (dtype) {
        case LORA_F32: launch_sigma_init<float>(p, f, per_row, s); break;
        case LORA_F16: launch_sigma_init<half_t>(p, f, per_row, s); break;
        default: launch_sigma_init<bf16_t>(p, f, per_row, s); break;
    }
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}

extern "C" int ddpm_sample_sigma(float* x, float* xs, float* hist, const void* model_out, void* model_in, float* t_model,
                                 const int* cursor, const float* timesteps, const float* coef, const int* plan, float* z_out,
                                 const float* mask, const float* init, const float* keep_coef, int B, int64_t per_row, int64_t hw,
                                 int I, int cfg, int shared, float guidance_scale, int dtype, void* stream) {
    if (!x || !xs || !hist || !model_out || !model_in || !t_model || !cursor || !timesteps || !coef || !plan || B < 1 ||
        per_row < 1 || I < 1 || !known_dtype(dtype))
        return LORA_E_BADARG;
    const bool keep = mask != nullptr;
    if (keep && !keep_args_ok(mask, init, keep_coef, per_row, hw)) return LORA_E_BADARG;
    KeepSigmaParams m{};
    SampleParams& p = m.s;
    p.x = x; p.out = model_out; p.in = model_in; p.cursor = const_cast<int*>(cursor); p.coef = coef; p.z_out = z_out;
    p.n_total = (int64_t)B * per_row; p.rows = cfg ? 2 * B : B; p.S = I; p.cfg = cfg ? 1 : 0;
    p.guidance = guidance_scale;
    p.shared_row = shared ? per_row : 0;
    m.xs = xs; m.hist = hist; m.plan = plan; m.t_model = t_model; m.timesteps = timesteps;
    if (keep) m.k = KeepParams{mask, init, keep_coef, per_row, hw};
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (dtype) {
        case LORA_F32: launch_sigma<float>(m, per_row, keep, s); break;
        case LORA_F16: launch_sigma<half_t>(m, per_row, keep, s); break;
        default: launch_sigma<bf16_t>(m, per_row, keep, s); break;
    }
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}

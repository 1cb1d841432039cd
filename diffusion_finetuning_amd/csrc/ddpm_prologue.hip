// The training step's prologues that draw their own randomness: timesteps and noise, the latents from the VAE's moments, and
// offset noise (the add_noise entry on noise the caller drew: ddpm_loss.hip).
//   prologue  : training_scripts/train_lora_dreambooth.py:824-853 (DDPM add_noise / get_velocity)
//   posterior : training_scripts/train_lora_dreambooth.py:818-821, lora_diffusion/cli_lora_pti.py:180-184
#include "ddpm_common.h"

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
    return by_dtype(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        hipLaunchKernelGGL(noise_prologue_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, s, x0, sqrt_acp, sqrt_1macp,
                           static_cast<T*>(noisy), static_cast<T*>(target), eps_out, t_out, B, per_row, n_timesteps, sd, st,
                           v_prediction);
    });
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

// torch.clamp's semantics (a NaN stays a NaN), then diffusers' std = exp(0.5·logvar)
__device__ __forceinline__ float posterior_x0(float mean, float logvar, float z, float scale) {
    const float lv = logvar < -30.f ? -30.f : (logvar > 20.f ? 20.f : logvar);
    return fmaf(expf(0.5f * lv), z, mean) * scale;
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

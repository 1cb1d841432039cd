// The latent sampler's launches around the UNet forward: the per-step kernels (DDPM / DDIM, linear multistep, sigma space), their
// keep-mask forms, the one start kernel and the cursor advance — every ddpm_sample_* entry of include/lora_hip.h.  Device code
// first, section by section; the host side (parameter blocks, instantiation choice, entries) at the end.
#include <type_traits>

#include "ddpm_common.h"

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
// streams of their own next to eps (0), the timesteps (1) and the posterior z (2) of ddpm_prologue.hip; Box–Muller as there.
// The draw depends on (seed, i, B·per_row) alone: not on the dtype, the access path or guidance.
// QUAD as in posterior_prologue_kernel (ddpm_prologue.hip): per_row % 4 == 0 and every pointer aligned to its 4-element access.
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

}  // namespace

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

// The start of a run, one kernel for every entry: the state
//     x = init ? k·init + nn·ε : nn·ε,    ε the x_T draw (stream 3, key (seed, 0)),
// the first model input cast(fp32(c_in·x)), t_model = timesteps[start] and cursor = {start, seed}.  TT is the type of the timestep
// table it reads and of the timestep tensor it writes: float on the fractional sigma grid, int64_t everywhere else.
//   ddpm_sample_sigma_init : as written — x_T = σ₀·ε or the noised image, c_in(σ) of the first evaluation;
//   ddpm_sample_init       : init = nullptr, start = 0, nn = 1, c_in = 1 — x_T = ε;
//   ddpm_sample_init_from  : c_in = 1, (k, nn) = (√ᾱ, √(1−ᾱ)) at timesteps[start] — image-to-image ("Making Img2Img Inference
//       with LoRA", README.md:287-289 and scripts/run_img2img.ipynb of the reference: `pipe(image=init_image, strength=0.75)`): a
//       run that starts part-way down the grid is the same recorded iteration with another cursor.
// The unit factors change no bit: sigma_scaled is a strict IEEE fp32 multiply, 1.0f·v == v for every finite v, −0 included, and
// the Box–Muller normals are finite and never denormal (a denormal k·init + n·ε survives too: the library is built with fp32
// denormals kept, hipcc's default for gfx950).  So the state, eps_out, the model input, t_model and the cursor of the two
// integer-grid entries are the bits their own kernels (a plain store of ε; k·init + n·ε) wrote.
template <typename TT>
struct StartParams {
    const float* init;  // nullable: text-to-image, x = nn·ε
    float* eps_out;     // nullable
    TT* t_model;           // [rows]
    const TT* timesteps;   // [S]
    int start;
    float k, nn, c_in;
};

template <typename T, bool QUAD, typename TT>
__global__ __launch_bounds__(256) void sample_sigma_init_kernel(SampleParams p, StartParams<TT> f) {
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nthreads = (int64_t)gridDim.x * 256;
    const TT t0 = f.timesteps[f.start];
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

// ---------------------------------------------------------------------------------------------------------
// Host side.  Every entry fills its parameter block with sample_params, picks the element type with by_dtype and the access path
// with by_quad; the twins with and without `_shared` are one-line wrappers over an implementation with a `shared` flag, and the
// entries with and without a keep mask share one launcher each.

// What every entry fills alike.  t_model / timesteps are the integer grid's: null where the entry's own block carries them.
SampleParams sample_params(float* x, const void* out, void* in, int64_t* t_model, const int* cursor, const int64_t* timesteps,
                           const float* coef, float* z_out, int B, int64_t per_row, int S, int cfg, float guidance, uint64_t seed,
                           bool shared) {
    SampleParams p{};
    p.x = x; p.out = out; p.in = in; p.t_model = t_model; p.cursor = const_cast<int*>(cursor);
    p.timesteps = timesteps; p.coef = coef; p.z_out = z_out;
    p.n_total = (int64_t)B * per_row; p.rows = cfg ? 2 * B : B; p.S = S; p.cfg = cfg ? 1 : 0;
    p.guidance = guidance; p.seed = (uint32_t)seed;
    p.shared_row = shared ? per_row : 0;
    return p;
}

bool keep_args_ok(const float* mask, const float* init, const float* keep_coef, int64_t per_row, int64_t hw) {
    return mask && init && keep_coef && per_row >= 1 && hw >= 1 && per_row % hw == 0;
}

// QUAD for the pointers every block has (a null one has nothing to access); what a block adds is AND-ed on:
template <typename T>
bool sample_quad(const SampleParams& p, int64_t per_row) {
    return (per_row % 4) == 0 && quad_aligned<float>(p.x) && quad_aligned<T>(p.out) && quad_aligned<T>(p.in) &&
           quad_aligned<float>(p.z_out);
}
// the keep mask (hw % 4 == 0: a group of four then lies inside one channel, its mask values four consecutive, aligned floats)
bool keep_quad(const KeepParams& k) { return (k.hw % 4) == 0 && quad_aligned<float>(k.init) && quad_aligned<float>(k.mask); }
// and the saved state and the history (n_total % 4 == 0: every slot of the ring is aligned as hist is).
bool history_quad(const float* xs, const float* hist) { return quad_aligned<float>(xs) && quad_aligned<float>(hist); }

// Calls f with std::true_type for the 4-element instantiation, std::false_type for the element-wise one.
template <typename F>
void by_quad(bool quad, F&& f) {
    if (quad)
        f(std::true_type{});
    else
        f(std::false_type{});
}

// The three step launchers: with `keep` the instantiation that blends, on the whole block; without, the plain one, on the block
// with the keep part sliced off.
template <typename T>
void launch_step(const KeepSampleParams& p, int64_t per_row, bool keep, hipStream_t s) {
    const dim3 grid(posterior_blocks(p.n_total));
    by_quad(sample_quad<T>(p, per_row) && (!keep || keep_quad(p.k)), [&](auto quad) {
        constexpr bool Q = decltype(quad)::value;
        const SampleParams& plain = p;
        if (keep)
            hipLaunchKernelGGL((sample_step_kernel<T, Q, KeepSampleParams>), grid, dim3(256), 0, s, p);
        else
            hipLaunchKernelGGL((sample_step_kernel<T, Q, SampleParams>), grid, dim3(256), 0, s, plain);
    });
}

template <typename T>
void launch_multistep(const KeepMultistepParams& m, int64_t per_row, bool keep, hipStream_t s) {
    const dim3 grid(posterior_blocks(m.s.n_total));
    by_quad(sample_quad<T>(m.s, per_row) && history_quad(m.xs, m.hist) && (!keep || keep_quad(m.k)), [&](auto quad) {
        constexpr bool Q = decltype(quad)::value;
        const MultistepParams& plain = m;
        if (keep)
            hipLaunchKernelGGL((sample_multistep_kernel<T, Q, KeepMultistepParams>), grid, dim3(256), 0, s, m);
        else
            hipLaunchKernelGGL((sample_multistep_kernel<T, Q, MultistepParams>), grid, dim3(256), 0, s, plain);
    });
}

template <typename T>
void launch_sigma(const KeepSigmaParams& m, int64_t per_row, bool keep, hipStream_t s) {
    const dim3 grid(posterior_blocks(m.s.n_total));
    by_quad(sample_quad<T>(m.s, per_row) && history_quad(m.xs, m.hist) && (!keep || keep_quad(m.k)), [&](auto quad) {
        constexpr bool Q = decltype(quad)::value;
        const SigmaParams& plain = m;
        if (keep)
            hipLaunchKernelGGL((sample_sigma_kernel<T, Q, KeepSigmaParams>), grid, dim3(256), 0, s, m);
        else
            hipLaunchKernelGGL((sample_sigma_kernel<T, Q, SigmaParams>), grid, dim3(256), 0, s, plain);
    });
}

template <typename TT>
int sample_start(float* x, void* model_in, TT* t_model, int* cursor, const TT* timesteps, const float* init, float* eps_out, int B,
                 int64_t per_row, int S, int start, float k, float nn, float c_in, int cfg, uint64_t seed, int dtype, void* stream,
                 bool shared) {
    if (!x || !model_in || !t_model || !cursor || !timesteps || B < 1 || per_row < 1 || S < 1 || start < 0 || start >= S)
        return LORA_E_BADARG;
    const SampleParams p =
        sample_params(x, nullptr, model_in, nullptr, cursor, nullptr, nullptr, nullptr, B, per_row, S, cfg, 0.f, seed, shared);
    const StartParams<TT> f{init, eps_out, t_model, timesteps, start, k, nn, c_in};
    const dim3 grid(posterior_blocks(p.n_total));
    hipStream_t s = static_cast<hipStream_t>(stream);
    return by_dtype(dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        by_quad(sample_quad<T>(p, per_row) && quad_aligned<float>(init) && quad_aligned<float>(eps_out), [&](auto quad) {
            hipLaunchKernelGGL((sample_sigma_init_kernel<T, decltype(quad)::value, TT>), grid, dim3(256), 0, s, p, f);
        });
    });
}

int sample_step(float* x, const void* model_out, void* model_in, int64_t* t_model, const int* cursor, const int64_t* timesteps,
                const float* coef, float* z_out, const float* mask, const float* init, const float* keep_coef, int B,
                int64_t per_row, int64_t hw, int S, int cfg, float guidance_scale, int dtype, void* stream, bool keep,
                bool shared) {
    if (!x || !model_out || !model_in || !t_model || !cursor || !timesteps || !coef || B < 1 || per_row < 1 || S < 1 ||
        (keep && !keep_args_ok(mask, init, keep_coef, per_row, hw)))
        return LORA_E_BADARG;
    const KeepSampleParams p{sample_params(x, model_out, model_in, t_model, cursor, timesteps, coef, z_out, B, per_row, S, cfg,
                                           guidance_scale, 0, shared),
                             KeepParams{mask, init, keep_coef, per_row, hw}};
    hipStream_t s = static_cast<hipStream_t>(stream);
    return by_dtype(dtype, [&](auto tag) { launch_step<typename decltype(tag)::type>(p, per_row, keep, s); });
}

int sample_multistep(float* x, float* xs, float* hist, const void* model_out, void* model_in, int64_t* t_model, const int* cursor,
                     const int64_t* timesteps, const float* coef, const int* plan, const float* mask, const float* init,
                     const float* keep_coef, int B, int64_t per_row, int64_t hw, int I, int cfg, float guidance_scale, int dtype,
                     void* stream, bool keep, bool shared) {
    if (!x || !xs || !hist || !model_out || !model_in || !t_model || !cursor || !timesteps || !coef || !plan || B < 1 ||
        per_row < 1 || I < 1 || (keep && !keep_args_ok(mask, init, keep_coef, per_row, hw)))
        return LORA_E_BADARG;
    const KeepMultistepParams m{{sample_params(x, model_out, model_in, t_model, cursor, timesteps, coef, nullptr, B, per_row, I,
                                               cfg, guidance_scale, 0, shared),
                                 xs, hist, plan},
                                KeepParams{mask, init, keep_coef, per_row, hw}};
    hipStream_t s = static_cast<hipStream_t>(stream);
    return by_dtype(dtype, [&](auto tag) { launch_multistep<typename decltype(tag)::type>(m, per_row, keep, s); });
}

}  // namespace

extern "C" int ddpm_sample_init(float* x, void* model_in, int64_t* t_model, int* cursor, const int64_t* timesteps, int B,
                                int64_t per_row, int S, int cfg, uint64_t seed, int dtype, void* stream) {
    return sample_start<int64_t>(x, model_in, t_model, cursor, timesteps, nullptr, nullptr, B, per_row, S, 0, 0.f, 1.f, 1.f, cfg,
                                 seed, dtype, stream, false);
}
extern "C" int ddpm_sample_init_shared(float* x, void* model_in, int64_t* t_model, int* cursor, const int64_t* timesteps, int B,
                                       int64_t per_row, int S, int cfg, uint64_t seed, int dtype, void* stream) {
    return sample_start<int64_t>(x, model_in, t_model, cursor, timesteps, nullptr, nullptr, B, per_row, S, 0, 0.f, 1.f, 1.f, cfg,
                                 seed, dtype, stream, true);
}

extern "C" int ddpm_sample_init_from(float* x, void* model_in, int64_t* t_model, int* cursor, const int64_t* timesteps,
                                     const float* init, float* eps_out, int B, int64_t per_row, int S, int start, float k,
                                     float n, int cfg, uint64_t seed, int dtype, void* stream) {
    if (!init) return LORA_E_BADARG;
    return sample_start<int64_t>(x, model_in, t_model, cursor, timesteps, init, eps_out, B, per_row, S, start, k, n, 1.f, cfg,
                                 seed, dtype, stream, false);
}
extern "C" int ddpm_sample_init_from_shared(float* x, void* model_in, int64_t* t_model, int* cursor, const int64_t* timesteps,
                                            const float* init, float* eps_out, int B, int64_t per_row, int S, int start, float k,
                                            float n, int cfg, uint64_t seed, int dtype, void* stream) {
    if (!init) return LORA_E_BADARG;
    return sample_start<int64_t>(x, model_in, t_model, cursor, timesteps, init, eps_out, B, per_row, S, start, k, n, 1.f, cfg,
                                 seed, dtype, stream, true);
}

extern "C" int ddpm_sample_sigma_init(float* x, void* model_in, float* t_model, int* cursor, const float* timesteps,
                                      const float* init, float* eps_out, int B, int64_t per_row, int I, int start, float k,
                                      float nn, float c_in, int cfg, int shared, uint64_t seed, int dtype, void* stream) {
    return sample_start<float>(x, model_in, t_model, cursor, timesteps, init, eps_out, B, per_row, I, start, k, nn, c_in, cfg,
                               seed, dtype, stream, shared != 0);
}

extern "C" int ddpm_sample_step(float* x, const void* model_out, void* model_in, int64_t* t_model, const int* cursor,
                                const int64_t* timesteps, const float* coef, float* z_out, int B, int64_t per_row, int S,
                                int cfg, float guidance_scale, int dtype, void* stream) {
    return sample_step(x, model_out, model_in, t_model, cursor, timesteps, coef, z_out, nullptr, nullptr, nullptr, B, per_row, 0,
                       S, cfg, guidance_scale, dtype, stream, false, false);
}
extern "C" int ddpm_sample_step_shared(float* x, const void* model_out, void* model_in, int64_t* t_model, const int* cursor,
                                       const int64_t* timesteps, const float* coef, float* z_out, int B, int64_t per_row, int S,
                                       int cfg, float guidance_scale, int dtype, void* stream) {
    return sample_step(x, model_out, model_in, t_model, cursor, timesteps, coef, z_out, nullptr, nullptr, nullptr, B, per_row, 0,
                       S, cfg, guidance_scale, dtype, stream, false, true);
}
extern "C" int ddpm_sample_step_keep(float* x, const void* model_out, void* model_in, int64_t* t_model, const int* cursor,
                                     const int64_t* timesteps, const float* coef, float* z_out, const float* mask,
                                     const float* init, const float* keep_coef, int B, int64_t per_row, int64_t hw, int S, int cfg,
                                     float guidance_scale, int dtype, void* stream) {
    return sample_step(x, model_out, model_in, t_model, cursor, timesteps, coef, z_out, mask, init, keep_coef, B, per_row, hw, S,
                       cfg, guidance_scale, dtype, stream, true, false);
}
extern "C" int ddpm_sample_step_keep_shared(float* x, const void* model_out, void* model_in, int64_t* t_model, const int* cursor,
                                            const int64_t* timesteps, const float* coef, float* z_out, const float* mask,
                                            const float* init, const float* keep_coef, int B, int64_t per_row, int64_t hw, int S,
                                            int cfg, float guidance_scale, int dtype, void* stream) {
    return sample_step(x, model_out, model_in, t_model, cursor, timesteps, coef, z_out, mask, init, keep_coef, B, per_row, hw, S,
                       cfg, guidance_scale, dtype, stream, true, true);
}

extern "C" int ddpm_sample_advance(int* cursor, int S, void* stream) {
    if (!cursor || S < 1) return LORA_E_BADARG;
    hipLaunchKernelGGL(sample_advance_kernel, dim3(1), dim3(1), 0, static_cast<hipStream_t>(stream), cursor, S);
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}

extern "C" int ddpm_sample_multistep(float* x, float* xs, float* hist, const void* model_out, void* model_in, int64_t* t_model,
                                     const int* cursor, const int64_t* timesteps, const float* coef, const int* plan, int B,
                                     int64_t per_row, int I, int cfg, float guidance_scale, int dtype, void* stream) {
    return sample_multistep(x, xs, hist, model_out, model_in, t_model, cursor, timesteps, coef, plan, nullptr, nullptr, nullptr, B,
                            per_row, 0, I, cfg, guidance_scale, dtype, stream, false, false);
}
extern "C" int ddpm_sample_multistep_keep(float* x, float* xs, float* hist, const void* model_out, void* model_in,
                                          int64_t* t_model, const int* cursor, const int64_t* timesteps, const float* coef,
                                          const int* plan, const float* mask, const float* init, const float* keep_coef, int B,
                                          int64_t per_row, int64_t hw, int I, int cfg, float guidance_scale, int dtype,
                                          void* stream) {
    return sample_multistep(x, xs, hist, model_out, model_in, t_model, cursor, timesteps, coef, plan, mask, init, keep_coef, B,
                            per_row, hw, I, cfg, guidance_scale, dtype, stream, true, false);
}
extern "C" int ddpm_sample_multistep_keep_shared(float* x, float* xs, float* hist, const void* model_out, void* model_in,
                                                 int64_t* t_model, const int* cursor, const int64_t* timesteps, const float* coef,
                                                 const int* plan, const float* mask, const float* init, const float* keep_coef,
                                                 int B, int64_t per_row, int64_t hw, int I, int cfg, float guidance_scale,
                                                 int dtype, void* stream) {
    return sample_multistep(x, xs, hist, model_out, model_in, t_model, cursor, timesteps, coef, plan, mask, init, keep_coef, B,
                            per_row, hw, I, cfg, guidance_scale, dtype, stream, true, true);
}

extern "C" int ddpm_sample_sigma(float* x, float* xs, float* hist, const void* model_out, void* model_in, float* t_model,
                                 const int* cursor, const float* timesteps, const float* coef, const int* plan, float* z_out,
                                 const float* mask, const float* init, const float* keep_coef, int B, int64_t per_row, int64_t hw,
                                 int I, int cfg, int shared, float guidance_scale, int dtype, void* stream) {
    const bool keep = mask != nullptr;
    if (!x || !xs || !hist || !model_out || !model_in || !t_model || !cursor || !timesteps || !coef || !plan || B < 1 ||
        per_row < 1 || I < 1 || (keep && !keep_args_ok(mask, init, keep_coef, per_row, hw)))
        return LORA_E_BADARG;
    const KeepSigmaParams m{{sample_params(x, model_out, model_in, nullptr, cursor, nullptr, coef, z_out, B, per_row, I, cfg,
                                           guidance_scale, 0, shared != 0),
                             xs, hist, plan, t_model, timesteps},
                            KeepParams{mask, init, keep_coef, per_row, hw}};
    hipStream_t s = static_cast<hipStream_t>(stream);
    return by_dtype(dtype, [&](auto tag) { launch_sigma<typename decltype(tag)::type>(m, per_row, keep, s); });
}

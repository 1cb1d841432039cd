// Prodigy (K. Mishchenko, A. Defazio, "Prodigy: An Expeditiously Adaptive Parameter-Free Learner", arXiv:2306.06101) over the flat
// LoRA slab: AdamW whose step size is d·lr, d an on-line estimate of the distance to the solution.  Restated from the published
// definition ("Prodigy"); no line of the reference, which has no such optimizer.
// Two streaming launches behind lora_grad_sqnorm, all state in device memory (no host sync, valid under a replayed graph):
//   lora_prodigy_moments : m, v, s per element, the two global sums Σ num_i and Σ |s_i| reduced in the launch, and — in the block
//                          that arrives last — the scalar step d → d_new in double
//   lora_prodigy_apply   : the parameter update, which needs d_new in its eps term, [+ the EMA of the parameters]
// The scalar block (fp32 [8], device):  [0] d  [1] d_max  [2] numerator  [3] d_prev  [4] d_hat  [5] denom  [6] [7] unused (0).
#include "common.h"

namespace {

constexpr int kMaxBlocks = 1024;
constexpr int kMaxRanges = 4;

// contiguous ranges of the slab, each with its own learning rate and weight decay (UNet factors | text-encoder factors)
struct ProdigyRanges {
    int64_t end[kMaxRanges];  // exclusive ends, increasing; the unused ones hold n
    float lr[kMaxRanges];     // γ_j = lr_j·λ(step)
    float wd[kMaxRanges];
};

__device__ __forceinline__ int range_of(int64_t i, const int64_t (&e)[kMaxRanges]) {
    return (i >= e[0] ? 1 : 0) + (i >= e[1] ? 1 : 0) + (i >= e[2] ? 1 : 0);
}
__device__ __forceinline__ float sel(int j, const float (&c)[kMaxRanges]) {
    return j == 0 ? c[0] : j == 1 ? c[1] : j == 2 ? c[2] : c[3];
}

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
__device__ __forceinline__ double block_sum_256d(double v, double* s_wave) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) s_wave[w] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0) t = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
    __syncthreads();
    return t;
}

// sqrt(1 − β2^t)/(1 − β1^t) in double from the device's count of applied steps, as the AdamW bias terms; 1 without the option
__device__ __forceinline__ double bias_correction(const float* norm_in, float beta1, float beta2, int on) {
    if (!on) return 1.0;
    const double t = (double)norm_in[2];
    return sqrt(1.0 - pow((double)beta2, t)) / (1.0 - pow((double)beta1, t));
}

// Phase A on one element.  The coefficients are doubles rounded once to fp32 (c_num = (d/d0)·dlr, c_m = d·(1 − β1),
// c_v = d²·(1 − β2), c_s = (d/d0)·(d or dlr)); num and den are the thread's running sums.
__device__ __forceinline__ void prodigy_moments_element(float p, float p0, float g, float& m, float& v, float& s, float c_num,
                                                        float c_m, float c_v, float c_s, float beta1, float beta2, float beta3,
                                                        float& num, float& den) {
    num += (c_num * g) * (p0 - p);
    m = beta1 * m + c_m * g;
    v = beta2 * v + (c_v * g) * g;
    s = beta3 * s + c_s * g;
    den += fabsf(s);
}

struct MomentsParams {
    const float* p;
    const float* p0;
    const float* g;
    float* m;
    float* v;
    float* s;
    int64_t n;
    const float* norm_in;
    float* scalars;
    float* partials;  // [2][kMaxBlocks]: Σ num, Σ |s| per block
    unsigned* ticket;
    ProdigyRanges r;
    float grad_mul, max_norm, beta1, beta2, beta3, d0, d_coef, growth_rate;
    int bias_correction, safeguard;
};

__global__ __launch_bounds__(256) void prodigy_moments_kernel(MomentsParams a) {
    if (a.norm_in[1] != 0.f) return;  // overflow: skip the step (GradScaler semantics), every block alike
    __shared__ float s_wave[4];
    __shared__ double s_dwave[4];
    __shared__ bool s_last;
    float clip = 1.f;
    if (a.max_norm > 0.f) {
        const float c = a.max_norm / (sqrtf(a.norm_in[0]) + 1e-6f);
        clip = c < 1.f ? c : 1.f;
    }
    const float gm = a.grad_mul * clip;
    const double d = (double)a.scalars[0];
    const double bc = bias_correction(a.norm_in, a.beta1, a.beta2, a.bias_correction);
    const double ratio = d / (double)a.d0;
    const float c_m = (float)(d * (1.0 - (double)a.beta1));
    const float c_v = (float)(d * d * (1.0 - (double)a.beta2));
    int64_t e[kMaxRanges];
    float c_num[kMaxRanges], c_s[kMaxRanges];
#pragma unroll
    for (int j = 0; j < kMaxRanges; ++j) {
        const double dlr = d * (double)a.r.lr[j] * bc;
        e[j] = a.r.end[j];
        c_num[j] = (float)(ratio * dlr);
        c_s[j] = (float)(ratio * (a.safeguard ? d : dlr));
    }
    float num = 0.f, den = 0.f;
    const int64_t nvec = a.n >> 2;
    const float4* p4 = reinterpret_cast<const float4*>(a.p);
    const float4* q4 = reinterpret_cast<const float4*>(a.p0);
    const float4* g4 = reinterpret_cast<const float4*>(a.g);
    float4* m4 = reinterpret_cast<float4*>(a.m);
    float4* v4 = reinterpret_cast<float4*>(a.v);
    float4* s4 = reinterpret_cast<float4*>(a.s);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256) {
        const float4 P = p4[i], Q = q4[i], G = g4[i];
        float4 M = m4[i], V = v4[i], S = s4[i];
        const int64_t b = i << 2;
        const int j0 = range_of(b, e), j1 = range_of(b + 1, e), j2 = range_of(b + 2, e), j3 = range_of(b + 3, e);
        prodigy_moments_element(P.x, Q.x, G.x * gm, M.x, V.x, S.x, sel(j0, c_num), c_m, c_v, sel(j0, c_s), a.beta1, a.beta2, a.beta3, num, den);
        prodigy_moments_element(P.y, Q.y, G.y * gm, M.y, V.y, S.y, sel(j1, c_num), c_m, c_v, sel(j1, c_s), a.beta1, a.beta2, a.beta3, num, den);
        prodigy_moments_element(P.z, Q.z, G.z * gm, M.z, V.z, S.z, sel(j2, c_num), c_m, c_v, sel(j2, c_s), a.beta1, a.beta2, a.beta3, num, den);
        prodigy_moments_element(P.w, Q.w, G.w * gm, M.w, V.w, S.w, sel(j3, c_num), c_m, c_v, sel(j3, c_s), a.beta1, a.beta2, a.beta3, num, den);
        m4[i] = M;
        v4[i] = V;
        s4[i] = S;
    }
    if (blockIdx.x == 0) {
        for (int64_t i = (nvec << 2) + threadIdx.x; i < a.n; i += 256) {
            const int j = range_of(i, e);
            float m = a.m[i], v = a.v[i], s = a.s[i];
            prodigy_moments_element(a.p[i], a.p0[i], a.g[i] * gm, m, v, s, sel(j, c_num), c_m, c_v, sel(j, c_s), a.beta1, a.beta2, a.beta3, num, den);
            a.m[i] = m;
            a.v[i] = v;
            a.s[i] = s;
        }
    }
    const float bnum = block_sum_256(num, s_wave);
    const float bden = block_sum_256(den, s_wave);
    if (threadIdx.x == 0) {
        // the hand-off of grad_sqnorm_kernel: plain stores, drained, released at agent scope, drained again, then the ticket
        a.partials[blockIdx.x] = bnum;
        a.partials[kMaxBlocks + blockIdx.x] = bden;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned t = __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool last = (t == gridDim.x - 1);
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        s_last = last;
    }
    __syncthreads();
    if (s_last) {
        // fixed order, in double: thread k adds the partials k, k + 256, …; the 256 sums go through one butterfly.  No atomics
        // on data: the same bits on every run.
        double tn = 0.0, td = 0.0;
        for (int i = threadIdx.x; i < (int)gridDim.x; i += 256) {
            tn += (double)a.partials[i];
            td += (double)a.partials[kMaxBlocks + i];
        }
        tn = block_sum_256d(tn, s_dwave);
        td = block_sum_256d(td, s_dwave);
        if (threadIdx.x == 0) {
            const float d_f = a.scalars[0];
            double d_max = (double)a.scalars[1];
            double d_new = d;
            bool any_lr = false;
#pragma unroll
            for (int j = 0; j < kMaxRanges; ++j) any_lr = any_lr || a.r.lr[j] > 0.f;
            a.scalars[3] = d_f;  // d_prev: what lora_prodigy_apply forms dlr from
            a.scalars[5] = (float)td;
            a.scalars[4] = 0.f;  // d_hat of THIS step: 0 where the step forms none (denom == 0, every γ == 0)
            if (td > 0.0) {  // denom == 0: numerator, d and d_max keep their values
                const double numerator = (double)a.beta3 * (double)a.scalars[2] + tn;
                a.scalars[2] = (float)numerator;
                if (any_lr) {
                    const double d_hat = (double)a.d_coef * numerator / td;
                    if (d_f == a.d0) d_new = d_hat > d ? d_hat : d;  // the first growth is not rate-limited
                    if (d_hat > d_max) d_max = d_hat;
                    const double grown = d_new * (double)a.growth_rate;
                    d_new = d_max < grown ? d_max : grown;
                    a.scalars[1] = (float)d_max;
                    a.scalars[4] = (float)d_hat;
                    a.scalars[0] = (float)d_new;
                }
            }
        }
    }
}

// Phase B on one element: decoupled weight decay and the Adam term at the step size dlr, eps scaled by the NEW d.  Which of the
// two products joins the subtraction in an fma is spelled out (the decayed parameter is a rounded fp32 value, rounded_f32): left
// to the compiler, the plain and the EMA instantiation of the kernel below chose differently and p differed in its last bit.
__device__ __forceinline__ void prodigy_apply_element(float& p, float m, float v, float decay, float dlr, float eps_d) {
    const float q = m / (sqrtf(v) + eps_d);
    p = fmaf(-dlr, q, rounded_f32(p * decay));
}

struct ApplyParams {
    float* p;
    const float* m;
    const float* v;
    int64_t n;
    const float* norm_in;
    const float* scalars;
    ProdigyRanges r;
    float beta1, beta2, eps;
    int bias_correction;
};

// kEma: the EMA of the parameters in `shadow`, on the p just computed, with adamw_ema_kernel's decay (common.h: ema_element).
// The plain form is its own instantiation: the option adds nothing to it.
template <bool kEma>
__global__ __launch_bounds__(256) void prodigy_apply_kernel(ApplyParams a, float* shadow, float ema_max_decay, int ema_update_after) {
    if (a.norm_in[1] != 0.f) return;  // overflow: nothing is written, the shadow included
    const double d_prev = (double)a.scalars[3];
    const float eps_d = a.scalars[0] * a.eps;
    const double bc = bias_correction(a.norm_in, a.beta1, a.beta2, a.bias_correction);
    int64_t e[kMaxRanges];
    float dlr[kMaxRanges], decay[kMaxRanges];
#pragma unroll
    for (int j = 0; j < kMaxRanges; ++j) {
        e[j] = a.r.end[j];
        dlr[j] = (float)(d_prev * (double)a.r.lr[j] * bc);
        decay[j] = fmaf(-a.r.wd[j], dlr[j], 1.f);
    }
    float omd = 0.f;
    if constexpr (kEma) {
        const double n_ema = (double)a.norm_in[2] - (double)ema_update_after - 1.0;
        double dec = 0.0;
        if (n_ema > 0.0) {
            dec = (1.0 + n_ema) / (10.0 + n_ema);
            if (dec > (double)ema_max_decay) dec = (double)ema_max_decay;
        }
        omd = (float)(1.0 - dec);
    }
    const int64_t nvec = a.n >> 2;
    float4* p4 = reinterpret_cast<float4*>(a.p);
    const float4* m4 = reinterpret_cast<const float4*>(a.m);
    const float4* v4 = reinterpret_cast<const float4*>(a.v);
    float4* h4 = reinterpret_cast<float4*>(shadow);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256) {
        float4 P = p4[i];
        const float4 M = m4[i], V = v4[i];
        const int64_t b = i << 2;
        const int j0 = range_of(b, e), j1 = range_of(b + 1, e), j2 = range_of(b + 2, e), j3 = range_of(b + 3, e);
        prodigy_apply_element(P.x, M.x, V.x, sel(j0, decay), sel(j0, dlr), eps_d);
        prodigy_apply_element(P.y, M.y, V.y, sel(j1, decay), sel(j1, dlr), eps_d);
        prodigy_apply_element(P.z, M.z, V.z, sel(j2, decay), sel(j2, dlr), eps_d);
        prodigy_apply_element(P.w, M.w, V.w, sel(j3, decay), sel(j3, dlr), eps_d);
        p4[i] = P;
        if constexpr (kEma) {
            float4 H = h4[i];
            ema_element(H.x, P.x, omd);
            ema_element(H.y, P.y, omd);
            ema_element(H.z, P.z, omd);
            ema_element(H.w, P.w, omd);
            h4[i] = H;
        }
    }
    if (blockIdx.x == 0) {
        for (int64_t i = (nvec << 2) + threadIdx.x; i < a.n; i += 256) {
            const int j = range_of(i, e);
            float p = a.p[i];
            prodigy_apply_element(p, a.m[i], a.v[i], sel(j, decay), sel(j, dlr), eps_d);
            a.p[i] = p;
            if constexpr (kEma) {
                float h = shadow[i];
                ema_element(h, p, omd);
                shadow[i] = h;
            }
        }
    }
}

// The ranges of a call into the by-value block of a launch; false for a count outside 1..4, ends that do not increase from above 0
// to exactly n, or a learning rate / weight decay that is negative or not a number.
bool fill_ranges(ProdigyRanges& r, const int64_t* range_end, const float* lr, const float* wd, int n_ranges, int64_t n) {
    if (n_ranges < 1 || n_ranges > kMaxRanges) return false;
    int64_t prev = 0;
    for (int j = 0; j < kMaxRanges; ++j) {
        const bool used = j < n_ranges;
        if (used) {
            if (range_end[j] <= prev) return false;
            if (!(lr[j] >= 0.f) || (wd && !(wd[j] >= 0.f))) return false;
            prev = range_end[j];
        }
        r.end[j] = used ? range_end[j] : n;
        r.lr[j] = used ? lr[j] : 0.f;
        r.wd[j] = used && wd ? wd[j] : 0.f;
    }
    return prev == n;
}

bool beta_ok(float b) { return b >= 0.f && b < 1.f; }

int64_t stream_blocks(int64_t n) {
    int64_t blocks = (n / 4 + 255) / 256;
    if (blocks > kMaxBlocks) blocks = kMaxBlocks;
    if (blocks < 1) blocks = 1;
    return blocks;
}

}  // namespace

extern "C" int64_t lora_prodigy_workspace_bytes(void) { return 16 + 2 * kMaxBlocks * 4; }

extern "C" int lora_prodigy_moments(const float* param, const float* param0, const float* grad, float* exp_avg, float* exp_avg_sq,
                                    float* s, int64_t n, const int64_t* range_end, const float* lr, int n_ranges,
                                    const float* norm_in, float* scalars, void* workspace, float grad_mul, float max_norm,
                                    float beta1, float beta2, float beta3, float d0, float d_coef, float growth_rate,
                                    int use_bias_correction, int safeguard_warmup, void* stream) {
    if (!param || !param0 || !grad || !exp_avg || !exp_avg_sq || !s || !range_end || !lr || !norm_in || !scalars || !workspace ||
        n < 1)
        return LORA_E_BADARG;
    MomentsParams a{};
    if (!fill_ranges(a.r, range_end, lr, nullptr, n_ranges, n)) return LORA_E_BADARG;
    if (!beta_ok(beta1) || !beta_ok(beta2) || !beta_ok(beta3)) return LORA_E_BADARG;
    if (!(d0 > 0.f) || !(d_coef > 0.f) || !(growth_rate >= 1.f)) return LORA_E_BADARG;
    if (!aligned16(param) || !aligned16(param0) || !aligned16(grad) || !aligned16(exp_avg) || !aligned16(exp_avg_sq) ||
        !aligned16(s) || !aligned16(workspace))
        return LORA_E_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!lora_zero_ticket(workspace, st)) return LORA_E_LAUNCH;
    char* ws = static_cast<char*>(workspace);
    a.p = param; a.p0 = param0; a.g = grad; a.m = exp_avg; a.v = exp_avg_sq; a.s = s; a.n = n;
    a.norm_in = norm_in; a.scalars = scalars; a.partials = reinterpret_cast<float*>(ws + 16);
    a.ticket = reinterpret_cast<unsigned*>(ws);
    a.grad_mul = grad_mul; a.max_norm = max_norm; a.beta1 = beta1; a.beta2 = beta2; a.beta3 = beta3;
    a.d0 = d0; a.d_coef = d_coef; a.growth_rate = growth_rate;
    a.bias_correction = use_bias_correction ? 1 : 0; a.safeguard = safeguard_warmup ? 1 : 0;
    hipLaunchKernelGGL(prodigy_moments_kernel, dim3((unsigned)stream_blocks(n)), dim3(256), 0, st, a);
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}

extern "C" int lora_prodigy_apply(float* param, const float* exp_avg, const float* exp_avg_sq, float* shadow, int64_t n,
                                  const int64_t* range_end, const float* lr, const float* weight_decay, int n_ranges,
                                  const float* norm_in, const float* scalars, float beta1, float beta2, float eps,
                                  int use_bias_correction, float ema_max_decay, int ema_update_after, void* stream) {
    if (!param || !exp_avg || !exp_avg_sq || !range_end || !lr || !weight_decay || !norm_in || !scalars || n < 1)
        return LORA_E_BADARG;
    ApplyParams a{};
    if (!fill_ranges(a.r, range_end, lr, weight_decay, n_ranges, n)) return LORA_E_BADARG;
    if (!beta_ok(beta1) || !beta_ok(beta2) || !(eps >= 0.f)) return LORA_E_BADARG;
    if (shadow && (!(ema_max_decay >= 0.f && ema_max_decay <= 1.f) || ema_update_after < 0)) return LORA_E_BADARG;
    if (!aligned16(param) || !aligned16(exp_avg) || !aligned16(exp_avg_sq) || !aligned16(shadow)) return LORA_E_ALIGN;
    a.p = param; a.m = exp_avg; a.v = exp_avg_sq; a.n = n; a.norm_in = norm_in; a.scalars = scalars;
    a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.bias_correction = use_bias_correction ? 1 : 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)stream_blocks(n));
    if (shadow)
        hipLaunchKernelGGL(prodigy_apply_kernel<true>, grid, dim3(256), 0, st, a, shadow, ema_max_decay, ema_update_after);
    else
        hipLaunchKernelGGL(prodigy_apply_kernel<false>, grid, dim3(256), 0, st, a, shadow, ema_max_decay, ema_update_after);
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}

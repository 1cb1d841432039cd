// GroupNorm of the UNet's convolution trunk with what surrounds it folded in: y = act(GroupNorm(x + a)), x [N,C,H,W],
// a an optional per-(n,c) addend (the time embedding and the preceding convolution's bias), act = SiLU or identity.
// Stock PyTorch runs moments → normalise → SiLU as three kernels forward and three more backward, about 13 passes over the
// activation; here it is a statistics pass and an apply pass each way (5 passes through HBM), and the backward recomputes
// the normalised value and SiLU' from x, so only x is kept alive.  Where an NCHW (n,group) slab is small enough (the planner
// nchw_one_limit, from measurement) the two passes are one launch: a workgroup keeps its slab in registers, reduces and writes.
//
// Two layouts, both with 16-byte accesses:
//   * NCHW, two launches: one wave per (n,c) row of H·W elements in the statistics kernels, so the partials are per channel;
//     the apply kernels work on a slice of one (n,group) slab per workgroup and fold that group's ≤ cpg channel partials first.
//   * NCHW, one launch: one workgroup of 1024 threads per (n,group) slab, 2, 5 or 8 chunks per thread; the workspace is unused.
//   * channels-last (NHWC): a thread owns 8 fixed consecutive channels (which may straddle groups: the group width need not be
//     a multiple of 8) over a block of rows; a workgroup reduces its rows × all channels through LDS to one partial per group,
//     S partials per (n,group) in all, and the apply kernels fold them.
// Every fold runs in a fixed order and there are no float atomics: two runs are bit-identical.  Statistics, the normalised
// value and the activation are fp32 up to the single rounding of the output.
//
// Statistics are sums of d and d² about a shift, merged in centred form, so a mean that is large against the deviation costs
// no digits:
//   * NCHW: the shift of a row is its first element and the row leaves (mean, M2 = Σd² − (Σd)²/HW); the group's cpg rows are
//     merged about the group mean.  An element far from the rest of its row costs up to about H·W·2⁻²⁴ of the group's
//     variance when it is the row's first one (2.4e-5 of rstd measured at H·W = 4096).
//   * NCHW, one launch: a true two-pass from the registers: the mean, then the sums of e = x + a − mean and e² (the first
//     corrects the mean by what its own rounding left).  No shift, so no element is special.
//   * NHWC: a thread's shift per channel is its OWN first row, over the n_t rows it reads of one row block (4 … 32 for the
//     planner's splits unless H·W exceeds 64·RP·32), and it leaves (n_t, mean_t, M2_t).  The workgroup's fold through LDS and
//     the fold of the S row blocks merge such triples in two passes: the weighted mean μ of the means, then
//     S1 = Σ n(mean_t − μ) and S2 = Σ M2_t + n(mean_t − μ)², giving (μ + S1/n, S2 − S1²/n) with S1 ≈ 0.  An element far from
//     the rest of its group, wherever it sits, costs at most about n_t·2⁻²³ of the variance.  (One shift per group, the
//     group's first element, lost up to 9.5e-2 of rstd at 262 144 elements: tests/test_gpu_norm_edges.py.)
// The mean is within a few fp32 roundings of the exact one at its own magnitude.
#include "common.h"

namespace {

constexpr int kNhwcThreads = 512;   // NHWC kernels: rows-per-pass RP = 512 / (C/8) row lanes × C/8 channel columns
constexpr int kNhwcLds = 4096;      // RP·C ≤ 4096 floats per reduction array
constexpr int kMaxGroups = 256;
constexpr int kMaxSplit = 64;       // S: statistics partials per (n,group) in NHWC

template <typename T> __device__ __forceinline__ Chunk<T> load_chunk(const T* p) { return *reinterpret_cast<const Chunk<T>*>(p); }

__device__ __forceinline__ float sigmoid_f(float z) { return __builtin_amdgcn_rcpf(1.f + __expf(-z)); }
template <bool SILU> __device__ __forceinline__ float act_f(float z) { return SILU ? z * sigmoid_f(z) : z; }
template <bool SILU> __device__ __forceinline__ float act_grad_f(float z) {
    if (!SILU) return 1.f;
    const float s = sigmoid_f(z);
    return s * fmaf(z, 1.f - s, 1.f);
}

// ---------------------------------------------------------------------------------------------------------- NCHW
// part[(n·C + c)·3 + {0,1}] = mean and centred sum of squares of row (n,c) of x + a
template <typename T>
__global__ __launch_bounds__(256) void nchw_stats_fwd_kernel(const T* x, const T* a, float* part, int rows, int HW) {
    constexpr int VEC = ElemTraits<T>::kVec;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const T* xr = x + (int64_t)row * HW;
    const float x0 = to_f32<T>(xr[0]);
    float s = 0.f, ss = 0.f;
    const int chunks = HW / VEC;
#pragma unroll 4
    for (int i = lane; i < chunks; i += 64) {
        const Chunk<T> v = load_chunk(xr + i * VEC);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const float d = to_f32<T>(v.v[e]) - x0;
            s += d;
            ss = fmaf(d, d, ss);
        }
    }
    s = wave_sum(s);
    ss = wave_sum(ss);
    if (lane == 0) {
        const float m = s / (float)HW;
        part[(int64_t)row * 3 + 0] = x0 + (a ? to_f32<T>(a[row]) : 0.f) + m;
        part[(int64_t)row * 3 + 1] = fmaxf(ss - s * m, 0.f);
    }
}

// mean / rstd of group (n,g) from its cpg channel partials (equal counts), by wave 0 in a fixed order → LDS
__device__ __forceinline__ void nchw_fold_group(const float* part, int64_t row0, int cpg, int HW, float eps, float* out2) {
    if (threadIdx.x < 64) {
        float sm = 0.f;
        for (int c = threadIdx.x; c < cpg; c += 64) sm += part[(row0 + c) * 3];
        const float mean = wave_sum(sm) / (float)cpg;
        float m2 = 0.f;
        for (int c = threadIdx.x; c < cpg; c += 64) {
            const float d = part[(row0 + c) * 3] - mean;
            m2 += fmaf((float)HW * d, d, part[(row0 + c) * 3 + 1]);
        }
        const float var = wave_sum(m2) / ((float)cpg * (float)HW);
        if (threadIdx.x == 0) {
            out2[0] = mean;
            out2[1] = rsqrtf(var + eps);
        }
    }
    __syncthreads();
}

template <typename T, bool SILU>
__global__ __launch_bounds__(256) void nchw_apply_fwd_kernel(const T* x, const T* a, const T* gamma, const T* beta, T* y,
                                                             float* mean_out, float* rstd_out, const float* part, int C, int HW,
                                                             int G, float eps) {
    constexpr int VEC = ElemTraits<T>::kVec;
    __shared__ float st[2];
    const int ng = blockIdx.y, n = ng / G, g = ng - n * G, cpg = C / G;
    const int64_t row0 = (int64_t)n * C + (int64_t)g * cpg;
    nchw_fold_group(part, row0, cpg, HW, eps, st);
    const float mean = st[0], rstd = st[1];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        mean_out[ng] = mean;
        rstd_out[ng] = rstd;
    }
    const int cpr = HW / VEC, total = cpg * cpr;
    const int per = (total + gridDim.x - 1) / gridDim.x;
    const int end = min(total, (int)(blockIdx.x + 1) * per);
    for (int i = blockIdx.x * per + threadIdx.x; i < end; i += 256) {
        const int cl = i / cpr, c = g * cpg + cl;
        const float sc = rstd * to_f32<T>(gamma[c]), b = to_f32<T>(beta[c]);
        const float d = (a ? to_f32<T>(a[row0 + cl]) : 0.f) - mean;
        const int64_t off = row0 * HW + (int64_t)i * VEC;
        const Chunk<T> v = load_chunk(x + off);
        Chunk<T> o;
#pragma unroll
        for (int e = 0; e < VEC; ++e) o.v[e] = from_f32<T>(act_f<SILU>(fmaf(to_f32<T>(v.v[e]) + d, sc, b)));
        *reinterpret_cast<Chunk<T>*>(y + off) = o;
    }
}

// part[(n·C + c)·3 + {0,1,2}] = Σ dz, Σ dz·x̂, Σ x̂ over row (n,c);  dz = dy·act'(x̂γ+β)
template <typename T, bool SILU>
__global__ __launch_bounds__(256) void nchw_stats_bwd_kernel(const T* dy, const T* x, const T* a, const T* gamma, const T* beta,
                                                             const float* mean, const float* rstd, float* part, int rows, int C,
                                                             int HW, int G) {
    constexpr int VEC = ElemTraits<T>::kVec;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const int n = row / C, c = row - n * C, ng = n * G + c / (C / G);
    const float rs = rstd[ng], d = (a ? to_f32<T>(a[row]) : 0.f) - mean[ng];
    const float gm = to_f32<T>(gamma[c]), b = to_f32<T>(beta[c]);
    const T* xr = x + (int64_t)row * HW;
    const T* dr = dy + (int64_t)row * HW;
    float p = 0.f, q = 0.f, sx = 0.f;
    const int chunks = HW / VEC;
#pragma unroll 2
    for (int i = lane; i < chunks; i += 64) {
        const Chunk<T> v = load_chunk(xr + i * VEC), w = load_chunk(dr + i * VEC);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const float xh = (to_f32<T>(v.v[e]) + d) * rs;
            const float dz = to_f32<T>(w.v[e]) * act_grad_f<SILU>(fmaf(xh, gm, b));
            p += dz;
            q = fmaf(dz, xh, q);
            sx += xh;
        }
    }
    p = wave_sum(p);
    q = wave_sum(q);
    sx = wave_sum(sx);
    if (lane == 0) {
        part[(int64_t)row * 3 + 0] = p;
        part[(int64_t)row * 3 + 1] = q;
        part[(int64_t)row * 3 + 2] = sx;
    }
}

template <typename T, bool SILU>
__global__ __launch_bounds__(256) void nchw_apply_bwd_kernel(const T* dy, const T* x, const T* a, const T* gamma, const T* beta,
                                                             const float* mean_in, const float* rstd_in, T* dx, T* da,
                                                             const float* part, int C, int HW, int G, const T* dh) {
    constexpr int VEC = ElemTraits<T>::kVec;
    __shared__ float st[2];
    const int ng = blockIdx.y, n = ng / G, g = ng - n * G, cpg = C / G;
    const int64_t row0 = (int64_t)n * C + (int64_t)g * cpg;
    if (threadIdx.x < 64) {  // c2 = Σ γ·Σdz, c1 = Σ γ·Σdz·x̂ over the group's channels, fixed order
        float c2 = 0.f, c1 = 0.f;
        for (int c = threadIdx.x; c < cpg; c += 64) {
            const float gm = to_f32<T>(gamma[g * cpg + c]);
            c2 = fmaf(gm, part[(row0 + c) * 3 + 0], c2);
            c1 = fmaf(gm, part[(row0 + c) * 3 + 1], c1);
        }
        c2 = wave_sum(c2);
        c1 = wave_sum(c1);
        if (threadIdx.x == 0) {
            const float inv = 1.f / ((float)cpg * (float)HW);
            st[0] = c1 * inv;
            st[1] = c2 * inv;
        }
    }
    __syncthreads();
    const float k1 = st[0], k2 = st[1], mean = mean_in[ng], rs = rstd_in[ng];
    // Σ_hw dx of each channel, from the same channel sums.  dx sums to zero over a group, so a group of one channel has
    // da = 0 exactly: written as such, not as what the three terms leave of each other in fp32
    if (da && blockIdx.x == 0 && (int)threadIdx.x < cpg) {
        for (int c = threadIdx.x; c < cpg; c += 256) {
            const float* pc = part + (row0 + c) * 3;
            const float v = rs * (to_f32<T>(gamma[g * cpg + c]) * pc[0] - (float)HW * k2 - k1 * pc[2]);
            da[row0 + c] = from_f32<T>(cpg == 1 ? 0.f : v);
        }
    }
    const int cpr = HW / VEC, total = cpg * cpr;
    const int per = (total + gridDim.x - 1) / gridDim.x;
    const int end = min(total, (int)(blockIdx.x + 1) * per);
    for (int i = blockIdx.x * per + threadIdx.x; i < end; i += 256) {
        const int cl = i / cpr, c = g * cpg + cl;
        const float gm = to_f32<T>(gamma[c]), b = to_f32<T>(beta[c]);
        const float d = (a ? to_f32<T>(a[row0 + cl]) : 0.f) - mean;
        const int64_t off = row0 * HW + (int64_t)i * VEC;
        const Chunk<T> v = load_chunk(x + off), w = load_chunk(dy + off);
        float r[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const float xh = (to_f32<T>(v.v[e]) + d) * rs;
            const float dz = to_f32<T>(w.v[e]) * act_grad_f<SILU>(fmaf(xh, gm, b));
            r[e] = rs * (fmaf(dz, gm, -k2) - xh * k1);
        }
        if (dh) {  // the gradient that reaches x along the residual path joins before the one rounding (a uniform branch)
            const Chunk<T> u = load_chunk(dh + off);
#pragma unroll
            for (int e = 0; e < VEC; ++e) r[e] += to_f32<T>(u.v[e]);
        }
        Chunk<T> o;
#pragma unroll
        for (int e = 0; e < VEC; ++e) o.v[e] = from_f32<T>(r[e]);
        *reinterpret_cast<Chunk<T>*>(dx + off) = o;
    }
}

// ------------------------------------------------------------------------------------------- NCHW, one launch per direction
// One workgroup of kOneThreads per (n,group) slab whose cpg·H·W/8 16-byte chunks fit in K per thread, held in registers: chunk
// i = thread + j·kOneThreads, j < K, lies in channel i / (H·W/8).  All loads are issued before the first use (an index past the
// slab is clamped to its last chunk and the value masked), the reductions run wave → LDS → every thread in wave order, and the
// slab is read from memory once.
constexpr int kOneThreads = 1024, kOneWaves = kOneThreads / 64;
constexpr int kOneMaxK = 8, kOneMaxKBwd = 5;  // chunks of x per thread, and of x and of dy in the backward: 128 VGPRs per lane

// two 16-bit values in one register: a thread keeps γ, β and the addend of each of its chunks' channels this way
template <typename T> __device__ __forceinline__ uint32_t pack2(T lo, T hi) {
    return (uint32_t)__builtin_bit_cast(uint16_t, lo) | ((uint32_t)__builtin_bit_cast(uint16_t, hi) << 16);
}
template <typename T> __device__ __forceinline__ float pack_lo(uint32_t p) { return to_f32<T>(__builtin_bit_cast(T, (uint16_t)(p & 0xffffu))); }
template <typename T> __device__ __forceinline__ float pack_hi(uint32_t p) { return to_f32<T>(__builtin_bit_cast(T, (uint16_t)(p >> 16))); }

// Between two passes over the registers: the 16-bit values stay as loaded.  Without it the compiler converts the slab to fp32
// once and keeps that, twice the registers, and spills.
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
template <typename T, int K> __device__ __forceinline__ void one_keep_packed(Chunk<T> (&v)[K]) {
#pragma unroll
    for (int j = 0; j < K; ++j) {
        u32x4 u = __builtin_bit_cast(u32x4, v[j]);
        asm volatile("" : "+v"(u));
        v[j] = __builtin_bit_cast(Chunk<T>, u);
    }
}
template <int K> __device__ __forceinline__ void one_keep_packed(uint32_t (&p)[K]) {
#pragma unroll
    for (int j = 0; j < K; ++j) asm volatile("" : "+v"(p[j]));
}

// Σ over the workgroup of NV values per thread; every thread gets the totals, summed in wave order
template <int NV> __device__ __forceinline__ void one_block_sum(float (&v)[NV], float (*red)[kOneWaves]) {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        v[k] = wave_sum(v[k]);
        if ((threadIdx.x & 63) == 0) red[k][threadIdx.x >> 6] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < kOneWaves; ++w) t += red[k][w];
        v[k] = t;
    }
}

template <typename T, bool SILU, int K>
__global__ __launch_bounds__(kOneThreads) void nchw_one_fwd_kernel(const T* x, const T* a, const T* gamma, const T* beta, T* y,
                                                                   float* mean_out, float* rstd_out, int C, int HW, int G,
                                                                   float eps) {
    constexpr int VEC = ElemTraits<T>::kVec;
    __shared__ float red1[1][kOneWaves], red2[2][kOneWaves];
    const int ng = blockIdx.x, n = ng / G, g = ng - n * G, cpg = C / G;
    const int64_t row0 = (int64_t)n * C + (int64_t)g * cpg;
    const int cpr = HW / VEC, chunks = cpg * cpr;
    const T* xs = x + row0 * HW;
    Chunk<T> v[K];
    uint32_t gb[K], ad[K];  // (γ, β) and (addend, unused) of the chunk's channel
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const int i = min((int)threadIdx.x + j * kOneThreads, chunks - 1), cl = i / cpr;
        v[j] = load_chunk(xs + i * VEC);
        gb[j] = pack2<T>(gamma[g * cpg + cl], beta[g * cpg + cl]);
        ad[j] = a ? pack2<T>(a[row0 + cl], a[row0 + cl]) : 0u;
    }
    const float cnt = (float)cpg * (float)HW;
    // the mean of x + a, then the sums of e = x + a − mean and of e² from the registers: the first corrects the mean by what
    // its own rounding left, the second is centred
    float s0[1] = {0.f};
    one_keep_packed(v), one_keep_packed(ad);
#pragma unroll
    for (int j = 0; j < K; ++j) {
        if ((int)threadIdx.x + j * kOneThreads < chunks) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) s0[0] += to_f32<T>(v[j].v[e]) + pack_lo<T>(ad[j]);
        }
    }
    one_block_sum(s0, red1);
    one_keep_packed(v), one_keep_packed(ad);
    const float mean0 = s0[0] / cnt;
    float s[2] = {0.f, 0.f};
#pragma unroll
    for (int j = 0; j < K; ++j) {
        if ((int)threadIdx.x + j * kOneThreads < chunks) {
            const float d0 = pack_lo<T>(ad[j]) - mean0;
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const float u = to_f32<T>(v[j].v[e]) + d0;
                s[0] += u;
                s[1] = fmaf(u, u, s[1]);
            }
        }
    }
    one_block_sum(s, red2);
    one_keep_packed(v), one_keep_packed(ad), one_keep_packed(gb);
    const float cm = s[0] / cnt, mean = mean0 + cm, rstd = rsqrtf(fmaxf(s[1] - s[0] * cm, 0.f) / cnt + eps);
    if (threadIdx.x == 0) {
        mean_out[ng] = mean;
        rstd_out[ng] = rstd;
    }
    T* ys = y + row0 * HW;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const int i = threadIdx.x + j * kOneThreads;
        if (i < chunks) {
            const float sc = rstd * pack_lo<T>(gb[j]), d = pack_lo<T>(ad[j]) - mean;
            Chunk<T> o;
#pragma unroll
            for (int e = 0; e < VEC; ++e) o.v[e] = from_f32<T>(act_f<SILU>(fmaf(to_f32<T>(v[j].v[e]) + d, sc, pack_hi<T>(gb[j]))));
            *reinterpret_cast<Chunk<T>*>(ys + i * VEC) = o;
        }
    }
}

// The backward with x and dy of the slab in registers.  The group constants are Σ γ·dz and Σ γ·dz·x̂ over the slab; every chunk
// lies in one channel, so a thread folds γ into its own chunks' sums.  With DA each chunk's (γ·Σdz, Σx̂) also goes to LDS and the
// waves sum them per channel from there in a fixed order.  dh is fetched with x and dy where the registers allow (K = 2).
template <typename T, bool SILU, bool DA, int K>
__global__ __launch_bounds__(kOneThreads) void nchw_one_bwd_kernel(const T* dy, const T* x, const T* a, const T* gamma,
                                                                   const T* beta, const float* mean_in, const float* rstd_in,
                                                                   T* dx, T* da, int C, int HW, int G, const T* dh) {
    constexpr int VEC = ElemTraits<T>::kVec;
    __shared__ float red[2][kOneWaves];
    __shared__ float2 chan[DA ? K * kOneThreads : 1];
    const int ng = blockIdx.x, n = ng / G, g = ng - n * G, cpg = C / G;
    const int64_t row0 = (int64_t)n * C + (int64_t)g * cpg;
    const int cpr = HW / VEC, chunks = cpg * cpr;
    const T* xs = x + row0 * HW;
    const T* ds = dy + row0 * HW;
    Chunk<T> v[K], w[K];
    uint32_t gb[K], ad[K];  // (γ, β) and (addend, unused) of the chunk's channel
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const int i = min((int)threadIdx.x + j * kOneThreads, chunks - 1), cl = i / cpr;
        v[j] = load_chunk(xs + i * VEC);
        w[j] = load_chunk(ds + i * VEC);
        gb[j] = pack2<T>(gamma[g * cpg + cl], beta[g * cpg + cl]);
        ad[j] = a ? pack2<T>(a[row0 + cl], a[row0 + cl]) : 0u;
    }
    constexpr int KH = K <= 2 ? K : 1;  // dh chunks fetched up front
    const T* hs = dh ? dh + row0 * HW : nullptr;
    Chunk<T> h[KH];
    if (K <= 2 && hs) {
#pragma unroll
        for (int j = 0; j < KH; ++j) h[j] = load_chunk(hs + min((int)threadIdx.x + j * kOneThreads, chunks - 1) * VEC);
    }
    const float mean = mean_in[ng], rs = rstd_in[ng];
    float c[2] = {0.f, 0.f};  // Σ γ·dz·x̂, Σ γ·dz
    one_keep_packed(v), one_keep_packed(w), one_keep_packed(ad), one_keep_packed(gb);
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const int i = threadIdx.x + j * kOneThreads;
        if (i < chunks) {
            const float d = pack_lo<T>(ad[j]) - mean;
            float p = 0.f, q = 0.f, sx = 0.f;
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const float xh = (to_f32<T>(v[j].v[e]) + d) * rs;
                const float dz = to_f32<T>(w[j].v[e]) * act_grad_f<SILU>(fmaf(xh, pack_lo<T>(gb[j]), pack_hi<T>(gb[j])));
                p += dz;
                q = fmaf(dz, xh, q);
                sx += xh;
            }
            c[0] = fmaf(pack_lo<T>(gb[j]), q, c[0]);
            c[1] = fmaf(pack_lo<T>(gb[j]), p, c[1]);
            if (DA) chan[i] = make_float2(pack_lo<T>(gb[j]) * p, sx);
        }
    }
    one_block_sum(c, red);  // its barrier also publishes chan
    one_keep_packed(v), one_keep_packed(w), one_keep_packed(ad), one_keep_packed(gb);
    const float inv = 1.f / ((float)cpg * (float)HW), k1 = c[0] * inv, k2 = c[1] * inv;
    if (DA) {  // Σ_hw dx of each channel; one channel per group: Σ_hw dx = 0 exactly, written as such
        // lanes per channel: a power of two, no more than a row has chunks and few enough that the workgroup takes all channels
        // at once where it can (every halving step of the fold costs an LDS round trip)
        int L = 1;
        while (L < cpr && L < 64 && 2 * L * cpg <= kOneThreads) L <<= 1;
        const int lane = threadIdx.x & 63, per = 64 / L, sub = lane / L, sl = lane & (L - 1);
        for (int c0 = (threadIdx.x >> 6) * per; c0 < cpg; c0 += kOneWaves * per) {
            const int cl = c0 + sub;
            float gp = 0.f, sxc = 0.f;
            if (cl < cpg)
                for (int t = sl; t < cpr; t += L) {
                    const float2 u = chan[cl * cpr + t];
                    gp += u.x;
                    sxc += u.y;
                }
            for (int off = L >> 1; off > 0; off >>= 1) {
                gp += __shfl_xor(gp, off, 64);
                sxc += __shfl_xor(sxc, off, 64);
            }
            if (cl < cpg && sl == 0) da[row0 + cl] = from_f32<T>(cpg == 1 ? 0.f : rs * (gp - (float)HW * k2 - k1 * sxc));
        }
    }
    T* os = dx + row0 * HW;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const int i = threadIdx.x + j * kOneThreads;
        if (i < chunks) {
            const float d = pack_lo<T>(ad[j]) - mean;
            float r[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const float xh = (to_f32<T>(v[j].v[e]) + d) * rs;
                const float dz = to_f32<T>(w[j].v[e]) * act_grad_f<SILU>(fmaf(xh, pack_lo<T>(gb[j]), pack_hi<T>(gb[j])));
                r[e] = rs * (fmaf(dz, pack_lo<T>(gb[j]), -k2) - xh * k1);
            }
            if (hs) {  // the gradient that reaches x along the residual path joins before the one rounding (a uniform branch)
                const Chunk<T> u = K <= 2 ? h[j < KH ? j : 0] : load_chunk(hs + i * VEC);
#pragma unroll
                for (int e = 0; e < VEC; ++e) r[e] += to_f32<T>(u.v[e]);
            }
            Chunk<T> o;
#pragma unroll
            for (int e = 0; e < VEC; ++e) o.v[e] = from_f32<T>(r[e]);
            *reinterpret_cast<Chunk<T>*>(os + i * VEC) = o;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- NHWC
// Geometry shared by the four NHWC kernels: thread t owns channels [8·cx, 8·cx+8) of rows ry, ry+RP, … of its workgroup's
// row block; threads with ry ≥ RP (512 is not a multiple of C/8) idle.
struct NhwcThread {
    int cx, ry, RP;
    bool active;
    __device__ NhwcThread(int C) {
        const int CH = C / 8;
        RP = kNhwcThreads / CH;
        ry = threadIdx.x / CH;
        cx = threadIdx.x - ry * CH;
        active = ry < RP;
    }
};

__device__ __forceinline__ void lds_put8(float* dst, const float* v) {
    *reinterpret_cast<f32x4*>(dst) = f32x4{v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(dst + 4) = f32x4{v[4], v[5], v[6], v[7]};
}

// rows of row block s (rpb rows each, the last one short) and how many of them the thread row ry of RP reads
__device__ __forceinline__ int nhwc_block_rows(int s, int rpb, int HW) { return min(HW, (s + 1) * rpb) - s * rpb; }
__device__ __forceinline__ int nhwc_thread_rows(int rows, int ry, int RP) { return rows / RP + (ry < rows % RP); }

// gpart[((n·G + g)·S + s)·2 + {0,1}] = mean and centred sum of squares of x + a over the row block and the group's channels
template <typename T>
__global__ __launch_bounds__(kNhwcThreads) void nhwc_stats_fwd_kernel(const T* x, const T* a, float* gpart, int C, int HW, int G,
                                                                      int rpb) {
    __shared__ float red[2][kNhwcLds];
    const NhwcThread th(C);
    const int n = blockIdx.y, S = gridDim.x, cpg = C / G, c0 = th.cx * 8;
    const T* xn = x + (int64_t)n * HW * C;
    const T* an = a ? a + (int64_t)n * C : nullptr;
    const int rb = blockIdx.x * rpb, rows = nhwc_block_rows(blockIdx.x, rpb, HW), r1 = rb + rows;
    if (th.active) {
        // per channel the thread's (cnt, mean, M2) about its own first row (a thread without rows: cnt = 0, any row's value)
        const int cnt = nhwc_thread_rows(rows, th.ry, th.RP);
        const Chunk<T> f = load_chunk(xn + (int64_t)min(rb + th.ry, r1 - 1) * C + c0);
        float sh[8], s[8], ss[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            sh[e] = to_f32<T>(f.v[e]);
            s[e] = ss[e] = 0.f;
        }
#pragma unroll 4
        for (int r = rb + th.ry; r < r1; r += th.RP) {
            const Chunk<T> v = load_chunk(xn + (int64_t)r * C + c0);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float u = to_f32<T>(v.v[e]) - sh[e];
                s[e] += u;
                ss[e] = fmaf(u, u, ss[e]);
            }
        }
        const float inv = cnt ? 1.f / (float)cnt : 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float q = s[e] * inv;
            ss[e] = fmaxf(ss[e] - s[e] * q, 0.f);
            s[e] = cnt ? sh[e] + q + (an ? to_f32<T>(an[c0 + e]) : 0.f) : 0.f;
        }
        lds_put8(&red[0][th.ry * C + c0], s);
        lds_put8(&red[1][th.ry * C + c0], ss);
    }
    __syncthreads();
    for (int g = threadIdx.x; g < G; g += kNhwcThreads) {  // merge the RP × cpg triples of group g, fixed order
        const int ca = g * cpg, cb = ca + cpg, full = rows / th.RP, rem = rows - full * th.RP;
        float sm = 0.f;
        for (int r = 0; r < th.RP; ++r) {
            const float w = (float)(full + (r < rem));
            for (int c = ca; c < cb; ++c) sm = fmaf(w, red[0][r * C + c], sm);
        }
        const float tot = (float)cpg * (float)rows, mu = sm / tot;
        float s1 = 0.f, s2 = 0.f;
        for (int r = 0; r < th.RP; ++r) {
            const float w = (float)(full + (r < rem));
            for (int c = ca; c < cb; ++c) {
                const float d = red[0][r * C + c] - mu, wd = w * d;
                s1 += wd;
                s2 += fmaf(wd, d, red[1][r * C + c]);
            }
        }
        const float cm = s1 / tot;
        float* o = gpart + (((int64_t)n * G + g) * S + blockIdx.x) * 2;
        o[0] = mu + cm;
        o[1] = fmaxf(s2 - s1 * cm, 0.f);
    }
}

template <typename T, bool SILU>
__global__ __launch_bounds__(kNhwcThreads) void nhwc_apply_fwd_kernel(const T* x, const T* a, const T* gamma, const T* beta, T* y,
                                                                      float* mean_out, float* rstd_out, const float* gpart, int C,
                                                                      int HW, int G, int S, int rpb_stats, int rpb, float eps) {
    __shared__ float st[2][kMaxGroups];
    const NhwcThread th(C);
    const int n = blockIdx.y, cpg = C / G, c0 = th.cx * 8;
    const T* xn = x + (int64_t)n * HW * C;
    const T* an = a ? a + (int64_t)n * C : nullptr;
    for (int g = threadIdx.x; g < G; g += kNhwcThreads) {  // merge the S row blocks' (rows·cpg, mean, M2), fixed order
        const float* p = gpart + ((int64_t)n * G + g) * S * 2;
        float sm = 0.f;
        for (int i = 0; i < S; ++i) sm = fmaf((float)nhwc_block_rows(i, rpb_stats, HW), p[2 * i], sm);
        const float mu = sm / (float)HW;
        float s1 = 0.f, s2 = 0.f;
        for (int i = 0; i < S; ++i) {
            const float d = p[2 * i] - mu, wd = (float)(nhwc_block_rows(i, rpb_stats, HW) * cpg) * d;
            s1 += wd;
            s2 += fmaf(wd, d, p[2 * i + 1]);
        }
        const float tot = (float)cpg * (float)HW, cm = s1 / tot;
        const float mean = mu + cm, rstd = rsqrtf(fmaxf(s2 - s1 * cm, 0.f) / tot + eps);
        st[0][g] = mean;
        st[1][g] = rstd;
        if (blockIdx.x == 0) {
            mean_out[n * G + g] = mean;
            rstd_out[n * G + g] = rstd;
        }
    }
    __syncthreads();
    if (!th.active) return;
    float d[8], sc[8], b[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int c = c0 + e, g = c / cpg;
        d[e] = (an ? to_f32<T>(an[c]) : 0.f) - st[0][g];
        sc[e] = st[1][g] * to_f32<T>(gamma[c]);
        b[e] = to_f32<T>(beta[c]);
    }
    T* yn = y + (int64_t)n * HW * C;
    const int r1 = min(HW, (int)(blockIdx.x + 1) * rpb);
#pragma unroll 4
    for (int r = blockIdx.x * rpb + th.ry; r < r1; r += th.RP) {
        const Chunk<T> v = load_chunk(xn + (int64_t)r * C + c0);
        Chunk<T> o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o.v[e] = from_f32<T>(act_f<SILU>(fmaf(to_f32<T>(v.v[e]) + d[e], sc[e], b[e])));
        *reinterpret_cast<Chunk<T>*>(yn + (int64_t)r * C + c0) = o;
    }
}

// gpart[((n·G + g)·S + s)·2 + {0,1}] = Σ γ·dz·x̂, Σ γ·dz over the row block and the group's channels;
// with DA also cpart[((n·S + s)·3 + {0,1,2})·C + c] = Σ dz, Σ dz·x̂, Σ x̂ over the row block per channel
template <typename T, bool SILU, bool DA>
__global__ __launch_bounds__(kNhwcThreads) void nhwc_stats_bwd_kernel(const T* dy, const T* x, const T* a, const T* gamma,
                                                                      const T* beta, const float* mean, const float* rstd,
                                                                      float* gpart, float* cpart, int C, int HW, int G, int rpb) {
    __shared__ float red[DA ? 3 : 2][kNhwcLds];
    const NhwcThread th(C);
    const int n = blockIdx.y, S = gridDim.x, cpg = C / G, c0 = th.cx * 8;
    const T* xn = x + (int64_t)n * HW * C;
    const T* dn = dy + (int64_t)n * HW * C;
    if (th.active) {
        float d[8], rs[8], gm[8], b[8], p[8], q[8], sx[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int c = c0 + e, ng = n * G + c / cpg;
            d[e] = (a ? to_f32<T>(a[(int64_t)n * C + c]) : 0.f) - mean[ng];
            rs[e] = rstd[ng];
            gm[e] = to_f32<T>(gamma[c]);
            b[e] = to_f32<T>(beta[c]);
            p[e] = q[e] = sx[e] = 0.f;
        }
        const int r1 = min(HW, (int)(blockIdx.x + 1) * rpb);
#pragma unroll 2
        for (int r = blockIdx.x * rpb + th.ry; r < r1; r += th.RP) {
            const Chunk<T> v = load_chunk(xn + (int64_t)r * C + c0), w = load_chunk(dn + (int64_t)r * C + c0);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float xh = (to_f32<T>(v.v[e]) + d[e]) * rs[e];
                const float dz = to_f32<T>(w.v[e]) * act_grad_f<SILU>(fmaf(xh, gm[e], b[e]));
                p[e] += dz;
                q[e] = fmaf(dz, xh, q[e]);
                if (DA) sx[e] += xh;
            }
        }
        lds_put8(&red[0][th.ry * C + c0], p);
        lds_put8(&red[1][th.ry * C + c0], q);
        if (DA) lds_put8(&red[2][th.ry * C + c0], sx);
    }
    __syncthreads();
    for (int g = threadIdx.x; g < G; g += kNhwcThreads) {
        float c1 = 0.f, c2 = 0.f;
        for (int c = g * cpg; c < (g + 1) * cpg; ++c) {
            float pc = 0.f, qc = 0.f;
            for (int r = 0; r < th.RP; ++r) {
                pc += red[0][r * C + c];
                qc += red[1][r * C + c];
            }
            const float gmc = to_f32<T>(gamma[c]);
            c2 = fmaf(gmc, pc, c2);
            c1 = fmaf(gmc, qc, c1);
        }
        float* o = gpart + (((int64_t)n * G + g) * S + blockIdx.x) * 2;
        o[0] = c1;
        o[1] = c2;
    }
    if (DA) {
        for (int c = threadIdx.x; c < C; c += kNhwcThreads) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                float v = 0.f;
                for (int r = 0; r < th.RP; ++r) v += red[j][r * C + c];
                cpart[(((int64_t)n * S + blockIdx.x) * 3 + j) * C + c] = v;
            }
        }
    }
}

template <typename T, bool SILU>
__global__ __launch_bounds__(kNhwcThreads) void nhwc_apply_bwd_kernel(const T* dy, const T* x, const T* a, const T* gamma,
                                                                      const T* beta, const float* mean, const float* rstd, T* dx,
                                                                      T* da, const float* gpart, const float* cpart, int C, int HW,
                                                                      int G, int S, int rpb) {
    __shared__ float st[2][kMaxGroups];
    const NhwcThread th(C);
    const int n = blockIdx.y, cpg = C / G, c0 = th.cx * 8;
    for (int g = threadIdx.x; g < G; g += kNhwcThreads) {
        const float* p = gpart + ((int64_t)n * G + g) * S * 2;
        float c1 = 0.f, c2 = 0.f;
        for (int i = 0; i < S; ++i) {
            c1 += p[2 * i];
            c2 += p[2 * i + 1];
        }
        const float inv = 1.f / ((float)cpg * (float)HW);
        st[0][g] = c1 * inv;
        st[1][g] = c2 * inv;
    }
    __syncthreads();
    if (da && blockIdx.x == 0) {  // Σ_hw dx of each channel from the per-channel partials, fixed order over the row blocks
        for (int c = threadIdx.x; c < C; c += kNhwcThreads) {
            float pc = 0.f, sxc = 0.f;
            for (int i = 0; i < S; ++i) {
                pc += cpart[(((int64_t)n * S + i) * 3 + 0) * C + c];
                sxc += cpart[(((int64_t)n * S + i) * 3 + 2) * C + c];
            }
            const int g = c / cpg;
            const float v = rstd[n * G + g] * (to_f32<T>(gamma[c]) * pc - (float)HW * st[1][g] - st[0][g] * sxc);
            da[(int64_t)n * C + c] = from_f32<T>(cpg == 1 ? 0.f : v);  // one channel per group: Σ_hw dx = 0 exactly
        }
    }
    if (!th.active) return;
    float d[8], rs[8], gm[8], b[8], k1[8], k2[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int c = c0 + e, g = c / cpg;
        d[e] = (a ? to_f32<T>(a[(int64_t)n * C + c]) : 0.f) - mean[n * G + g];
        rs[e] = rstd[n * G + g];
        gm[e] = to_f32<T>(gamma[c]);
        b[e] = to_f32<T>(beta[c]);
        k1[e] = st[0][g];
        k2[e] = st[1][g];
    }
    const T* xn = x + (int64_t)n * HW * C;
    const T* dn = dy + (int64_t)n * HW * C;
    T* on = dx + (int64_t)n * HW * C;
    const int r1 = min(HW, (int)(blockIdx.x + 1) * rpb);
#pragma unroll 2
    for (int r = blockIdx.x * rpb + th.ry; r < r1; r += th.RP) {
        const Chunk<T> v = load_chunk(xn + (int64_t)r * C + c0), w = load_chunk(dn + (int64_t)r * C + c0);
        Chunk<T> o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float xh = (to_f32<T>(v.v[e]) + d[e]) * rs[e];
            const float dz = to_f32<T>(w.v[e]) * act_grad_f<SILU>(fmaf(xh, gm[e], b[e]));
            o.v[e] = from_f32<T>(rs[e] * (fmaf(dz, gm[e], -k2[e]) - xh * k1[e]));
        }
        *reinterpret_cast<Chunk<T>*>(on + (int64_t)r * C + c0) = o;
    }
}

// ---------------------------------------------------------------------------------------------------------- host side
struct NhwcPlan {
    int S, rpb_stats;   // statistics: S row blocks of rpb_stats rows per sample
    int SA, rpb_apply;  // apply: SA row blocks of rpb_apply rows per sample
};

// About 256 statistics workgroups (one per CU; each also costs every apply workgroup a partial to fold) and about 1024 apply
// workgroups over the N samples, and at least 4 (2) rows per thread where the tensor is small.
NhwcPlan nhwc_plan(int N, int C, int HW) {
    const int RP = kNhwcThreads / (C / 8);
    auto split = [&](int want, int min_rows, int cap) {
        int s = (want + N - 1) / N;
        const int most = (HW + RP * min_rows - 1) / (RP * min_rows);
        if (s > most) s = most;
        if (s > cap) s = cap;
        if (s < 1) s = 1;
        return (HW + s - 1) / s;  // rows per block
    };
    NhwcPlan p;
    p.rpb_stats = split(256, 4, kMaxSplit);
    p.S = (HW + p.rpb_stats - 1) / p.rpb_stats;
    p.rpb_apply = split(1024, 2, 65535);
    p.SA = (HW + p.rpb_apply - 1) / p.rpb_apply;
    return p;
}

int nchw_slices(int N, int G, int chunks_per_slab) {  // apply workgroups per (n,group) slab: about 2048 in all, ≥ 512 chunks each
    int s = (2048 + N * G - 1) / (N * G);
    const int most = (chunks_per_slab + 511) / 512;
    if (s > most) s = most;
    return s < 1 ? 1 : s;
}

int64_t align16(int64_t b) { return (b + 15) & ~(int64_t)15; }

int check_shape(int N, int C, int HW, int G, int channels_last) {
    if (N < 1 || C < 1 || HW < 1 || G < 1 || C % G) return LORA_E_BADARG;
    if (G > kMaxGroups) return LORA_E_UNSUPPORTED;
    if (channels_last ? (C % 8 != 0 || C / 8 > kNhwcThreads) : (HW % 8 != 0)) return LORA_E_UNSUPPORTED;
    if ((int64_t)N * G > 65535 || N > 65535) return LORA_E_UNSUPPORTED;
    return LORA_OK;
}

// Chunks per thread of the one-launch NCHW form for this call, or 0 for the two-launch form: a function of the shape and the
// direction alone.  One workgroup per slab leaves CUs idle when there are fewer slabs than CUs, and the 16-bit ↔ fp32 and SiLU
// arithmetic of a large slab then takes longer on one CU than the second launch costs, so the largest slab (in 16-byte chunks)
// that goes to one launch grows with the number of slabs.  The limits are the largest size classes at which one launch was
// faster inside a replayed graph for the identity, SiLU and SiLU + addend variants at N·G = 32, 128 and 256 slabs
// (profiles/r13_norm_one_launch_sweep.log; profiles/README.md says which comparison each limit rests on); slab counts in
// between take the limit of the count below them.
constexpr int kOneCapFwd = kOneMaxK * kOneThreads, kOneCapBwd = kOneMaxKBwd * kOneThreads;
int nchw_one_limit(int slabs, bool backward) {
#ifdef NORM_ONE_FORCE  // dev builds of tools/norm_one_launch_sweep.py: 0 = two launches everywhere, 1 = one wherever the registers allow
    return NORM_ONE_FORCE ? (backward ? kOneCapBwd : kOneCapFwd) : 0;
#else
    if (slabs >= 256) return backward ? kOneCapBwd : kOneCapFwd;  // 80 KB / 128 KB of 16-bit elements
    if (slabs >= 128) return backward ? 2880 : 2560;              // 45 KB / 40 KB
    return backward ? 1280 : 1920;                                // 20 KB / 30 KB
#endif
}

int nchw_one_k(int N, int C, int HW, int G, bool backward) {
    const int64_t chunks = (int64_t)(C / G) * (HW / 8);
    if (chunks > nchw_one_limit(N * G, backward)) return 0;
    return chunks <= 2 * kOneThreads ? 2 : chunks <= 5 * kOneThreads ? 5 : kOneMaxK;
}

template <typename T, bool SILU, int K>
void launch_one_fwd(const T* x, const T* a, const T* gamma, const T* beta, T* y, float* mean, float* rstd, int N, int C, int HW,
                    int G, float eps, hipStream_t s) {
    hipLaunchKernelGGL((nchw_one_fwd_kernel<T, SILU, K>), dim3(N * G), dim3(kOneThreads), 0, s, x, a, gamma, beta, y, mean, rstd, C,
                       HW, G, eps);
}

template <typename T, bool SILU, int K>
void launch_one_bwd(const T* dy, const T* x, const T* a, const T* gamma, const T* beta, const float* mean, const float* rstd, T* dx,
                    T* da, int N, int C, int HW, int G, const T* dh, hipStream_t s) {
    if (da)
        hipLaunchKernelGGL((nchw_one_bwd_kernel<T, SILU, true, K>), dim3(N * G), dim3(kOneThreads), 0, s, dy, x, a, gamma, beta,
                           mean, rstd, dx, da, C, HW, G, dh);
    else
        hipLaunchKernelGGL((nchw_one_bwd_kernel<T, SILU, false, K>), dim3(N * G), dim3(kOneThreads), 0, s, dy, x, a, gamma, beta,
                           mean, rstd, dx, da, C, HW, G, dh);
}

template <typename T, bool SILU>
int run_fwd(const void* x_, const void* a_, const void* gamma_, const void* beta_, void* y_, float* mean, float* rstd, void* ws,
            int N, int C, int HW, int G, float eps, int channels_last, hipStream_t s) {
    const T *x = static_cast<const T*>(x_), *a = static_cast<const T*>(a_), *gamma = static_cast<const T*>(gamma_),
            *beta = static_cast<const T*>(beta_);
    T* y = static_cast<T*>(y_);
    float* part = static_cast<float*>(ws);
    if (channels_last) {
        const NhwcPlan p = nhwc_plan(N, C, HW);
        hipLaunchKernelGGL(nhwc_stats_fwd_kernel<T>, dim3(p.S, N), dim3(kNhwcThreads), 0, s, x, a, part, C, HW, G, p.rpb_stats);
        hipLaunchKernelGGL((nhwc_apply_fwd_kernel<T, SILU>), dim3(p.SA, N), dim3(kNhwcThreads), 0, s, x, a, gamma, beta, y, mean,
                           rstd, part, C, HW, G, p.S, p.rpb_stats, p.rpb_apply, eps);
    } else if (const int k = nchw_one_k(N, C, HW, G, false)) {
        if (k == 2) launch_one_fwd<T, SILU, 2>(x, a, gamma, beta, y, mean, rstd, N, C, HW, G, eps, s);
        else if (k == 5) launch_one_fwd<T, SILU, 5>(x, a, gamma, beta, y, mean, rstd, N, C, HW, G, eps, s);
        else launch_one_fwd<T, SILU, kOneMaxK>(x, a, gamma, beta, y, mean, rstd, N, C, HW, G, eps, s);
    } else {
        const int rows = N * C;
        hipLaunchKernelGGL(nchw_stats_fwd_kernel<T>, dim3((rows + 3) / 4), dim3(256), 0, s, x, a, part, rows, HW);
        hipLaunchKernelGGL((nchw_apply_fwd_kernel<T, SILU>), dim3(nchw_slices(N, G, C / G * (HW / 8)), N * G), dim3(256), 0, s, x,
                           a, gamma, beta, y, mean, rstd, part, C, HW, G, eps);
    }
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}

template <typename T, bool SILU>
int run_bwd(const void* dy_, const void* x_, const void* a_, const void* gamma_, const void* beta_, const float* mean,
            const float* rstd, void* dx_, void* da_, void* ws, int N, int C, int HW, int G, int channels_last, hipStream_t s,
            const void* dh_ = nullptr) {
    const T *dy = static_cast<const T*>(dy_), *dh = static_cast<const T*>(dh_), *x = static_cast<const T*>(x_), *a = static_cast<const T*>(a_),
            *gamma = static_cast<const T*>(gamma_), *beta = static_cast<const T*>(beta_);
    T *dx = static_cast<T*>(dx_), *da = static_cast<T*>(da_);
    float* part = static_cast<float*>(ws);
    if (channels_last) {
        const NhwcPlan p = nhwc_plan(N, C, HW);
        float* cpart = part + align16((int64_t)N * G * p.S * 2 * 4) / 4;
        if (da)
            hipLaunchKernelGGL((nhwc_stats_bwd_kernel<T, SILU, true>), dim3(p.S, N), dim3(kNhwcThreads), 0, s, dy, x, a, gamma, beta,
                               mean, rstd, part, cpart, C, HW, G, p.rpb_stats);
        else
            hipLaunchKernelGGL((nhwc_stats_bwd_kernel<T, SILU, false>), dim3(p.S, N), dim3(kNhwcThreads), 0, s, dy, x, a, gamma, beta,
                               mean, rstd, part, cpart, C, HW, G, p.rpb_stats);
        hipLaunchKernelGGL((nhwc_apply_bwd_kernel<T, SILU>), dim3(p.SA, N), dim3(kNhwcThreads), 0, s, dy, x, a, gamma, beta, mean,
                           rstd, dx, da, part, cpart, C, HW, G, p.S, p.rpb_apply);
    } else if (const int k = nchw_one_k(N, C, HW, G, true)) {
        if (k == 2) launch_one_bwd<T, SILU, 2>(dy, x, a, gamma, beta, mean, rstd, dx, da, N, C, HW, G, dh, s);
        else launch_one_bwd<T, SILU, kOneMaxKBwd>(dy, x, a, gamma, beta, mean, rstd, dx, da, N, C, HW, G, dh, s);
    } else {
        const int rows = N * C;
        hipLaunchKernelGGL((nchw_stats_bwd_kernel<T, SILU>), dim3((rows + 3) / 4), dim3(256), 0, s, dy, x, a, gamma, beta, mean,
                           rstd, part, rows, C, HW, G);
        hipLaunchKernelGGL((nchw_apply_bwd_kernel<T, SILU>), dim3(nchw_slices(N, G, C / G * (HW / 8)), N * G), dim3(256), 0, s, dy,
                           x, a, gamma, beta, mean, rstd, dx, da, part, C, HW, G, dh);
    }
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}

}  // namespace

extern "C" int64_t group_norm_act_workspace_bytes(int N, int C, int HW, int groups, int channels_last, int want_da) {
    if (check_shape(N, C, HW, groups, channels_last) != LORA_OK) return 0;
    if (!channels_last) return align16((int64_t)N * C * 3 * 4);
    const NhwcPlan p = nhwc_plan(N, C, HW);
    return align16((int64_t)N * groups * p.S * 2 * 4) + (want_da ? align16((int64_t)N * p.S * 3 * C * 4) : 0);
}

extern "C" int group_norm_act_plan(int N, int C, int HW, int groups, int channels_last, int backward) {
    if (check_shape(N, C, HW, groups, channels_last) != LORA_OK) return 0;
    return !channels_last && nchw_one_k(N, C, HW, groups, backward != 0) ? 1 : 2;
}

extern "C" int group_norm_act_fwd(const void* x, const void* addend, const void* gamma, const void* beta, void* y, float* mean,
                                  float* rstd, void* workspace, int N, int C, int HW, int groups, float eps, int act,
                                  int channels_last, int dtype, void* stream) {
    if (!x || !gamma || !beta || !y || !mean || !rstd || !workspace || (act != 0 && act != 1)) return LORA_E_BADARG;
    if (const int st = check_shape(N, C, HW, groups, channels_last)) return st;
    if (!aligned16(x) || !aligned16(y) || !aligned16(workspace)) return LORA_E_ALIGN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (dtype) {
        case LORA_F16:
            return act ? run_fwd<half_t, true>(x, addend, gamma, beta, y, mean, rstd, workspace, N, C, HW, groups, eps, channels_last, s)
                       : run_fwd<half_t, false>(x, addend, gamma, beta, y, mean, rstd, workspace, N, C, HW, groups, eps, channels_last, s);
        case LORA_BF16:
            return act ? run_fwd<bf16_t, true>(x, addend, gamma, beta, y, mean, rstd, workspace, N, C, HW, groups, eps, channels_last, s)
                       : run_fwd<bf16_t, false>(x, addend, gamma, beta, y, mean, rstd, workspace, N, C, HW, groups, eps, channels_last, s);
        case LORA_F32: return LORA_E_UNSUPPORTED;
        default: return LORA_E_BADARG;
    }
}

namespace {
int bwd_entry(const void* dy, const void* dh, const void* x, const void* addend, const void* gamma, const void* beta,
              const float* mean, const float* rstd, void* dx, void* da, void* workspace, int N, int C, int HW, int groups, int act,
              int channels_last, int dtype, void* stream) {
    if (!dy || !x || !gamma || !beta || !mean || !rstd || !dx || !workspace || (act != 0 && act != 1)) return LORA_E_BADARG;
    if (da && !addend) return LORA_E_BADARG;
    if (const int st = check_shape(N, C, HW, groups, channels_last)) return st;
    if (dh && channels_last) return LORA_E_UNSUPPORTED;
    if (!aligned16(dy) || !aligned16(dh) || !aligned16(x) || !aligned16(dx) || !aligned16(workspace)) return LORA_E_ALIGN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (dtype) {
        case LORA_F16:
            return act ? run_bwd<half_t, true>(dy, x, addend, gamma, beta, mean, rstd, dx, da, workspace, N, C, HW, groups, channels_last, s, dh)
                       : run_bwd<half_t, false>(dy, x, addend, gamma, beta, mean, rstd, dx, da, workspace, N, C, HW, groups, channels_last, s, dh);
        case LORA_BF16:
            return act ? run_bwd<bf16_t, true>(dy, x, addend, gamma, beta, mean, rstd, dx, da, workspace, N, C, HW, groups, channels_last, s, dh)
                       : run_bwd<bf16_t, false>(dy, x, addend, gamma, beta, mean, rstd, dx, da, workspace, N, C, HW, groups, channels_last, s, dh);
        case LORA_F32: return LORA_E_UNSUPPORTED;
        default: return LORA_E_BADARG;
    }
}
}  // namespace

extern "C" int group_norm_act_bwd(const void* dy, const void* x, const void* addend, const void* gamma, const void* beta,
                                  const float* mean, const float* rstd, void* dx, void* da, void* workspace, int N, int C, int HW,
                                  int groups, int act, int channels_last, int dtype, void* stream) {
    return bwd_entry(dy, nullptr, x, addend, gamma, beta, mean, rstd, dx, da, workspace, N, C, HW, groups, act, channels_last, dtype,
                     stream);
}

extern "C" int group_norm_act_bwd_res(const void* dy, const void* dh, const void* x, const void* addend, const void* gamma,
                                      const void* beta, const float* mean, const float* rstd, void* dx, void* da, void* workspace,
                                      int N, int C, int HW, int groups, int act, int dtype, void* stream) {
    return bwd_entry(dy, dh, x, addend, gamma, beta, mean, rstd, dx, da, workspace, N, C, HW, groups, act, 0, dtype, stream);
}

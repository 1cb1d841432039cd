// Every ResNet block's time-embedding projection in ONE launch:
//     out_l[n, c] = round( Σ_e W_l[c, e] · silu(t[n, e]) + b_l[c] + cb_l[c] ),   l = 0 .. L-1,
// t [N, E] and W_l [C_l, E] row-major 16-bit (f16 or bf16), b_l / cb_l [C_l] of that dtype and each nullable per layer (the
// projection's own bias and the bias of the convolution whose output the addend joins).  1 <= N <= 16, E % 8 == 0, any C_l >= 1.
// The blocks' 22 projections read the same silu(t), depend on nothing in the trunk and have frozen weights: as 22 × (silu, M = N
// GEMM, broadcast add) they are 66 launches of 5–8 µs each that stream 51.6 MB of weights between them (SD1.5, E = 1280).
//
// Shape: a GEMV with N right-hand sides, bound by the one pass over the weights.  The output rows of all layers are numbered
// through (row0[l] = Σ_{j<l} C_j); a workgroup of 4 waves takes 16 consecutive rows, a wave 4 of them, whatever layers they fall
// in.  E is walked in passes of 512 elements, one 16-byte chunk per lane:
//   * a lane loads its chunk of each of its wave's 4 weight rows straight into registers (global_load_dwordx4, no LDS round trip:
//     a weight is used by one wave, once), one pass AHEAD: the loads of pass p + 1 are issued at the top of pass p and waited for
//     at its end, so they are in flight across p's staging, barriers and FMAs.  Every load is unconditional, from an address
//     clamped into its row, and a lane past the end of E clears what it got with an AND (a select may become a branch around
//     the load, which the compiler then waits for on the spot);
//   * the workgroup stages silu(t) of the pass for all N rows in LDS as fp32 ([n][half][lane] float4, so a lane's two ds_read_b128
//     per n are conflict-free), evaluated in fp32 from the stored 16-bit t (also fetched a pass ahead) and never rounded back;
//   * a lane keeps 4 × NB fp32 accumulators (NB = N rounded up to 1, 2, 4, 8, 16; rows n >= N are staged as zeros) and adds its
//     8 products per (row, n) in ascending e.
// After the last pass the wave sums each accumulator over its lanes with the xor butterfly of wave_sum, lane n adds the biases
// in fp32 ((Σ + b) + cb) and stores out_l[n, c] with a plain 2-byte vector store.  The order of every sum is fixed by the shape
// alone: no atomics, no workspace, bit-identical from run to run and under graph replay.
//
// silu(x) = x · rcp(1 + exp2(−log2(e) · x)) with v_exp_f32 and v_rcp_f32 (1 ulp each).  The product −log2(e)·x carries a relative
// error of at most 2⁻²³ (its rounding and the constant's), i.e. an absolute one of |x|·2⁻²³ in the exponent of e = exp(−x), so
// e is off by at most (|x| + 1)·2⁻²³ relative; 1 + e, the reciprocal and the product add 2⁻²⁴ + 2⁻²³ + 2⁻²⁴, and e enters the
// quotient with weight e / (1 + e) < 1 (times |x| it is below 0.37 for x > 0):
//     |silu_kernel(x) − silu(x)| <= (|x| + 3) · 2⁻²³ · |silu(x)|          (+ 1e-30: below x = −88 e overflows and the result is −0
// where silu(x) is of the order 1e-37).  No NaN for finite x: 1 + e >= 1, and rcp(inf) = 0.  tests/test_gpu_time_proj.py uses it.
//
// Layer descriptors (pointers and the row prefix) travel by value in the kernel-argument segment, at most 32 layers per launch;
// the entry cuts longer lists into further launches.  There is no device-side table, no cached state, nothing to allocate or
// upload: under stream capture a call is an ordinary kernel node.  A wave finds the layer of a row by counting the prefix entries
// not above it (scalar code: rows, layers and pointers are wave-uniform).
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): DESIGN.md §4 has the table; no scratch in any instantiation.
#include <limits.h>

#include "common.h"

namespace {

constexpr int kMaxLayers = 32;   // per launch
constexpr int kWaves = 4;        // per workgroup
constexpr int kRows = 4;         // output rows per wave
constexpr int kPassE = 64 * 8;   // elements of E per pass: one chunk per lane
constexpr float kNegLog2e = -1.44269504088896340736f;

struct TimeProjLayers {
    const void* W[kMaxLayers];
    const void* b[kMaxLayers];   // nullable
    const void* cb[kMaxLayers];  // nullable
    int row0[kMaxLayers + 1];    // first output row of layer l among this launch's rows; row0[L] = their number
    int L;
};

__device__ __forceinline__ float silu_f(float x) {
    return x * __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(kNegLog2e * x));
}

template <typename T> __device__ __forceinline__ Chunk<T> load_chunk(const T* p) { return *reinterpret_cast<const Chunk<T>*>(p); }

// the chunk where keep, +0.0 in every element otherwise, as an AND on its four dwords: a select on a just-loaded value may
// become a branch around the load, which is then waited for on the spot
template <typename T> __device__ __forceinline__ Chunk<T> keep_if(Chunk<T> c, bool keep) {
    union {
        Chunk<T> c;
        uint32_t u[4];
    } x;
    x.c = c;
    const uint32_t m = keep ? 0xffffffffu : 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) x.u[i] &= m;
    return x.c;
}

// layer of output row g: the number of prefix entries row0[1 .. L-1] that are <= g
__device__ __forceinline__ int layer_of(const TimeProjLayers& d, int g) {
    int l = 0;
    for (int j = 1; j < d.L; ++j) l += g >= d.row0[j] ? 1 : 0;
    return l;
}

// grid ⌈rows / 16⌉; out is this launch's first layer's block, layer l at out + N·row0[l]
template <typename T, int NB>
__global__ __launch_bounds__(kWaves * 64) void time_proj_kernel(const T* __restrict__ t, T* __restrict__ out, const TimeProjLayers d,
                                                                 int N, int E) {
    __shared__ float4 s_silu[NB * 2 * 64];  // [n][half of the chunk][lane]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int rows = d.row0[d.L];
    const int g0 = ((int)blockIdx.x * kWaves + wave) * kRows;  // < rows + 16: the entry keeps rows below INT_MAX − 16

    const T* wrow[kRows];  // a row past the end reads the last row again and stores nothing
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const int g = min(g0 + r, rows - 1), l = layer_of(d, g);
        wrow[r] = static_cast<const T*>(d.W[l]) + (int64_t)(g - d.row0[l]) * E;
    }

    float acc[kRows][NB];
#pragma unroll
    for (int r = 0; r < kRows; ++r)
#pragma unroll
        for (int n = 0; n < NB; ++n) acc[r][n] = 0.f;

    // this thread's share of a pass's staging: chunk `lane` of rows sn0, sn0 + 4, ... of t (NB / 4 of them, one for NB <= 4)
    constexpr int kStage = NB > kWaves ? NB / kWaves : 1;
    const int sn0 = (int)threadIdx.x >> 6;

    // every load below is unconditional, from an address clamped into its row, and a lane past the end zeroes what it got: a
    // load under a branch would be waited for inside the branch, one at a time
    Chunk<T> w[kRows], wn[kRows], tv[kStage], tvn[kStage];
    const T* trow[kStage];
#pragma unroll
    for (int k = 0; k < kStage; ++k) trow[k] = t + (int64_t)min(sn0 + k * kWaves, N - 1) * E;
#pragma unroll
    for (int r = 0; r < kRows; ++r) w[r] = keep_if(load_chunk(wrow[r] + min(lane * 8, E - 8)), lane * 8 < E);
#pragma unroll
    for (int k = 0; k < kStage; ++k)  // silu(0) = 0: rows n >= N and the tail of E add nothing
        tv[k] = keep_if(load_chunk(trow[k] + min(lane * 8, E - 8)), sn0 + k * kWaves < N && lane * 8 < E);

    for (int e0 = 0; e0 < E; e0 += kPassE) {
        // the NEXT pass's weights and t are requested first and stay in flight across this pass's staging, barriers and FMAs:
        // what this pass uses was requested a pass ago
        const int en = e0 + kPassE + lane * 8, enc = min(en, E - 8);
#pragma unroll
        for (int r = 0; r < kRows; ++r) wn[r] = load_chunk(wrow[r] + enc);
#pragma unroll
        for (int k = 0; k < kStage; ++k) tvn[k] = load_chunk(trow[k] + enc);
        if (e0) __syncthreads();  // the previous pass's readers are done
#pragma unroll
        for (int k = 0; k < kStage; ++k) {
            const int n = sn0 + k * kWaves;
            if (n < NB) {
                const Chunk<T>& v = tv[k];
                s_silu[(n * 2 + 0) * 64 + lane] = {silu_f(to_f32<T>(v.v[0])), silu_f(to_f32<T>(v.v[1])), silu_f(to_f32<T>(v.v[2])),
                                                   silu_f(to_f32<T>(v.v[3]))};
                s_silu[(n * 2 + 1) * 64 + lane] = {silu_f(to_f32<T>(v.v[4])), silu_f(to_f32<T>(v.v[5])), silu_f(to_f32<T>(v.v[6])),
                                                   silu_f(to_f32<T>(v.v[7]))};
            }
        }
        __syncthreads();
#pragma unroll
        for (int n = 0; n < NB; ++n) {  // a lane past the end of E multiplies zeros by staged zeros
            const float4 lo = s_silu[(n * 2 + 0) * 64 + lane], hi = s_silu[(n * 2 + 1) * 64 + lane];
#pragma unroll
            for (int r = 0; r < kRows; ++r) {
                float a = acc[r][n];
                a = fmaf(to_f32<T>(w[r].v[0]), lo.x, a);
                a = fmaf(to_f32<T>(w[r].v[1]), lo.y, a);
                a = fmaf(to_f32<T>(w[r].v[2]), lo.z, a);
                a = fmaf(to_f32<T>(w[r].v[3]), lo.w, a);
                a = fmaf(to_f32<T>(w[r].v[4]), hi.x, a);
                a = fmaf(to_f32<T>(w[r].v[5]), hi.y, a);
                a = fmaf(to_f32<T>(w[r].v[6]), hi.z, a);
                a = fmaf(to_f32<T>(w[r].v[7]), hi.w, a);
                acc[r][n] = a;
            }
        }
#pragma unroll
        for (int r = 0; r < kRows; ++r) w[r] = keep_if(wn[r], en < E);
#pragma unroll
        for (int k = 0; k < kStage; ++k) tv[k] = keep_if(tvn[k], sn0 + k * kWaves < N && en < E);
    }

#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const int g = g0 + r;
        if (g >= rows) break;  // wave-uniform
        float v = 0.f;
#pragma unroll
        for (int n = 0; n < NB; ++n) {
            const float s = wave_sum(acc[r][n]);
            if (lane == n) v = s;
        }
        if (lane < N) {
            const int l = layer_of(d, g), c = g - d.row0[l], C = d.row0[l + 1] - d.row0[l];
            const T* b = static_cast<const T*>(d.b[l]);
            const T* cb = static_cast<const T*>(d.cb[l]);
            if (b) v += to_f32<T>(b[c]);
            if (cb) v += to_f32<T>(cb[c]);
            out[(int64_t)N * d.row0[l] + (int64_t)lane * C + c] = from_f32<T>(v);
        }
    }
}

int check_time_proj(int N, int E, int dtype) {
    if (N < 1 || E < 1) return LORA_E_BADARG;
    if (dtype == LORA_F32) return LORA_E_UNSUPPORTED;
    if (dtype != LORA_F16 && dtype != LORA_BF16) return LORA_E_BADARG;
    if (N > 16 || E % 8) return LORA_E_UNSUPPORTED;
    return LORA_OK;
}

template <typename T, int NB> void launch_time_proj(const void* t, void* out, const TimeProjLayers& d, int N, int E, hipStream_t s) {
    const int rows = d.row0[d.L], per = kWaves * kRows;
    hipLaunchKernelGGL((time_proj_kernel<T, NB>), dim3((unsigned)((rows + per - 1) / per)), dim3(kWaves * 64), 0, s,
                       static_cast<const T*>(t), static_cast<T*>(out), d, N, E);
}

template <typename T> int run_time_proj(const void* t, void* out, const TimeProjLayers& d, int N, int E, hipStream_t s) {
    if (N <= 1) launch_time_proj<T, 1>(t, out, d, N, E, s);
    else if (N <= 2) launch_time_proj<T, 2>(t, out, d, N, E, s);
    else if (N <= 4) launch_time_proj<T, 4>(t, out, d, N, E, s);
    else if (N <= 8) launch_time_proj<T, 8>(t, out, d, N, E, s);
    else launch_time_proj<T, 16>(t, out, d, N, E, s);
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}

}  // namespace

extern "C" int time_proj_supported(int N, int E, int dtype) { return check_time_proj(N, E, dtype) == LORA_OK; }

extern "C" int time_proj_all(const void* t, const void* const* W, const void* const* b, const void* const* cb, const int* C, void* out,
                             int L, int N, int E, int dtype, void* stream) {
    if (!t || !W || !C || !out || L < 1) return LORA_E_BADARG;
    for (int l = 0; l < L; ++l)
        if (!W[l] || C[l] < 1) return LORA_E_BADARG;
    if (const int st = check_time_proj(N, E, dtype)) return st;
    for (int l0 = 0; l0 < L; l0 += kMaxLayers) {  // a launch's rows stay an int with room for the last workgroup's overhang
        int64_t rows = 0;
        for (int l = l0; l < L && l < l0 + kMaxLayers; ++l) rows += C[l];
        if (rows > INT_MAX - kWaves * kRows) return LORA_E_UNSUPPORTED;
    }
    if (!aligned16(t)) return LORA_E_ALIGN;
    for (int l = 0; l < L; ++l)
        if (!aligned16(W[l])) return LORA_E_ALIGN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t esize = 2;
    char* o = static_cast<char*>(out);
    for (int l0 = 0; l0 < L; l0 += kMaxLayers) {
        TimeProjLayers d = {};
        d.L = L - l0 < kMaxLayers ? L - l0 : kMaxLayers;
        for (int j = 0; j < d.L; ++j) {
            d.W[j] = W[l0 + j];
            d.b[j] = b ? b[l0 + j] : nullptr;
            d.cb[j] = cb ? cb[l0 + j] : nullptr;
            d.row0[j + 1] = d.row0[j] + C[l0 + j];
        }
        const int st = dtype == LORA_F16 ? run_time_proj<half_t>(t, o, d, N, E, s) : run_time_proj<bf16_t>(t, o, d, N, E, s);
        if (st) return st;
        o += (size_t)N * d.row0[d.L] * esize;
    }
    return LORA_OK;
}

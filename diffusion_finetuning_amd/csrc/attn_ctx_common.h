// What the single-key-tile attention kernels share (attn_ctx.hip: cross-attention over ≤ 128 keys; attn_causal.hip: its
// causal self-attention form): tile geometry, K/V staging, the in-register softmax and the ordered sum of the backward's per-workgroup
// dK/dV partials.
#pragma once
#include "attn_common.h"

namespace {

constexpr int kCtxSumFrags = 32;  // accumulator fragments per wave and phase of the backward's closing sum (4 × 32 KB of LDS)

template <int KS, int DF, int NKF> struct CtxShape {
    static constexpr int DP = KS * 32;       // head dim padded for the Q·Kᵀ contraction
    static constexpr int DV = DF * 16;       // head dim padded as an MFMA output extent
    static constexpr int NK = NKF * 16;      // keys padded
    // LDS row strides (halfs).  K/V/Q/dO tiles: +32 B — a stride ≡ 32 (mod 64) bytes is what makes the fragment reads
    // (ds_read_b128, serviced in the lane groups {0–3,12–15,20–27}, …) and the transposing reads (two groups of 32 lanes)
    // conflict-free on gfx950's 64 banks; +16 B made every one of them a 2-way conflict (attn_flash.hip, FlashShape).  P/dS
    // tiles: +32 B halves their transposing reads' conflicts (3-way → 2-way: four 8-byte pieces 16 bytes apart per row).
    static constexpr int KROW = DP + 16;
    static constexpr int TROW = NK + 16;
};

// K (or V) of one (batch, head) → registers: thread owns chunks idx = tid + i*256 of the [NK][DP/8] chunk grid
template <typename T, int KS, int DF, int NKF> struct StageRegs {
    using S = CtxShape<KS, DF, NKF>;
    static constexpr int CPR = S::DP / 8;
    static constexpr int N = S::NK * CPR;
    static constexpr int IT = (N + 255) / 256;
    Chunk<T> v[IT];
    __device__ __forceinline__ void load(const T* src, int64_t row_stride, int Tk, int d) {
#pragma unroll
        for (int i = 0; i < IT; ++i) {
            const int idx = threadIdx.x + i * 256;
            const int key = idx / CPR, c = (idx - key * CPR) * 8;
            const bool ok = idx < N && key < Tk && c < d;
            v[i] = load_or_zero<T>(ok ? src + key * row_stride + c : src, ok);
        }
    }
    // row-major [NK][KROW] (operand rows = keys), zero beyond Tk and d
    __device__ __forceinline__ void store_rows(T* dst) const {
#pragma unroll
        for (int i = 0; i < IT; ++i) {
            const int idx = threadIdx.x + i * 256;
            const int key = idx / CPR, c = (idx - key * CPR) * 8;
            if (idx < N) *reinterpret_cast<Chunk<T>*>(dst + key * S::KROW + c) = v[i];
        }
    }
};

// softmax over the keys of one query row held as Sᵀ accumulators (lane = query l15; keys nf*16 + lq*4 + r).
// In: raw scores.  Out: normalised probabilities in place; returns the row max (log2 domain) and 1/sum.
// Round 5 (the kernels are bound by vector issue; this routine was 60 % of the forward loop's instructions): the scale rides in the
// exponent's fma — p = exp2(fma(s, c, −c·max s)), c = scale·log2 e > 0, no separate multiply and subtract pass; the exponent is the bare
// v_exp_f32 (arguments ≤ 0: the library exp2f's denormal-range fix-ups were a compare, an ldexp and two selects per score); keys
// past Tk arrive masked: their scores START at −inf — key_mask() is the initial accumulator of the score chains (a per-lane constant,
// built once per kernel: "row constants as the initial accumulator", here a key constant), so masking costs the loop nothing.
template <int NKF>
__device__ __forceinline__ void key_mask(f32x4 (&k0)[NKF], int lq, int Tk) {
#pragma unroll
    for (int nf = 0; nf < NKF; ++nf)
#pragma unroll
        for (int r = 0; r < 4; ++r) k0[nf][r] = nf * 16 + lq * 4 + r >= Tk ? -INFINITY : 0.f;
}
template <int NKF>
__device__ __forceinline__ void softmax_rows(f32x4 (&s)[NKF], float scale_log2e, float& m, float& inv_l) {
    float mr = -INFINITY;
#pragma unroll
    for (int nf = 0; nf < NKF; ++nf) mr = fmaxf(mr, fmaxf(fmaxf(s[nf][0], s[nf][1]), fmaxf(s[nf][2], s[nf][3])));
    mr = fmaxf(mr, __shfl_xor(mr, 16, 64));
    mr = fmaxf(mr, __shfl_xor(mr, 32, 64));
    m = mr * scale_log2e;
    const float nm = -m;
    float l = 0.f;
#pragma unroll
    for (int nf = 0; nf < NKF; ++nf)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float p = __builtin_amdgcn_exp2f(fmaf(s[nf][r], scale_log2e, nm));  // exp2(−inf) = 0 for masked keys
            s[nf][r] = p;
            l += p;
        }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    inv_l = 1.f / l;
#pragma unroll
    for (int nf = 0; nf < NKF; ++nf)
#pragma unroll
        for (int r = 0; r < 4; ++r) s[nf][r] *= inv_l;
}

// dK/dV [B, Tk, H·d] = Σ_chunk partials, summed in chunk order (deterministic), cast to T.  A thread owns one 16-byte
// accumulator of the partial image (fragment order [tensor][nf][df][lane][r]: four consecutive keys of one head-dim column),
// so the partials — the bulk of the traffic — are read as whole coalesced lines; the four outputs go out as 2-byte stores
// into the (small) [B, Tk, H·d] gradients.  (The first form walked the OUTPUT in memory order and gathered 4 bytes out of
// every 16 of the partials: 7 – 9.5 µs per launch against 4 – 6 now.)
template <typename T>
__global__ __launch_bounds__(256) void attn_ctx_reduce_kernel(const float* __restrict__ part, T* __restrict__ dK,
                                                               T* __restrict__ dV, int B, int Tk, int H, int d,
                                                               int chunks, int slices, int NK, int DV, int64_t ld_dk) {
    const int per_img = (NK * DV) >> 2;                 // f32x4 per tensor of one partial
    const int64_t per_grp = 2 * (int64_t)per_img;       // ... per (batch, head, slice)
    const int64_t total = (int64_t)B * H * slices * per_grp;
    const int dfs = DV >> 4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t grp = i / per_grp;                // (b·H + h)·slices + sl
        const int e = (int)(i - grp * per_grp);
        const int ten = e >= per_img ? 1 : 0, f = e - ten * per_img;
        const int lane = f & 63, frag = f >> 6;
        const int nf = frag / dfs, df = frag - nf * dfs;
        const int sl = (int)(grp % slices);
        const int64_t bh = grp / slices;
        const int h = (int)(bh % H), b = (int)(bh / H);
        const int c = sl * DV + df * 16 + (lane & 15);
        const int key0 = nf * 16 + (lane >> 4) * 4;
        if (c >= d || key0 >= Tk) continue;
        // partial of chunk ch of this group: ((bh·chunks + ch)·slices + sl)·2·NK·DV floats
        const f32x4* p = reinterpret_cast<const f32x4*>(part + ((bh * chunks) * slices + sl) * 2 * (int64_t)NK * DV) + e;
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int ch = 0; ch < chunks; ++ch) acc += p[(int64_t)ch * slices * per_grp];
        T* out = (ten ? dV : dK) + ((int64_t)b * Tk + key0) * ld_dk + (int64_t)h * d + c;
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (key0 + r < Tk) out[(int64_t)r * ld_dk] = from_f32<T>(acc[r]);
    }
}

}  // namespace

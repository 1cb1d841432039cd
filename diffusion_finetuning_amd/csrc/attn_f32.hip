// fp32 attention core for gfx950:  O = softmax(Q·Kᵀ·scale)·V  per head on fp32 tensors, any number of queries and keys — the
// attention of the routes the reference runs in fp32 (diffusers CrossAttention.forward under cli_lora_pti.py:685,
// mixed_precision=False: PTI's textual-inversion phase; BASELINE config 1).  Layout contract of attn_flash_*: Q/O/dO/dQ
// [B, Tq, H·d], K/V/dK/dV [B, Tk, H·d] as to_q/to_k/to_v produce and to_out consumes them, no head split/merge, nothing of
// size Tq×Tk in memory.
//
// Every product runs on the exact f32-input MFMA v_mfma_f32_16x16x4_f32 (gfx950 has no xf32): lane l supplies A[l&15][l>>4]
// and B[l>>4][l&15] — ONE float each — and receives D[4·(l>>4) + r][l&15], r = 0..3.  Its result is a k-ordered fmaf chain.
//
// Forward / dQ (query-owned): a workgroup of four waves owns 64 query rows, a wave 16 of them, and walks the keys in tiles
// of 64 staged in LDS ([64][16·DF + 4] floats each for K and V; the + 4 makes both read patterns below conflict-free).
//   Sᵀ = K·Qᵀ   A = K[key l15][c], B = Q[query l15][c] with c = 16j + 4·lq + r for step r of column chunk j: both operands
//               are float4 reads (K from LDS, Q once from global into registers, pre-multiplied by scale·log2 e).  The lane
//               then holds S[query l15][key 16·nf + 4·lq + r]: a row's maximum and sum are a 16-register reduction and
//               two cross-lane steps (xor 16, 32); the running sum stays a per-lane partial until the end.
//   Oᵀ = Vᵀ·Pᵀ  B = P[query l15][key 4·lq + r] is the lane's own register r — P never goes through LDS — and
//               A = V[key 4·lq + r][16·df + l15] one float from LDS.  The lane receives O[query l15][16·df + 4·lq + r]: the
//               online rescale is per lane, the store one float4.
// dQ recomputes P = exp2(S − LSE), forms dPᵀ = V·dOᵀ the way Sᵀ is formed, dS = P·(dP − Δ)·scale, dQᵀ = Kᵀ·dSᵀ the way Oᵀ
// is formed, and writes Δ = Σ dO·O per query row for the key-owned launch.
// dK/dV (key-owned): a wave owns 16 keys (K pre-multiplied by scale·log2 e, V in registers) and walks the queries in tiles
// of 64 (Q, dO, LSE, Δ in LDS).  S = Q·Kᵀ and dP = dO·Vᵀ leave the lane with [query 16·nq + 4·lq + r][key l15], the B
// operand of dVᵀ = dOᵀ·P and dKᵀ = Qᵀ·dS, whose results are float4 stores of the lane's key row.
// Every output element has one owner; no atomics; run-to-run bit-identical.  Four independent score accumulators and DF
// independent output accumulators per wave cover the MFMA's 40-cycle dependent latency.
#include "common.h"

namespace {

constexpr int kF32Tile = 64;  // rows per LDS tile (keys in forward / dQ, queries in dK/dV) and query / key rows per workgroup

template <int DF> struct F32Shape {
    static constexpr int DP = DF * 16;  // head dim rounded up to the instantiation's width (columns d.. are zeros)
    static constexpr int ROW = DP + 4;  // LDS row stride in floats: rows 4 apart land 16 banks apart, rows 1 apart 4 banks
};

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// rows r0 .. r0+63 of the head's [T, d] slice (row stride ld) → dst [64][ROW]; zeros past row T and past column d
template <int DF>
__device__ __forceinline__ void stage_tile(float* dst, const float* __restrict__ src, int64_t ld, int r0, int T, int d) {
    constexpr int C4 = DF * 4;  // 16-byte chunks per row
#pragma unroll
    for (int i = 0; i < DF; ++i) {  // 64·C4 chunks over 256 threads
        const int e = i * 256 + threadIdx.x;
        const int row = e / C4, c = (e - row * C4) * 4;
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (r0 + row < T && c < d) v = *reinterpret_cast<const f32x4*>(src + (int64_t)(r0 + row) * ld + c);
        *reinterpret_cast<f32x4*>(dst + row * F32Shape<DF>::ROW + c) = v;
    }
}

// the lane's share of one row: columns 16j + 4·lq .. + 3 for every chunk j, times mul; zeros for an absent row or column
template <int DF>
__device__ __forceinline__ void load_row(f32x4 (&f)[DF], const float* __restrict__ row, bool valid, int d, int lq, float mul) {
#pragma unroll
    for (int j = 0; j < DF; ++j) {
        const int c = j * 16 + lq * 4;
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (valid && c < d) v = *reinterpret_cast<const f32x4*>(row + c);
        f[j] = v * mul;
    }
}

template <int DF>
__device__ __forceinline__ void store_row(float* __restrict__ row, const f32x4 (&f)[DF], bool valid, int d, int lq, float mul) {
#pragma unroll
    for (int j = 0; j < DF; ++j) {
        const int c = j * 16 + lq * 4;
        if (valid && c < d) *reinterpret_cast<f32x4*>(row + c) = f[j] * mul;
    }
}

__device__ __forceinline__ float quad_sum(float v) {  // over the four lanes that share l15
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}

// initial accumulators of the four score fragments of a key tile: −inf for the lane's keys at or past Tk
__device__ __forceinline__ void key_mask(f32x4 (&s)[4], int k0, int lq, int Tk) {
#pragma unroll
    for (int nf = 0; nf < 4; ++nf)
#pragma unroll
        for (int r = 0; r < 4; ++r) s[nf][r] = k0 + nf * 16 + lq * 4 + r < Tk ? 0.f : -INFINITY;
}

template <int DF>
__global__ __launch_bounds__(256) void attn_f32_fwd_kernel(const float* __restrict__ Q, const float* __restrict__ K,
                                                            const float* __restrict__ V, float* __restrict__ O,
                                                            float* __restrict__ LSE, int Tq, int Tk, int H, int d,
                                                            float scale_log2e, int qblocks) {
    using S = F32Shape<DF>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* Ks = reinterpret_cast<float*>(smem);  // [64][ROW]
    float* Vs = Ks + kF32Tile * S::ROW;           // [64][ROW]

    const int qb = blockIdx.x % qblocks, bh = blockIdx.x / qblocks;
    const int b = bh / H, h = bh - b * H;
    const int64_t HD = (int64_t)H * d;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, lq = lane >> 4;
    const int t = qb * kF32Tile + wave * 16 + l15;
    const bool valid = t < Tq;
    const float* Kh = K + (int64_t)b * Tk * HD + h * d;
    const float* Vh = V + (int64_t)b * Tk * HD + h * d;

    f32x4 qf[DF], o[DF];
    load_row<DF>(qf, Q + ((int64_t)b * Tq + t) * HD + h * d, valid, d, lq, scale_log2e);
#pragma unroll
    for (int df = 0; df < DF; ++df) o[df] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;  // running row maximum (log2 units); the lane's partial of the running row sum

    for (int k0 = 0; k0 < Tk; k0 += kF32Tile) {
        __syncthreads();  // the previous tile has been read
        stage_tile<DF>(Ks, Kh, HD, k0, Tk, d);
        stage_tile<DF>(Vs, Vh, HD, k0, Tk, d);
        __syncthreads();

        f32x4 s[4];
        key_mask(s, k0, lq, Tk);
#pragma unroll
        for (int j = 0; j < DF; ++j) {
            f32x4 kf[4];
#pragma unroll
            for (int nf = 0; nf < 4; ++nf)
                kf[nf] = *reinterpret_cast<const f32x4*>(Ks + (nf * 16 + l15) * S::ROW + j * 16 + lq * 4);
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int nf = 0; nf < 4; ++nf) s[nf] = mfma4(kf[nf][r], qf[j][r], s[nf]);
        }
        float mt = -INFINITY;
#pragma unroll
        for (int nf = 0; nf < 4; ++nf) mt = fmaxf(mt, fmaxf(fmaxf(s[nf][0], s[nf][1]), fmaxf(s[nf][2], s[nf][3])));
        mt = fmaxf(mt, __shfl_xor(mt, 16, 64));
        mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
        const float mn = fmaxf(m, mt);  // finite: every tile holds at least one key
        const float alpha = __builtin_amdgcn_exp2f(m - mn);  // 0 at the first tile
        m = mn;
        float lt = 0.f;
#pragma unroll
        for (int nf = 0; nf < 4; ++nf)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = __builtin_amdgcn_exp2f(s[nf][r] - mn);  // exp2(−inf) = 0 past Tk
                s[nf][r] = p;
                lt += p;
            }
        l = fmaf(l, alpha, lt);
#pragma unroll
        for (int df = 0; df < DF; ++df) o[df] *= alpha;
#pragma unroll
        for (int nf = 0; nf < 4; ++nf)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float* vrow = Vs + (nf * 16 + lq * 4 + r) * S::ROW + l15;
#pragma unroll
                for (int df = 0; df < DF; ++df) o[df] = mfma4(vrow[df * 16], s[nf][r], o[df]);
            }
    }
    l = quad_sum(l);
    store_row<DF>(O + ((int64_t)b * Tq + t) * HD + h * d, o, valid, d, lq, 1.f / l);
    if (LSE != nullptr && valid && lq == 0) LSE[((int64_t)b * H + h) * Tq + t] = m + __builtin_amdgcn_logf(l);  // v_log_f32 = log2
}

template <int DF>
__global__ __launch_bounds__(256) void attn_f32_dq_kernel(const float* __restrict__ Q, const float* __restrict__ K,
                                                           const float* __restrict__ V, const float* __restrict__ O,
                                                           const float* __restrict__ dO, const float* __restrict__ LSE,
                                                           float* __restrict__ dQ, float* __restrict__ Delta, int Tq, int Tk,
                                                           int H, int d, float scale, float scale_log2e, int qblocks) {
    using S = F32Shape<DF>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* Ks = reinterpret_cast<float*>(smem);
    float* Vs = Ks + kF32Tile * S::ROW;

    const int qb = blockIdx.x % qblocks, bh = blockIdx.x / qblocks;
    const int b = bh / H, h = bh - b * H;
    const int64_t HD = (int64_t)H * d;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, lq = lane >> 4;
    const int t = qb * kF32Tile + wave * 16 + l15;
    const bool valid = t < Tq;
    const int64_t row = ((int64_t)b * Tq + t) * HD + h * d;
    const float* Kh = K + (int64_t)b * Tk * HD + h * d;
    const float* Vh = V + (int64_t)b * Tk * HD + h * d;

    f32x4 qf[DF], gf[DF], g[DF];
    load_row<DF>(qf, Q + row, valid, d, lq, scale_log2e);
    load_row<DF>(gf, dO + row, valid, d, lq, 1.f);
    // Δ = Σ_c dO·O of the row, summed by the MFMA in the order dP's products are summed below (the diagonal of O·dOᵀ): where
    // a row's O is one V row — a single key — Δ equals dP bit for bit and dS is exactly 0, as the stock softmax backward gives
    float delta;
    {
        f32x4 of[DF], dd = f32x4{0.f, 0.f, 0.f, 0.f};
        load_row<DF>(of, O + row, valid, d, lq, 1.f);
#pragma unroll
        for (int j = 0; j < DF; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) dd = mfma4(of[j][r], gf[j][r], dd);  // dd[r] = Σ_c O[row 4·lq + r]·dO[row l15]
        const int r = l15 & 3;
        const float mine = r == 0 ? dd[0] : r == 1 ? dd[1] : r == 2 ? dd[2] : dd[3];
        delta = quad_sum((l15 >> 2) == lq ? mine : 0.f);  // one of the four lanes holds the diagonal element
    }
    if (valid && lq == 0) Delta[((int64_t)b * H + h) * Tq + t] = delta;
    const float lse = valid ? LSE[((int64_t)b * H + h) * Tq + t] : 0.f;  // (an absent row: Q = dO = 0, so dS = 0 whatever P is)
#pragma unroll
    for (int df = 0; df < DF; ++df) g[df] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int k0 = 0; k0 < Tk; k0 += kF32Tile) {
        __syncthreads();
        stage_tile<DF>(Ks, Kh, HD, k0, Tk, d);
        stage_tile<DF>(Vs, Vh, HD, k0, Tk, d);
        __syncthreads();

        f32x4 s[4], dp[4];
        key_mask(s, k0, lq, Tk);
#pragma unroll
        for (int nf = 0; nf < 4; ++nf) dp[nf] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < DF; ++j) {
            f32x4 kf[4], vf[4];
#pragma unroll
            for (int nf = 0; nf < 4; ++nf) {
                const int off = (nf * 16 + l15) * S::ROW + j * 16 + lq * 4;
                kf[nf] = *reinterpret_cast<const f32x4*>(Ks + off);
                vf[nf] = *reinterpret_cast<const f32x4*>(Vs + off);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int nf = 0; nf < 4; ++nf) {
                    s[nf] = mfma4(kf[nf][r], qf[j][r], s[nf]);
                    dp[nf] = mfma4(vf[nf][r], gf[j][r], dp[nf]);
                }
        }
#pragma unroll
        for (int nf = 0; nf < 4; ++nf)
#pragma unroll
            for (int r = 0; r < 4; ++r)  // dS; exactly 0 past Tk (P = exp2(−inf), dP finite: V's rows there are zeros)
                s[nf][r] = __builtin_amdgcn_exp2f(s[nf][r] - lse) * (dp[nf][r] - delta) * scale;
#pragma unroll
        for (int nf = 0; nf < 4; ++nf)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float* krow = Ks + (nf * 16 + lq * 4 + r) * S::ROW + l15;
#pragma unroll
                for (int df = 0; df < DF; ++df) g[df] = mfma4(krow[df * 16], s[nf][r], g[df]);
            }
    }
    store_row<DF>(dQ + row, g, valid, d, lq, 1.f);
}

template <int DF>
__global__ __launch_bounds__(256) void attn_f32_dkdv_kernel(const float* __restrict__ Q, const float* __restrict__ K,
                                                             const float* __restrict__ V, const float* __restrict__ dO,
                                                             const float* __restrict__ LSE, const float* __restrict__ Delta,
                                                             float* __restrict__ dK, float* __restrict__ dV, int Tq, int Tk,
                                                             int H, int d, float scale, float scale_log2e, int kblocks) {
    using S = F32Shape<DF>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* Qs = reinterpret_cast<float*>(smem);  // [64][ROW]
    float* Gs = Qs + kF32Tile * S::ROW;           // [64][ROW]  dO
    float* Ls = Gs + kF32Tile * S::ROW;           // [64] LSE of the tile's rows (+inf for an absent row: P = 0)
    float* Ds = Ls + kF32Tile;                    // [64] Δ

    const int kb = blockIdx.x % kblocks, bh = blockIdx.x / kblocks;
    const int b = bh / H, h = bh - b * H;
    const int64_t HD = (int64_t)H * d;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, lq = lane >> 4;
    const int key = kb * kF32Tile + wave * 16 + l15;
    const bool valid = key < Tk;
    const int64_t row = ((int64_t)b * Tk + key) * HD + h * d;
    const float* Qh = Q + (int64_t)b * Tq * HD + h * d;
    const float* Gh = dO + (int64_t)b * Tq * HD + h * d;
    const float* Lh = LSE + ((int64_t)b * H + h) * Tq;
    const float* Dh = Delta + ((int64_t)b * H + h) * Tq;

    f32x4 kf[DF], vf[DF], dk[DF], dv[DF];
    load_row<DF>(kf, K + row, valid, d, lq, scale_log2e);
    load_row<DF>(vf, V + row, valid, d, lq, 1.f);
#pragma unroll
    for (int df = 0; df < DF; ++df) dk[df] = dv[df] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int q0 = 0; q0 < Tq; q0 += kF32Tile) {
        __syncthreads();
        stage_tile<DF>(Qs, Qh, HD, q0, Tq, d);
        stage_tile<DF>(Gs, Gh, HD, q0, Tq, d);
        if (threadIdx.x < kF32Tile) {
            const int t = q0 + threadIdx.x;
            Ls[threadIdx.x] = t < Tq ? Lh[t] : INFINITY;
            Ds[threadIdx.x] = t < Tq ? Dh[t] : 0.f;
        }
        __syncthreads();

        f32x4 s[4], dp[4];
#pragma unroll
        for (int nq = 0; nq < 4; ++nq) s[nq] = dp[nq] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < DF; ++j) {
            f32x4 qa[4], ga[4];
#pragma unroll
            for (int nq = 0; nq < 4; ++nq) {
                const int off = (nq * 16 + l15) * S::ROW + j * 16 + lq * 4;
                qa[nq] = *reinterpret_cast<const f32x4*>(Qs + off);
                ga[nq] = *reinterpret_cast<const f32x4*>(Gs + off);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int nq = 0; nq < 4; ++nq) {
                    s[nq] = mfma4(qa[nq][r], kf[j][r], s[nq]);
                    dp[nq] = mfma4(ga[nq][r], vf[j][r], dp[nq]);
                }
        }
        // the lane holds [query 16·nq + 4·lq + r][key l15]:  s → P,  dp → dS
#pragma unroll
        for (int nq = 0; nq < 4; ++nq) {
            const f32x4 ls = *reinterpret_cast<const f32x4*>(Ls + nq * 16 + lq * 4);
            const f32x4 dl = *reinterpret_cast<const f32x4*>(Ds + nq * 16 + lq * 4);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = valid ? __builtin_amdgcn_exp2f(s[nq][r] - ls[r]) : 0.f;
                s[nq][r] = p;
                dp[nq][r] = p * (dp[nq][r] - dl[r]) * scale;
            }
        }
#pragma unroll
        for (int nq = 0; nq < 4; ++nq)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int off = (nq * 16 + lq * 4 + r) * S::ROW + l15;
#pragma unroll
                for (int df = 0; df < DF; ++df) {
                    dv[df] = mfma4(Gs[off + df * 16], s[nq][r], dv[df]);
                    dk[df] = mfma4(Qs[off + df * 16], dp[nq][r], dk[df]);
                }
            }
    }
    store_row<DF>(dK + row, dk, valid, d, lq, 1.f);
    store_row<DF>(dV + row, dv, valid, d, lq, 1.f);
}

// The instantiation for a head dim: the narrowest compiled width 16·DF that holds it.
int plan_f32(int B, int Tq, int Tk, int H, int d) {
    if (B < 1 || Tq < 1 || Tk < 1 || H < 1 || d < 8 || (d % 8) != 0 || d > 160) return 0;
    const int64_t qblocks = ((int64_t)Tq + kF32Tile - 1) / kF32Tile, kblocks = ((int64_t)Tk + kF32Tile - 1) / kF32Tile;
    if ((int64_t)B * H * qblocks > 0x7fffffff || (int64_t)B * H * kblocks > 0x7fffffff) return 0;  // one grid dimension
    if (d <= 32) return 2;
    if (d <= 48) return 3;
    if (d <= 64) return 4;
    if (d <= 96) return 6;
    if (d <= 128) return 8;
    return 10;
}

template <int DF> constexpr int f32_lds() { return (2 * kF32Tile * F32Shape<DF>::ROW + 2 * kF32Tile) * 4; }

struct F32Args {
    const float *Q, *K, *V, *O, *dO, *LSE;
    float *Out, *Lse, *dQ, *dK, *dV, *ws;
    int B, Tq, Tk, H, d;
    float scale;
};

template <typename Kern> bool f32_allow_lds(Kern kern, int lds) {
    return lds <= 48 * 1024 ||
           hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds) == hipSuccess;
}

template <int DF, bool BWD> int launch_f32(const F32Args& a, hipStream_t stream) {
    constexpr int lds = f32_lds<DF>();
    const float l2e = a.scale * 1.4426950408889634f;
    const int qblocks = (a.Tq + kF32Tile - 1) / kF32Tile, kblocks = (a.Tk + kF32Tile - 1) / kF32Tile;
    if constexpr (!BWD) {
        static const bool ok = f32_allow_lds(attn_f32_fwd_kernel<DF>, lds);
        if (!ok) return LORA_E_LAUNCH;
        LORA_LAUNCH(PK_FLASH_FWD, attn_f32_fwd_kernel<DF>, dim3((unsigned)(a.B * a.H * qblocks)), dim3(256), lds, stream, a.Q,
                    a.K, a.V, a.Out, a.Lse, a.Tq, a.Tk, a.H, a.d, l2e, qblocks);
        LORA_LAUNCH_CHECK();
    } else {
        static const bool ok = f32_allow_lds(attn_f32_dq_kernel<DF>, lds) && f32_allow_lds(attn_f32_dkdv_kernel<DF>, lds);
        if (!ok) return LORA_E_LAUNCH;
        LORA_LAUNCH(PK_FLASH_DQ, attn_f32_dq_kernel<DF>, dim3((unsigned)(a.B * a.H * qblocks)), dim3(256), lds, stream, a.Q, a.K,
                    a.V, a.O, a.dO, a.LSE, a.dQ, a.ws, a.Tq, a.Tk, a.H, a.d, a.scale, l2e, qblocks);
        LORA_LAUNCH_CHECK();
        LORA_LAUNCH(PK_FLASH_DKDV, attn_f32_dkdv_kernel<DF>, dim3((unsigned)(a.B * a.H * kblocks)), dim3(256), lds, stream, a.Q,
                    a.K, a.V, a.dO, a.LSE, static_cast<const float*>(a.ws), a.dK, a.dV, a.Tq, a.Tk, a.H, a.d, a.scale, l2e,
                    kblocks);
        LORA_LAUNCH_CHECK();
    }
    return LORA_OK;
}

template <bool BWD> int dispatch_f32(const F32Args& a, hipStream_t stream) {
    const int df = plan_f32(a.B, a.Tq, a.Tk, a.H, a.d);
#define F32_CASE(DF_) \
    if (df == DF_) return launch_f32<DF_, BWD>(a, stream);
    F32_CASE(2) F32_CASE(3) F32_CASE(4) F32_CASE(6) F32_CASE(8) F32_CASE(10)
#undef F32_CASE
    return LORA_E_BADARG;
}

}  // namespace

extern "C" int attn_f32_supported(int B, int Tq, int Tk, int H, int d) { return plan_f32(B, Tq, Tk, H, d) != 0 ? 1 : 0; }

extern "C" int attn_f32_fwd(const float* Q, const float* K, const float* V, float* O, float* LSE, int B, int Tq, int Tk, int H,
                            int d, float scale, void* stream) {
    if (!Q || !K || !V || !O) return LORA_E_BADARG;
    if (plan_f32(B, Tq, Tk, H, d) == 0) return LORA_E_BADARG;
    if (!aligned16(Q) || !aligned16(K) || !aligned16(V) || !aligned16(O)) return LORA_E_ALIGN;
    F32Args a{};
    a.Q = Q; a.K = K; a.V = V; a.Out = O; a.Lse = LSE; a.B = B; a.Tq = Tq; a.Tk = Tk; a.H = H; a.d = d; a.scale = scale;
    return dispatch_f32<false>(a, static_cast<hipStream_t>(stream));
}

extern "C" int64_t attn_f32_bwd_workspace_bytes(int B, int Tq, int H) {
    if (B < 1 || Tq < 1 || H < 1) return -1;
    return (int64_t)B * H * Tq * 4;
}

extern "C" int attn_f32_bwd(const float* Q, const float* K, const float* V, const float* O, const float* dO, const float* LSE,
                            float* dQ, float* dK, float* dV, float* workspace, int B, int Tq, int Tk, int H, int d, float scale,
                            void* stream) {
    if (!Q || !K || !V || !O || !dO || !LSE || !dQ || !dK || !dV || !workspace) return LORA_E_BADARG;
    if (plan_f32(B, Tq, Tk, H, d) == 0) return LORA_E_BADARG;
    if (!aligned16(Q) || !aligned16(K) || !aligned16(V) || !aligned16(O) || !aligned16(dO) || !aligned16(dQ) || !aligned16(dK) ||
        !aligned16(dV))
        return LORA_E_ALIGN;
    F32Args a{};
    a.Q = Q; a.K = K; a.V = V; a.O = O; a.dO = dO; a.LSE = LSE; a.dQ = dQ; a.dK = dK; a.dV = dV; a.ws = workspace;
    a.B = B; a.Tq = Tq; a.Tk = Tk; a.H = H; a.d = d; a.scale = scale;
    return dispatch_f32<true>(a, static_cast<hipStream_t>(stream));
}

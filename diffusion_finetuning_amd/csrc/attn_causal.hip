// Causal short-context attention core for gfx950:  O = softmax(mask(Q·Kᵀ·scale))·V  per head with mask(i, j) = −inf for
// j > i, self-attention over at most 128 tokens — the text encoder's attention (transformers CLIPAttention.forward, the
// caller of the q_proj/k_proj/v_proj/out_proj LoRA linears wrapped per lora_diffusion/lora.py:54; 77 tokens, heads of 64).
//
// Same structure as attn_ctx.hip (attn_ctx_common.h holds what the two share): K/V of one (batch, head) in LDS, a wave per
// block of 16 query rows, Sᵀ = K·Qᵀ so that a lane owns one query row and 4 consecutive keys per fragment, P fed to the
// next MFMA from registers; backward recomputes P, uses Σ_key P·dP for the softmax correction, writes dQ directly and
// leaves dK/dV as per-workgroup fp32 partials that attn_ctx_reduce_kernel folds in chunk order.  No atomics.
//
// The triangle: query blocks start at multiples of 16 (plan_causal: chunks of 64 or 128 rows, a wave's blocks 64 apart), so
// for the block at row t0 the key fragments nf < t0/16 are fully visible, fragment nd = t0/16 is the diagonal one and every
// fragment above it is masked whole.  The diagonal fragment's mask — key lq*4 + r against query l15 — does not depend on
// the block: it is a per-lane constant and the INITIAL ACCUMULATOR of that fragment's score chain, like key_mask() of
// attn_ctx.hip.  Fragments above the diagonal are skipped with branches on nd, which is wave-uniform (the wave index goes
// through readfirstlane, so the branches are scalar and EXEC stays all ones for the transposing LDS reads): no Q·Kᵀ, no
// exponentials, no P·V, no dP, no dS·K and no dK/dV products for them — at 77 tokens 15 of 30 (block, fragment) pairs.
// Their probabilities are exact zeros wherever a neighbour reads them (the upper half of a 32-key operand pair), so dS
// there is exactly 0.  Keys past T need no mask of their own: a valid row never sees them, and the rows past T of the last
// block carry Q = dO = 0 and are not stored.
//
// Q, K, V share one row stride (dense, or the three column slices of a grouped projection's [B·T, 3·H·d] buffer), dQ, dK,
// dV another; O and dO are dense.
#include "attn_ctx_common.h"

namespace {

// mask of the diagonal fragment: the lane's keys lq*4 + r against its query row l15
__device__ __forceinline__ f32x4 diag_mask(int l15, int lq) {
    f32x4 m;
#pragma unroll
    for (int r = 0; r < 4; ++r) m[r] = lq * 4 + r > l15 ? -INFINITY : 0.f;
    return m;
}

// softmax_rows() over the fragments 0 … nd of a block (nd wave-uniform); the fragments above come back as exact zeros
template <int NKF>
__device__ __forceinline__ void softmax_rows_causal(f32x4 (&s)[NKF], int nd, float scale_log2e, float& inv_l) {
    float mr = -INFINITY;
#pragma unroll
    for (int nf = 0; nf < NKF; ++nf)
        if (nf <= nd) mr = fmaxf(mr, fmaxf(fmaxf(s[nf][0], s[nf][1]), fmaxf(s[nf][2], s[nf][3])));
    mr = fmaxf(mr, __shfl_xor(mr, 16, 64));
    mr = fmaxf(mr, __shfl_xor(mr, 32, 64));  // finite: a row always sees its own key
    const float nm = -mr * scale_log2e;
    float l = 0.f;
#pragma unroll
    for (int nf = 0; nf < NKF; ++nf)
        if (nf <= nd) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = __builtin_amdgcn_exp2f(fmaf(s[nf][r], scale_log2e, nm));  // exp2(−inf) = 0 past the diagonal
                s[nf][r] = p;
                l += p;
            }
        }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    inv_l = 1.f / l;
#pragma unroll
    for (int nf = 0; nf < NKF; ++nf)
#pragma unroll
        for (int r = 0; r < 4; ++r) s[nf][r] = nf <= nd ? s[nf][r] * inv_l : 0.f;
}

template <typename T, int KS, int DF, int NKF>
__global__ __launch_bounds__(256) void attn_causal_fwd_kernel(const T* __restrict__ Q, const T* __restrict__ K,
                                                               const T* __restrict__ V, T* __restrict__ O, int Tn, int H,
                                                               int d, float scale_log2e, int rq, int chunks, int64_t ldq) {
    using S = CtxShape<KS, DF, NKF>;
    using F8 = typename Mma<T>::F8;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* Ks = reinterpret_cast<T*>(smem);          // [NK][KROW]
    T* Vs = Ks + S::NK * S::KROW;                 // [NK][KROW]  row-major; Vᵀ fragments by transposing LDS reads

    const int chunk = blockIdx.x % chunks;
    const int bh = blockIdx.x / chunks;
    const int b = bh / H, h = bh - b * H;
    const int64_t HD = (int64_t)H * d;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l15 = lane & 15, lq = lane >> 4;
    const int row_end = min(Tn, (chunk + 1) * rq);  // (also the number of keys this chunk's rows can see)

    {
        StageRegs<T, KS, DF, NKF> kr, vr;  // both tensors in flight before the first LDS write; zero from key row_end on
        kr.load(K + (int64_t)b * Tn * ldq + h * d, ldq, row_end, d);
        vr.load(V + (int64_t)b * Tn * ldq + h * d, ldq, row_end, d);
        kr.store_rows(Ks);
        vr.store_rows(Vs);
    }
    __syncthreads();

    const T* Qh = Q + (int64_t)b * Tn * ldq + h * d;
    F8 qf[KS];
    {
        const int t = chunk * rq + wave * 16 + l15;
        load_row_frags<T, KS>(Qh + (int64_t)t * ldq, Qh, t < row_end, d, lq, qf);
    }
    const f32x4 dmask = diag_mask(l15, lq);
    const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int t0 = chunk * rq + wave * 16; t0 < row_end; t0 += 64) {
        const int nd = __builtin_amdgcn_readfirstlane(t0 >> 4);  // the diagonal fragment (t0 is a multiple of 16: plan_causal)
        const int t = t0 + l15;
        const bool valid = t < row_end;
        F8 qn[KS];  // next block's rows: in flight while this block is computed
        load_row_frags<T, KS>(Qh + (int64_t)(t + 64) * ldq, Qh, t + 64 < row_end, d, lq, qn);

        f32x4 s[NKF];
#pragma unroll
        for (int nf = 0; nf < NKF; ++nf) {
            s[nf] = nf == nd ? dmask : zero;
            if (nf <= nd) {
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const F8 kf = *reinterpret_cast<const F8*>(Ks + (nf * 16 + l15) * S::KROW + ks * 32 + lq * 8);
                    s[nf] = Mma<T>::k32(kf, qf[ks], s[nf]);
                }
            }
        }
        float inv_l;
        softmax_rows_causal<NKF>(s, nd, scale_log2e, inv_l);

        f32x4 o[DF];
#pragma unroll
        for (int df = 0; df < DF; ++df) o[df] = zero;
#pragma unroll
        for (int kk = 0; kk < NKF / 2; ++kk) {
            if (2 * kk <= nd) {  // (fragment 2kk + 1 may lie above the diagonal: its probabilities are zeros, its V rows finite)
                const F8 pf = pair_frag<T>(s[2 * kk], s[2 * kk + 1]);
#pragma unroll
                for (int df = 0; df < DF; ++df) {
                    // lane = head-dim column; slots = keys kk*32 + {0,16} + lq*4 + (0..3), the order of the P registers
                    const F8 vf = tr_pair<T>(lds_tr_block(Vs + (kk * 32) * S::KROW + df * 16, S::KROW, lane),
                                             lds_tr_block(Vs + (kk * 32 + 16) * S::KROW + df * 16, S::KROW, lane));
                    o[df] = Mma<T>::k32(vf, pf, o[df]);
                }
            }
        }
        T* orow = O + ((int64_t)b * Tn + t) * HD + h * d;
#pragma unroll
        for (int df = 0; df < DF; ++df) {
            const int c = df * 16 + lq * 4;  // the lane owns head-dim values c..c+3 of query row t
            if (valid && c < d) {
                Quad4<T> out;
#pragma unroll
                for (int r = 0; r < 4; ++r) out.v[r] = from_f32<T>(o[df][r]);
                *reinterpret_cast<Quad4<T>*>(orow + c) = out;
            }
        }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) qf[ks] = qn[ks];
    }
}

// Closing sum of the backward kernel: the four waves' dK/dV accumulators (lane = head-dim column l15 of fragment
// df; keys nf*16 + lq*4 + r) → one fp32 partial image per workgroup (of the [grid.x][grid.y] images at `part`), fragment order [tensor][nf][df][lane][r].
// The scheme of attn_ctx_bwd_kernel's closing sum (kept inline there: as a shared function it changed that kernel's register
// allocation): all four waves deposit a run of accumulator fragments in LDS at once (one image per wave, fragment order
// [fragment][lane][r], whole 16-byte accumulators), then all 256 threads add the four images — ((w0 + w1) + w2) + w3 — and
// store the sums straight to the global partial.
// `red` overlays the kernel's staging buffers (4 · CH · 64 · 16 bytes: bwd_lds()).
template <int NKF, int DF>
__device__ __forceinline__ void sum_wave_images(const f32x4 (&dk)[NKF][DF], const f32x4 (&dv)[NKF][DF], float* red,
                                                float* part, int wave, int lane) {
    __syncthreads();  // staging buffers are dead
    constexpr int F = 2 * NKF * DF;                  // fragments per wave: dk then dv
    constexpr int PH = (F + kCtxSumFrags - 1) / kCtxSumFrags;
    constexpr int CH = (F + PH - 1) / PH;            // fragments per phase (≤ kCtxSumFrags)
    f32x4* img = reinterpret_cast<f32x4*>(red);      // [4 waves][CH][64]
    float* out = part + ((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * 2 * (NKF * 16) * (DF * 16);
#pragma unroll
    for (int ph = 0; ph < PH; ++ph) {
#pragma unroll
        for (int fl = 0; fl < CH; ++fl) {
            const int f = ph * CH + fl;  // compile-time after unrolling
            if (f < F) {
                const int ten = f / (NKF * DF), rem = f - ten * (NKF * DF);
                img[(wave * CH + fl) * 64 + lane] = ten == 0 ? dk[rem / DF][rem % DF] : dv[rem / DF][rem % DF];
            }
        }
        __syncthreads();
        const int n_here = (F - ph * CH < CH ? F - ph * CH : CH) * 64;
        for (int e = threadIdx.x; e < n_here; e += 256) {
            const f32x4 v = ((img[e] + img[CH * 64 + e]) + img[2 * CH * 64 + e]) + img[3 * CH * 64 + e];
            *reinterpret_cast<f32x4*>(out + ((int64_t)(ph * CH) * 64 + e) * 4) = v;
        }
        if (ph + 1 < PH) __syncthreads();
    }
}

template <typename T, int KS, int DF, int NKF>
__global__ __launch_bounds__(256) void attn_causal_bwd_kernel(const T* __restrict__ Q, const T* __restrict__ K,
                                                               const T* __restrict__ V, const T* __restrict__ dO,
                                                               T* __restrict__ dQ, float* __restrict__ part, int Tn, int H,
                                                               int d, float scale, float scale_log2e, int rq, int chunks,
                                                               int64_t ldq, int64_t ld_dq) {
    using S = CtxShape<KS, DF, NKF>;
    using F8 = typename Mma<T>::F8;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    T* Ks = reinterpret_cast<T*>(smem);          // [NK][KROW]   rows = keys, for Sᵀ and S
    T* Vs = Ks + S::NK * S::KROW;                 // [NK][KROW]   rows = keys, for dPᵀ and dP
    T* Qw = Vs + S::NK * S::KROW + wave * 2 * 16 * S::KROW;  // this wave's [16][KROW] copy of its Q rows
    T* Gw = Qw + 16 * S::KROW;                    //                            ... and of its dO rows
    T* Pw = Vs + S::NK * S::KROW + 4 * 2 * 16 * S::KROW + wave * 2 * 16 * S::TROW;  // wave's P  [16][TROW]
    T* Sw = Pw + 16 * S::TROW;                                                        // wave's dS [16][TROW]
    float* red = reinterpret_cast<float*>(smem);  // overlay after the main loop: the waves' accumulator images

    const int chunk = blockIdx.x % chunks;
    const int bh = blockIdx.x / chunks;
    const int b = bh / H, h = bh - b * H;
    const int64_t HD = (int64_t)H * d;
    const int l15 = lane & 15, lq = lane >> 4;
    const int row_end = min(Tn, (chunk + 1) * rq);

    {
        StageRegs<T, KS, DF, NKF> kr, vr;  // zero from key row_end on: no row of this chunk sees those
        kr.load(K + (int64_t)b * Tn * ldq + h * d, ldq, row_end, d);
        vr.load(V + (int64_t)b * Tn * ldq + h * d, ldq, row_end, d);
        kr.store_rows(Ks);
        vr.store_rows(Vs);
    }
    __syncthreads();

    const f32x4 zero = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 dk[NKF][DF], dv[NKF][DF];  // lane = head-dim column l15 of fragment df; keys nf*16 + lq*4 + r
#pragma unroll
    for (int nf = 0; nf < NKF; ++nf)
#pragma unroll
        for (int df = 0; df < DF; ++df) dk[nf][df] = dv[nf][df] = zero;

    const T* Qh = Q + (int64_t)b * Tn * ldq + h * d;
    const T* Gh = dO + (int64_t)b * Tn * HD + h * d;
    F8 qf[KS], gf[KS];
    {
        const int t = chunk * rq + wave * 16 + l15;
        load_row_frags<T, KS>(Qh + (int64_t)t * ldq, Qh, t < row_end, d, lq, qf);
        load_row_frags<T, KS>(Gh + (int64_t)t * HD, Gh, t < row_end, d, lq, gf);
    }
    const f32x4 dmask = diag_mask(l15, lq);
    for (int t0 = chunk * rq + wave * 16; t0 < row_end; t0 += 64) {
        const int nd = __builtin_amdgcn_readfirstlane(t0 >> 4);  // the diagonal fragment
        const int t = t0 + l15;
        const bool valid = t < row_end;
        // this block's rows into the wave's LDS tiles (source of the transposed operands below) ...
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            *reinterpret_cast<F8*>(Qw + l15 * S::KROW + ks * 32 + lq * 8) = qf[ks];
            *reinterpret_cast<F8*>(Gw + l15 * S::KROW + ks * 32 + lq * 8) = gf[ks];
        }
        // ... and the next block's rows into flight
        F8 qn[KS], gn[KS];
        load_row_frags<T, KS>(Qh + (int64_t)(t + 64) * ldq, Qh, t + 64 < row_end, d, lq, qn);
        load_row_frags<T, KS>(Gh + (int64_t)(t + 64) * HD, Gh, t + 64 < row_end, d, lq, gn);

        // ---- query-per-lane layout: P, dP, the softmax correction, dS → dQ ----------------
        f32x4 s[NKF], dp[NKF];
#pragma unroll
        for (int nf = 0; nf < NKF; ++nf) {
            s[nf] = nf == nd ? dmask : zero;
            dp[nf] = zero;
            if (nf <= nd) {
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const int off = (nf * 16 + l15) * S::KROW + ks * 32 + lq * 8;
                    s[nf] = Mma<T>::k32(*reinterpret_cast<const F8*>(Ks + off), qf[ks], s[nf]);
                    dp[nf] = Mma<T>::k32(*reinterpret_cast<const F8*>(Vs + off), gf[ks], dp[nf]);
                }
            }
        }
        float inv_l;
        softmax_rows_causal<NKF>(s, nd, scale_log2e, inv_l);
        // P in the permuted key order, one row per query: re-read below with the keys along the lanes
#pragma unroll
        for (int kk = 0; kk < NKF / 2; ++kk)
            if (2 * kk <= nd)
                *reinterpret_cast<F8*>(Pw + l15 * S::TROW + kk * 32 + lq * 8) = pair_frag<T>(s[2 * kk], s[2 * kk + 1]);
        float corr = 0.f;  // Σ_key P·dP  (= Σ_c dO·O of this query row)
#pragma unroll
        for (int nf = 0; nf < NKF; ++nf)
            if (nf <= nd) {
#pragma unroll
                for (int r = 0; r < 4; ++r) corr += s[nf][r] * dp[nf][r];
            }
        corr += __shfl_xor(corr, 16, 64);
        corr += __shfl_xor(corr, 32, 64);
#pragma unroll
        for (int nf = 0; nf < NKF; ++nf)
            if (nf <= nd) {
#pragma unroll
                for (int r = 0; r < 4; ++r) s[nf][r] = s[nf][r] * (dp[nf][r] - corr) * scale;  // dS; 0 where P is 0
            }
        {
            f32x4 g[DF];
#pragma unroll
            for (int df = 0; df < DF; ++df) g[df] = zero;
#pragma unroll
            for (int kk = 0; kk < NKF / 2; ++kk) {
                if (2 * kk <= nd) {
                    const F8 dsf = pair_frag<T>(s[2 * kk], s[2 * kk + 1]);
                    *reinterpret_cast<F8*>(Sw + l15 * S::TROW + kk * 32 + lq * 8) = dsf;
#pragma unroll
                    for (int df = 0; df < DF; ++df) {
                        // Kᵀ fragment of this head-dim slice from the row-major K tile (two transposing block reads)
                        const F8 kf = tr_pair<T>(lds_tr_block(Ks + (kk * 32) * S::KROW + df * 16, S::KROW, lane),
                                                 lds_tr_block(Ks + (kk * 32 + 16) * S::KROW + df * 16, S::KROW, lane));
                        g[df] = Mma<T>::k32(kf, dsf, g[df]);
                    }
                }
            }
            T* qrow = dQ + ((int64_t)b * Tn + t) * ld_dq + h * d;
#pragma unroll
            for (int df = 0; df < DF; ++df) {
                const int c = df * 16 + lq * 4;
                if (valid && c < d) {
                    Quad4<T> out;
#pragma unroll
                    for (int r = 0; r < 4; ++r) out.v[r] = from_f32<T>(g[df][r]);
                    *reinterpret_cast<Quad4<T>*>(qrow + c) = out;
                }
            }
        }

        // ---- dK, dV: contraction over the 16 query rows.  Operands with the keys (resp. head-dim columns) along the
        // lanes and 4 query rows per lane, read back transposed from the wave's LDS tiles --------------------------
        tr4 qT[DF], gT[DF];  // lane = head-dim column df*16 + l15, the block's rows lq*4 .. +3
#pragma unroll
        for (int df = 0; df < DF; ++df) {
            qT[df] = lds_tr_block(Qw + df * 16, S::KROW, lane);
            gT[df] = lds_tr_block(Gw + df * 16, S::KROW, lane);
        }
#pragma unroll
        for (int nf = 0; nf < NKF; ++nf) {
            if (nf <= nd) {  // keys above the diagonal fragment receive nothing from this block
                // lane = key nf*16 + l15, which sits at position (nf>>1)*32 + 8·(l15>>2) + 4·(nf&1) + (l15&3) of a P row:
                // lane 4q+p of a group supplies row lq*4 + q, the four positions of key group p
                const int off = (lq * 4 + (l15 >> 2)) * S::TROW + (nf >> 1) * 32 + (l15 & 3) * 8 + (nf & 1) * 4;
                const tr4 pa = lds_tr_at(Pw + off), dsa = lds_tr_at(Sw + off);
#pragma unroll
                for (int df = 0; df < DF; ++df) {
                    dv[nf][df] = Mma<T>::k16rr(pa, gT[df], dv[nf][df]);
                    dk[nf][df] = Mma<T>::k16rr(dsa, qT[df], dk[nf][df]);
                }
            }
        }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            qf[ks] = qn[ks];
            gf[ks] = gn[ks];
        }
    }

    // ---- sum the four waves' dK/dV in wave order, one fp32 partial per workgroup ----------------------------------------
    sum_wave_images<NKF, DF>(dk, dv, red, part, wave, lane);
}

struct CausalPlan {
    int ks, df, nkf;  // template selection, as plan_ctx's for heads of at most 96
    int chunks, rq;   // query rows per workgroup: 64 or 128, so every wave's blocks start at multiples of 16
};

bool plan_causal(int B, int T, int H, int d, bool backward, CausalPlan* pl) {
    if (B < 1 || T < 1 || T > 128 || H < 1 || d < 8 || (d % 8) != 0 || d > 96) return false;
    pl->ks = d <= 64 ? 2 : 3;
    pl->df = (d + 15) / 16;
    if (pl->df < 3) pl->df = 3;
    pl->nkf = T <= 96 ? 6 : 8;
    // two workgroups per (batch, head) — rows 0–63 and 64–127 — while that still adds workgroups the chip has room for (forward
    // 512, backward, at one workgroup per CU, 256); the second re-stages K/V and, in backward, writes a second partial
    const int64_t bh = (int64_t)B * H;
    pl->rq = (T > 64 && 2 * bh <= (backward ? 256 : 512)) ? 64 : 128;
    pl->chunks = (T + pl->rq - 1) / pl->rq;
    return (pl->rq % 64) == 0;  // whole rounds of the four waves: the block at t0 has its diagonal in fragment t0 / 16
}

template <int KS, int DF, int NKF> constexpr int causal_fwd_lds() {
    using S = CtxShape<KS, DF, NKF>;
    return 2 * S::NK * S::KROW * 2;
}
template <int KS, int DF, int NKF> constexpr int causal_bwd_lds() {
    using S = CtxShape<KS, DF, NKF>;
    constexpr int stage = (2 * S::NK * S::KROW + 4 * 2 * 16 * S::KROW + 4 * 2 * 16 * S::TROW) * 2;
    constexpr int F = 2 * NKF * DF, PH = (F + kCtxSumFrags - 1) / kCtxSumFrags, CH = (F + PH - 1) / PH;
    constexpr int red = 4 * CH * 64 * 16;  // four waves' images of one phase of the closing sum
    return stage > red ? stage : red;
}

struct CausalArgs {
    const void *Q, *K, *V, *dO;
    void *O, *dQ, *dK, *dV;
    float* part;
    int B, T, H, d;
    float scale;
    int64_t ldq, ld_dq;  // row strides (elements) of Q/K/V and of dQ/dK/dV
};

template <typename T, int KS, int DF, int NKF, bool BWD>
int launch_causal(const CausalArgs& a, const CausalPlan& pl, hipStream_t stream) {
    const float l2e = a.scale * 1.4426950408889634f;
    const dim3 grid((unsigned)(a.B * a.H * pl.chunks));
    if constexpr (!BWD) {
        constexpr int lds = causal_fwd_lds<KS, DF, NKF>();
        auto kern = attn_causal_fwd_kernel<T, KS, DF, NKF>;
        if (lds > 48 * 1024) {
            static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                                               hipFuncAttributeMaxDynamicSharedMemorySize, lds);
            if (attr != hipSuccess) return LORA_E_LAUNCH;
        }
        LORA_LAUNCH(PK_OTHER, kern, grid, dim3(256), lds, stream, static_cast<const T*>(a.Q), static_cast<const T*>(a.K),
                    static_cast<const T*>(a.V), static_cast<T*>(a.O), a.T, a.H, a.d, l2e, pl.rq, pl.chunks, a.ldq);
        LORA_LAUNCH_CHECK();
        return LORA_OK;
    } else {
        constexpr int lds = causal_bwd_lds<KS, DF, NKF>();
        auto kern = attn_causal_bwd_kernel<T, KS, DF, NKF>;
        if (lds > 48 * 1024) {
            static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                                               hipFuncAttributeMaxDynamicSharedMemorySize, lds);
            if (attr != hipSuccess) return LORA_E_LAUNCH;
        }
        LORA_LAUNCH(PK_OTHER, kern, grid, dim3(256), lds, stream, static_cast<const T*>(a.Q), static_cast<const T*>(a.K),
                    static_cast<const T*>(a.V), static_cast<const T*>(a.dO), static_cast<T*>(a.dQ), a.part, a.T, a.H, a.d,
                    a.scale, l2e, pl.rq, pl.chunks, a.ldq, a.ld_dq);
        LORA_LAUNCH_CHECK();
        const int64_t total = (int64_t)a.B * a.H * 2 * (NKF * 16) * (DF * 16) / 4;  // 16-byte accumulators of one partial set
        const unsigned blocks = (unsigned)((total + 255) / 256 > 2048 ? 2048 : (total + 255) / 256);
        LORA_LAUNCH(PK_OTHER, attn_ctx_reduce_kernel<T>, dim3(blocks), dim3(256), 0, stream, a.part, static_cast<T*>(a.dK),
                    static_cast<T*>(a.dV), a.B, a.T, a.H, a.d, pl.chunks, 1, NKF * 16, DF * 16, a.ld_dq);
        LORA_LAUNCH_CHECK();
        return LORA_OK;
    }
}

template <typename T>
int dispatch_causal(const CausalArgs& a, const CausalPlan& pl, bool backward, hipStream_t stream) {
#define CAUSAL_CASE(KS_, DF_, NKF_)                                                              \
    if (pl.ks == KS_ && pl.df == DF_ && pl.nkf == NKF_)                                              \
        return backward ? launch_causal<T, KS_, DF_, NKF_, true>(a, pl, stream) : launch_causal<T, KS_, DF_, NKF_, false>(a, pl, stream);
    CAUSAL_CASE(2, 3, 6) CAUSAL_CASE(2, 4, 6) CAUSAL_CASE(3, 5, 6) CAUSAL_CASE(3, 6, 6)
    CAUSAL_CASE(2, 3, 8) CAUSAL_CASE(2, 4, 8) CAUSAL_CASE(3, 5, 8) CAUSAL_CASE(3, 6, 8)
#undef CAUSAL_CASE
    return LORA_E_BADARG;
}

int run_causal(const CausalArgs& a, bool backward, int dtype, hipStream_t stream) {
    CausalPlan pl;
    if (!plan_causal(a.B, a.T, a.H, a.d, backward, &pl)) return LORA_E_BADARG;
    switch (dtype) {
        case LORA_F16: return dispatch_causal<half_t>(a, pl, backward, stream);
        case LORA_BF16: return dispatch_causal<bf16_t>(a, pl, backward, stream);
        default: return LORA_E_BADARG;  // fp32 tensors stay on the caller's own attention
    }
}

}  // namespace

extern "C" int attn_causal_supported(int B, int T, int H, int d, int dtype) {
    CausalPlan pl;
    return (dtype == LORA_F16 || dtype == LORA_BF16) && plan_causal(B, T, H, d, false, &pl) ? 1 : 0;
}

extern "C" int64_t attn_causal_bwd_workspace_bytes(int B, int T, int H, int d) {
    CausalPlan pl;
    if (!plan_causal(B, T, H, d, true, &pl)) return -1;
    return (int64_t)B * H * pl.chunks * 2 * (pl.nkf * 16) * (pl.df * 16) * 4;
}

extern "C" int attn_causal_fwd_strided(const void* Q, const void* K, const void* V, void* O, int64_t ldq, int B, int T,
                                       int H, int d, float scale, int dtype, void* stream) {
    if (!Q || !K || !V || !O) return LORA_E_BADARG;
    if (!aligned16(Q) || !aligned16(K) || !aligned16(V) || !aligned16(O)) return LORA_E_BADARG;
    if (ldq < (int64_t)H * d || (ldq % 8) != 0) return LORA_E_BADARG;
    CausalArgs a{};
    a.Q = Q; a.K = K; a.V = V; a.O = O; a.B = B; a.T = T; a.H = H; a.d = d; a.scale = scale;
    a.ldq = ldq; a.ld_dq = (int64_t)H * d;
    return run_causal(a, false, dtype, static_cast<hipStream_t>(stream));
}

extern "C" int attn_causal_bwd_strided(const void* Q, const void* K, const void* V, const void* dO, void* dQ, void* dK,
                                       void* dV, void* workspace, int64_t ldq, int64_t ld_dq, int B, int T, int H, int d,
                                       float scale, int dtype, void* stream) {
    if (!Q || !K || !V || !dO || !dQ || !dK || !dV || !workspace) return LORA_E_BADARG;
    if (!aligned16(Q) || !aligned16(K) || !aligned16(V) || !aligned16(dO) || !aligned16(dQ) || !aligned16(workspace))
        return LORA_E_BADARG;
    if (ldq < (int64_t)H * d || (ldq % 8) != 0 || ld_dq < (int64_t)H * d || (ld_dq % 8) != 0) return LORA_E_BADARG;
    CausalArgs a{};
    a.Q = Q; a.K = K; a.V = V; a.dO = dO; a.dQ = dQ; a.dK = dK; a.dV = dV; a.part = static_cast<float*>(workspace);
    a.B = B; a.T = T; a.H = H; a.d = d; a.scale = scale; a.ldq = ldq; a.ld_dq = ld_dq;
    return run_causal(a, true, dtype, static_cast<hipStream_t>(stream));
}

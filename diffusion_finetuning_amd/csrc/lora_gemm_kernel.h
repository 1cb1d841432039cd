// LoRA-fused GEMM for gfx950.
//
// One kernel template serves both big contractions of the hot path:
//   forward   (lora_diffusion/lora.py:49-50):   Y  = X·Wᵀ + b + s·(X·Aᵀ)·Bᵀ     and  T = X·Aᵀ
//   backward  (autograd of the same line):      dX = dY·W   + s·(dY·B)·A        and  U = dY·B
// written once as
//   C[M,Nc] = Am[M,Kc]·Bm[Nc,Kc]ᵀ + bias + s·P·Qᵀ ,   P[M,r] = Am·Fᵀ  (stored unscaled)
// with (Am,Bm,F,Q) = (X, W, A, B) forward and (dY, Wᵀ, Bᵀ, Aᵀ) backward.  Both big operands are
// contraction-contiguous ("NT" GEMM), which is why the frozen weight is cached in both
// orientations.  F arrives PACKED: [16, Kc] in the compute dtype, rows ≥ r zero
// (lora_pack_factors), so it is staged exactly like an operand tile.
//
// Structure per workgroup of NW waves (2 row waves × NW/2 column waves; 256 threads in every instantiated form), BM×BN output
// tile (128×128, 128×160, 64×160, 64×128, 64×64), 128-byte K-steps:
//   - PIPE main loop: an LDS ring of STG = 2–4 stages filled by LDS-DMA (global_load_lds, 16 B per lane, no VGPR staging),
//     STG−1 K-steps in flight behind a COUNTED s_waitcnt vmcnt and one raw s_barrier per step.  The XOR swizzle of the 16-B
//     chunks is applied to the per-lane SOURCE address (the DMA writes LDS in lane order) and again on the fragment reads,
//     which are then bank-conflict-free ds_read_b128.  Two workgroups per CU by construction (≤ 80 KB LDS, ≤ 256 registers);
//   - fallback main loop (contraction not a multiple of the K-step): register-staged, 2 barriers per step;
//   - base contraction on MFMA 16x16x32 (f16/bf16) or 16x16x4 (f32, exact), issued with the Bm fragment as the
//     first operand: a lane then owns 4 CONSECUTIVE COLUMNS of one output row (and 4 consecutive rank entries of
//     P), so the epilogue moves 8/16 bytes per LDS access instead of one element;
//   - the rank-r factor rides along as a 16-row tile: the X fragments already in VGPRs are multiplied
//     with it (one extra MFMA per row fragment, K-steps split between the two column waves), so T
//     costs no extra HBM or LDS traffic for X;
//   - epilogue on the ring's own buffers: the partial P tiles of the column waves meet in the buffer that is free after the
//     last K-step; thread (row, half) sums them, writes P out and leaves s·P as ONE packed record per row — a high and a low
//     16-bit part in MFMA operand order — so every wave fetches a fragment with one 16-byte read and s·P·Qᵀ enters the
//     accumulators as ONE extra MFMA K-step ([hi | lo] × [Q | Q]: P keeps ~fp32 precision).  The Q tile itself is fetched by
//     DMA during the last K-step into the same free buffer (no LDS of its own: what lets two 128×160 tiles share a CU);
//   - bias is added in fp32, the tile is transposed through the buffer of the last K-step and stored as whole 16-B row chunks;
//   - GATE instantiation (the `proj` layer of a GEGLU block): a column tile is 64 hidden columns plus the 64 gate columns behind
//     them, and the store pass writes h·gelu(g) next to (or instead of) the [h | g] tile — diffusers GEGLU.forward in the epilogue.
//   - SPLITK instantiations (long contractions on grids too small for the chip): the K-slices of a tile are workgroups of the
//     SAME launch; each stores its fp32 partials write-through (sc1), draws a ticket, and the last arriver adds the slices in
//     index order and runs the epilogue above — deterministic, no second launch (plan_splitk()).
//   - RS instantiations (forward, inference: lora_linear_fwd_rows / lora_linear_geglu_fwd_rows): the factor s of the rank-r term
//     becomes s·G[sample of the row, rank slot] from an fp32 gate table — formed in fp32 FIRST, then multiplied into P, wherever
//     an epilogue form builds s·P; instantiations of their own, so that every other kernel is compiled exactly as before.
// Workgroups are dealt to XCDs so that the column tiles of one row panel (or the row tiles of one column panel, whichever
// re-fetches the smaller operand) share an L2 — or, for square-ish problems, so that each XCD owns a rectangle of the tile grid.
// Tile / ring / split choice per shape: launch_pipe(), gate_tile_width(), plan_splitk() of lora_gemm.hip — all measured with
// cold weights.
//
// This header is the kernel and its argument block.  lora_gemm.hip, which picks and launches the instantiations, is its ONE
// includer: a second one would compile every instantiation again.

#pragma once
#include "common.h"

namespace {

struct GemmParams {
    const void* Am;
    const void* Bm;
    const void* bias;
    const void* Fp;  // packed main-loop factor   [16, Kc] (dtype T), rows >= r zero
    const void* Qp;  // packed epilogue factor    [Nc, 16] (dtype T), columns >= r zero
    void* C;
    float* P;
    int64_t M;
    int Kc, Nc, r;
    float scale;
    int tiles_m, tiles_n;
    int col_major;  // 1: consecutive tiles walk down M inside a column tile (an XCD then owns a slice of Bm)
    int xcd_m;      // > 1: the 8 XCDs form an xcd_m × (8/xcd_m) grid over the tile grid, each XCD owns a RECTANGLE of tiles
                    // (both splits exact) — an XCD's L2 then fetches |Am|/xcd_m + |Bm|·xcd_m/8 instead of all of one operand
    int64_t lda;    // row stride of Am in elements (>= Kc: Am may be a column slice of a wider buffer)
    // Grouped launches (several LoRA layers that share Am in one launch; nullptr = one layer):
    //  MAIN:  tile_part[tn] = part | first << 16 for every column tile — the tile multiplies with the part's own
    //         factor rows Fp + part·16·Kc, and the part's first tile writes P + part·M·r (column tiles never
    //         straddle parts: the host picks BN accordingly);
    // !MAIN:  part_table[g] = {column offset into Am, contraction length, element offset into Fp, float offset
    //         into P} — blockIdx covers (row tile, part), every part contracts its own column range of Am.
    const int* tile_part;
    const int64_t* part_table;
    // Equal-width parts without a table (grouped q/k/v at any rank <= 16: lora_gemm_parts):
    //  n_parts > 0, parts_on_k == 0 (forward):  the Nc output columns are n_parts runs of part_n; a column tile lies inside one
    //         part (the host picks BN | part_n), multiplies with that part's factor rows Fp + part·16·Kc, and the part's first
    //         tile writes its P columns [part·r, part·r + r) of the [M, ldp] buffer;
    //  n_parts > 0, parts_on_k == 1 (backward-input, KP kernels): the CONTRACTION is n_parts runs of part_n — Fp [16, Kc]
    //         holds part g's factor rows in its own column run, P_g = Am[:, run g]·F_gᵀ accumulates per part, and the
    //         epilogue adds s·Σ_g P_g·Q_gᵀ with Qp = [n_parts][Nc, 16].
    int n_parts, part_n, parts_on_k;
    int ldp;  // row stride of P in floats (r for a single layer)
    // Split-K (contractions on grids too small for the chip): slice s of a tile contracts K-steps [s·steps_per_slice, …),
    // STORES its fp32 accumulators at ws_c[tile][s] (BM·BN floats in the lanes' own register order) and its partial P at
    // ws_p[tile][s][BM][16], and takes a ticket of the tile.  The workgroup that draws the LAST ticket adds the slices
    // 0..S-1 in index order — whoever arrives last, the sum has one order: deterministic — and runs the normal epilogue
    // (rank-r term, bias, store) on the totals; it leaves the ticket at zero for the next launch.  splitk <= 1: off.
    int splitk, steps_per_slice;
    float* ws_c;
    float* ws_p;
    unsigned* tickets;  // one per output tile, zero on entry, zero again on exit
    int split_bm;       // (host only) row-tile height of a split launch
    // GEGLU gate in the epilogue (GATE kernels; diffusers GEGLU.forward behind the `proj` LoraInjectedLinear): Nc = 2·gateF,
    // a column tile owns BN/2 columns of h = C[:, :gateF] AND the matching BN/2 columns of g = C[:, gateF:], and the
    // epilogue writes C2[M, gateF] = h·gelu(g) next to C (C may be null: nothing is saved for a backward pass).
    void* C2;
    int gateF;
    // Per-row gates of the rank-r term (RS kernels; inference only): row m multiplies rank slot j with scale·row_scale[(m /
    // rs_rps)·rs_ld + j] instead of scale — the fp32 table holds one row of gates per SAMPLE, a sample is rs_rps consecutive
    // rows of Am.  P is written out un-gated.  Unused (null) in every other instantiation.
    const float* row_scale;
    int64_t rs_rps;
    int rs_ld;
};

constexpr int kRowBytes = 128;  // one K-step of one tile row  (kRP, the padded rank: common.h)
constexpr int kSPS = 20;       // fp32 row stride of the P image in LDS: 80 B keeps the 16-B row reads conflict-free
template <typename T> struct alignas(sizeof(T) * 4) Quad { T v[4]; };

__device__ __forceinline__ int lds_off(int row, int chunk) {
    return row * kRowBytes + ((chunk ^ (row & 7)) << 4);
}

__device__ __forceinline__ void glds16(const void* gsrc, char* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gsrc),
                                     (__attribute__((address_space(3))) void*)(lds_wave_base), 16, 0, 0);
}

template <typename T> struct Mfma;
template <> struct Mfma<half_t> {
    using Frag = f16x8;
    static __device__ __forceinline__ f32x4 run(Frag a, Frag b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
    }
};
template <> struct Mfma<bf16_t> {
    using Frag = bf16x8;
    static __device__ __forceinline__ f32x4 run(Frag a, Frag b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
};

#ifdef LORA_STAMPS  // diagnostic build only (tools/wg_timeline.py): per-workgroup phase timestamps
__device__ unsigned long long g_stamps[8192 * 16];
#define STAMP(i)                                                                  \
    do {                                                                          \
        if (tid == 0 && blockIdx.x < 8192) g_stamps[blockIdx.x * 16 + (i)] = __builtin_readcyclecounter(); \
    } while (0)
#define STAMP_WALL(i)                                                             \
    do {                                                                          \
        if (tid == 0 && blockIdx.x < 8192) g_stamps[blockIdx.x * 16 + (i)] = wall_clock64(); \
    } while (0)
#else
#define STAMP(i)
#define STAMP_WALL(i)
#endif

// Diagnostic ablation of the pipelined main loop, timing only — the results are wrong (tools/skeleton_per_class.py builds it
// as a variant library with -DLORA_GEMM_DBG=N): bit 1 = no DMA after the prologue, bit 2 = no MFMA work.
#ifndef LORA_GEMM_DBG
#define LORA_GEMM_DBG 0
#endif

// One stage of the ring / the single staging buffer: A rows, B rows, 16 factor rows.  Only the first two waves load the
// factor rows, so they carry one more DMA per stage than the others: the counted waits are picked per wave.
template <int BM, int BN, bool MAIN, int STG, int NW> constexpr int stage_bytes() {  // (same for every wave layout)
    return (BM + (MAIN ? BN : 0) + kRP) * kRowBytes;
}
template <int BM, int BN, typename T, bool MAIN, int STG, int NW, int WM> constexpr int gemm_lds_bytes() {
    constexpr int ring = (STG > 0 ? STG : 1) * stage_bytes<BM, BN, MAIN, STG, NW>();
    constexpr int sq = MAIN && STG == 0 ? BN * kRP * (int)sizeof(T) : 0;  // ring kernels stage Q in a free ring buffer
    constexpr int ep = sizeof(T) == 4 ? 2 : 1;
    constexpr int sc = (MAIN && STG == 0) || (MAIN && sizeof(T) == 4) ? (BM / ep) * (BN * (int)sizeof(T) + 16) : 0;
    constexpr int sp = (NW / WM) * BM * kSPS * 4;
    constexpr int a = ring + sq;
    constexpr int b = sc > sp ? sc : sp;
    return a > b ? a : b;
}

// STG: LDS ring depth of the DMA pipeline (2 or 3); 0 selects the register-staged fallback loop.
// NW waves as WM row waves × NW/WM column waves; every wave owns a (BM/WM) × (BN·WM/NW) piece of the tile.
// SPLITK: the launch cuts its contraction into K-slices (in-launch combine, below) — instantiations of their own, so that the
// unsplit kernels carry none of that code and profilers can tell the two apart by name
// KP > 1: the contraction consists of KP equal parts with a factor pair each (grouped q/k/v backward-input at 3r > 16)
// RS: per-row gates of the rank-r term from GemmParams::row_scale (forward launches of one layer)
template <typename T, int BM, int BN, bool MAIN, int STG, int NW, int WM, int GATE = 0, bool SPLITK = false, int KP = 1, bool RS = false>  // GATE: 0 none, 1 GEGLU forward, 2 GEGLU backward
__global__ __launch_bounds__(NW * 64, NW == 4 ? 2 : 1) void lora_gemm_kernel(GemmParams p) {  // 4-wave tiles: two per CU
    constexpr bool PIPE = STG > 0;
    constexpr int kStages = PIPE ? STG : 1;
    constexpr int NT = NW * 64;        // threads
    constexpr int WN = NW / WM;        // column waves
    constexpr int WTN = BN / WN;       // wave tile width
    constexpr int RPP = NW * 8;        // tile rows covered by one staging pass
    constexpr int VEC = ElemTraits<T>::kVec;
    constexpr int BK = kRowBytes / (int)sizeof(T);
    constexpr int WTM = BM / WM;       // wave tile height
    constexpr int MI = WTM / 16;  // 16-row fragments per wave
    constexpr int NI = WTN / 16;
    constexpr int PA = BM / RPP;  // staging passes
    constexpr int PB = BN / RPP;
    constexpr bool F32 = sizeof(T) == 4;
    constexpr int STAGE = stage_bytes<BM, BN, MAIN, STG, NW>();
    constexpr int OFF_B = BM * kRowBytes;
    constexpr int OFF_F = (BM + (MAIN ? BN : 0)) * kRowBytes;

    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sQ = smem + kStages * STAGE;  // (ring kernels: re-pointed into the ring when the Q tile is fetched, below)
    float* sP = reinterpret_cast<float*>(smem);  // epilogue overlay: [NW/2][BM][kSPS] (ring kernels: a free ring buffer)

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN;
    const int wn = wave % WN;
    const int l15 = lane & 15;
    const int lq = lane >> 4;

    STAMP_WALL(0);
    STAMP(1);
#ifdef LORA_STAMPS
    if (tid == 0 && blockIdx.x < 8192) {
        g_stamps[blockIdx.x * 16 + 10] = __builtin_amdgcn_s_getreg((31 << 11) | 4);   // HW_ID
        g_stamps[blockIdx.x * 16 + 11] = __builtin_amdgcn_s_getreg((31 << 11) | 20);  // XCC_ID
    }
#endif
    // XCD-aware tile assignment: blocks b and b+8 share an XCD (round-robin dispatch), so give
    // every XCD a contiguous run of tiles; column tiles of one row panel are consecutive.
    // Pull every kernel argument into SGPRs now: one scalar-load round trip instead of two dependent ones.
    asm volatile("" ::"s"(p.Am), "s"(p.Bm), "s"(p.bias), "s"(p.Fp), "s"(p.Qp), "s"(p.C), "s"(p.P), "s"(p.M), "s"(p.Kc),
                 "s"(p.Nc), "s"(p.scale), "s"(p.tiles_m), "s"(p.tiles_n), "s"(p.col_major), "s"(p.lda), "s"(p.tile_part),
                 "s"(p.part_table), "s"(p.splitk), "s"(p.steps_per_slice), "s"(p.ws_c), "s"(p.ws_p), "s"(p.tickets), "s"(p.xcd_m));
    int tile, slice = 0;
    {
        const int S = SPLITK ? p.splitk : 1;
        const int total = p.tiles_m * p.tiles_n * S;
        const int id = blockIdx.x;
        const int q = total >> 3, rem = total & 7;
        const int xcd = id & 7, slot = id >> 3;
        tile = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + slot;
        if (S > 1) {  // the slices of one tile are neighbours: they read the same operand rows, a K-range each
            slice = tile % S;
            tile = tile / S;
        }
    }
    // Which operand should stay inside one XCD's L2?  Row-major tile order keeps a row panel of Am there and makes
    // every XCD stream all of Bm; column-major order keeps a slice of Bm there and streams Am instead.  The host
    // picks the order that re-fetches the SMALLER operand eight times (col_major when Bm is the bigger one).
    int tm, tn;
    if (p.xcd_m > 1) {
        // 2-D XCD ownership (square-ish problems: neither operand is small enough to be re-fetched by all eight L2s).
        // Block id → (XCD, slot) as above; the XCD's rectangle is rm × rn tiles, walked column by column.
        const int xn = 8 / p.xcd_m;
        const unsigned rm = p.tiles_m / p.xcd_m, rn = p.tiles_n / xn;
        const unsigned xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
        const unsigned ln = slot / rm, lm = slot - ln * rm;
        tm = (xcd / xn) * rm + lm;
        tn = (xcd % xn) * rn + ln;
        tile = tm * p.tiles_n + tn;
    } else {
        const unsigned inner = p.col_major ? p.tiles_m : p.tiles_n;  // tiles along the fast direction
        const unsigned t_slow = (unsigned)tile / inner, t_fast = (unsigned)tile - t_slow * inner;
        tm = p.col_major ? t_fast : t_slow;
        tn = p.col_major ? t_slow : t_fast;
    }
    STAMP(12);
    const int64_t m0 = (int64_t)tm * BM;
    const int n0 = tn * BN;
    // tile-local column → column of C / row of Bm.  GATE: the first half of the tile is a run of h columns, the second
    // half the run of g columns that gates them (both halves are whole: gateF % (BN/2) == 0).
    auto gcol = [&](int c) {
        if constexpr (GATE == 1) return c < BN / 2 ? tn * (BN / 2) + c : p.gateF + tn * (BN / 2) + (c - BN / 2);
        else return n0 + c;
    };

    const T* Ag = static_cast<const T*>(p.Am);
    const T* Bg = static_cast<const T*>(p.Bm);
    const T* Fg = static_cast<const T*>(p.Fp);
    float* Pout = p.P;
    int Kc = p.Kc;
    bool write_p = p.P != nullptr && tn == 0;
    if constexpr (MAIN) {
        if (p.tile_part != nullptr) {
            const int e = p.tile_part[tn];
            const int part = e & 0xffff;
            Fg += (int64_t)part * kRP * Kc;
            if (Pout != nullptr) Pout += (int64_t)part * p.M * p.r;
            write_p = p.P != nullptr && (e >> 16) != 0;
        } else if (KP == 1 && p.n_parts > 0) {  // equal parts over the output columns (lora_gemm_parts, forward form)
            const int part = n0 / p.part_n;
            Fg += (int64_t)part * kRP * Kc;
            if (Pout != nullptr) Pout += part * p.r;
            write_p = p.P != nullptr && n0 == part * p.part_n;
        }
    } else {
        if (p.part_table != nullptr) {
            const int64_t* e = p.part_table + (int64_t)tn * 4;
            Ag += e[0];
            Kc = (int)e[1];
            Fg += e[2];
            if (Pout != nullptr) Pout += e[3];
            write_p = p.P != nullptr;
        }
    }

    // ---- staging addresses: thread = (row ld_row (+32·pass), 16-B chunk ld_chunk) ------------
    const int ld_chunk = tid & 7;
    const int ld_row = tid >> 3;
    const T* a_ptr[PA];
    const T* b_ptr[MAIN ? PB : 1];
#pragma unroll
    for (int i = 0; i < PA; ++i) {
        int64_t m = m0 + ld_row + RPP * i;
        if (m > p.M - 1) m = p.M - 1;  // clamp: rows past M are loaded from a valid row, never stored
        a_ptr[i] = Ag + m * p.lda;
    }
    if constexpr (MAIN) {
#pragma unroll
        for (int i = 0; i < PB; ++i) {
            int n = gcol(ld_row + RPP * i);
            if (n > p.Nc - 1) n = p.Nc - 1;
            b_ptr[i] = Bg + (int64_t)n * Kc;
        }
    }
    const T* f_ptr = Fg + (int64_t)(ld_row & 15) * Kc;

    // ---- Q tile (epilogue factor): BN packed rows of 16 values, 16-B chunks, rows clamped at the edge -----
    // Ring kernels fetch it by DMA during the LAST K-step into the ring buffer that is free by then (issue_q below): it
    // costs no LDS of its own — which is what lets two 128×160 workgroups share a CU — and stays off the prologue.
    constexpr int CPRQ = kRP * (int)sizeof(T) / 16;  // chunks per packed row (2 for 16-bit, 4 for f32)
    constexpr int QOFF = WN * BM * kSPS * 4;         // behind the P image when both land in the same buffer
    auto issue_q = [&](char* dst, int part = 0) {
        const T* Qg = static_cast<const T*>(p.Qp) + (int64_t)part * p.Nc * kRP;
        for (int base = wave * 64; base < BN * CPRQ; base += NT) {
            const int idx = base + lane;
            const int n = idx / CPRQ, ch = idx - n * CPRQ;
            const int nn = gcol(n) < p.Nc ? gcol(n) : p.Nc - 1;
            glds16(Qg + (int64_t)nn * kRP + ch * VEC, dst + base * 16);
        }
    };
    if constexpr (MAIN && !PIPE) {
        const T* Qg = static_cast<const T*>(p.Qp);
        for (int idx = tid; idx < BN * CPRQ; idx += NT) {
            const int n = idx / CPRQ, ch = idx - n * CPRQ;
            const int nn = gcol(n) < p.Nc ? gcol(n) : p.Nc - 1;
            *reinterpret_cast<Chunk<T>*>(sQ + idx * 16) =
                *reinterpret_cast<const Chunk<T>*>(Qg + (int64_t)nn * kRP + ch * VEC);
        }
    }

    // bias of the lane's 4·NI output columns (4 consecutive columns per fragment: ONE 8-/16-byte load each), fetched
    // now so the epilogue never waits on it
    float bias_v[MAIN ? NI : 1][4];
    if constexpr (MAIN) {
        if (p.bias != nullptr) {
            const T* bias = static_cast<const T*>(p.bias);
#pragma unroll
            for (int ni = 0; ni < NI; ++ni) {
                int col = gcol(wn * WTN + ni * 16 + lq * 4);
                if (col > p.Nc - 4) col = p.Nc - 4;  // Nc % VEC == 0 here: a group of 4 is inside or past the edge
                const Quad<T> q = *reinterpret_cast<const Quad<T>*>(bias + col);
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) bias_v[ni][reg] = to_f32<T>(q.v[reg]);
            }
        }
    }
    STAMP(13);

    f32x4 acc[MAIN ? MI : 1][MAIN ? NI : 1];
    f32x4 pacc[MI];
    f32x4 pacc_x[KP > 1 ? KP - 1 : 1][MI];  // KP kernels: parts 1.. (part 0 uses pacc)
#pragma unroll
    for (int i = 0; i < (MAIN ? MI : 1); ++i)
#pragma unroll
        for (int j = 0; j < (MAIN ? NI : 1); ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < MI; ++i) pacc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int g = 0; g < (KP > 1 ? KP - 1 : 1); ++g)
#pragma unroll
        for (int i = 0; i < MI; ++i) pacc_x[g][i] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int steps_per_part = KP > 1 ? p.part_n / BK : 1;  // (part_n % BK == 0: checked on the host)

    // ---- one K-step of MFMA work out of a staged buffer ------------------------------------
    auto compute = [&](const char* st, int kt) {
        const char* sA = st;
        const char* sB = st + OFF_B;
        const char* sF = st + OFF_F;
        if constexpr (!F32) {
            using Frag = typename Mfma<T>::Frag;
            // (round 3, measured: issuing ALL fragment reads of the K-step up front, both 32-wide halves, so that the MFMAs wait
            //  on counted lgkmcnt instead of the lgkmcnt(0) hipcc puts in front of every MFMA group here, changes nothing —
            //  1024×1280×1280 15.5 / 15.4 / 15.4 µs for none / small tiles / all tiles, every other shape within 1 %: the
            //  lone-workgroup main loop is not paced by exposed LDS latency)
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const int chunk = ks * 4 + lq;
                Frag af[MI];
#pragma unroll
                for (int mi = 0; mi < MI; ++mi)
                    af[mi] = *reinterpret_cast<const Frag*>(sA + lds_off(wm * WTM + mi * 16 + l15, chunk));
                if ((kt * 2 + ks) % WN == wn) {
                    const Frag ff = *reinterpret_cast<const Frag*>(sF + lds_off(l15, chunk));
                    if constexpr (KP > 1) {
                        const int part = kt / steps_per_part;  // wave-uniform: the K-step lies inside one part's column run
                        if (part == 0) {
#pragma unroll
                            for (int mi = 0; mi < MI; ++mi) pacc[mi] = Mfma<T>::run(ff, af[mi], pacc[mi]);
                        }
#pragma unroll
                        for (int g = 1; g < KP; ++g)
                            if (part == g) {
#pragma unroll
                                for (int mi = 0; mi < MI; ++mi) pacc_x[g - 1][mi] = Mfma<T>::run(ff, af[mi], pacc_x[g - 1][mi]);
                            }
                    } else {
#pragma unroll
                    for (int mi = 0; mi < MI; ++mi) pacc[mi] = Mfma<T>::run(ff, af[mi], pacc[mi]);
                    }
                }
                if constexpr (MAIN) {
                    Frag bf[NI];
#pragma unroll
                    for (int ni = 0; ni < NI; ++ni)
                        bf[ni] = *reinterpret_cast<const Frag*>(sB + lds_off(wn * WTN + ni * 16 + l15, chunk));
#pragma unroll
                    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                        for (int ni = 0; ni < NI; ++ni) acc[mi][ni] = Mfma<T>::run(bf[ni], af[mi], acc[mi][ni]);
                }
            }
        } else {
            // f32: lane (row l15, group lq) holds chunk lq+4h = 4 consecutive k; element e of every
            // lane feeds k-step e, so A and B agree on k per lane group (the sum order is free).
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int chunk = lq + 4 * h;
                f32x4 af[MI];
#pragma unroll
                for (int mi = 0; mi < MI; ++mi)
                    af[mi] = *reinterpret_cast<const f32x4*>(sA + lds_off(wm * WTM + mi * 16 + l15, chunk));
                if ((kt * 2 + h) % WN == wn) {
                    const f32x4 ff = *reinterpret_cast<const f32x4*>(sF + lds_off(l15, chunk));
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int mi = 0; mi < MI; ++mi)
                            pacc[mi] = __builtin_amdgcn_mfma_f32_16x16x4f32(ff[e], af[mi][e], pacc[mi], 0, 0, 0);
                }
                if constexpr (MAIN) {
                    f32x4 bf[NI];
#pragma unroll
                    for (int ni = 0; ni < NI; ++ni)
                        bf[ni] = *reinterpret_cast<const f32x4*>(sB + lds_off(wn * WTN + ni * 16 + l15, chunk));
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                            for (int ni = 0; ni < NI; ++ni)
                                acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(bf[ni][e], af[mi][e],
                                                                                  acc[mi][ni], 0, 0, 0);
                }
            }
        }
    };

    int nk = (Kc + BK - 1) / BK;
    const int kt0 = slice * p.steps_per_slice;  // first K-step of this workgroup (0 unless split-K)
    if constexpr (SPLITK) nk = nk - kt0 < p.steps_per_slice ? nk - kt0 : p.steps_per_slice;
    int buf = 0;  // ring position: after the loop, the buffer that would be filled next — i.e. a FREE one
    if constexpr (PIPE) {
        // ---- LDS-DMA ring.  Lane (row, physical chunk c') fetches logical chunk c' ^ (row & 7): the DMA
        // writes lane-linearly, so the swizzle lives on the source address and on the fragment reads.
        constexpr int L = PA + (MAIN ? PB : 0);  // DMA loads per lane per stage (+1 on the two factor-loading waves)
        static_assert(kStages <= 6 && 4 * (L + 1) < 64, "counted waits cover up to four newer stages; vmcnt is a 6-bit field");
        const int src_off = (ld_chunk ^ (ld_row & 7)) * VEC;
        const int wave_rows = wave * 8 * kRowBytes;
        auto issue = [&](int kt, int buf) {
            char* st = smem + buf * STAGE + wave_rows;
            const int k0 = (kt0 + kt) * BK + src_off;
#pragma unroll
            for (int i = 0; i < PA; ++i) glds16(a_ptr[i] + k0, st + RPP * i * kRowBytes);
            if constexpr (MAIN) {
#pragma unroll
                for (int i = 0; i < PB; ++i) glds16(b_ptr[i] + k0, st + OFF_B + RPP * i * kRowBytes);
            }
            if (wave < 2) glds16(f_ptr + k0, st + OFF_F);
        };
        constexpr int DIST = kStages - 1;  // K-steps in flight ahead of the one being multiplied
#pragma unroll
        for (int i = 0; i < DIST; ++i)
            if (i < nk) issue(i, i);
        STAMP(2);
        for (int kt = 0; kt < nk; ++kt) {
            // stage kt has landed for this wave once only the loads of the stages issued after it are outstanding:
            // `ahead` of them, L loads each (L + 1 on the two waves that also fetch the factor rows)
            const int left = nk - 1 - kt;
            const int ahead = left < DIST - 1 ? left : DIST - 1;
            const bool fw = wave < 2;
            switch (ahead) {
                case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
                case 1:
                    if (fw) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(L + 1) : "memory");
                    else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(L) : "memory");
                    break;
                case 2:
                    if (fw) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * (L + 1)) : "memory");
                    else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * L) : "memory");
                    break;
                case 3:
                    if (fw) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * (L + 1)) : "memory");
                    else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * L) : "memory");
                    break;
                default:
                    if (fw) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * (L + 1)) : "memory");
                    else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * L) : "memory");
                    break;
            }
            __builtin_amdgcn_s_barrier();  // every wave's part of stage kt is in; stage kt-1 is fully read
            if (kt == 0) STAMP(3);
            char* const refill = smem + (buf >= 1 ? buf - 1 : kStages - 1) * STAGE;  // the buffer read last step
            if (kt + DIST < nk) {
                if (!(LORA_GEMM_DBG & 1)) issue(kt + DIST, buf >= 1 ? buf - 1 : kStages - 1);
            } else if (MAIN && kt == nk - 1) {  // (every K-slice of a split tile: any of them may turn out to be the last arriver)
                sQ = refill + QOFF;  // nothing left to prefetch: the epilogue's Q tile takes the free buffer
                issue_q(sQ);
            }
            // (round 3, measured: the refill's DMA instructions spread BETWEEN this step's MFMAs instead of issued as one burst
            //  here — same counted waits, same buffers — is slower on every shape: 4096×640×640 12.6 → 14.0 µs, 1024×1280×1280
            //  equal, and the 128-row tiles spill (address registers stay live across the MFMA stream): 35.7 → 51.6 µs)
            if (!(LORA_GEMM_DBG & 2)) compute(smem + buf * STAGE, kt);
            buf = buf + 1 == kStages ? 0 : buf + 1;
        }
    } else {
        // ---- register-staged fallback (ragged contraction): unconditional clamped loads, zero on write ----
        Chunk<T> ra[PA];
        Chunk<T> rb[MAIN ? PB : 1];
        Chunk<T> rfc;
        int staged_k = 0;
        auto load_step = [&](int k0) {
            const int kc = k0 + ld_chunk * VEC;
            const int kld = kc < Kc ? kc : Kc - VEC;  // Kc % VEC == 0 on this path
            staged_k = kc;
#pragma unroll
            for (int i = 0; i < PA; ++i) ra[i] = *reinterpret_cast<const Chunk<T>*>(a_ptr[i] + kld);
            if constexpr (MAIN) {
#pragma unroll
                for (int i = 0; i < PB; ++i) rb[i] = *reinterpret_cast<const Chunk<T>*>(b_ptr[i] + kld);
            }
            rfc = *reinterpret_cast<const Chunk<T>*>(f_ptr + kld);
        };
        auto store_step = [&]() {
            if (staged_k >= Kc) {
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
#pragma unroll
                    for (int i = 0; i < PA; ++i) ra[i].v[e] = from_f32<T>(0.f);
                    if constexpr (MAIN) {
#pragma unroll
                        for (int i = 0; i < PB; ++i) rb[i].v[e] = from_f32<T>(0.f);
                    }
                    rfc.v[e] = from_f32<T>(0.f);
                }
            }
#pragma unroll
            for (int i = 0; i < PA; ++i)
                *reinterpret_cast<Chunk<T>*>(smem + lds_off(ld_row + RPP * i, ld_chunk)) = ra[i];
            if constexpr (MAIN) {
#pragma unroll
                for (int i = 0; i < PB; ++i)
                    *reinterpret_cast<Chunk<T>*>(smem + OFF_B + lds_off(ld_row + RPP * i, ld_chunk)) = rb[i];
            }
            if (ld_row < kRP) *reinterpret_cast<Chunk<T>*>(smem + OFF_F + lds_off(ld_row, ld_chunk)) = rfc;
        };
        load_step(kt0 * BK);
        for (int kt = 0; kt < nk; ++kt) {
            if (kt > 0) __syncthreads();
            store_step();
            __syncthreads();
            if (kt + 1 < nk) load_step((kt0 + kt + 1) * BK);
            compute(smem, kt);
        }
    }

    STAMP(4);
    // ---- epilogue 1: combine the two partial P tiles through LDS --------------------------
    // Ring kernels put the P image into the ring buffer that is FREE after the last step (nothing in flight, last
    // read one step ago behind a barrier) and, for 16-bit types, the C tile into the buffer of the last step (free
    // once every wave has passed the barrier below): two workgroup barriers in the whole epilogue instead of four.
    constexpr bool FREEBUF = PIPE;
    constexpr bool FASTC = PIPE && MAIN && !F32;
    static_assert(!FREEBUF || QOFF + (MAIN ? BN * kRP * (int)sizeof(T) : 0) <= STAGE, "P image + Q tile must fit one ring buffer");
    char* const last_buf = smem + (buf == 0 ? kStages - 1 : buf - 1) * STAGE;
    if constexpr (FREEBUF) {
        sP = reinterpret_cast<float*>(smem + buf * STAGE);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's share of the Q tile has landed (barrier below: everyone's)
    } else {
        __syncthreads();
    }
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
        const int row = wm * WTM + mi * 16 + l15;
        *reinterpret_cast<f32x4*>(&sP[(wn * BM + row) * kSPS + lq * 4]) = pacc[mi];
    }
    __syncthreads();

    if constexpr (SPLITK) {
        static_assert(PIPE && GATE == 0, "split-K exists on the ungated ring kernels");
        {
            // In-launch split-K combine (cdna_hip_programming.md, "Projection GEMM" item 2, the sc1 form): every byte that
            // crosses workgroups is stored WRITE-THROUGH (sc1) and loaded sc1 — the XCDs' L2s are not coherent with each
            // other and a CU's L1 is never refreshed, so plain accesses would need an agent-scope release in every slice
            // (an L2 write-back: measured 4–10× the whole kernel) and an acquire in the reducer.  Order: sc1 stores → every
            // wave drains its stores (vmcnt(0)) → workgroup barrier → ONE lane draws the ticket (agent-scope atomic).
            typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
            const int S = p.splitk;
            const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(
                p.ws_c + (int64_t)tile * S * (BM * BN), 0, MAIN ? S * BM * BN * 4 : 0, 0x00020000);
            const __amdgpu_buffer_rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc(
                p.ws_p + (int64_t)tile * S * (BM * kRP), 0, S * BM * kRP * 4, 0x00020000);
            // (a) this slice's partial sums: P (all 16 rank slots; every column tile keeps its own copy, its last arriver
            // needs it) and the fp32 accumulators in the lanes' own register order — perfectly coalesced 16-byte stores,
            // no edge handling (rows / columns past the edge are never stored to C)
            {
                const int half = tid & 1;
                for (int row = tid >> 1; row < BM; row += NT / 2) {
                    f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int w = 0; w < WN; ++w) {
                        const f32x4* src = reinterpret_cast<const f32x4*>(&sP[(w * BM + row) * kSPS + half * 8]);
                        a += src[0];
                        b += src[1];
                    }
                    const int off = ((slice * BM + row) * kRP + half * 8) * 4;
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, a), rp, off, 0, 16);
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, b), rp, off + 16, 0, 16);
                }
            }
            if constexpr (MAIN) {
#pragma unroll
                for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                    for (int ni = 0; ni < NI; ++ni)
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, acc[mi][ni]), rc,
                                                               (slice * (BM * BN) + ((mi * NI + ni) * NT + tid) * 4) * 4, 0, 16);
            }
            // (b) ticket.  The flag lives in the buffer of the last K-step, free since the barrier behind the P exchange.
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // EVERY storing wave drains before the barrier
            __syncthreads();
            volatile unsigned* flag = reinterpret_cast<volatile unsigned*>(last_buf);
            if (tid == 0) {
                const unsigned old = __hip_atomic_fetch_add(p.tickets + tile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const bool last = old == (unsigned)(S - 1);
                if (last) __hip_atomic_store(p.tickets + tile, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                *flag = last ? 1u : 0u;
            }
            __syncthreads();
            STAMP(14);  // (diagnostic build: slab stored, ticket drawn)
            if (*flag == 0u) {
                STAMP(8);
                STAMP_WALL(9);
                return;
            }
            // (c) the last arriver: totals over the slices in index order (its own contribution included, from memory, so
            // that the order of the additions never depends on who came last).  EVERY load of a slab is an sc1 load.
            if constexpr (MAIN) {
#pragma unroll
                for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                    for (int ni = 0; ni < NI; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
                for (int s = 0; s < S; ++s) {
                    u32x4 v[MI][NI];
#pragma unroll
                    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                        for (int ni = 0; ni < NI; ++ni)
                            v[mi][ni] = __builtin_amdgcn_raw_buffer_load_b128(
                                rc, (s * (BM * BN) + ((mi * NI + ni) * NT + tid) * 4) * 4, 0, 16);
#pragma unroll
                    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                        for (int ni = 0; ni < NI; ++ni) acc[mi][ni] += __builtin_bit_cast(f32x4, v[mi][ni]);
                }
            }
            {
                // total P of the tile's rows goes into wave slot 0 of the P image, zeros into the other slots: everything
                // below sums the slots exactly as it does for an unsplit tile
                const int half = tid & 1;
                for (int row = tid >> 1; row < BM; row += NT / 2) {
                    f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
                    for (int s = 0; s < S; ++s) {
                        const int off = ((s * BM + row) * kRP + half * 8) * 4;
                        a += __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rp, off, 0, 16));
                        b += __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rp, off + 16, 0, 16));
                    }
                    f32x4* dst = reinterpret_cast<f32x4*>(&sP[row * kSPS + half * 8]);
                    dst[0] = a;
                    dst[1] = b;
#pragma unroll
                    for (int w = 1; w < WN; ++w) {
                        f32x4* z = reinterpret_cast<f32x4*>(&sP[(w * BM + row) * kSPS + half * 8]);
                        z[0] = f32x4{0.f, 0.f, 0.f, 0.f};
                        z[1] = f32x4{0.f, 0.f, 0.f, 0.f};
                    }
                }
            }
            __syncthreads();
        }
    }
    static_assert(!RS || (MAIN && GATE != 2 && KP == 1), "row gates exist on the single-layer forward kernels");
    // RS: factor of rank slot j in tile row `row` — scale·G[sample][j], formed in fp32 before it meets P (slots >= r hold P = 0 and
    // have no table column: factor 0; rows past M read the last row's sample and are never stored)
    auto gate_row = [&](int row) -> const float* {
        int64_t m = m0 + row;
        if (m > p.M - 1) m = p.M - 1;
        return p.row_scale + (m / p.rs_rps) * p.rs_ld;
    };
    auto gate_factor = [&](const float* g, int j) -> float {
        const float f = p.scale * g[j < p.r ? j : p.r - 1];
        return j < p.r ? f : 0.f;
    };
    constexpr bool PACKED_P = MAIN && !F32 && PIPE;  // the rank-r term's operand is built ONCE per row, cooperatively
    constexpr int kPkStride = 80;                     // bytes per row of the packed image [hi j0..15 | lo j0..15] (+16 pad)
    char* const sPk = reinterpret_cast<char*>(sP) + QOFF + (MAIN ? BN * kRP * (int)sizeof(T) : 0);
    static_assert(KP == 1 || (PACKED_P && !SPLITK && GATE == 0), "part-wise contractions exist on the plain 16-bit ring kernels");
    // thread = (row, half of the 16 rank slots): sums the wave partials, writes P out, and leaves s·P split into a
    // high and a low 16-bit part in MFMA operand order — every wave then fetches a fragment with ONE 16-byte read
    // instead of rebuilding it from 2·WN fp32 reads and 40 conversions per lane (4× redundantly across the workgroup)
    auto build_packed = [&](int part) {
        if constexpr (PACKED_P) {
        static_assert(!PACKED_P || QOFF + BN * kRP * (int)sizeof(T) + BM * kPkStride <= STAGE, "P partials + Q tile + packed P fit one buffer");
        const int half = tid & 1;
        for (int row = tid >> 1; row < BM; row += NT / 2) {
            f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int w = 0; w < WN; ++w) {
                const f32x4* src = reinterpret_cast<const f32x4*>(&sP[(w * BM + row) * kSPS + half * 8]);
                a += src[0];
                b += src[1];
            }
            const float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
            if (write_p && m0 + row < p.M) {
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (half * 8 + e < p.r) Pout[(m0 + row) * p.ldp + part * p.r + half * 8 + e] = v[e];
            }
            Chunk<T> hi, lo;
            float fac[8];
            if constexpr (RS) {
                const float* g = gate_row(row);
#pragma unroll
                for (int e = 0; e < 8; ++e) fac[e] = gate_factor(g, half * 8 + e);
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float sv;
                if constexpr (RS) sv = v[e] * fac[e];
                else sv = v[e] * p.scale;
                hi.v[e] = from_f32<T>(sv);
                lo.v[e] = from_f32<T>(sv - to_f32<T>(hi.v[e]));
            }
            *reinterpret_cast<Chunk<T>*>(sPk + row * kPkStride + half * 16) = hi;
            *reinterpret_cast<Chunk<T>*>(sPk + row * kPkStride + 32 + half * 16) = lo;
        }
        __syncthreads();
        }
    };
    // acc += s·P·Qᵀ as ONE extra MFMA K-step out of the packed record and the Q tile at `q_base`
    auto rank_step_packed = [&](const char* q_base) {
        if constexpr (PACKED_P) {
            using Frag = typename Mfma<T>::Frag;
            const int j0 = 8 * (lq & 1);
            Frag qf[NI];
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
                qf[ni] = *reinterpret_cast<const Frag*>(q_base + ((wn * WTN + ni * 16 + l15) * kRP + j0) * (int)sizeof(T));
            Frag pf[MI];
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
                pf[mi] = *reinterpret_cast<const Frag*>(sPk + (wm * WTM + mi * 16 + l15) * kPkStride + lq * 16);
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int ni = 0; ni < NI; ++ni) acc[mi][ni] = Mfma<T>::run(qf[ni], pf[mi], acc[mi][ni]);
        }
    };
    if constexpr (PACKED_P) {
        if constexpr (KP > 1) {
            // Parts 1.. of the epilogue factor go into the buffer of the last K-step (free since the barrier behind the P
            // exchange; the C tile lands there only after the last part): fetched by DMA while part 0 is worked on.
            constexpr int QB = BN * kRP * (int)sizeof(T);
            static_assert((KP - 1) * QB <= STAGE, "the epilogue factors of parts 1.. fit the last step's buffer");
#pragma unroll
            for (int g = 1; g < KP; ++g) issue_q(last_buf + (g - 1) * QB, g);
            build_packed(0);
            rank_step_packed(sQ);
#pragma unroll
            for (int g = 1; g < KP; ++g) {
                __syncthreads();  // every wave is done with the previous part's partials and packed record
#pragma unroll
                for (int mi = 0; mi < MI; ++mi) {
                    const int row = wm * WTM + mi * 16 + l15;
                    *reinterpret_cast<f32x4*>(&sP[(wn * BM + row) * kSPS + lq * 4]) = pacc_x[g - 1][mi];
                }
                if (g == 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's share of Q_1.. has landed
                __syncthreads();
                build_packed(g);
                rank_step_packed(last_buf + (g - 1) * QB);
            }
            __syncthreads();  // the Q tiles in the last step's buffer are dead: the C tile may land there
        } else {
            build_packed(0);
        }
    } else if (write_p) {
        const int half = tid & 1;
        for (int row = tid >> 1; row < BM && m0 + row < p.M; row += NT / 2) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int j = half * 8 + e;
                if (j < p.r) {
                    float v = 0.f;
#pragma unroll
                    for (int w = 0; w < WN; ++w) v += sP[(w * BM + row) * kSPS + j];
                    Pout[(m0 + row) * p.ldp + j] = v;
                }
            }
        }
    }

    STAMP(5);
    if constexpr (MAIN) {
        // ---- epilogue 2: acc += s·P·Qᵀ as one extra MFMA K-step ---------------------------
        if constexpr (!F32) {
            using Frag = typename Mfma<T>::Frag;
            if constexpr (PACKED_P) {
                if constexpr (KP == 1) rank_step_packed(sQ);
            } else {
            const int j0 = 8 * (lq & 1);
            Frag qf[NI];
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
                qf[ni] = *reinterpret_cast<const Frag*>(
                    sQ + ((wn * WTN + ni * 16 + l15) * kRP + j0) * (int)sizeof(T));
            constexpr int MG = MI < 4 ? MI : 4;  // row fragments whose P image is fetched together
#pragma unroll
            for (int mg = 0; mg < MI; mg += MG) {
                f32x4 pimg[MG][WN][2];
#pragma unroll
                for (int i = 0; i < MG; ++i) {
                    const int row = wm * WTM + (mg + i) * 16 + l15;
#pragma unroll
                    for (int w = 0; w < WN; ++w) {
                        const f32x4* src = reinterpret_cast<const f32x4*>(&sP[(w * BM + row) * kSPS + j0]);
                        pimg[i][w][0] = src[0];
                        pimg[i][w][1] = src[1];
                    }
                }
#pragma unroll
                for (int i = 0; i < MG; ++i) {
                    Frag pf;
                    float fac[8];
                    if constexpr (RS) {
                        const float* g = gate_row(wm * WTM + (mg + i) * 16 + l15);
#pragma unroll
                        for (int e = 0; e < 8; ++e) fac[e] = gate_factor(g, j0 + e);
                    }
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        float v = 0.f;
#pragma unroll
                        for (int w = 0; w < WN; ++w) v += pimg[i][w][e >> 2][e & 3];
                        if constexpr (RS) v *= fac[e];
                        else v *= p.scale;
                        const T hi = from_f32<T>(v);
                        const T lo = from_f32<T>(v - to_f32<T>(hi));
                        pf[e] = lq < 2 ? hi : lo;
                    }
#pragma unroll
                    for (int ni = 0; ni < NI; ++ni) acc[mg + i][ni] = Mfma<T>::run(qf[ni], pf, acc[mg + i][ni]);
                }
            }
            }
        } else {
            const float* q = reinterpret_cast<const float*>(sQ);
#pragma unroll
            for (int st = 0; st < 4; ++st) {
                const int j = 4 * st + lq;
                float qv[NI];
#pragma unroll
                for (int ni = 0; ni < NI; ++ni) qv[ni] = q[(wn * WTN + ni * 16 + l15) * kRP + j];
#pragma unroll
                for (int mi = 0; mi < MI; ++mi) {
                    const int row = wm * WTM + mi * 16 + l15;
                    float pv = 0.f;
#pragma unroll
                    for (int w = 0; w < WN; ++w) pv += sP[(w * BM + row) * kSPS + j];
                    if constexpr (RS) pv *= gate_factor(gate_row(row), j);
                    else pv *= p.scale;
#pragma unroll
                    for (int ni = 0; ni < NI; ++ni)
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(qv[ni], pv, acc[mi][ni], 0, 0, 0);
                }
            }
        }

        STAMP(6);
        // ---- epilogue 3: bias (fp32), transpose through LDS, 16-B row stores -------------
        if (p.bias != nullptr) {
#pragma unroll
            for (int ni = 0; ni < NI; ++ni)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg)
#pragma unroll
                    for (int mi = 0; mi < MI; ++mi) acc[mi][ni][reg] += bias_v[ni][reg];
        }
        constexpr int SC_STRIDE = BN * (int)sizeof(T) + 16;
        // the C tile leaves in EP passes of ROWS rows (one pass when it fits the LDS area it is staged in)
        constexpr int EP = F32 ? 2 : (FASTC && BM * SC_STRIDE > STAGE ? 2 : 1);
        static_assert(WM % EP == 0, "a pass covers whole row waves");
        constexpr int ROWS = BM / EP;
        constexpr int CPR = BN / VEC;  // 16-B chunks per tile row
        static_assert(!FASTC || ROWS * SC_STRIDE <= STAGE, "C tile must fit one ring buffer");
        char* const sC = FASTC ? last_buf : smem;
        T* Cg = static_cast<T*>(p.C);
#pragma unroll
        for (int ep = 0; ep < EP; ++ep) {
            if (!FASTC || ep > 0) __syncthreads();  // sP / sQ (or the previous pass) are dead
            if (EP == 1 || wm / (WM / EP) == ep) {
#pragma unroll
                for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                    for (int ni = 0; ni < NI; ++ni) {
                        // the lane owns 4 consecutive columns of one row: one 8-/16-byte LDS write
                        const int row = (EP == 1 ? wm : wm % (WM / EP)) * WTM + mi * 16 + l15;
                        const int col = wn * WTN + ni * 16 + lq * 4;
                        Quad<T> q;
#pragma unroll
                        for (int reg = 0; reg < 4; ++reg) q.v[reg] = from_f32<T>(acc[mi][ni][reg]);
                        *reinterpret_cast<Quad<T>*>(sC + row * SC_STRIDE + col * (int)sizeof(T)) = q;
                    }
            }
            __syncthreads();
            STAMP(7);
            if constexpr (GATE == 2) {
                // GEGLU BACKWARD in the epilogue of the GEMM that produces its incoming gradient: this launch is
                //     dout[M,F] = dZ[M,Nz]·W2        (backward-input of the linear layer behind the gate: ff.net.2)
                // and the tile in LDS is dout, rounded to the storage type exactly as the separate tensor would be.  Thread =
                // (row, chunk): it loads the h and g chunks of Y = [h | g] (p.C2, read-only) and writes the two halves of
                //     dY[:, :F] = dout·gelu(g),   dY[:, F:] = dout·h·gelu'(g)        (p.C)
                // — the arithmetic of geglu_bwd_kernel on the same values; dout itself never goes to memory.
                // (Per pass of ROWS rows; a chunk count that does not divide over the threads runs its last trip on clamped
                //  indices with the stores predicated — loads are never under a per-lane condition.)
                static_assert(FASTC, "the gate epilogue reads the C tile from a ring buffer");
                constexpr int TOT = ROWS * CPR;
                constexpr int NST = (TOT + NT - 1) / NT;
                constexpr int H0 = (NST + 1) / 2;  // two register batches
                const T* Yg = static_cast<const T*>(p.C2);
                const int F = p.gateF;
#pragma unroll
                for (int hb = 0; hb < 2; ++hb) {
                    const int first = hb == 0 ? 0 : H0, cnt = hb == 0 ? H0 : NST - H0;
                    Chunk<T> dv[H0], hv[H0], gv[H0];
#pragma unroll
                    for (int i = 0; i < H0; ++i) {
                        if (i < cnt) {
                            int idx = tid + (first + i) * NT;
                            if (TOT % NT != 0 && idx > TOT - 1) idx = TOT - 1;
                            const int row = idx / CPR, ch = idx - row * CPR;
                            int64_t m = m0 + ep * ROWS + row;
                            if (m > p.M - 1) m = p.M - 1;  // rows past the end: loaded from a valid row, never stored
                            const T* yrow = Yg + m * (2 * (int64_t)F) + n0 + ch * VEC;
                            hv[i] = *reinterpret_cast<const Chunk<T>*>(yrow);
                            gv[i] = *reinterpret_cast<const Chunk<T>*>(yrow + F);
                            dv[i] = *reinterpret_cast<const Chunk<T>*>(sC + row * SC_STRIDE + ch * 16);
                        }
                    }
#pragma unroll
                    for (int i = 0; i < H0; ++i) {
                        if (i < cnt) {
                            const int idx = tid + (first + i) * NT;
                            const int row = idx / CPR, ch = idx - row * CPR;
                            const int64_t m = m0 + ep * ROWS + row;
                            Chunk<T> dh, dg;
#pragma unroll
                            for (int e = 0; e < VEC; ++e) {
                                const float g = to_f32<T>(gv[i].v[e]), d = to_f32<T>(dv[i].v[e]);
                                dh.v[e] = from_f32<T>(d * gelu_f<T>(g));
                                dg.v[e] = from_f32<T>(d * to_f32<T>(hv[i].v[e]) * gelu_grad_f<T>(g));
                            }
                            if (idx < TOT && m < p.M) {
                                T* drow = Cg + m * (2 * (int64_t)F) + n0 + ch * VEC;
                                *reinterpret_cast<Chunk<T>*>(drow) = dh;
                                *reinterpret_cast<Chunk<T>*>(drow + F) = dg;
                            }
                        }
                    }
                }
                continue;
            }
            if constexpr (GATE == 1) {
                // thread = (row, 16-B chunk of the h half) and the chunk of g behind it: y leaves as it is (when a backward
                // pass will want it), out = h·gelu(g) from the SAME rounded values the separate gate kernel would read
                static_assert(FASTC, "the gate epilogue reads the C tile from a ring buffer");
                constexpr int HC = CPR / 2;                 // chunks per half row
                constexpr int TOT = ROWS * HC;
                constexpr int NG = (TOT + NT - 1) / NT;     // (row, chunk) pairs per thread (last trip clamped / predicated)
                T* Og = static_cast<T*>(p.C2);
                const int F = p.gateF;
                Chunk<T> hv[NG], gv[NG];
#pragma unroll
                for (int i = 0; i < NG; ++i) {
                    int idx = tid + i * NT;
                    if (TOT % NT != 0 && idx > TOT - 1) idx = TOT - 1;
                    const int row = idx / HC, ch = idx - row * HC;
                    hv[i] = *reinterpret_cast<const Chunk<T>*>(sC + row * SC_STRIDE + ch * 16);
                    gv[i] = *reinterpret_cast<const Chunk<T>*>(sC + row * SC_STRIDE + (HC + ch) * 16);
                }
                if (Cg != nullptr) {
#pragma unroll
                    for (int i = 0; i < NG; ++i) {
                        const int idx = tid + i * NT;
                        const int row = idx / HC, ch = idx - row * HC;
                        const int64_t m = m0 + ep * ROWS + row;
                        const int col = tn * (BN / 2) + ch * VEC;
                        if (idx < TOT && m < p.M) {
                            *reinterpret_cast<Chunk<T>*>(Cg + m * p.Nc + col) = hv[i];
                            *reinterpret_cast<Chunk<T>*>(Cg + m * p.Nc + F + col) = gv[i];
                        }
                    }
                }
#pragma unroll
                for (int i = 0; i < NG; ++i) {
                    const int idx = tid + i * NT;
                    const int row = idx / HC, ch = idx - row * HC;
                    const int64_t m = m0 + ep * ROWS + row;
                    Chunk<T> o;
#pragma unroll
                    for (int e = 0; e < VEC; ++e) o.v[e] = from_f32<T>(to_f32<T>(hv[i].v[e]) * gelu_f<T>(to_f32<T>(gv[i].v[e])));
                    if (idx < TOT && m < p.M) *reinterpret_cast<Chunk<T>*>(Og + m * F + tn * (BN / 2) + ch * VEC) = o;
                }
                continue;
            }
            constexpr int NST = ROWS * CPR / NT;  // 16-B chunks per thread
            static_assert(ROWS * CPR % NT == 0, "tile rows must split evenly over the threads");
            Chunk<T> out[NST];
#pragma unroll
            for (int i = 0; i < NST; ++i) {
                const int idx = tid + i * NT;
                const int row = idx / CPR, ch = idx - row * CPR;
                out[i] = *reinterpret_cast<const Chunk<T>*>(sC + row * SC_STRIDE + ch * 16);
            }
#pragma unroll
            for (int i = 0; i < NST; ++i) {
                const int idx = tid + i * NT;
                const int row = idx / CPR, ch = idx - row * CPR;
                const int64_t m = m0 + ep * ROWS + row;
                const int col = n0 + ch * VEC;
                if (m < p.M && col < p.Nc) *reinterpret_cast<Chunk<T>*>(Cg + m * p.Nc + col) = out[i];
            }
        }
    }
    STAMP(8);
    STAMP_WALL(9);
}

}  // namespace

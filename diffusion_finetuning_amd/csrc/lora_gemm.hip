// Host side of the LoRA-fused GEMM: which instantiation of lora_gemm_kernel (lora_gemm_kernel.h: the kernel, its structure and
// its argument block) a shape runs on — plan_splitk(), gate_tile_width(), launch_pipe(), launch_typed() — and the C entries.
// Shapes the kernel does not take fall back to lora_gemm_generic.h.  The factor packing the fast path expects: lora_pack.hip.
#include "lora_gemm_kernel.h"
#include "lora_gemm_generic.h"

namespace {

// Split-K plan.  Splitting buys chip occupancy with a combine that costs the tile ≈ 5–6 µs (write-through slab stores, the
// ticket's round trip, the last arriver's serial slab reads at the cross-XCD rate), so it pays only for LONG contractions on
// under-filled grids: measured (profiles/r03_splitk_sweep_*.log, weights cold) the 20-K-step 1280-wide projections LOSE 2–3 µs at
// every slice count (1024×1280×1280: 15.7 → 18.5 µs), the 60-K-step grouped q/k/v backward gains 5–8 µs (35 → 30, 26 → 19),
// the 80/160-K-step GEGLU `proj` backward 18–30 µs (66 → 48, 84 → 54, 62 → 31).  Returns the slice count (1 = off) and the
// row-tile height of the split launch: ≈ 480 workgroups, 64-row tiles on the small grids (two per CU overlap each other's
// phases), at least 10 K-steps left per slice.
struct SplitPlan {
    int S, bm;
};
// The S slices of a tile run as neighbours on one XCD.  Round 4 measured slice s on XCD s % S instead
// (profiles/r04_splitk_xcd_affinity_ab.log, weights cold): it cuts the operand fetch to |Am| + |Bm| as intended, but the last
// arriver's slab reads then cross the fabric instead of hitting the L2 that holds the neighbours' write-through stores —
// 4096×5120→640 49.5 → 64.0 µs, 1024×10240→1280 57.7 → 71.4, 256×10240→1280 29.8 → 35.1, grouped q/k/v backward at 1024 rows
// 30.6 → 39.7: these launches are paced by the combine and their fixed phases, not by operand traffic.
constexpr int kTicketBytes = LORA_GEMM_WS_TICKET_BYTES;  // ticket header of the workspace: one u32 per output tile
SplitPlan plan_splitk(int64_t M, int Kc, int Nc, int esize) {
    SplitPlan off{1, 128};
    const int nk = (Kc * esize + kRowBytes - 1) / kRowBytes;
    const int64_t tiles128 = ((M + 127) / 128) * ((Nc + 127) / 128);
    const int64_t tiles64 = ((M + 63) / 64) * ((Nc + 127) / 128);
    if ((Nc & 7) != 0 || (Kc * esize) % kRowBytes != 0 || tiles128 >= 192) return off;
    if (nk < 48) return off;
    int bm = tiles128 <= 96 ? 64 : 128;
    // round 5 (profiles/r05_splitk_plan_sweep.log, weights cold): a split launch is paced by its MAIN LOOP — 74 % of the 48-µs
    // 1024×10240→1280 launch, 0.67 µs per K-step at two workgroups per CU: the L1-fill bound of the unsplit kernels — not by the
    // combine (slab store + ticket 2 µs, the last arriver's sum 3.7 µs).  So the longest contractions take the 128-row tile (0.65× the
    // L1 bytes per flop) with more slices where that still fills the chip: 80 tiles × 6 slices, 58.2 → 53.5 µs.
    if (tiles128 >= 64 && nk >= 128) bm = 128;
    const int64_t tiles = bm == 64 ? tiles64 : tiles128;
    if (tiles > kTicketBytes / 4) return off;
    int S = (int)((480 + tiles / 2) / tiles);
    if (S > 8) S = 8;
    const int min_steps = 10;
    while (S > 1 && nk / S < min_steps) --S;
    while (S > 1 && (S - 1) * ((nk + S - 1) / S) >= nk) --S;  // every slice owns at least one K-step
    return SplitPlan{S, bm};
}
int64_t splitk_ws_bytes(int64_t M, int Nc, const SplitPlan& sp) {
    const int64_t tm = (M + sp.bm - 1) / sp.bm, tn = (Nc + 127) / 128;
    return kTicketBytes + tm * tn * sp.S * ((int64_t)sp.bm * 128 + (int64_t)sp.bm * kRP) * 4;
}

// Launches one instantiation of lora_gemm_kernel under profiler id PROF.  The LDS limit is raised once per instantiation: the
// function-local static belongs to this function's own instantiation, of which there is one per kernel.
template <auto Kern, int LDS, int PROF>
int launch_instance(int blocks, int threads, const GemmParams& p, hipStream_t stream) {
    static const hipError_t attr =
        hipFuncSetAttribute(reinterpret_cast<const void*>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
    if (attr != hipSuccess) return LORA_E_LAUNCH;
    LORA_LAUNCH(PROF, Kern, dim3(blocks), dim3(threads), LDS, stream, p);
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}

template <typename T, int BM, int BN, bool MAIN, int STG, int NW = 4, int WM = 2>
int launch_tile(GemmParams p, hipStream_t stream) {
    p.tiles_m = (int)((p.M + BM - 1) / BM);
    p.tiles_n = MAIN ? (p.Nc + BN - 1) / BN : (p.part_table ? p.tiles_n : 1);  // skinny grouped: tiles_n = parts
    if (p.ldp == 0) p.ldp = p.r;
    p.col_major = MAIN && (int64_t)p.Nc > p.M ? 1 : 0;
    p.xcd_m = 1;
    if (MAIN && p.splitk <= 1 && p.tile_part == nullptr && p.n_parts == 0) {
        // Which XCD grid re-fetches the fewest operand bytes?  An xm × xn grid (xm·xn = 8) makes the eight L2s fetch
        // xn·|Am| + xm·|Bm| in total; (8,1) and (1,8) are the row- / column-major runs above (any tile counts), the 2-D
        // grids need exact splits.  Only square-ish problems (the 1280-wide layers at 1024 / 256 rows) pick one.
        const double am = (double)p.M * p.Kc, bm = (double)p.Nc * p.Kc;
        double best = p.col_major ? 8.0 * am + bm : am + 8.0 * bm;
        for (int xm = 2; xm <= 4; xm *= 2) {
            const int xn = 8 / xm;
            if (p.tiles_m % xm != 0 || p.tiles_n % xn != 0) continue;
            const double cost = xn * am + xm * bm;
            if (cost < 0.8 * best) {
                best = cost;
                p.xcd_m = xm;
            }
        }
    }
    constexpr int lds = gemm_lds_bytes<BM, BN, T, MAIN, STG, NW, WM>();
    constexpr bool CAN_SPLIT = MAIN && STG > 0 && NW == 4 && BN == 128 && (BM == 64 || BM == 128);  // what plan_splitk hands out
    constexpr int prof_id = MAIN ? (BM >= 256 ? PK_GEMM_256x128 : (BM == 128 ? PK_GEMM_128x128 : PK_GEMM_64x64))
                                 : (BM == 128 ? PK_SKINNY_128 : PK_SKINNY_64);
    // per-row gates: the RS twin of whatever kernel the shape would run on (MAIN kernels only; grouped launches carry no gates)
    const bool rs = MAIN && p.row_scale != nullptr;
    if (rs && (p.tile_part != nullptr || p.n_parts != 0)) return LORA_E_UNSUPPORTED;
    if constexpr (CAN_SPLIT) {
        if (p.splitk > 1) {  // workspace = [tickets | fp32 tiles | P tiles] (splitk_ws_bytes)
            p.ws_c = reinterpret_cast<float*>(reinterpret_cast<char*>(p.tickets) + kTicketBytes);
            p.ws_p = p.ws_c + (int64_t)p.tiles_m * p.tiles_n * p.splitk * (BM * BN);
            const int blocks = p.tiles_m * p.tiles_n * p.splitk;
            if (rs) return launch_instance<lora_gemm_kernel<T, BM, BN, MAIN, STG, NW, WM, 0, true, 1, true>, lds, PK_GEMM_SPLITK>(blocks, NW * 64, p, stream);
            return launch_instance<lora_gemm_kernel<T, BM, BN, MAIN, STG, NW, WM, 0, true>, lds, PK_GEMM_SPLITK>(blocks, NW * 64, p, stream);
        }
    }
    p.splitk = 0;
    const int blocks = p.tiles_m * p.tiles_n;
    if constexpr (MAIN) {
        if (rs) return launch_instance<lora_gemm_kernel<T, BM, BN, MAIN, STG, NW, WM, 0, false, 1, true>, lds, prof_id>(blocks, NW * 64, p, stream);
    }
    return launch_instance<lora_gemm_kernel<T, BM, BN, MAIN, STG, NW, WM>, lds, prof_id>(blocks, NW * 64, p, stream);
}

// Column-tile width of the big launches.  Every SD width is a multiple of 128 AND of 160, so both tiles are exact; a
// 128×160 tile costs ≈ 1.2× a 128×128 one and the chip holds 512 of either (two workgroups per CU), so the grid with fewer,
// fatter tiles wins wherever the 128-wide grid leaves its last round mostly empty: 1024×1280→2·5120 is 640 tiles of 128 (two
// rounds, the second a quarter full) or 512 tiles of 160 (ONE round).  `gated`: the measured rule of the gated launches
// (tools/gemm_bench.py --geglu --cold-read with LORA_GATE_BN=128|160, µs 128 → 160; forward: 16384 rows 65.1 → 67.1,
// 4096 rows 60.2 → 51.0, 1024 rows 57.0 → 39.1, 256 rows 27.1 → 29.6; backward: 53.1 → 53.6, 41.0 → 35.9, 40.4 → 36.8,
// 30.1 → 34.7): 160 for grids of 257..2047 128-wide tiles.  Ungated launches use the round-count model only.
int gate_tile_width(int64_t tiles_m, int cols, bool gated) {
    if (cols % 160 != 0) return 128;
    const int64_t t128 = tiles_m * (cols / 128), t160 = tiles_m * (cols / 160);
    if (gated) return t128 > 256 && t128 < 2048 ? 160 : 128;
    const double c128 = (double)((t128 + 511) / 512), c160 = 1.25 * (double)((t160 + 511) / 512);
    return c160 < c128 ? 160 : 128;
}

// GEGLU-gated forward: the two-stage ring kernel, a tile = BN/2 h columns + their BN/2 g columns.
template <typename T, int BN>
int launch_gate_bn(GemmParams p, hipStream_t stream) {
    constexpr int BM = 128;
    p.tiles_m = (int)((p.M + BM - 1) / BM);
    p.tiles_n = p.gateF / (BN / 2);
    p.ldp = p.r;
    p.col_major = (int64_t)p.Nc > p.M ? 1 : 0;
    constexpr int lds = gemm_lds_bytes<BM, BN, T, true, 2, 4, 2>();
    const int blocks = p.tiles_m * p.tiles_n;
    if (p.row_scale != nullptr)  // per-row gates of the rank-r term: the RS twin
        return launch_instance<lora_gemm_kernel<T, BM, BN, true, 2, 4, 2, 1, false, 1, true>, lds, PK_GEMM_128x128>(blocks, 256, p, stream);
    return launch_instance<lora_gemm_kernel<T, BM, BN, true, 2, 4, 2, 1>, lds, PK_GEMM_128x128>(blocks, 256, p, stream);
}
template <typename T>
int launch_gate(GemmParams p, hipStream_t stream) {
    // (the h / g halves of a tile are column runs of 64 resp. 80: both divide every SD hidden width)
    if (gate_tile_width((p.M + 127) / 128, 2 * p.gateF, true) == 160 && p.gateF % 80 == 0) return launch_gate_bn<T, 160>(p, stream);
    return launch_gate_bn<T, 128>(p, stream);
}

// GEGLU backward in the epilogue of dout = dZ·W2: 128-row tiles over [M, F].
template <typename T, int BN>
int launch_gate_bwd_bn(GemmParams p, hipStream_t stream) {
    constexpr int BM = 128;
    p.tiles_m = (int)((p.M + BM - 1) / BM);
    p.tiles_n = p.Nc / BN;
    p.ldp = p.r;
    p.col_major = (int64_t)p.Nc > p.M ? 1 : 0;
    constexpr int lds = gemm_lds_bytes<BM, BN, T, true, 2, 4, 2>();
    return launch_instance<lora_gemm_kernel<T, BM, BN, true, 2, 4, 2, 2>, lds, PK_GATED_BWD>(p.tiles_m * p.tiles_n, 256, p, stream);
}
template <typename T>
int launch_gate_bwd(GemmParams p, hipStream_t stream) {
    if (gate_tile_width((p.M + 127) / 128, p.Nc, true) == 160) return launch_gate_bwd_bn<T, 160>(p, stream);
    return launch_gate_bwd_bn<T, 128>(p, stream);
}

// Backward-input of a grouped projection whose contraction consists of KP equal parts (lora_gemm_parts, parts_on_k): the
// part-wise kernels exist on 64-row tiles — 64×160 where the output width wants it (320, 960), else 64×128, else 64×64.
template <typename T, int BM, int BN, int STG, int KP>
int launch_kparts_tile(GemmParams p, hipStream_t stream) {
    p.tiles_m = (int)((p.M + BM - 1) / BM);
    p.tiles_n = (p.Nc + BN - 1) / BN;
    p.col_major = (int64_t)p.Nc > p.M ? 1 : 0;
    p.xcd_m = 1;
    p.splitk = 0;
    constexpr int lds = gemm_lds_bytes<BM, BN, T, true, STG, 4, 2>();
    return launch_instance<lora_gemm_kernel<T, BM, BN, true, STG, 4, 2, 0, false, KP>, lds, PK_GEMM_64x64>(p.tiles_m * p.tiles_n, 256, p, stream);
}
template <typename T, int KP>
int launch_kparts(const GemmParams& p, hipStream_t stream) {
    if constexpr (sizeof(T) == 2) {
        const int64_t tm = (p.M + 63) / 64;
        if ((p.Nc % 160) == 0 && (p.Nc % 128) != 0) return launch_kparts_tile<T, 64, 160, 2, KP>(p, stream);
        if ((p.Nc % 128) == 0) {
            if (tm * (p.Nc / 128) >= 256) return launch_kparts_tile<T, 64, 128, 2, KP>(p, stream);
            return launch_kparts_tile<T, 64, 128, 3, KP>(p, stream);
        }
        return launch_kparts_tile<T, 64, 64, 3, KP>(p, stream);
    } else {
        return LORA_E_UNSUPPORTED;
    }
}

// Tile and ring-depth choice, from tools/gemm_bench.py sweeps on MI355X — hot and with cold weights (--cold-read) — and from
// the in-model launch-class table (tools/summarize_profile.py shapes; profiles/README.md):
//  * occupancy beats prefetch depth: a 2-stage ring lets two 128-row workgroups share a CU (≤ 78 KB LDS each) and
//    is 25-35 % faster than the 3-stage ring at one workgroup per CU on every shape that fills the chip;
//  * 128×160 for widths that are multiples of 160 but not of 128 (320, 960): no padding columns;
//  * 128×128 once its grid has >= 256 tiles (and the last column tile is not mostly padding); 64×128 (2 stages) for
//    128..255-tile grids, 64×128 behind a 3-stage ring for 64..127-tile grids;
//  * 64×64 below that: 2 stages (3 workgroups per CU) when there are >= 512 tiles to overlap, else 3, or 4 stages on
//    contractions of >= 8 K-steps (the 6-stage one-workgroup form lost once the weights are cold).  128×64 never won;
//  * 256×128 / 128×256 (one 4- or 8-wave workgroup per CU, with or without a ping-pong DMA order) are correct but 5-100 %
//    slower than two independent 128-row workgroups per CU on every hot-path shape.  Not instantiated (the template
//    still supports them).
template <typename T, bool MAIN>
int launch_pipe(const GemmParams& p, hipStream_t stream) {
    if (!MAIN) return launch_tile<T, 64, 64, false, 3>(p, stream);
    if (p.splitk > 1) {  // (tile height from plan_splitk: the workspace was sized for it)
        if (p.split_bm == 64) return launch_tile<T, 64, 128, true, 3, 4>(p, stream);
        return launch_tile<T, 128, 128, true, 2, 4>(p, stream);
    }
    if (p.tile_part != nullptr) {  // grouped: 64-wide column tiles never straddle two parts
        const int64_t t64 = ((p.M + 63) / 64) * ((p.Nc + 63) / 64);
        return t64 < 512 ? launch_tile<T, 64, 64, true, 3>(p, stream) : launch_tile<T, 64, 64, true, 2>(p, stream);
    }
    const int64_t tiles128 = ((p.M + 127) / 128) * ((p.Nc + 127) / 128);
    const int64_t tiles64 = ((p.M + 63) / 64) * ((p.Nc + 63) / 64);
    const int padded = (p.Nc + 127) / 128 * 128;
    // equal parts over the output columns: a column tile must lie inside one part
    const bool p128 = p.n_parts == 0 || (p.part_n % 128) == 0, p160 = p.n_parts == 0 || (p.part_n % 160) == 0;
    const bool big = tiles128 >= 128 && (padded - p.Nc) * 4 <= p.Nc && p128;
    // (8-wave workgroups — 128×256 as 2×4 waves, 256×128 as 4×2 waves, one per CU, 26 % fewer L2→LDS bytes per flop —
    //  are supported by the template (WM parameter) and were measured: correct, 5–100 % slower on every hot-path shape,
    //  e.g. 16384×320×2560 54 vs 50 µs; not instantiated.)
    if constexpr (sizeof(T) == 2) {
        // widths that are whole multiples of 160 but not of 128 (320, 960: every q/k/v/out projection of the widest SD
        // level): 128×160 tiles waste no MFMA, LDS or L2→LDS traffic on padding columns (128-wide tiles pad 320 to 384)
        // and re-read the X panel twice instead of three times; two workgroups still share a CU (77.8 KB each)
        const int64_t tiles160 = ((p.M + 127) / 128) * (p.Nc / 160);
        const bool w160 = (p.Nc % 160) == 0 && ((p.Nc % 128) != 0 || !p128) && tiles160 >= 128 && p160;
        // ... and when that grid has fewer than 384 tiles (the 320-wide projections at 16384 rows: 256 tiles, one per CU),
        // 64×160 tiles double the count — two workgroups per CU overlap each other's fixed phases: 16384×320×320
        // 12.1 → 11.4 µs, 16384×1280→320 27.9 → 27.0 (round 3; wider outputs lose: 16384×320→1280 26.4 → 30.6)
        if (w160 && tiles160 < 384) return launch_tile<T, 64, 160, true, 2, 4>(p, stream);
        if (w160) return launch_tile<T, 128, 160, true, 2, 4>(p, stream);
        // 128×128 grids of 128..255 tiles leave a third of the CUs idle (4096×640×640: 160 tiles): 64×128 tiles double the
        // count at 3/4 of the flops per staged byte — 12.5 → 11.0 µs there, 32.8 → 28.2 µs at K = 2560
        if (big && tiles128 < 256) return launch_tile<T, 64, 128, true, 2, 4>(p, stream);
        // grids too small for 128-row tiles, measured with the weights COLD (tools/gemm_bench.py --cold-read: in the model every
        // frozen weight comes from HBM): 64×128 tiles behind a 3-stage ring (two workgroups per CU, two K-steps in flight)
        // for 64..127-tile grids — 1024×1280×1280: 17.3 → 15.0 µs, the grouped q/k/v backward at 1024 rows 39 → 34 µs
        // (round 3: the same tile behind a 4- or 5-stage ring — one workgroup per CU, as these 160-workgroup grids have anyway —
        //  is SLOWER, 15.4 → 16.0 → 16.3 µs: a lone workgroup is not waiting on prefetch depth)
        // (also measured on this grid, round 3: the same tile as ONE 8-wave workgroup — 4×2 waves, two per SIMD instead of
        //  one — 15.1 vs 15.2 µs behind 3 stages, 19.2 behind 2: neither the wave count nor a ring deeper than 3 moves it)
        if (!big && tiles128 >= 64 && (p.Nc % 128) == 0 && p128) return launch_tile<T, 64, 128, true, 3, 4>(p, stream);
        // chip-filling grids whose width divides by 128 AND 160: the tile whose grid wastes less of its last round
        if (big && p160 && tiles128 >= 256 && gate_tile_width((p.M + 127) / 128, p.Nc, false) == 160)
            return launch_tile<T, 128, 160, true, 2, 4>(p, stream);
    }
    // (a 3-stage ring on grids of <= 256 tiles — one workgroup per CU anyway — was measured: no gain, 12.8 → 13.6 µs on
    //  4096×640×640; a lone workgroup is paced by the CU's vector-memory path issuing its own DMAs, not by latency)
    if (big) return launch_tile<T, 128, 128, true, 2, 4>(p, stream);
    // long contractions on grids that leave at most ~1 workgroup per CU: only prefetch depth hides the L2/HBM latency
    // of each K-step there (4 stages = 2 workgroups per CU, 6 stages = 1)
    const bool deep = tiles64 < 512;
    const int nk = (p.Kc * (int)sizeof(T) + kRowBytes - 1) / kRowBytes;
    int ring = deep ? 3 : 2;
    if (deep && nk >= 8) ring = 4;  // (6 stages at one workgroup per CU lost to 4 stages at two once the weights are cold)
    switch (ring) {
        case 4: return launch_tile<T, 64, 64, true, 4>(p, stream);
        case 3: return launch_tile<T, 64, 64, true, 3>(p, stream);
        default: return launch_tile<T, 64, 64, true, 2>(p, stream);
    }
}

// What an entry point knows: the kernel's argument block as far as the entry can fill it (operands, sizes, scale, lda with
// 0 = Kc, tile_part / part_table of a grouped launch with tiles_n = parts of a skinny one, the per-row gates; all else zero —
// launch_typed() and the launch_* functions set the rest), and what only the host needs.
struct CallArgs : GemmParams {
    const float* F;    // fp32 master of the main-loop factor, strided (generic path)
    int64_t f_sr, f_sk;
    const float* Q;
    int64_t q_sn, q_sj;
    bool packed_only;  // no fp32 masters behind Fp/Qp: the shape-agnostic kernels cannot run
    void* workspace;   // optional fp32 scratch for split-K (lora_gemm_workspace_bytes)
    int64_t ws_bytes;
};

template <typename T>
int launch_typed(const CallArgs& c, bool main_part, hipStream_t stream) {
    constexpr int VEC = ElemTraits<T>::kVec;
    constexpr int BK = kRowBytes / (int)sizeof(T);
    const int64_t lda = c.lda > 0 ? c.lda : c.Kc;
    const bool grouped = c.tile_part != nullptr || c.part_table != nullptr;
    const bool fast = c.r <= kRP && c.Fp != nullptr && (c.Qp != nullptr || !main_part) && (c.Kc % VEC) == 0 &&
                      (lda % VEC) == 0 && aligned16(c.Am) && aligned16(c.Fp) && aligned16(c.Qp) &&
                      (!main_part || ((c.Nc % VEC) == 0 && aligned16(c.Bm) && aligned16(c.C)));
    if (fast) {
        GemmParams p = c;
        p.lda = lda;
        if (main_part && !grouped && c.workspace != nullptr && aligned16(c.workspace) && (c.Kc % BK) == 0) {
            const SplitPlan sp = plan_splitk(c.M, c.Kc, c.Nc, (int)sizeof(T));
            if (sp.S > 1 && c.ws_bytes >= splitk_ws_bytes(c.M, c.Nc, sp)) {
                const int nk = c.Kc / BK;
                p.splitk = sp.S;
                p.split_bm = sp.bm;
                p.steps_per_slice = (nk + sp.S - 1) / sp.S;
                p.tickets = static_cast<unsigned*>(c.workspace);
            }
        }
        if ((c.Kc % BK) == 0) return main_part ? launch_pipe<T, true>(p, stream) : launch_pipe<T, false>(p, stream);
        if (grouped) return LORA_E_UNSUPPORTED;  // grouped launches exist only on the LDS-DMA path
        return main_part ? launch_tile<T, 64, 64, true, 0>(p, stream) : launch_tile<T, 64, 64, false, 0>(p, stream);
    }
    if (grouped || c.packed_only || lda != c.Kc) return LORA_E_UNSUPPORTED;
    const GenericParams g{c.Am, c.Bm, c.bias, c.F, c.f_sr, c.f_sk, c.Q, c.q_sn, c.q_sj, c.C, c.P, c.M, c.Kc, c.Nc, c.r, c.scale,
                          c.row_scale, c.rs_rps, c.rs_ld};  // (every field, in the struct's order)
    const auto blocks = [](int64_t n) { return dim3((unsigned)((n + 255) / 256)); };
    hipLaunchKernelGGL(lora_skinny_generic_kernel<T>, blocks(g.M * g.r), dim3(256), 0, stream, g);
    LORA_LAUNCH_CHECK();
    if (main_part) {
        if (g.row_scale != nullptr)
            hipLaunchKernelGGL((lora_gemm_generic_kernel<T, true>), blocks(g.M * g.Nc), dim3(256), 0, stream, g);
        else
            hipLaunchKernelGGL(lora_gemm_generic_kernel<T>, blocks(g.M * g.Nc), dim3(256), 0, stream, g);
        LORA_LAUNCH_CHECK();
    }
    return LORA_OK;
}

int launch_gemm(const CallArgs& c, bool main_part, int dtype, hipStream_t stream) {
    return status_by_dtype(dtype, [&](auto tag) { return launch_typed<typename decltype(tag)::type>(c, main_part, stream); });
}

int check_common(int64_t M, int K, int N, int r, int dtype) {
    if (M < 0 || K <= 0 || N <= 0) return LORA_E_BADARG;
    if (!known_dtype(dtype)) return LORA_E_BADARG;
    if (r < 1 || r > (K < N ? K : N)) return LORA_E_RANK;
    return LORA_OK;
}

double esize(int dtype) { return dtype == LORA_F32 ? 4.0 : 2.0; }

// The gate table of a `_rows` entry: one row of >= r gates per sample, a sample being M / n_samples consecutive rows.
int check_rows(int64_t M, int r, const float* row_scale, int n_samples, int ld_scale) {
    if (row_scale == nullptr || n_samples < 1 || M % n_samples != 0 || ld_scale < r) return LORA_E_BADARG;
    return LORA_OK;
}

// lora_linear_fwd_ws (rows = false: no gate table, its three arguments unread) and lora_linear_fwd_rows (rows = true).
int linear_fwd(const void* X, const void* W, const void* bias, const float* A, const float* B, const void* Apack,
               const void* Bpack, void* Y, float* T_out, int64_t M, int K, int N, int r, float scale, bool rows,
               const float* row_scale, int n_samples, int ld_scale, int dtype, void* workspace, int64_t ws_bytes, void* stream) {
    int st = check_common(M, K, N, r, dtype);
    if (st == LORA_OK && rows) st = check_rows(M, r, row_scale, n_samples, ld_scale);
    if (st != LORA_OK) return st;
    if (M == 0) return LORA_OK;  // empty batch: nothing to do (pointers may be null)
    if (!X || !W || !A || !B || !Y || !T_out) return LORA_E_BADARG;
    CallArgs c{};
    c.Am = X; c.Bm = W; c.bias = bias;
    const size_t es = dtype == LORA_F32 ? 4 : 2;
    c.Fp = Apack;                                                              // A16  [16,K]
    c.Qp = Bpack ? static_cast<const char*>(Bpack) + (size_t)kRP * N * es : nullptr;  // B16  [N,16]
    c.F = A; c.f_sr = K; c.f_sk = 1;               // F[j,k] = A[j,k]
    c.Q = B; c.q_sn = r; c.q_sj = 1;               // Q[n,j] = B[n,j]
    c.C = Y; c.P = T_out;
    c.M = M; c.Kc = K; c.Nc = N; c.r = r; c.scale = scale;
    c.workspace = workspace; c.ws_bytes = ws_bytes;
    if (rows) {
        c.row_scale = row_scale; c.rs_rps = M / n_samples; c.rs_ld = ld_scale;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const double e = esize(dtype);
    ProfWork work(e * ((double)M * K + (double)N * K + (double)M * N) + e * r * (K + N) + (bias ? e * N : 0.0),
                  2.0 * M * K * N + 2.0 * M * r * (double)(K + N));
    return launch_gemm(c, true, dtype, s);
}

// lora_linear_geglu_fwd (rows = false) and lora_linear_geglu_fwd_rows (rows = true), as above.
int linear_geglu_fwd(const void* X, const void* W, const void* bias, const void* Apack, const void* Bpack, void* Y, void* Out,
                     float* T_out, int64_t M, int K, int N, int r, float scale, bool rows, const float* row_scale,
                     int n_samples, int ld_scale, int dtype, void* stream) {
    int st = check_common(M, K, N, r, dtype);
    if (st == LORA_OK && (N & 1) != 0) st = LORA_E_BADARG;
    if (st == LORA_OK && rows) st = check_rows(M, r, row_scale, n_samples, ld_scale);
    if (st != LORA_OK) return st;
    if (M == 0) return LORA_OK;
    if (!X || !W || !Out || !T_out) return LORA_E_BADARG;
    // the fused epilogue exists on the LDS-DMA ring kernel for 16-bit types only; everything else: LORA_E_UNSUPPORTED, and
    // the caller runs lora_linear_fwd + geglu_gate_fwd
    const int F = N / 2;
    if (dtype == LORA_F32 || r > kRP || !Apack || !Bpack || (K % 64) != 0 || (F % 64) != 0) return LORA_E_UNSUPPORTED;
    if (!aligned16(X) || !aligned16(W) || !aligned16(Apack) || !aligned16(Bpack) || !aligned16(Out) || (Y && !aligned16(Y)) ||
        (bias && (reinterpret_cast<uintptr_t>(bias) & 7u)))
        return LORA_E_UNSUPPORTED;
    GemmParams p{};
    p.Am = X; p.Bm = W; p.bias = bias;
    p.Fp = Apack;                                                   // A16 [16,K]
    p.Qp = static_cast<const char*>(Bpack) + (size_t)kRP * N * 2;   // B16 [N,16]
    p.C = Y; p.C2 = Out; p.gateF = F; p.P = T_out;
    p.M = M; p.Kc = K; p.Nc = N; p.r = r; p.scale = scale; p.lda = K;
    if (rows) {
        p.row_scale = row_scale; p.rs_rps = M / n_samples; p.rs_ld = ld_scale;
    }
    const double e = 2.0;
    ProfWork work(e * ((double)M * K + (double)N * K + (Y ? (double)M * N : 0.0) + (double)M * F) + e * r * (K + N) +
                      (bias ? e * N : 0.0),
                  2.0 * M * K * N + 2.0 * M * r * (double)(K + N));
    hipStream_t s = static_cast<hipStream_t>(stream);
    return dtype == LORA_F16 ? launch_gate<half_t>(p, s) : launch_gate<bf16_t>(p, s);
}

}  // namespace

#ifdef LORA_STAMPS
extern "C" int lora_debug_stamps(unsigned long long* host_out, int n_words) {
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_stamps), (size_t)n_words * 8) == hipSuccess ? 0 : -1;
}
extern "C" int lora_debug_stamps_reset() {
    void* d = nullptr;
    if (hipGetSymbolAddress(&d, HIP_SYMBOL(g_stamps)) != hipSuccess) return -1;
    return hipMemset(d, 0, sizeof(g_stamps)) == hipSuccess ? 0 : -1;
}
#endif

extern "C" int lora_linear_fwd(const void* X, const void* W, const void* bias, const float* A, const float* B,
                               const void* Apack, const void* Bpack, void* Y, float* T_out, int64_t M, int K, int N,
                               int r, float scale, int dtype, void* stream) {
    return lora_linear_fwd_ws(X, W, bias, A, B, Apack, Bpack, Y, T_out, M, K, N, r, scale, dtype, nullptr, 0, stream);
}

extern "C" int lora_linear_fwd_ws(const void* X, const void* W, const void* bias, const float* A, const float* B,
                                  const void* Apack, const void* Bpack, void* Y, float* T_out, int64_t M, int K, int N,
                                  int r, float scale, int dtype, void* workspace, int64_t ws_bytes, void* stream) {
    return linear_fwd(X, W, bias, A, B, Apack, Bpack, Y, T_out, M, K, N, r, scale, false, nullptr, 0, 0, dtype, workspace,
                      ws_bytes, stream);
}

extern "C" int lora_linear_fwd_rows(const void* X, const void* W, const void* bias, const float* A, const float* B,
                                    const void* Apack, const void* Bpack, void* Y, float* T_out, int64_t M, int K, int N,
                                    int r, float scale, const float* row_scale, int n_samples, int ld_scale, int dtype,
                                    void* workspace, int64_t ws_bytes, void* stream) {
    return linear_fwd(X, W, bias, A, B, Apack, Bpack, Y, T_out, M, K, N, r, scale, true, row_scale, n_samples, ld_scale, dtype,
                      workspace, ws_bytes, stream);
}

extern "C" int lora_linear_geglu_fwd(const void* X, const void* W, const void* bias, const void* Apack, const void* Bpack,
                                     void* Y, void* Out, float* T_out, int64_t M, int K, int N, int r, float scale,
                                     int dtype, void* stream) {
    return linear_geglu_fwd(X, W, bias, Apack, Bpack, Y, Out, T_out, M, K, N, r, scale, false, nullptr, 0, 0, dtype, stream);
}

extern "C" int lora_linear_geglu_fwd_rows(const void* X, const void* W, const void* bias, const void* Apack,
                                          const void* Bpack, void* Y, void* Out, float* T_out, int64_t M, int K, int N, int r,
                                          float scale, const float* row_scale, int n_samples, int ld_scale, int dtype,
                                          void* stream) {
    return linear_geglu_fwd(X, W, bias, Apack, Bpack, Y, Out, T_out, M, K, N, r, scale, true, row_scale, n_samples, ld_scale,
                            dtype, stream);
}

extern "C" int geglu_linear_bwd(const void* dZ, const void* W2t, const void* Y, void* dY, const void* zeros, int64_t M,
                                int Nz, int F, int dtype, void* stream) {
    if (M < 0 || Nz <= 0 || F <= 0) return LORA_E_BADARG;
    if (!known_dtype(dtype)) return LORA_E_BADARG;
    if (M == 0) return LORA_OK;
    if (!dZ || !W2t || !Y || !dY || !zeros) return LORA_E_BADARG;
    if (dtype == LORA_F32 || (Nz % 64) != 0 || (F % 128) != 0) return LORA_E_UNSUPPORTED;
    if (!aligned16(dZ) || !aligned16(W2t) || !aligned16(Y) || !aligned16(dY) || !aligned16(zeros)) return LORA_E_UNSUPPORTED;
    GemmParams p{};
    p.Am = dZ; p.Bm = W2t; p.bias = nullptr;
    p.Fp = zeros;  // no rank-r term in this launch: a zero factor tile [16, Nz] and a zero epilogue factor [F, 16]
    p.Qp = zeros;
    p.C = dY; p.C2 = const_cast<void*>(Y); p.gateF = F; p.P = nullptr;
    p.M = M; p.Kc = Nz; p.Nc = F; p.r = 1; p.scale = 0.f; p.lda = Nz;
    const double e = 2.0;
    ProfWork work(e * ((double)M * Nz + (double)F * Nz + 4.0 * (double)M * F), 2.0 * M * (double)Nz * F);
    hipStream_t s = static_cast<hipStream_t>(stream);
    return dtype == LORA_F16 ? launch_gate_bwd<half_t>(p, s) : launch_gate_bwd<bf16_t>(p, s);
}

extern "C" int64_t lora_gemm_workspace_bytes(int64_t M, int Kc, int Nc, int dtype) {
    if (M < 1 || Kc < 1 || Nc < 1) return 0;
    const SplitPlan sp = plan_splitk(M, Kc, Nc, dtype == LORA_F32 ? 4 : 2);
    return sp.S > 1 ? splitk_ws_bytes(M, Nc, sp) : 0;
}

extern "C" int lora_linear_bwd_input(const void* dY, const void* Wt, const float* A, const float* B,
                                     const void* Apack, const void* Bpack, void* dX, float* U_out, int64_t M, int K,
                                     int N, int r, float scale, int dtype, void* stream) {
    return lora_linear_bwd_input_ws(dY, Wt, A, B, Apack, Bpack, dX, U_out, M, K, N, r, scale, dtype, nullptr, 0, stream);
}

extern "C" int lora_linear_bwd_input_ws(const void* dY, const void* Wt, const float* A, const float* B,
                                        const void* Apack, const void* Bpack, void* dX, float* U_out, int64_t M, int K,
                                        int N, int r, float scale, int dtype, void* workspace, int64_t ws_bytes,
                                        void* stream) {
    const int st = check_common(M, K, N, r, dtype);
    if (st != LORA_OK) return st;
    if (M == 0) return LORA_OK;
    if (!dY || !A || !B || !U_out) return LORA_E_BADARG;
    if (dX && !Wt) return LORA_E_BADARG;
    CallArgs c{};
    c.Am = dY; c.Bm = Wt; c.bias = nullptr;
    const size_t es = dtype == LORA_F32 ? 4 : 2;
    c.Fp = Bpack;                                                              // Bt16 [16,N]
    c.Qp = Apack ? static_cast<const char*>(Apack) + (size_t)kRP * K * es : nullptr;  // At16 [K,16]
    c.F = B; c.f_sr = 1; c.f_sk = r;               // F[j,n] = B[n,j]
    c.Q = A; c.q_sn = 1; c.q_sj = K;               // Q[k,j] = A[j,k]
    c.C = dX; c.P = U_out;
    c.M = M; c.Kc = N; c.Nc = K; c.r = r; c.scale = scale;
    c.workspace = workspace; c.ws_bytes = ws_bytes;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const double e = esize(dtype);
    const double bytes = dX ? e * ((double)M * N + (double)N * K + (double)M * K) + e * r * (K + N)
                            : e * (double)M * N + e * r * N;
    const double flops = dX ? 2.0 * M * K * N + 2.0 * M * r * (double)(K + N) : 2.0 * M * r * (double)N;
    ProfWork work(bytes, flops);
    return launch_gemm(c, dX != nullptr, dtype, s);
}

extern "C" int lora_gemm_packed(const void* Am, int64_t lda, const void* Bm, const void* bias, const void* Fp,
                                const void* Qp, const int* tile_part, const int64_t* part_table, int n_parts, void* C,
                                float* P_out, int64_t M, int Kc, int Nc, int r, float scale, int64_t work_cols,
                                void* workspace, int64_t ws_bytes, int dtype, void* stream) {
    if (M < 0 || Kc <= 0 || r < 1 || r > kRP) return LORA_E_BADARG;
    if (!known_dtype(dtype)) return LORA_E_BADARG;
    if (M == 0) return LORA_OK;
    const bool main_part = C != nullptr;
    if (!Am || !Fp || (main_part && (!Bm || !Qp || Nc <= 0))) return LORA_E_BADARG;
    if (tile_part && !main_part) return LORA_E_BADARG;
    if (part_table && (main_part || n_parts < 1)) return LORA_E_BADARG;
    CallArgs c{};
    c.Am = Am; c.Bm = Bm; c.bias = bias; c.Fp = Fp; c.Qp = Qp; c.C = C; c.P = P_out;
    c.M = M; c.Kc = Kc; c.Nc = main_part ? Nc : 1; c.r = r; c.scale = scale; c.lda = lda;
    c.tile_part = tile_part; c.part_table = part_table; c.tiles_n = n_parts; c.packed_only = true;
    c.workspace = workspace; c.ws_bytes = ws_bytes;
    const double e = esize(dtype);
    const double kc = work_cols > 0 ? (double)work_cols : (double)Kc;
    ProfWork work(main_part ? e * ((double)M * Kc + (double)Nc * Kc + (double)M * Nc) + e * r * (double)(Kc + Nc) +
                                  (bias ? e * Nc : 0.0)
                            : e * (double)M * kc + e * r * kc,
                  main_part ? 2.0 * M * (double)Kc * Nc + 2.0 * M * r * (double)(Kc + Nc) : 2.0 * M * r * kc);
    return launch_gemm(c, main_part, dtype, static_cast<hipStream_t>(stream));
}

extern "C" int lora_gemm_parts(const void* Am, const void* Bm, const void* bias, const void* Fp, const void* Qp, void* C,
                               float* P_out, int64_t ldp, int64_t M, int Kc, int Nc, int r, int n_parts, int parts_on_k,
                               float scale, int dtype, void* stream) {
    if (M < 0 || Kc <= 0 || Nc <= 0 || r < 1 || r > kRP || n_parts < 2 || n_parts > 4) return LORA_E_BADARG;
    if (!known_dtype(dtype)) return LORA_E_BADARG;
    if (M == 0) return LORA_OK;
    if (!Am || !Bm || !Fp || !Qp || !C || !P_out || ldp < (int64_t)n_parts * r) return LORA_E_BADARG;
    const int split = parts_on_k ? Kc : Nc;  // the axis that is cut into parts
    if (split % n_parts != 0) return LORA_E_BADARG;
    const int part_n = split / n_parts;
    if (dtype == LORA_F32 || (part_n % 64) != 0 || (Kc % 64) != 0 || (Nc % 8) != 0) return LORA_E_UNSUPPORTED;
    if (!aligned16(Am) || !aligned16(Bm) || !aligned16(Fp) || !aligned16(Qp) || !aligned16(C) ||
        (bias && (reinterpret_cast<uintptr_t>(bias) & 7u)))
        return LORA_E_UNSUPPORTED;
    GemmParams p{};
    p.Am = Am; p.Bm = Bm; p.bias = bias; p.Fp = Fp; p.Qp = Qp; p.C = C; p.P = P_out;
    p.M = M; p.Kc = Kc; p.Nc = Nc; p.r = r; p.scale = scale; p.lda = Kc; p.ldp = (int)ldp;
    p.n_parts = n_parts; p.part_n = part_n; p.parts_on_k = parts_on_k ? 1 : 0;
    const double e = 2.0;
    ProfWork work(e * ((double)M * Kc + (double)Nc * Kc + (double)M * Nc) + e * r * (double)(Kc + Nc) * 1.0 + (bias ? e * Nc : 0.0),
                  2.0 * M * (double)Kc * Nc + 2.0 * M * r * (double)(Kc + Nc));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!parts_on_k) return dtype == LORA_F16 ? launch_pipe<half_t, true>(p, s) : launch_pipe<bf16_t, true>(p, s);
    if (n_parts != 3) return LORA_E_UNSUPPORTED;  // (the part-wise backward is instantiated for q / k / v groups)
    return dtype == LORA_F16 ? launch_kparts<half_t, 3>(p, s) : launch_kparts<bf16_t, 3>(p, s);
}

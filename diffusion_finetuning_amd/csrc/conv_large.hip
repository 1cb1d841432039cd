// 3x3, stride 1, padding 1 convolution of NCHW f16 / bf16 tensors with MANY pixels (the UNet's 32x32 and 64x64 levels) on the
// packed frozen weights of conv_small.hip (same pack, same contract):  y = conv(x, w) (+ b), fp32 accumulation, one rounding.
//
// Where conv_small.hip gets its parallelism from channel tiles x K-slices and streams each wave's weights from global memory,
// here the pixels alone fill the chip and every weight byte is wanted by all pixel tiles, so:
//   - a workgroup owns MT consecutive pixels (128 on 4 x 2 waves, or 64 on 2 x 2 waves where 128-pixel tiles would not fill
//     the 256 CUs once; a wave has 32 pixels x 80 channels either way) and 160 output channels, over the WHOLE K range: it
//     adds the bias, rounds and writes NCHW itself (a lane's four accumulator registers are four consecutive pixels of one
//     channel: one 8-byte store).  No fp32 partials, no second launch, no workspace.  160 divides every channel count of
//     these levels (320 ... 1920), which 128 does not.
//   - the weights of three taps (30 fragments of 1 KB, lane-linear in the pack) go through LDS by LDS-DMA, three buffers: one
//     fetch serves both pixel-waves, and the request for a step (three taps) is issued two steps ahead of its use.  The
//     barrier between steps waits with a COUNTED vmcnt for the requests of the step it opens only; what was issued since stays
//     in flight across it (a __syncthreads() would drain it all, and every step would pay the latency of its own weights).
//   - the activation is staged as in conv_small.hip (padded image coordinates, 80-byte positions, unconditional loads, the
//     zero selected at the LDS write), but a thread's unit of work is (position, 8 channels), so the 1056 units of a 128-pixel
//     tile of a 64-wide image cost 512 threads three units each, and the area is sized to the tile.  Two activation buffers:
//     the next chunk is written while the current one is multiplied, one barrier per three taps.
// Grid: pixel tiles fastest inside a channel tile, contiguous runs per XCD, so the tiles that share weights share an L2.
#include <atomic>

#include "conv_common.h"

namespace {

constexpr int kNTL = 160;                 // output channels per workgroup: 2 waves x 5 fragments of 16
constexpr int kFragsN = kNTL / 16;        // 10
constexpr int kGroupFrags = 3 * kFragsN;  // weight fragments of one step (three taps)
constexpr int kWBuf = kGroupFrags * 1024; // bytes of one weight buffer
constexpr int kWBufs = 3;                 // weight buffers: step g uses buffer g % 3, i.e. its tap row
constexpr int kPieceSlots = 32;           // LDS-DMA requests per workgroup and step (>= 30 fragments), an equal share a wave

// every wave's LDS reads and writes of the step are through, and all but its youngest N vector-memory operations have landed
template <int N> __device__ __forceinline__ void wait_barrier() {
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(N) : "memory");
}

__device__ __forceinline__ void glds16(const void* gsrc, unsigned char* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gsrc),
                                     (__attribute__((address_space(3))) void*)(lds_wave_base), 16, 0, 0);
}

// MT pixels per workgroup on WM x 2 waves; PER staging units (one position, 8 channels) a thread handles per chunk:
// threads * PER >= 4 * positions.
template <typename T, int MT, int PER, int WM>
__global__ __launch_bounds__(WM * 128) void conv_large_kernel(const T* __restrict__ x, const T* __restrict__ wp,
                                                              const T* __restrict__ bias, T* __restrict__ y, int Cin, int Cout,
                                                              int H, int W, int M, int mtiles, int chunks, int Pcap) {
    using Frag = typename Mfma<T>::Frag;
    constexpr int NTHR = WM * 128, NW = WM * 2, kPieces = kPieceSlots / NW;
    constexpr int MF = MT / (16 * WM);  // 16-pixel fragments per wave (WM waves along the pixels)
    constexpr int NF = kFragsN / 2;
    extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
    unsigned char* const wlds = smem;                     // kWBufs x kWBuf
    unsigned char* const alds = smem + kWBufs * kWBuf;    // 2 x Pcap positions, then 16 bytes per thread that nobody reads
    const int abytes = Pcap * kPitch;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), wm = wave % WM, wn = wave / WM;

    int mt, nt;
    {
        const unsigned total = gridDim.x, id = blockIdx.x;
        const unsigned q = total >> 3, rem = total & 7, xcd = id & 7, slot = id >> 3;
        const unsigned n = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + slot;
        mt = (int)(n % (unsigned)mtiles);
        nt = (int)(n / (unsigned)mtiles);
    }
    const int HW = H * W, W2 = W + 2, PP = (H + 2) * W2;
    const int m0 = mt * MT;
    const int q0 = padded_pos(m0, H, W);
    const int P = tile_positions(m0, MT, M, H, W);
    const int qlo = q0 - (W2 + 1);
    const float inv_pp = 1.f / (float)PP, inv_w2 = 1.f / (float)W2, inv_p = 1.f / (float)P;

    // staging plan of this thread, chunk-invariant: units tid, tid + 256, ...; unit i is channels 8*(i / P) ... of position i % P
    int xoff[PER];  // element offset of the unit's first channel in x (chunk 0); -1: border (zero) or no unit
    int aoff[PER];  // its LDS byte offset; no unit: this thread's 16 bytes of the dump area behind the buffers (a store under
                    // a condition would let the compiler sink the unit's loads to the store, behind the barriers they must precede)
#pragma unroll
    for (int s = 0; s < PER; ++s) {
        const int i = tid + s * NTHR, cg = fast_div(i, P, inv_p), p = i - cg * P;
        const bool unit = cg < 4;
        const int q = qlo + p, img = fast_div(q, PP, inv_pp), r = q - img * PP, hp = fast_div(r, W2, inv_w2), wq = r - hp * W2;
        const bool inside = unit && hp >= 1 && hp <= H && wq >= 1 && wq <= W;
        xoff[s] = inside ? (img * Cin + cg * 8) * HW + (hp - 1) * W + (wq - 1) : -1;
        aoff[s] = unit ? p * kPitch + cg * 16 : 2 * abytes + tid * 16;  // (tid < NTHR)
    }
    T raw[PER][8];
    auto load_stage = [&](int cc) {
        const T* base = x + (size_t)cc * kChunk * HW;
#pragma unroll
        for (int s = 0; s < PER; ++s) {
            // every lane loads (a border lane from offset 0, which is inside x): a conditional load makes a branch per element
            const int o = xoff[s] >= 0 ? xoff[s] : 0;
#pragma unroll
            for (int c = 0; c < 8; ++c) raw[s][c] = base[o + c * HW];
        }
    };
    auto write_stage = [&](int buf) {
#pragma unroll
        for (int s = 0; s < PER; ++s) {
            Frag v;
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = xoff[s] >= 0 ? raw[s][j] : static_cast<T>(0.f);
            *reinterpret_cast<Frag*>(alds + (aoff[s] < 2 * abytes ? buf * abytes : 0) + aoff[s]) = v;
        }
    };

    // LDS byte address of tap (0,0) of this lane's pixel in each of the wave's fragments; pixels past M repeat the last one
    int lpos[MF];
    const float inv_hw = 1.f / (float)HW, inv_w = 1.f / (float)W;
#pragma unroll
    for (int f = 0; f < MF; ++f) {
        const int m = min(m0 + wm * (MT / WM) + f * 16 + (lane & 15), M - 1);
        const int img = fast_div(m, HW, inv_hw), r = m - img * HW, h = fast_div(r, W, inv_w);
        lpos[f] = (img * PP + (h + 1) * W2 + (r - h * W) + 1 - q0) * kPitch + (lane >> 4) * 16;
    }

    // weight requests of step st (chunk st / 3, taps 3 * (st % 3) ...) into buffer `slot`: fragment j of the step goes to wave
    // j % NW, pieces [lo, hi) of that wave's kPieces (the two pieces past the 30th fetch the 30th again, so that every wave
    // issues the same number of requests); channel tiles past C_out repeat the last one (computed, not stored)
    const int KO = Cout >> 4;
    const size_t tap_stride = (size_t)KO * 512;
    // K order: pixel tile mt starts at chunk mt % chunks and wraps, so the tiles of one channel tile, which run side by side on
    // one XCD, ask for DIFFERENT weights at any moment: a line that misses L2 holds up one workgroup, not all of them in step
    const int c0 = mt % chunks;
    auto chunk_of = [&](int it) { const int c = c0 + it; return c >= chunks ? c - chunks : c; };
    auto load_w = [&](int st, int slot, int lo, int hi) {
        const T* src = wp + (size_t)(chunk_of(st / 3) * 3 + st % 3) * 3 * tap_stride + lane * 8;
        unsigned char* dst = wlds + slot * kWBuf;
#pragma unroll
        for (int i = lo; i < hi; ++i) {
            const int j = min(wave + NW * i, kGroupFrags - 1), t = j / kFragsN, f = j - t * kFragsN;
            glds16(src + t * tap_stride + (size_t)min(nt * kFragsN + f, KO - 1) * 512, dst + j * 1024);
        }
    };

    f32x4 acc[MF][NF];
#pragma unroll
    for (int f = 0; f < MF; ++f)
#pragma unroll
        for (int g = 0; g < NF; ++g) acc[f][g] = f32x4{0.f, 0.f, 0.f, 0.f};

    // Vector-memory operations of a wave, in issue order: step g issues the kPieces requests of step g + 2 and, in the first
    // step of a chunk, the 8 * PER activation loads of the next chunk.  The barrier that opens step g needs the requests of
    // step g, issued during step g - 2, to have landed: all but the operations of step g - 1 (the counter retires in order).
    // The source cannot enforce that count; it was read off the ISA of all six instantiations, and a compiler upgrade wants the
    // same reading (hipcc -S --cuda-device-only, the loop between the three s_barrier):
    //   - between two s_barrier there are exactly kPieces global_load_lds_dwordx4, plus 8 * PER global_load_ushort after the
    //     barrier of tap row 0 and none elsewhere (an earlier form lost eight of them to a conditional block behind a barrier);
    //   - the s_waitcnt in front of the three s_barrier read vmcnt(kPieces), vmcnt(kPieces + 8 * PER), vmcnt(kPieces);
    //   - any s_waitcnt vmcnt the compiler adds is stricter (it adds vmcnt(0) where the staged registers are first used);
    //   - no buffer_ / flat_ / scratch_ operation and no other global load sits inside the loop.
    static_assert(kPieces + 8 * PER <= 63, "vmcnt is a 6-bit counter");
    constexpr int kP1 = (kPieces * 3 + 7) / 8 + (kPieces < 8), kP2 = kP1 + (kPieces - kP1 + 1) / 2;  // 8: 3, 6; 4: 3, 4
    const int steps = chunks * 3;
    load_stage(c0);
    load_w(0, 0, 0, kPieces);
    load_w(min(1, steps - 1), 1, 0, kPieces);
    write_stage(0);
    for (int cc = 0; cc < chunks; ++cc) {
        const unsigned char* ab = alds + (cc & 1) * abytes;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int st = cc * 3 + r, ahead = min(st + 2, steps - 1), aslot = (r + 2) % 3;
            // every wave is through step st - 1: the weight buffer that step read and the other activation buffer are free,
            // and this step's weights and activation are in place
            if (r == 1) wait_barrier<kPieces + 8 * PER>();
            else wait_barrier<kPieces>();
            if (r == 2) write_stage((cc + 1) & 1);  // loaded two steps ago; read from the barrier of the next chunk on
            load_w(ahead, aslot, 0, kP1);  // (past the last step: the last step's again, into a free buffer, never read)
            if (r == 0) load_stage(chunk_of(min(cc + 1, chunks - 1)));
            __builtin_amdgcn_sched_barrier(0);
            const unsigned char* wb = wlds + r * kWBuf + wn * NF * 1024 + lane * 16;
            Frag xf[2][MF], bf[2][NF];
            {
                const int sh = (r * W2) * kPitch;
#pragma unroll
                for (int f = 0; f < MF; ++f) xf[0][f] = *reinterpret_cast<const Frag*>(ab + lpos[f] + sh);
#pragma unroll
                for (int g = 0; g < NF; ++g) bf[0][g] = *reinterpret_cast<const Frag*>(wb + g * 1024);
            }
#pragma unroll
            for (int tt = 0; tt < 3; ++tt) {
                if (tt + 1 < 3) {  // the next tap's fragments come out of LDS while this one is multiplied
                    const int sh = (r * W2 + tt + 1) * kPitch;
#pragma unroll
                    for (int f = 0; f < MF; ++f) xf[(tt + 1) & 1][f] = *reinterpret_cast<const Frag*>(ab + lpos[f] + sh);
#pragma unroll
                    for (int g = 0; g < NF; ++g)
                        bf[(tt + 1) & 1][g] = *reinterpret_cast<const Frag*>(wb + ((tt + 1) * kFragsN + g) * 1024);
                }
#pragma unroll
                for (int f = 0; f < MF; ++f)
#pragma unroll
                    for (int g = 0; g < NF; ++g) acc[f][g] = Mfma<T>::run(xf[tt & 1][f], bf[tt & 1][g], acc[f][g]);
                // the rest of the weight requests, spread behind the taps' MFMAs and kept there
                if (tt < 2) load_w(ahead, aslot, tt == 0 ? kP1 : kP2, tt == 0 ? kP2 : kPieces);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // no LDS-DMA may outlive the workgroup's LDS

    // direct epilogue: bias, one rounding, NCHW.  A lane's four registers are four consecutive pixels of one channel.
    const bool quad = (HW & 3) == 0;  // then M is a multiple of 4 and a quad never leaves its image
    struct alignas(8) Out4 { T v[4]; };
#pragma unroll
    for (int g = 0; g < NF; ++g) {
        const int k = nt * kNTL + (wn * NF + g) * 16 + (lane & 15);
        if (k >= Cout) continue;
        const float b = bias ? to_f32(bias[k]) : 0.f;
#pragma unroll
        for (int f = 0; f < MF; ++f) {
            const int m = m0 + wm * (MT / WM) + f * 16 + (lane >> 4) * 4;
            if (quad) {
                if (m < M) {
                    const int img = fast_div(m, HW, inv_hw);
                    Out4 o;
#pragma unroll
                    for (int i = 0; i < 4; ++i) o.v[i] = from_f32<T>(acc[f][g][i] + b);
                    *reinterpret_cast<Out4*>(y + (img * Cout + k) * HW + (m - img * HW)) = o;
                }
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (m + i < M) {
                        const int img = fast_div(m + i, HW, inv_hw);
                        y[(img * Cout + k) * HW + (m + i - img * HW)] = from_f32<T>(acc[f][g][i] + b);
                    }
            }
        }
    }
}

struct LGeo {
    int MT = 0, per = 0, mtiles = 0, ntiles = 0, chunks = 0, Pcap = 0, M = 0;
    bool ok = false;
};

// the instantiations of run_large: pixels per tile, staging units per thread, waves along the pixels
constexpr int kVariants = 3;
constexpr int kVarMT[kVariants] = {128, 64, 64};
constexpr int kVarPer[kVariants] = {3, 3, 6};
constexpr int kVarWM[kVariants] = {4, 2, 2};  // threads = 128 * WM; positions <= threads * units / 4

// most positions any tile of MT pixels stages.  A full tile's count depends on where in its image it starts, t * MT mod H*W,
// which repeats every H*W / gcd(MT, H*W) tiles, and the partial last tile has no more than a full one from the same start.
int max_positions(int MT, int M, int H, int W) {
    const int HW = H * W, mtiles = (M + MT - 1) / MT;
    int a = MT, b = HW;
    while (b) { const int c = a % b; a = b, b = c; }
    const int period = HW / a;
    int pmax = 0;
    for (int t = 0; t < mtiles && t < period; ++t) {
        const int p = tile_positions(t * MT, MT, M, H, W);
        pmax = p > pmax ? p : pmax;
    }
    return pmax;
}

// Tiling of one call: a function of the shape alone.  128-pixel tiles where they fill the 256 CUs at least once and fit their
// staging area; else 64-pixel tiles (three units a thread, or six for long rows).
LGeo large_geo(int N, int Cin, int Cout, int H, int W) {
    LGeo g;
    if (!conv_shape_in_range(N, Cin, Cout, H, W)) return g;
    const int M = N * H * W, ntiles = (Cout + kNTL - 1) / kNTL;
    const int p128 = max_positions(128, M, H, W), p64 = max_positions(64, M, H, W);
    const bool fits[kVariants] = {p128 <= 32 * kVarWM[0] * kVarPer[0], p64 <= 32 * kVarWM[1] * kVarPer[1],
                                  p64 <= 32 * kVarWM[2] * kVarPer[2]};
    int v = -1;
    if (fits[0] && (int64_t)((M + 127) / 128) * ntiles >= kCUs) v = 0;
    else if (fits[1]) v = 1;
    else if (fits[2]) v = 2;  // (where these do not fit, 128 pixels, with no smaller a staging area, do not either)
    if (v < 0) return g;
    g.MT = kVarMT[v], g.per = kVarPer[v], g.Pcap = v == 0 ? p128 : p64;
    g.mtiles = (M + g.MT - 1) / g.MT, g.ntiles = ntiles, g.chunks = Cin / kChunk, g.M = M;
    g.ok = (int64_t)g.mtiles * g.ntiles <= (1 << 20);
    return g;
}

template <typename T, int MT, int PER, int WM>
bool launch_large(const T* x, const T* wp, const T* bias, T* y, int Cin, int Cout, int H, int W, const LGeo& g, hipStream_t s) {
    const int lds = kWBufs * kWBuf + 2 * g.Pcap * kPitch + WM * 128 * 16;  // weights, activation x 2, dump area
    auto kern = conv_large_kernel<T, MT, PER, WM>;
    static std::atomic<int> lds_allowed{0};  // per instantiation: the dynamic-LDS limit is raised once, not on every launch
    if (lds > lds_allowed.load(std::memory_order_relaxed)) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
            return false;
        lds_allowed.store(lds, std::memory_order_relaxed);
    }
    hipLaunchKernelGGL(kern, dim3(g.mtiles * g.ntiles), dim3(WM * 128), lds, s, x, wp, bias, y, Cin, Cout, H, W, g.M, g.mtiles,
                       g.chunks, g.Pcap);
    return true;
}

template <typename T>
int run_large(const void* x_, const void* wp_, const void* bias_, void* y_, int Cin, int Cout, int H, int W, const LGeo& g,
              hipStream_t s) {
    const T *x = static_cast<const T*>(x_), *wp = static_cast<const T*>(wp_), *bias = static_cast<const T*>(bias_);
    T* y = static_cast<T*>(y_);
    const bool ok = g.MT == 128   ? launch_large<T, 128, 3, 4>(x, wp, bias, y, Cin, Cout, H, W, g, s)
                    : g.per == 3 ? launch_large<T, 64, 3, 2>(x, wp, bias, y, Cin, Cout, H, W, g, s)
                                 : launch_large<T, 64, 6, 2>(x, wp, bias, y, Cin, Cout, H, W, g, s);
    if (!ok) return LORA_E_LAUNCH;
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}

// The classes profiles/r15_conv_large_sweep.log shows faster than the stock call in BOTH directions inside a replayed graph
// (tools/conv_large_sweep.py), at exactly the measured pixel counts.  The backward of C_in -> C_out is the class C_out -> C_in.
// All ten classes of batch 4 at 64x64 latents won: 4096 pixels (32x32), 640 <-> {320, 640, 960, 1280, 1920} and 1280 <-> 1280;
// 16384 pixels (64x64), 320 <-> {320, 640, 960} and 640 <-> 640.  Nothing else was measured, so nothing else is routed.
bool large_plan_channels(int C_in, int C_out, int64_t pixels /* 0: any measured pixel count */) {
    const int lo = C_in < C_out ? C_in : C_out, hi = C_in < C_out ? C_out : C_in;
    const bool at4096 = (lo == 640 && (hi == 640 || hi == 960 || hi == 1280 || hi == 1920)) || (lo == 320 && hi == 640) ||
                        (lo == 1280 && hi == 1280);
    const bool at16384 = (lo == 320 && (hi == 320 || hi == 640 || hi == 960)) || (lo == 640 && hi == 640);
    return pixels == 4096 ? at4096 : pixels == 16384 ? at16384 : pixels == 0 ? (at4096 || at16384) : false;
}

}  // namespace

extern "C" int conv3x3_large_supported(int N, int C_in, int C_out, int H, int W, int dtype) {
    return (dtype == LORA_F16 || dtype == LORA_BF16) && large_geo(N, C_in, C_out, H, W).ok ? 1 : 0;
}

// No class is split along K, so no call needs a workspace: 0 for every shape, supported or not.
extern "C" int64_t conv3x3_large_workspace_bytes(int N, int C_in, int C_out, int H, int W, int dtype) {
    (void)N, (void)C_in, (void)C_out, (void)H, (void)W, (void)dtype;
    return 0;
}

// Whether this family (1) or another route (0) runs a frozen 3x3 convolution of `pixels` = N*H*W output pixels.  A function of
// its arguments alone.
extern "C" int conv3x3_large_plan(int64_t pixels, int C_in, int C_out, int dtype) {
    if (dtype != LORA_F16 && dtype != LORA_BF16) return 0;
    return pixels >= 1 && large_plan_channels(C_in, C_out, pixels) ? 1 : 0;
}

extern "C" int conv3x3_large_plan_channels(int C_in, int C_out, int dtype) {
    if (dtype != LORA_F16 && dtype != LORA_BF16) return 0;
    return large_plan_channels(C_in, C_out, 0) ? 1 : 0;
}

extern "C" int conv3x3_large(const void* x, const void* wpack, const void* bias, void* y, void* workspace, int64_t workspace_bytes,
                             int N, int C_in, int C_out, int H, int W, int dtype, void* stream) {
    if (!x || !wpack || !y || N < 1 || C_in < 1 || C_out < 1 || H < 1 || W < 1) return LORA_E_BADARG;
    if (dtype != LORA_F16 && dtype != LORA_BF16) return dtype == LORA_F32 ? LORA_E_UNSUPPORTED : LORA_E_BADARG;
    const LGeo g = large_geo(N, C_in, C_out, H, W);
    if (!g.ok) return LORA_E_UNSUPPORTED;
    if (workspace_bytes < 0) return LORA_E_BADARG;  // no split: no workspace is needed, a null one is accepted
    if (!aligned16(x) || !aligned16(wpack) || !aligned16(y) || !aligned16(workspace)) return LORA_E_ALIGN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return dtype == LORA_F16 ? run_large<half_t>(x, wpack, bias, y, C_in, C_out, H, W, g, s)
                             : run_large<bf16_t>(x, wpack, bias, y, C_in, C_out, H, W, g, s);
}

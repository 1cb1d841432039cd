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
//   - pixel-heavy tiles (256 or 128 pixels x 80 channels, MT / 32 x 1 waves) for the classes a sweep showed faster on them
//     (measured_tile): a staged position serves nine taps, a weight fragment one, so per chunk a tile pulls about MT * 66 bytes of
//     activations and 80 * WN * 9 * 64 bytes of weights, and 256 x 80 moves 80 KB where 128 x 160 moves 109 KB for the same
//     FLOPs.  They stage whole image rows with 16-byte loads (the rows form, at the kernel): 4 loads a thread and chunk for 24.
// Grid: pixel tiles fastest inside a channel tile, contiguous runs per XCD, so the tiles that share weights share an L2.
#include <atomic>

#include "conv_common.h"

namespace {

constexpr int kNTL = 160;                 // output channels per workgroup of the channel-heavy tiles: 2 waves x 5 fragments of 16
constexpr int kWaveFragsN = 5;            // 16-channel fragments of a wave: a workgroup has WN waves along the channels
constexpr int kWBufs = 3;                 // weight buffers: step g uses buffer g % 3, i.e. its tap row
// per WN: fragments of one tap, of one step (three taps), bytes of one weight buffer, and the LDS-DMA requests per workgroup and
// step (>= the step's fragments; 32 for 30, 16 for 15), an equal share a wave
constexpr int frags_n(int WN) { return kWaveFragsN * WN; }
constexpr int group_frags(int WN) { return 3 * frags_n(WN); }
constexpr int wbuf_bytes(int WN) { return group_frags(WN) * 1024; }
constexpr int piece_slots(int WN) { return 16 * WN; }

// every wave's LDS reads and writes of the step are through, and all but its youngest N vector-memory operations have landed
template <int N> __device__ __forceinline__ void wait_barrier() {
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(N) : "memory");
}

__device__ __forceinline__ void glds16(const void* gsrc, unsigned char* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gsrc),
                                     (__attribute__((address_space(3))) void*)(lds_wave_base), 16, 0, 0);
}

// MT pixels per workgroup on WM x WN waves, 80 * WN output channels.
// ROWS = false: PER staging units (one position, 8 channels) a thread handles per chunk: threads * PER >= 4 * positions.
// ROWS = true (W % 8 == 0, MT % W == 0, H*W % MT == 0, 2 * W <= MT: a tile is MT / W whole rows of one image): a unit is (staged
// row, channel pair, 8-pixel segment), two unconditional 16-byte loads and eight ds_write_b32; PER = 2 units a thread cover the
// 16 * (W / 8) * (MT / W + 2) = 2 * MT + 4 * W units of a chunk.  Lane -> unit: the low bit is the segment's low bit (where W / 8 is
// even: two lanes load 32 consecutive bytes), the next four the channel pair, the rest the remaining segment bits and then the
// row.  A ds_write_b32 is served in two groups of 32 lanes on 32 banks: a group is 16 channel pairs (16 consecutive dwords) x 2
// positions that lie 8 pixels (160 dwords = bank + 0) or a row (20 * (W + 2) dwords = bank + 8 at W = 8, 16, 32, 64) apart:
// two-way, which a ds_write_b32 hides behind its operand transfer.  The two padding columns of each staged row are zeroed once.
template <typename T, int MT, int PER, int WM, int WN = 2, bool ROWS = false>
__global__ __launch_bounds__(WM * WN * 64) void conv_large_kernel(const T* __restrict__ x, const T* __restrict__ wp,
                                                                  const T* __restrict__ bias, T* __restrict__ y, int Cin, int Cout,
                                                                  int H, int W, int M, int mtiles, int chunks, int Pcap) {
    using Frag = typename Mfma<T>::Frag;
    constexpr int kFragsN = frags_n(WN), kGroupFrags = group_frags(WN), kWBuf = wbuf_bytes(WN);
    constexpr int NTHR = WM * WN * 64, NW = WM * WN, kPieces = piece_slots(WN) / NW;
    constexpr int MF = MT / (16 * WM);  // 16-pixel fragments per wave (WM waves along the pixels)
    constexpr int NF = kWaveFragsN;
    constexpr int kLoads = ROWS ? 2 * PER : 8 * PER;  // activation loads a thread issues per chunk
    extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
    unsigned char* const wlds = smem;                     // kWBufs x kWBuf
    unsigned char* const alds = smem + kWBufs * kWBuf;    // 2 x Pcap positions, then (not ROWS) 16 bytes per thread that nobody reads
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
    // ROWS: xoff is the first channel's element offset of the unit's segment (a halo row outside the image: the nearest row inside,
    // cleared by `keep` at the LDS write), aoff the LDS byte offset of its first pixel's dword; a thread past the last unit
    // repeats its first unit, load and write: the same bytes to the same place, and no dump area
    unsigned keep[PER];
    if constexpr (ROWS) {
        const int S = W >> 3, lb = (S & 1) ^ 1, S2 = S >> lb, rows = MT / W + 2;
        const int img = fast_div(m0, HW, 1.f / (float)HW), h0 = (m0 - img * HW) / W;
        const float inv_s2 = 1.f / (float)S2;
#pragma unroll
        for (int s = 0; s < PER; ++s) {
            const int i = tid + s * NTHR, cp = (i >> lb) & 15, rest = i >> (4 + lb);
            const int sr = fast_div(rest, S2, inv_s2), seg = (i & lb) + ((rest - sr * S2) << lb);
            const int hr = h0 - 1 + sr, hc = min(max(hr, 0), H - 1);
            const bool unit = s == 0 || sr < rows;  // (unit 0 exists for every thread: 2 * MT threads)
            xoff[s] = unit ? (img * Cin + 2 * cp) * HW + hc * W + 8 * seg : xoff[0];
            aoff[s] = unit ? (sr * W2 + 1 + 8 * seg) * kPitch + cp * 4 : aoff[0];
            keep[s] = unit ? (hr == hc ? 0xffffffffu : 0u) : keep[0];
        }
    } else {
#pragma unroll
        for (int s = 0; s < PER; ++s) {
            const int i = tid + s * NTHR, cg = fast_div(i, P, inv_p), p = i - cg * P;
            const bool unit = cg < 4;
            const int q = qlo + p, img = fast_div(q, PP, inv_pp), r = q - img * PP, hp = fast_div(r, W2, inv_w2), wq = r - hp * W2;
            const bool inside = unit && hp >= 1 && hp <= H && wq >= 1 && wq <= W;
            xoff[s] = inside ? (img * Cin + cg * 8) * HW + (hp - 1) * W + (wq - 1) : -1;
            aoff[s] = unit ? p * kPitch + cg * 16 : 2 * abytes + tid * 16;  // (tid < NTHR)
        }
    }
    T raw[ROWS ? 1 : PER][8];
    uint4 rawr[ROWS ? PER : 1][2];  // ROWS: eight pixels of the unit's two channels
    auto load_stage = [&](int cc) {
        const T* base = x + (size_t)cc * kChunk * HW;
        if constexpr (ROWS) {
#pragma unroll
            for (int s = 0; s < PER; ++s) {
                rawr[s][0] = *reinterpret_cast<const uint4*>(base + xoff[s]);
                rawr[s][1] = *reinterpret_cast<const uint4*>(base + xoff[s] + HW);
            }
        } else {
#pragma unroll
            for (int s = 0; s < PER; ++s) {
                // every lane loads (a border lane from offset 0, which is inside x): a conditional load makes a branch per element
                const int o = xoff[s] >= 0 ? xoff[s] : 0;
#pragma unroll
                for (int c = 0; c < 8; ++c) raw[s][c] = base[o + c * HW];
            }
        }
    };
    auto write_stage = [&](int buf) {
        if constexpr (ROWS) {
#pragma unroll
            for (int s = 0; s < PER; ++s) {
                unsigned char* dst = alds + buf * abytes + aoff[s];
                const unsigned a[4] = {rawr[s][0].x, rawr[s][0].y, rawr[s][0].z, rawr[s][0].w};
                const unsigned b[4] = {rawr[s][1].x, rawr[s][1].y, rawr[s][1].z, rawr[s][1].w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {  // dword k of a load: pixels 2k (low half) and 2k + 1 of one channel
                    const unsigned ak = a[k] & keep[s], bk = b[k] & keep[s];
                    *reinterpret_cast<unsigned*>(dst + (2 * k) * kPitch) = (ak & 0xffffu) | (bk << 16);
                    *reinterpret_cast<unsigned*>(dst + (2 * k + 1) * kPitch) = (ak >> 16) | (bk & 0xffff0000u);
                }
            }
        } else {
#pragma unroll
            for (int s = 0; s < PER; ++s) {
                Frag v;
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = xoff[s] >= 0 ? raw[s][j] : static_cast<T>(0.f);
                *reinterpret_cast<Frag*>(alds + (aoff[s] < 2 * abytes ? buf * abytes : 0) + aoff[s]) = v;
            }
        }
    };
    if constexpr (ROWS) {  // the padding columns of every staged row, both buffers: written here and by nobody else
        const int rows = MT / W + 2;
        for (int i = tid; i < rows * 16; i += NTHR) {
            const int sr = i >> 4, b = (i >> 3) & 1, col = (i >> 2) & 1, piece = i & 3;
            *reinterpret_cast<uint4*>(alds + b * abytes + (sr * W2 + (col ? W + 1 : 0)) * kPitch + piece * 16) = uint4{0u, 0u, 0u, 0u};
        }
    }

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
    // step of a chunk, the kLoads activation loads of the next chunk.  The barrier that opens step g needs the requests of
    // step g, issued during step g - 2, to have landed: all but the operations of step g - 1 (the counter retires in order).
    // The source cannot enforce that count; it was read off the ISA of all ten instantiations, and a compiler upgrade wants the
    // same reading (hipcc -S --cuda-device-only, the loop between the three s_barrier):
    //   - between two s_barrier there are exactly kPieces global_load_lds_dwordx4, plus kLoads activation loads (8 * PER
    //     global_load_ushort; rows form: 2 * PER = 4 global_load_dwordx4) after the barrier of tap row 0 and none elsewhere (an
    //     earlier form lost eight of them to a conditional block behind a barrier);
    //   - the s_waitcnt in front of the three s_barrier read vmcnt(kPieces), vmcnt(kPieces + kLoads), vmcnt(kPieces): 4, 28, 4
    //     (128 x 160), 8, 32, 8 and 8, 56, 8 (64 x 160), 2, 6, 2 (256 x 80), 4, 8, 4 (128 x 80);
    //   - any s_waitcnt vmcnt the compiler adds is stricter: in every instantiation it adds one vmcnt(0), where the staged
    //     registers are first used, and has hoisted that use (the selects, or the rows form's AND and pack) in front of the third
    //     barrier's own wait.  It so sits behind the MFMAs of tap row 1 and in front of tap row 2's requests, and drains the
    //     requests of tap row 1, one step old, a step early; moving the LDS scatter moves that wait to the same distance from
    //     another step's requests, so it stays where the channel-heavy tiles have it;
    //   - no buffer_ / flat_ / scratch_ operation and no other global load sits inside the loop.
    static_assert(kPieces + kLoads <= 63, "vmcnt is a 6-bit counter");
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
            if (r == 1) wait_barrier<kPieces + kLoads>();
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
        const int k = nt * (kFragsN * 16) + (wn * NF + g) * 16 + (lane & 15);
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
    int tile = 0;  // 0: a channel-heavy tile of the shape rule (MT x 160); kTile256 / kTile128: a pixel-heavy rows-form tile
    bool ok = false;
};

// the pixel-heavy tiles (MT x 80 channels on MT / 32 x 1 waves, rows-form staging), named by conv3x3_large_tile
constexpr int kTile256 = 1, kTile128 = 2;
constexpr int kRowsPer = 2;                // units (two loads each) a thread stages per chunk
constexpr int kLdsBytes = 160 * 1024;

// Geometry of a rows-form tile, or !ok where its conditions fail: whole rows (W % 8 == 0 for the 16-byte loads, MT % W == 0)
// inside one image (H*W % MT == 0), at most MT / 2 pixels a row (two units a thread), the staging area within a CU's LDS.
LGeo rows_geo(int tile, int N, int Cin, int Cout, int H, int W) {
    LGeo g;
    if ((tile != kTile256 && tile != kTile128) || !conv_shape_in_range(N, Cin, Cout, H, W)) return g;
    const int MT = tile == kTile256 ? 256 : 128, HW = H * W;
    if (W % 8 || MT % W || HW % MT || 2 * W > MT) return g;
    g.MT = MT, g.per = kRowsPer, g.tile = tile, g.M = N * HW, g.mtiles = g.M / MT, g.ntiles = (Cout + 79) / 80;
    g.chunks = Cin / kChunk, g.Pcap = (MT / W + 2) * (W + 2);
    g.ok = (int64_t)g.mtiles * g.ntiles <= (1 << 20) && kWBufs * wbuf_bytes(1) + 2 * g.Pcap * kPitch <= kLdsBytes;
    return g;
}

// The classes profiles/r17_conv_large_tiles_sweep.log shows faster on a pixel-heavy tile than on the shape rule's tile in BOTH
// directions, by more than the spread of the class's replays (tools/conv_large_sweep.py): the tile, or 0 for every other shape.
// The backward of C_in -> C_out is the class C_out -> C_in, so the table is symmetric.  At 4096 pixels (32x32) 128 x 80 won for
// 640 <-> {320, 640, 960, 1280, 1920} and 256 x 80 for 1280 <-> 1280; at 16384 pixels (64x64) 256 x 80 won for 320 <-> {320, 960}
// and 640 <-> 640; 320 <-> 640 at 16384 pixels did not clear its spread and keeps the shape rule's tile.
int measured_tile(int64_t pixels, int C_in, int C_out) {
    const int lo = C_in < C_out ? C_in : C_out, hi = C_in < C_out ? C_out : C_in;
    if (pixels == 4096) {
        if (lo == 1280 && hi == 1280) return kTile256;
        if ((lo == 320 && hi == 640) || (lo == 640 && (hi == 640 || hi == 960 || hi == 1280 || hi == 1920))) return kTile128;
    } else if (pixels == 16384) {
        if ((lo == 320 && (hi == 320 || hi == 960)) || (lo == 640 && hi == 640)) return kTile256;
    }
    return 0;
}

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

// The shape rule: 128-pixel tiles where they fill the 256 CUs at least once and fit their staging area; else 64-pixel tiles (three
// units a thread, or six for long rows).
LGeo shape_geo(int N, int Cin, int Cout, int H, int W) {
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

// Tiling of one call: a function of the shape alone.  A measured class runs on its pixel-heavy tile, everything else by the
// shape rule.
LGeo large_geo(int N, int Cin, int Cout, int H, int W) {
    // (the sweep's classes are batch 4 of square images: 4096 pixels of 32x32, 16384 of 64x64; no other geometry was measured)
    const int tile = N == 4 && H == W && (H == 32 || H == 64) ? measured_tile((int64_t)N * H * W, Cin, Cout) : 0;
    if (tile) {
        const LGeo g = rows_geo(tile, N, Cin, Cout, H, W);
        if (g.ok) return g;
    }
    return shape_geo(N, Cin, Cout, H, W);
}

template <typename T, int MT, int PER, int WM, int WN = 2, bool ROWS = false>
bool launch_large(const T* x, const T* wp, const T* bias, T* y, int Cin, int Cout, int H, int W, const LGeo& g, hipStream_t s) {
    // weights, activation x 2, dump area (the rows form has none)
    const int lds = kWBufs * wbuf_bytes(WN) + 2 * g.Pcap * kPitch + (ROWS ? 0 : WM * WN * 64 * 16);
    auto kern = conv_large_kernel<T, MT, PER, WM, WN, ROWS>;
    static std::atomic<int> lds_allowed{0};  // per instantiation: the dynamic-LDS limit is raised once, not on every launch
    if (lds > lds_allowed.load(std::memory_order_relaxed)) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
            return false;
        lds_allowed.store(lds, std::memory_order_relaxed);
    }
    hipLaunchKernelGGL(kern, dim3(g.mtiles * g.ntiles), dim3(WM * WN * 64), lds, s, x, wp, bias, y, Cin, Cout, H, W, g.M, g.mtiles,
                       g.chunks, g.Pcap);
    return true;
}

template <typename T>
int run_large(const void* x_, const void* wp_, const void* bias_, void* y_, int Cin, int Cout, int H, int W, const LGeo& g,
              hipStream_t s) {
    const T *x = static_cast<const T*>(x_), *wp = static_cast<const T*>(wp_), *bias = static_cast<const T*>(bias_);
    T* y = static_cast<T*>(y_);
    const bool ok = g.tile == kTile256 ? launch_large<T, 256, kRowsPer, 8, 1, true>(x, wp, bias, y, Cin, Cout, H, W, g, s)
                    : g.tile == kTile128 ? launch_large<T, 128, kRowsPer, 4, 1, true>(x, wp, bias, y, Cin, Cout, H, W, g, s)
                    : g.MT == 128   ? launch_large<T, 128, 3, 4>(x, wp, bias, y, Cin, Cout, H, W, g, s)
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

// tile < 0: the tiling conv3x3_large chooses; 0: the shape rule's tile; kTile256 / kTile128: that pixel-heavy tile
static int large_call(const void* x, const void* wpack, const void* bias, void* y, void* workspace, int64_t workspace_bytes, int N,
                      int C_in, int C_out, int H, int W, int dtype, int tile, void* stream) {
    if (!x || !wpack || !y || N < 1 || C_in < 1 || C_out < 1 || H < 1 || W < 1) return LORA_E_BADARG;
    if (dtype != LORA_F16 && dtype != LORA_BF16) return dtype == LORA_F32 ? LORA_E_UNSUPPORTED : LORA_E_BADARG;
    const LGeo g = tile < 0 ? large_geo(N, C_in, C_out, H, W) : tile == 0 ? shape_geo(N, C_in, C_out, H, W)
                                                                           : rows_geo(tile, N, C_in, C_out, H, W);
    if (!g.ok) return LORA_E_UNSUPPORTED;
    if (workspace_bytes < 0) return LORA_E_BADARG;  // no split: no workspace is needed, a null one is accepted
    if (!aligned16(x) || !aligned16(wpack) || !aligned16(y) || !aligned16(workspace)) return LORA_E_ALIGN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return dtype == LORA_F16 ? run_large<half_t>(x, wpack, bias, y, C_in, C_out, H, W, g, s)
                             : run_large<bf16_t>(x, wpack, bias, y, C_in, C_out, H, W, g, s);
}

extern "C" int conv3x3_large(const void* x, const void* wpack, const void* bias, void* y, void* workspace, int64_t workspace_bytes,
                             int N, int C_in, int C_out, int H, int W, int dtype, void* stream) {
    return large_call(x, wpack, bias, y, workspace, workspace_bytes, N, C_in, C_out, H, W, dtype, -1, stream);
}

// The tile conv3x3_large runs a shape on: 0 (the shape rule's), kTile256 or kTile128; -1 where the family does not cover it.
extern "C" int conv3x3_large_tile_choice(int N, int C_in, int C_out, int H, int W, int dtype) {
    if (dtype != LORA_F16 && dtype != LORA_BF16) return -1;
    const LGeo g = large_geo(N, C_in, C_out, H, W);
    return g.ok ? g.tile : -1;
}

// conv3x3_large on a named tile, for the sweep and the tests: 0 is the shape rule's channel-heavy tile (whatever the measured
// table says), 1 is 256 pixels x 80 channels, 2 is 128 pixels x 80 channels, both rows-form.  LORA_E_UNSUPPORTED, and nothing
// written, where the tile's conditions fail; LORA_E_BADARG for an unknown tile.
extern "C" int conv3x3_large_tile(const void* x, const void* wpack, const void* bias, void* y, void* workspace,
                                  int64_t workspace_bytes, int N, int C_in, int C_out, int H, int W, int dtype, int tile,
                                  void* stream) {
    if (tile < 0 || tile > kTile128) return LORA_E_BADARG;
    return large_call(x, wpack, bias, y, workspace, workspace_bytes, N, C_in, C_out, H, W, dtype, tile, stream);
}

// 3x3, stride 1, padding 1 convolution of NCHW f16 / bf16 tensors with FEW pixels and WIDE filters (the UNet's 8x8 and 16x16
// levels), as an implicit GEMM on packed frozen weights:  y[n,k,h,w] = sum_{c,r,s} x[n,c,h+r-1,w+s-1] * w[k,c,r,s] (+ b[k]).
// The 32x32 and 64x64 levels run on conv_large.hip, which reads the same packs.
//
// Decomposition.  GEMM M = N*H*W pixels, N = C_out, K = 9*C_in.  A workgroup (256 threads, 2 x 2 waves) owns MT consecutive
// pixels (128, or 64 where 128 pixels with their halo exceed 256 padded positions), 128 output channels and one K-slice: a run of 32-channel
// chunks, all nine taps of each.  Pixels being few, the parallelism comes from channel tiles x K-slices (conv_geo sizes the
// grid to at most one round of the 256 CUs).  Per chunk the workgroup stages its pixels' 32 input channels in LDS in PADDED
// image coordinates, q = n*(H+2)*(W+2) + (h+1)*(W+2) + (w+1), halo and zero border materialised, 32 channels (64 bytes + 16
// of padding) per position: tap (r, s) of a pixel is then the position r*(W+2) + s further on, the main loop has no bounds test
// and each staged chunk is read nine times.  The next chunk's global loads are in flight while the current one is multiplied.
// The MFMA is 16x16x32 with the pixels as rows (A, from LDS, one ds_read_b128 per fragment) and the output channels as
// columns (B, straight from global memory: no other wave of the workgroup needs the same weights).
//
// Pack layout (conv3x3_small_pack, once per weight and direction).  Element j of lane l of the B fragment of (chunk cc, tap
// t = 3r+s, channel tile ko) is w[k = 16*ko + (l&15)][c = 32*cc + 8*(l>>4) + j][r][s], stored at
//     ((cc*9 + t) * (C_out/16) + ko) * 512 + l*8 + j
// so a wave fetches a fragment as 64 consecutive 16-byte runs and a workgroup's weights of one tap are one 4 KB run per wave.
// The backward-data pack holds w'[c,k,r,s] = w[k,c,2-r,2-s] in the same order with the channel roles swapped; dx = conv(dy, w').
//
// Reduction.  Every workgroup stores its fp32 partial tile to the workspace ([slice][channel][pixel], pixels padded to MT);
// a second small launch adds the slices of an element in slice order 0, 1, ..., adds the bias, rounds ONCE and writes NCHW.
// No atomics, no workgroup waits on another: the result is bit-identical from run to run.
//
// Workgroups that share weights (the pixel tiles of one channel tile and slice) get consecutive places in the XCD remap below,
// so they run on one XCD and the weights come from HBM once.
#include <atomic>

#include "conv_common.h"

namespace {

constexpr int kNT = 128;        // output channels per workgroup (2 waves x 4 tiles of 16)

// every wave's LDS reads and writes so far are through; vector-memory requests stay in flight across the barrier (a __syncthreads()
// would drain them all)
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// MT pixels per workgroup, two LDS stage buffers of PER * 256 positions each.
// RU = 0, the position form: a thread stages PER positions (all 32 channels of each) per chunk with 2-byte loads, 256*PER >=
// positions of a tile; a thread past the tile's last position writes zeros to a position of its own that nobody reads.
// RU = 1 or 2, the rows form (rows_units below: W % 8 == 0, a tile is whole rows, MT = 128, PER = 1): a unit is (image row, channel
// pair, 8-pixel segment), two unconditional 16-byte loads and eight ds_write_b32, RU units a thread; lane -> unit as in
// conv_large.hip.  The border positions and the halo rows outside the image are zeroed once, in both buffers, and never written
// again.  A thread without a unit repeats an existing one: the same bytes to the same place.
template <typename T, int MT, int PER, int RU>
__global__ __launch_bounds__(kThreads) void conv_small_kernel(const T* __restrict__ x, const T* __restrict__ wp,
                                                              float* __restrict__ part, int Cin, int Cout, int H, int W, int M,
                                                              int mtiles, int ntiles, int cps, int chunks, int Mpad) {
    using Frag = typename Mfma<T>::Frag;
    constexpr int MF = MT / 32;  // 16-pixel fragments per wave (two waves along the pixels)
    constexpr bool ROWS = RU > 0;
    constexpr int kBuf = PER * kThreads * kPitch;  // bytes of one stage buffer
    constexpr int NU = ROWS ? RU : 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave & 1, wn = wave >> 1;

    // XCD x owns a contiguous run of tiles (the remap of attn_flash_common.h); pixel tiles fastest, so the tiles that read the
    // same weights sit next to each other
    int mt, nt, sl;
    {
        const unsigned total = gridDim.x, id = blockIdx.x;
        const unsigned q = total >> 3, rem = total & 7, xcd = id & 7, slot = id >> 3;
        const unsigned n = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + slot;
        mt = (int)(n % (unsigned)mtiles);
        const unsigned rest = n / (unsigned)mtiles;
        nt = (int)(rest % (unsigned)ntiles);
        sl = (int)(rest / (unsigned)ntiles);
    }
    const int c_begin = sl * cps, c_end = min(c_begin + cps, chunks);
    const int HW = H * W, W2 = W + 2, PP = (H + 2) * W2;
    const int m0 = mt * MT;
    const int q0 = padded_pos(m0, H, W);
    const int P = tile_positions(m0, MT, M, H, W);
    const int qlo = q0 - (W2 + 1);
    const float inv_pp = 1.f / (float)PP, inv_w2 = 1.f / (float)W2;

    // staging plan of this thread, chunk-invariant
    // position form: positions tid, tid + 256, ... (PER of them), four 8-channel groups of each; xoff is the element offset of
    // (position, channel 0 of the chunk) in x, -1: border or past the tile (zeros are written)
    // rows form: xoff is the element offset of the unit's first channel and pixel, aoff the LDS byte offset of that pixel's dword
    int xoff[ROWS ? NU : PER];
    int aoff[NU];
    if constexpr (ROWS) {
        const int S = W >> 3, lb = (S & 1) ^ 1, S2 = S >> lb;
        const int img0 = m0 / HW, h0 = (m0 - img0 * HW) / W;
        const bool whole = MT % HW == 0;  // the tile is whole images (else: MT / W rows of one image and their two halo rows)
        const int images = min(MT / HW, (M - m0) / HW);
#pragma unroll
        for (int s = 0; s < RU; ++s) {
            const int i = tid + s * kThreads, cp = (i >> lb) & 15, rest = i >> (4 + lb);
            int k = rest / S2;
            const int seg = (i & lb) + ((rest - k * S2) << lb);
            const bool unit = whole ? k < images * H : (k < MT / W + 2 && h0 - 1 + k >= 0 && h0 - 1 + k < H);
            if (!unit) k = whole ? 0 : 1;  // a row that every tile has
            const int im = whole ? k / H : 0, hr = whole ? k - im * H : h0 - 1 + k;
            const int j = whole ? im * (H + 2) + hr + 1 : k;  // staged (padded) row
            xoff[s] = ((img0 + im) * Cin + 2 * cp) * HW + hr * W + 8 * seg;
            aoff[s] = (j * W2 + 1 + 8 * seg) * kPitch + cp * 4;
        }
    } else {
#pragma unroll
        for (int s = 0; s < PER; ++s) {
            const int p = tid + s * kThreads;
            const int q = qlo + p, img = fast_div(q, PP, inv_pp), r = q - img * PP, hp = fast_div(r, W2, inv_w2), wq = r - hp * W2;
            const bool inside = p < P && hp >= 1 && hp <= H && wq >= 1 && wq <= W;
            xoff[s] = inside ? img * Cin * HW + (hp - 1) * W + (wq - 1) : -1;
        }
    }
    // the loaded elements stay as they arrive until they are written to LDS at the end of the chunk; zero selection and packing
    // happen there, so nothing waits for these loads while the current chunk is multiplied
    T raw[ROWS ? 1 : PER][32];
    uint4 rawr[NU][2];  // rows form: eight pixels of the unit's two channels
    auto load_stage = [&](int cc) {
        const T* base = x + (size_t)cc * kChunk * HW;
        if constexpr (ROWS) {
#pragma unroll
            for (int s = 0; s < RU; ++s) {
                rawr[s][0] = *reinterpret_cast<const uint4*>(base + xoff[s]);
                rawr[s][1] = *reinterpret_cast<const uint4*>(base + xoff[s] + HW);
            }
        } else {
#pragma unroll
            for (int s = 0; s < PER; ++s) {
                // every lane loads (a border lane from offset 0, which is inside x): a conditional load makes a branch per element
                const int o = xoff[s] >= 0 ? xoff[s] : 0;
#pragma unroll
                for (int c = 0; c < 32; ++c) raw[s][c] = base[o + c * HW];
            }
        }
    };
    // unconditional: a store under a condition puts a branch around the first use of the loaded registers, and the compiler then
    // drains every request in front of it
    auto write_stage = [&](int buf) {
        unsigned char* dstb = smem + buf * kBuf;
        if constexpr (ROWS) {
#pragma unroll
            for (int s = 0; s < RU; ++s) {
                unsigned char* dst = dstb + aoff[s];
                const unsigned a[4] = {rawr[s][0].x, rawr[s][0].y, rawr[s][0].z, rawr[s][0].w};
                const unsigned b[4] = {rawr[s][1].x, rawr[s][1].y, rawr[s][1].z, rawr[s][1].w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {  // dword k of a load: pixels 2k (low half) and 2k + 1 of one channel
                    *reinterpret_cast<unsigned*>(dst + (2 * k) * kPitch) = (a[k] & 0xffffu) | (b[k] << 16);
                    *reinterpret_cast<unsigned*>(dst + (2 * k + 1) * kPitch) = (a[k] >> 16) | (b[k] & 0xffff0000u);
                }
            }
        } else {
#pragma unroll
            for (int s = 0; s < PER; ++s)
#pragma unroll
                for (int c8 = 0; c8 < 4; ++c8) {
                    Frag v;
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = xoff[s] >= 0 ? raw[s][c8 * 8 + j] : static_cast<T>(0.f);
                    *reinterpret_cast<Frag*>(dstb + (tid + s * kThreads) * kPitch + c8 * 16) = v;
                }
        }
    };
    if constexpr (ROWS) {  // both buffers: the borders and the halo rows outside the image stay zero, the rest is overwritten
#pragma unroll
        for (int i = 0; i < 2 * kBuf / (16 * kThreads); ++i)
            *reinterpret_cast<uint4*>(smem + (i * kThreads + tid) * 16) = uint4{0u, 0u, 0u, 0u};
        lds_barrier();
    }

    // LDS byte address of tap (0,0) of this lane's pixel in each of the wave's fragments; pixels past M repeat the last one
    int lpos[MF];
    const float inv_hw = 1.f / (float)HW, inv_w = 1.f / (float)W;
#pragma unroll
    for (int f = 0; f < MF; ++f) {
        const int m = min(m0 + wm * (MT / 2) + f * 16 + (lane & 15), M - 1);
        const int img = fast_div(m, HW, inv_hw), r = m - img * HW, h = fast_div(r, W, inv_w);
        lpos[f] = (img * PP + (h + 1) * W2 + (r - h * W) + 1 - q0) * kPitch + (lane >> 4) * 16;
    }
    // this wave's four channel tiles; tiles past C_out repeat the last one (computed, not stored)
    const int KO = Cout >> 4;
    int wofs[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) wofs[g] = min(nt * (kNT / 16) + wn * 4 + g, KO - 1) * 512 + lane * 8;
    const size_t tap_stride = (size_t)KO * 512;
    const int L_end = c_end * 9;
    Frag wf[9][4];  // a whole chunk of weights in flight: the same tap of the next chunk is requested as soon as one is used
    auto load_w = [&](int slot, int L) {
        const T* src = wp + (size_t)min(L, L_end - 1) * tap_stride;
#pragma unroll
        for (int g = 0; g < 4; ++g) wf[slot][g] = *reinterpret_cast<const Frag*>(src + wofs[g]);
    };

    f32x4 acc[MF][4];
#pragma unroll
    for (int f = 0; f < MF; ++f)
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[f][g] = f32x4{0.f, 0.f, 0.f, 0.f};

    // Vector-memory requests of a wave, in issue order: the activation loads of a chunk, then the 36 weight requests of the NEXT
    // use of each tap.  The prologue keeps that order (the sched_barrier), so on every path into the loop the activation loads
    // are the oldest requests and the compiler can count: the stage write waits for all but the 36 weight requests behind the
    // loads, tap t's MFMAs for all but what was issued after tap t's request a chunk earlier.  The request count of an
    // iteration is fixed: past the last chunk the loads repeat the last chunk and the weight requests the last tap.
    //
    // Stage buffers: chunk cc is read from buffer cc & 1; at the end of chunk cc the next chunk is written to the other buffer,
    // then ONE barrier.  That buffer was last read during chunk cc - 1, and every wave has passed the barrier that ended chunk
    // cc - 1 before any wave writes here: a buffer is rewritten one barrier after its last read, and read one barrier after
    // its write.
    load_stage(c_begin);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int t = 0; t < 9; ++t) load_w(t, c_begin * 9 + t);
    __builtin_amdgcn_sched_barrier(0);
    write_stage(c_begin & 1);
    lds_barrier();
    for (int cc = c_begin; cc < c_end; ++cc) {
        const unsigned char* ab = smem + (cc & 1) * kBuf;
        load_stage(min(cc + 1, c_end - 1));
        __builtin_amdgcn_sched_barrier(0);
        Frag xf[2][MF];
#pragma unroll
        for (int f = 0; f < MF; ++f) xf[0][f] = *reinterpret_cast<const Frag*>(ab + lpos[f]);
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            if (t + 1 < 9) {  // the next tap's pixels come out of LDS while this one is multiplied
                const int sh = (((t + 1) / 3) * W2 + ((t + 1) % 3)) * kPitch;
#pragma unroll
                for (int f = 0; f < MF; ++f) xf[(t + 1) & 1][f] = *reinterpret_cast<const Frag*>(ab + lpos[f] + sh);
            }
#pragma unroll
            for (int f = 0; f < MF; ++f)
#pragma unroll
                for (int g = 0; g < 4; ++g) acc[f][g] = Mfma<T>::run(xf[t & 1][f], wf[t][g], acc[f][g]);
            load_w(t, cc * 9 + t + 9);
            // keeps the request here, a chunk ahead of its use: left alone, the scheduler gathers all nine at the loop's end
            __builtin_amdgcn_sched_barrier(0);
        }
        write_stage((cc + 1) & 1);  // (past the last chunk: the last chunk again, into the buffer nobody reads any more)
        lds_barrier();
    }

    // partial tile: [slice][channel][pixel], a lane's four registers are four consecutive pixels of one channel
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int k = nt * kNT + wn * 64 + g * 16 + (lane & 15);
        if (k < Cout) {
            float* dst = part + ((size_t)sl * Cout + k) * Mpad + m0 + wm * (MT / 2) + (lane >> 4) * 4;
#pragma unroll
            for (int f = 0; f < MF; ++f) *reinterpret_cast<f32x4*>(dst + f * 16) = acc[f][g];
        }
    }
}

// V pixels per thread (4 where H*W is a multiple of 4: 16-byte loads of the partials, 8-byte stores); slices added in order
template <typename T, int V>
__global__ __launch_bounds__(256) void conv_small_reduce_kernel(const float* __restrict__ part, const T* __restrict__ bias,
                                                                T* __restrict__ y, int Cout, int HW, int M, int Mpad, int S) {
    const int idx = blockIdx.x * 256 + threadIdx.x, MV = M / V;
    if (idx >= Cout * MV) return;
    const int k = idx / MV, m = (idx - k * MV) * V;
    const float* src = part + (size_t)k * Mpad + m;
    const size_t stride = (size_t)Cout * Mpad;
    float v[V];
    if constexpr (V == 4) {
        f32x4 a = *reinterpret_cast<const f32x4*>(src);
        int s = 1;
        for (; s + 3 < S; s += 4) {  // four loads in flight, added in slice order
            const f32x4 b0 = *reinterpret_cast<const f32x4*>(src + s * stride), b1 = *reinterpret_cast<const f32x4*>(src + (s + 1) * stride),
                        b2 = *reinterpret_cast<const f32x4*>(src + (s + 2) * stride), b3 = *reinterpret_cast<const f32x4*>(src + (s + 3) * stride);
            a += b0, a += b1, a += b2, a += b3;
        }
        for (; s < S; ++s) a += *reinterpret_cast<const f32x4*>(src + s * stride);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = a[i];
    } else {
        v[0] = src[0];
        for (int s = 1; s < S; ++s) v[0] += src[s * stride];
    }
    const float b = bias ? to_f32(bias[k]) : 0.f;
    const int n = m / HW, p = m - n * HW;
    T* dst = y + ((size_t)n * Cout + k) * HW + p;
    if constexpr (V == 4) {
        struct alignas(8) Out4 { T v[4]; } o;
#pragma unroll
        for (int i = 0; i < 4; ++i) o.v[i] = from_f32<T>(v[i] + b);
        *reinterpret_cast<Out4*>(dst) = o;
    } else {
        dst[0] = from_f32<T>(v[0] + b);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void conv_small_pack_kernel(const T* __restrict__ w, T* __restrict__ out, int Cin, int Cout,
                                                              int backward) {
    // Cin / Cout are those of w [Cout, Cin, 3, 3]; the packed problem has (Ci, Co) = (Cin, Cout), or swapped for backward
    const int64_t total = (int64_t)Cin * Cout * 9, o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= total) return;
    const int Co = backward ? Cin : Cout, KO = Co >> 4;
    const int j = (int)(o & 7), l = (int)((o >> 3) & 63);
    const int64_t rest = o >> 9;
    const int ko = (int)(rest % KO);
    const int64_t rest2 = rest / KO;
    const int t = (int)(rest2 % 9), cc = (int)(rest2 / 9);
    const int ci = cc * 32 + (l >> 4) * 8 + j, co = ko * 16 + (l & 15);
    const int64_t src = backward ? ((int64_t)ci * Cin + co) * 9 + (8 - t) : ((int64_t)co * Cin + ci) * 9 + t;
    out[o] = w[src];
}

struct Geo {
    int MT = 0, per = 0, mtiles = 0, ntiles = 0, chunks = 0, cps = 0, S = 0, Pcap = 0, Mpad = 0, M = 0;
    int64_t ws_bytes = 0;
    bool ok = false;
};

// Tiling of one call: a function of the shape alone.
Geo conv_geo(int N, int Cin, int Cout, int H, int W) {
    Geo g;
    if (!conv_shape_in_range(N, Cin, Cout, H, W)) return g;
    const int M = N * H * W;
    const int mts[2] = {128, 64}, per[2] = {1, 3};  // the instantiations of run_conv
    for (int v = 0; v < 2 && !g.ok; ++v) {
        const int MT = mts[v], mtiles = (M + MT - 1) / MT;
        int pmax = 0;
        for (int t = 0; t < mtiles; ++t) {
            const int p = tile_positions(t * MT, MT, M, H, W);
            pmax = p > pmax ? p : pmax;
        }
        if (pmax > per[v] * kThreads) continue;
        g.MT = MT, g.per = per[v], g.mtiles = mtiles, g.Pcap = pmax, g.ok = true;
    }
    if (!g.ok) return g;
    g.M = M;
    g.Mpad = g.mtiles * g.MT;
    g.ntiles = (Cout + kNT - 1) / kNT;
    g.chunks = Cin / kChunk;
    // K-slices: as many as fill the CUs once, at least two chunks each where there are four or more (a one-chunk slice has
    // nothing to overlap its loads with and doubles the partial traffic)
    const int tiles = g.mtiles * g.ntiles, want = kCUs / tiles > 1 ? kCUs / tiles : 1;
    int cps = (g.chunks + want - 1) / want;
    if (g.chunks >= 4 && cps < 2) cps = 2;
    g.cps = cps;
    g.S = (g.chunks + cps - 1) / cps;
    g.ws_bytes = (int64_t)g.S * Cout * g.Mpad * 4;
    if ((int64_t)tiles * g.S > (1 << 20)) g.ok = false;
    return g;
}

// the forms of the main kernel's staging, named by conv3x3_small_form
constexpr int kFormPosition = 0, kFormRows = 1;

// Units a thread stages in the rows form (1 or 2), or 0 where that form does not cover the shape.  It needs 16-byte row segments
// (W % 8 == 0), the 128-pixel instantiation, and tiles that are whole rows laid out one of two ways: whole images (128 % H*W == 0:
// 2 * 128 = 256 units, one a thread), or 128 / W rows of one image with their two halo rows (H*W % 128 == 0: 256 + 4 * W units,
// two a thread).
int rows_units(const Geo& g, int H, int W) {
    if (!g.ok || g.MT != 128 || W % 8 || 128 % W) return 0;
    const int HW = H * W;
    if (128 % HW == 0) return 1;
    return HW % 128 == 0 && 256 + 4 * W <= 2 * kThreads ? 2 : 0;
}

template <typename T, int MT, int PER, int RU>
bool launch_main(const T* x, const T* wp, float* part, int Cin, int Cout, int H, int W, const Geo& g, hipStream_t s) {
    constexpr int lds = 2 * PER * kThreads * kPitch;  // two stage buffers
    auto kern = conv_small_kernel<T, MT, PER, RU>;
    static std::atomic<bool> raised{false};  // per instantiation: the dynamic-LDS limit is raised once, not on every launch
    if (lds > 48 * 1024 && !raised.load(std::memory_order_relaxed)) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
            return false;
        raised.store(true, std::memory_order_relaxed);
    }
    hipLaunchKernelGGL(kern, dim3(g.mtiles * g.ntiles * g.S), dim3(kThreads), lds, s, x, wp, part, Cin, Cout, H, W, g.M, g.mtiles,
                       g.ntiles, g.cps, g.chunks, g.Mpad);
    return true;
}

// ru: units a thread of the rows form (rows_units), 0 for the position form
template <typename T>
int run_conv(const void* x_, const void* wp_, const void* bias_, void* y_, void* ws, int Cin, int Cout, int H, int W, const Geo& g,
             int ru, hipStream_t s) {
    const T *x = static_cast<const T*>(x_), *wp = static_cast<const T*>(wp_), *bias = static_cast<const T*>(bias_);
    float* part = static_cast<float*>(ws);
    const bool ok = ru == 1     ? launch_main<T, 128, 1, 1>(x, wp, part, Cin, Cout, H, W, g, s)
                    : ru == 2   ? launch_main<T, 128, 1, 2>(x, wp, part, Cin, Cout, H, W, g, s)
                    : g.MT == 128 ? launch_main<T, 128, 1, 0>(x, wp, part, Cin, Cout, H, W, g, s)
                                  : launch_main<T, 64, 3, 0>(x, wp, part, Cin, Cout, H, W, g, s);
    if (!ok) return LORA_E_LAUNCH;
    if ((H * W) % 4 == 0) {
        const int total = Cout * (g.M / 4);
        hipLaunchKernelGGL((conv_small_reduce_kernel<T, 4>), dim3((total + 255) / 256), dim3(256), 0, s, part, bias, static_cast<T*>(y_),
                           Cout, H * W, g.M, g.Mpad, g.S);
    } else {
        const int total = Cout * g.M;
        hipLaunchKernelGGL((conv_small_reduce_kernel<T, 1>), dim3((total + 255) / 256), dim3(256), 0, s, part, bias, static_cast<T*>(y_),
                           Cout, H * W, g.M, g.Mpad, g.S);
    }
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}

}  // namespace

extern "C" int conv3x3_small_supported(int N, int C_in, int C_out, int H, int W, int dtype) {
    return (dtype == LORA_F16 || dtype == LORA_BF16) && conv_geo(N, C_in, C_out, H, W).ok ? 1 : 0;
}

extern "C" int64_t conv3x3_small_workspace_bytes(int N, int C_in, int C_out, int H, int W, int dtype) {
    if (!conv3x3_small_supported(N, C_in, C_out, H, W, dtype)) return 0;
    return conv_geo(N, C_in, C_out, H, W).ws_bytes;
}

// The classes profiles/r14_conv_small_sweep.log shows faster than the stock call in BOTH directions inside a replayed graph
// (tools/conv_small_sweep.py): 1280 channels on one side and these on the other, at exactly these pixel counts (batch 4 of the
// 8x8 and 16x16 levels).  The backward of C_in -> C_out is the class C_out -> C_in.  Nothing else was measured, so nothing else
// is routed: other pixel counts of the same channels (batch 8, 96x96 latents) stay on the stock convolution.
namespace {
bool plan_channels(int C_in, int C_out, int64_t pixels /* 0: any measured pixel count */) {
    if (C_in != 1280 && C_out != 1280) return false;
    const int other = C_in == 1280 ? C_out : C_in;
    const bool at256 = other == 1280 || other == 2560;
    const bool at1024 = other == 640 || other == 1280 || other == 1920 || other == 2560;
    return pixels == 256 ? at256 : pixels == 1024 ? at1024 : pixels == 0 ? (at256 || at1024) : false;
}

// The form conv3x3_small stages a shape with: the rows form for the classes profiles/r18_conv_small_pipeline_sweep.log shows
// faster on it than on the position form in BOTH directions by more than the spread of the replays (batch 4 of the 8x8 and 16x16
// levels, the planner's classes: no other geometry was measured); the position form for everything else.
int measured_form(const Geo& g, int N, int Cin, int Cout, int H, int W) {
    const bool swept = N == 4 && H == W && (H == 8 || H == 16) && plan_channels(Cin, Cout, (int64_t)N * H * W);
    return swept && rows_units(g, H, W) ? kFormRows : kFormPosition;
}

// form < 0: the form conv3x3_small chooses
int small_call(const void* x, const void* wpack, const void* bias, void* y, void* workspace, int64_t workspace_bytes, int N, int C_in,
               int C_out, int H, int W, int dtype, int form, void* stream) {
    if (!x || !wpack || !y || !workspace || N < 1 || C_in < 1 || C_out < 1 || H < 1 || W < 1) return LORA_E_BADARG;
    if (dtype != LORA_F16 && dtype != LORA_BF16) return dtype == LORA_F32 ? LORA_E_UNSUPPORTED : LORA_E_BADARG;
    const Geo g = conv_geo(N, C_in, C_out, H, W);
    if (!g.ok) return LORA_E_UNSUPPORTED;
    if (form < 0) form = measured_form(g, N, C_in, C_out, H, W);
    const int ru = form == kFormRows ? rows_units(g, H, W) : 0;
    if (form == kFormRows && !ru) return LORA_E_UNSUPPORTED;
    if (workspace_bytes < g.ws_bytes) return LORA_E_BADARG;
    if (!aligned16(x) || !aligned16(wpack) || !aligned16(y) || !aligned16(workspace)) return LORA_E_ALIGN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return dtype == LORA_F16 ? run_conv<half_t>(x, wpack, bias, y, workspace, C_in, C_out, H, W, g, ru, s)
                             : run_conv<bf16_t>(x, wpack, bias, y, workspace, C_in, C_out, H, W, g, ru, s);
}
}  // namespace

// Whether this library (1) or the stock convolution (0) runs a frozen 3x3 convolution of `pixels` = N*H*W output pixels.
// A function of its arguments alone.
extern "C" int conv3x3_small_plan(int64_t pixels, int C_in, int C_out, int dtype) {
    if (dtype != LORA_F16 && dtype != LORA_BF16) return 0;
    return pixels >= 1 && plan_channels(C_in, C_out, pixels) ? 1 : 0;
}

// Whether conv3x3_small_plan routes these channels at SOME pixel count: what tells a caller which filters are worth packing
// before the activation's size is known.
extern "C" int conv3x3_small_plan_channels(int C_in, int C_out, int dtype) {
    if (dtype != LORA_F16 && dtype != LORA_BF16) return 0;
    return plan_channels(C_in, C_out, 0) ? 1 : 0;
}

extern "C" int conv3x3_small_pack(const void* w, void* packed, int C_in, int C_out, int backward, int dtype, void* stream) {
    if (!w || !packed || C_in < 1 || C_out < 1 || (backward != 0 && backward != 1)) return LORA_E_BADARG;
    if (dtype != LORA_F16 && dtype != LORA_BF16) return dtype == LORA_F32 ? LORA_E_UNSUPPORTED : LORA_E_BADARG;
    if (C_in % 32 || C_out % 32) return LORA_E_UNSUPPORTED;
    if (!aligned16(packed)) return LORA_E_ALIGN;
    const int64_t total = (int64_t)C_in * C_out * 9;
    if (total >= (1ll << 31)) return LORA_E_UNSUPPORTED;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((total + 255) / 256));
    if (dtype == LORA_F16)
        hipLaunchKernelGGL(conv_small_pack_kernel<half_t>, grid, dim3(256), 0, s, static_cast<const half_t*>(w),
                           static_cast<half_t*>(packed), C_in, C_out, backward);
    else
        hipLaunchKernelGGL(conv_small_pack_kernel<bf16_t>, grid, dim3(256), 0, s, static_cast<const bf16_t*>(w),
                           static_cast<bf16_t*>(packed), C_in, C_out, backward);
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}

extern "C" int conv3x3_small(const void* x, const void* wpack, const void* bias, void* y, void* workspace, int64_t workspace_bytes,
                             int N, int C_in, int C_out, int H, int W, int dtype, void* stream) {
    return small_call(x, wpack, bias, y, workspace, workspace_bytes, N, C_in, C_out, H, W, dtype, -1, stream);
}

// The form conv3x3_small stages a shape with: 0 (position) or 1 (rows); -1 where the family does not cover the shape.
extern "C" int conv3x3_small_form_choice(int N, int C_in, int C_out, int H, int W, int dtype) {
    if (dtype != LORA_F16 && dtype != LORA_BF16) return -1;
    const Geo g = conv_geo(N, C_in, C_out, H, W);
    return g.ok ? measured_form(g, N, C_in, C_out, H, W) : -1;
}

// conv3x3_small with a named form of the staging, for the sweep and the tests: 0 stages positions with 2-byte loads (every
// shape), 1 stages whole rows with 16-byte loads.  LORA_E_UNSUPPORTED, and nothing launched, where the form does not cover the
// shape; LORA_E_BADARG for an unknown form.  The two forms give the same bits.
extern "C" int conv3x3_small_form(const void* x, const void* wpack, const void* bias, void* y, void* workspace,
                                  int64_t workspace_bytes, int N, int C_in, int C_out, int H, int W, int dtype, int form,
                                  void* stream) {
    if (form != kFormPosition && form != kFormRows) return LORA_E_BADARG;
    return small_call(x, wpack, bias, y, workspace, workspace_bytes, N, C_in, C_out, H, W, dtype, form, stream);
}

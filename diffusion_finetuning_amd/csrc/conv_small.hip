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
#include "conv_common.h"

namespace {

constexpr int kNT = 128;        // output channels per workgroup (2 waves x 4 tiles of 16)

// MT pixels per workgroup; PER positions (all 32 channels of each) a thread stages per chunk: 256*PER >= positions of a tile.
template <typename T, int MT, int PER>
__global__ __launch_bounds__(kThreads) void conv_small_kernel(const T* __restrict__ x, const T* __restrict__ wp,
                                                              float* __restrict__ part, int Cin, int Cout, int H, int W, int M,
                                                              int mtiles, int ntiles, int cps, int chunks, int Mpad) {
    using Frag = typename Mfma<T>::Frag;
    constexpr int MF = MT / 32;  // 16-pixel fragments per wave (two waves along the pixels)
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

    // staging plan of this thread, chunk-invariant: positions tid, tid + 256, ... (PER of them), four 8-channel groups of each
    int xoff[PER];     // element offset of (position, channel 0 of the chunk) in x; -1: border or past the tile (zero / nothing)
    bool in_tile[PER];
#pragma unroll
    for (int s = 0; s < PER; ++s) {
        const int p = tid + s * kThreads;
        const int q = qlo + p, img = fast_div(q, PP, inv_pp), r = q - img * PP, hp = fast_div(r, W2, inv_w2), wq = r - hp * W2;
        in_tile[s] = p < P;
        const bool inside = in_tile[s] && hp >= 1 && hp <= H && wq >= 1 && wq <= W;
        xoff[s] = inside ? img * Cin * HW + (hp - 1) * W + (wq - 1) : -1;
    }
    // the loaded elements stay as they arrive until they are written to LDS a chunk later; zero selection and packing happen
    // there, so nothing waits for these loads while the current chunk is multiplied
    T raw[PER][32];
    auto load_stage = [&](int cc) {
        const T* base = x + (size_t)cc * kChunk * HW;
#pragma unroll
        for (int s = 0; s < PER; ++s) {
            // every lane loads (a border lane from offset 0, which is inside x): a conditional load makes a branch per element
            const int o = xoff[s] >= 0 ? xoff[s] : 0;
#pragma unroll
            for (int c = 0; c < 32; ++c) raw[s][c] = base[o + c * HW];
        }
    };

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

    load_stage(c_begin);
#pragma unroll
    for (int t = 0; t < 9; ++t) load_w(t, c_begin * 9 + t);
    for (int cc = c_begin; cc < c_end; ++cc) {
        __syncthreads();  // the previous chunk has been read by every wave
#pragma unroll
        for (int s = 0; s < PER; ++s)
            if (in_tile[s]) {
#pragma unroll
                for (int c8 = 0; c8 < 4; ++c8) {
                    Frag v;
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = xoff[s] >= 0 ? raw[s][c8 * 8 + j] : static_cast<T>(0.f);
                    *reinterpret_cast<Frag*>(smem + (tid + s * kThreads) * kPitch + c8 * 16) = v;
                }
            }
        __syncthreads();
        load_stage(min(cc + 1, c_end - 1));
        __builtin_amdgcn_sched_barrier(0);
        Frag xf[2][MF];
#pragma unroll
        for (int f = 0; f < MF; ++f) xf[0][f] = *reinterpret_cast<const Frag*>(smem + lpos[f]);
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            if (t + 1 < 9) {  // the next tap's pixels come out of LDS while this one is multiplied
                const int sh = (((t + 1) / 3) * W2 + ((t + 1) % 3)) * kPitch;
#pragma unroll
                for (int f = 0; f < MF; ++f) xf[(t + 1) & 1][f] = *reinterpret_cast<const Frag*>(smem + lpos[f] + sh);
            }
#pragma unroll
            for (int f = 0; f < MF; ++f)
#pragma unroll
                for (int g = 0; g < 4; ++g) acc[f][g] = Mfma<T>::run(xf[t & 1][f], wf[t][g], acc[f][g]);
            load_w(t, cc * 9 + t + 9);
            // keeps the request here, a chunk ahead of its use: left alone, the scheduler gathers all nine at the loop's end
            __builtin_amdgcn_sched_barrier(0);
        }
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

template <typename T, int MT, int PER>
bool launch_main(const T* x, const T* wp, float* part, int Cin, int Cout, int H, int W, const Geo& g, hipStream_t s) {
    const int lds = g.Pcap * kPitch;
    auto kern = conv_small_kernel<T, MT, PER>;
    if (lds > 48 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess)
        return false;
    hipLaunchKernelGGL(kern, dim3(g.mtiles * g.ntiles * g.S), dim3(kThreads), lds, s, x, wp, part, Cin, Cout, H, W, g.M, g.mtiles,
                       g.ntiles, g.cps, g.chunks, g.Mpad);
    return true;
}

template <typename T>
int run_conv(const void* x_, const void* wp_, const void* bias_, void* y_, void* ws, int Cin, int Cout, int H, int W, const Geo& g,
             hipStream_t s) {
    const T *x = static_cast<const T*>(x_), *wp = static_cast<const T*>(wp_), *bias = static_cast<const T*>(bias_);
    float* part = static_cast<float*>(ws);
    const bool ok = g.MT == 128 ? launch_main<T, 128, 1>(x, wp, part, Cin, Cout, H, W, g, s)
                                : launch_main<T, 64, 3>(x, wp, part, Cin, Cout, H, W, g, s);
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
    if (!x || !wpack || !y || !workspace || N < 1 || C_in < 1 || C_out < 1 || H < 1 || W < 1) return LORA_E_BADARG;
    if (dtype != LORA_F16 && dtype != LORA_BF16) return dtype == LORA_F32 ? LORA_E_UNSUPPORTED : LORA_E_BADARG;
    const Geo g = conv_geo(N, C_in, C_out, H, W);
    if (!g.ok) return LORA_E_UNSUPPORTED;
    if (workspace_bytes < g.ws_bytes) return LORA_E_BADARG;
    if (!aligned16(x) || !aligned16(wpack) || !aligned16(y) || !aligned16(workspace)) return LORA_E_ALIGN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return dtype == LORA_F16 ? run_conv<half_t>(x, wpack, bias, y, workspace, C_in, C_out, H, W, g, s)
                             : run_conv<bf16_t>(x, wpack, bias, y, workspace, C_in, C_out, H, W, g, s);
}

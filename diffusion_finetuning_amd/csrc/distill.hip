// svd_distill of lora_diffusion/cli_svd.py:29-111: the top-r singular triplets of D = T(W1 − W0) for every target linear of a
// model, by batched block subspace iteration with Rayleigh–Ritz (DESIGN.md "svd_distill").  Every phase is one launch for all
// layers; a layer is one int64 table row {W1, W0, N, K, workspace byte offset, output float offset, layer index, 0}.
//
// Per-layer workspace (lora_distill_workspace_bytes): a state header, the Ritz data of the last left step (λ, Ũ in fp64) and
// three fp32 blocks of width 32: Y/U [N,32], Z [K,32], V [K,32].  Columns beyond min(N,K) carry zero eigenvalues and are
// masked, so the block width l = min(32, N, K) needs no special case.  Ranks 17–64 run on distill_wide.hip; the helpers both
// share (difference on load, start block, workgroup sum, quantile clamp) are in distill_common.h.
#include "distill_common.h"

namespace {

constexpr int kW = 32;               // block width l (columns of Y, Z, V)
constexpr int kMaxSweeps = 24;       // Jacobi sweeps (a 32×32 matrix converges in 6–9)

// workspace layout of one layer (bytes).  Twin: distill_wide.hip restates the header offsets, Layer, load_layer and the Jacobi
// body at a template width; a fix to any of them here is carried there.
constexpr int64_t kOffFlag = 0;     // int32: 0 running, 1 converged, 2 hit max_iters, 3 non-finite
constexpr int64_t kOffIters = 4;     // int32: iterations done
constexpr int64_t kOffRes = 8;       // double: last residual max_i ‖Dᵀu_i − σ_i v_i‖ / σ_1
constexpr int64_t kOffLam = 64;      // double[32]: λ of the last left step, descending, masked ones 0
constexpr int64_t kOffUt = 512;      // double[32][32]: the matching eigenvectors Ũ (columns)
constexpr int64_t kOffBlocks = 512 + 8 * kW * kW;

struct Layer {
    const void* w1;
    const void* w0;
    int64_t N, K;
    unsigned char* ws;
    int64_t out_off, id;
    __device__ int* flag() const { return reinterpret_cast<int*>(ws + kOffFlag); }
    __device__ double* lam() const { return reinterpret_cast<double*>(ws + kOffLam); }
    __device__ double* ut() const { return reinterpret_cast<double*>(ws + kOffUt); }
    __device__ float* Y() const { return reinterpret_cast<float*>(ws + kOffBlocks); }
    __device__ float* Z() const { return Y() + N * kW; }
    __device__ float* V() const { return Z() + K * kW; }
};

__device__ __forceinline__ Layer load_layer(const int64_t* table, unsigned char* ws, int64_t index) {
    const int64_t* row = table + 8 * index;
    Layer L;
    L.w1 = reinterpret_cast<const void*>(row[0]);
    L.w0 = reinterpret_cast<const void*>(row[1]);
    L.N = row[2];
    L.K = row[3];
    L.ws = ws + row[4];
    L.out_off = row[5];
    L.id = row[6];
    return L;
}

// ---------------------------------------------------------------------------------------------------------------------
// Diff-GEMM.  TRANS = false: Y[N,32] = D·V (V [K,32]).  TRANS = true: Z[K,32] = Dᵀ·U (U = the Y block [N,32]).
// One workgroup per 64 output rows of one layer (grid.y = layer), four waves of 16 rows × 32 columns each on
// v_mfma_f32_16x16x4_f32 (exact f32 products, k-ordered fp32 accumulation).  D is formed on load and never stored.
template <typename T, bool TRANS>
__global__ __launch_bounds__(256) void distill_diff_kernel(const int64_t* table, unsigned char* ws) {
    const Layer L = load_layer(table, ws, blockIdx.y);
    const int64_t M = TRANS ? L.K : L.N, Lr = TRANS ? L.N : L.K;
    const int64_t m0 = (int64_t)blockIdx.x * kTile;
    if (m0 >= M || *L.flag() != 0) return;
    const T* w1 = static_cast<const T*>(L.w1);
    const T* w0 = static_cast<const T*>(L.w0);
    const float* src = TRANS ? L.Y() : L.V();
    float* dst = TRANS ? L.Z() : L.Y();

    __shared__ float Ds[kTile][kTile + 1];  // Ds[output row][contraction index]
    __shared__ float Bs[kTile][kW + 1];     // Bs[contraction index][column]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    for (int64_t t0 = 0; t0 < Lr; t0 += kTile) {
#pragma unroll 4
        for (int i = 0; i < 16; ++i) {  // D tile in memory order: row a of the tile, 64 contiguous columns b
            const int e = tid + 256 * i, a = e >> 6, b = e & 63;
            const int64_t gr = (TRANS ? t0 : m0) + a, gc = (TRANS ? m0 : t0) + b;
            float d = 0.f;
            if (gr < L.N && gc < L.K) d = diff_of<T>(w1, w0, gr * L.K + gc);
            if (TRANS) Ds[b][a] = d;
            else Ds[a][b] = d;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int e = tid + 256 * i, t = e >> 5, j = e & 31;
            Bs[t][j] = (t0 + t < Lr) ? src[(t0 + t) * kW + j] : 0.f;
        }
        __syncthreads();
        const int ar = wave * 16 + (lane & 15), kq = lane >> 4;
#pragma unroll 4
        for (int kk = 0; kk < kTile; kk += 4) {
            const float a = Ds[ar][kk + kq];
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Bs[kk + kq][lane & 15], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Bs[kk + kq][16 + (lane & 15)], acc1, 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const int64_t m = m0 + wave * 16 + (lane >> 4) * 4 + v;
        if (m < M) {
            dst[m * kW + (lane & 15)] = acc0[v];
            dst[m * kW + 16 + (lane & 15)] = acc1[v];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// H (32×32, symmetric, LDS) → eigenvalues on its diagonal, eigenvectors in the columns of E: cyclic Jacobi in
// parallel (round-robin) order, 16 disjoint rotations per round, 31 rounds per sweep.
__device__ void jacobi32(double (*H)[kW + 1], double (*E)[kW + 1], double* red, double* cs) {
    const int tid = threadIdx.x;
    for (int e = tid; e < kW * kW; e += 256) E[e >> 5][e & 31] = (e >> 5) == (e & 31) ? 1.0 : 0.0;
    __syncthreads();
    for (int sweep = 0; sweep < kMaxSweeps; ++sweep) {
        double off = 0.0, dia = 0.0;
        for (int e = tid; e < kW * kW; e += 256) {
            const double h = H[e >> 5][e & 31];
            if ((e >> 5) == (e & 31)) dia += h * h;
            else off += h * h;
        }
        off = block_sum(off, red);
        dia = block_sum(dia, red);
        if (!(off > 1e-30 * dia)) break;  // also ends on a zero matrix
        for (int round = 0; round < kW - 1; ++round) {
            if (tid < 16) {
                // circle method: player 0 fixed, players 1..31 rotate
                const int p0 = tid == 0 ? 0 : ((tid - 1 + round) % (kW - 1)) + 1;
                const int q0 = ((kW - 2 - tid + round) % (kW - 1)) + 1;
                const int p = p0 < q0 ? p0 : q0, q = p0 < q0 ? q0 : p0;
                const double apq = H[p][q], app = H[p][p], aqq = H[q][q];
                double c = 1.0, s = 0.0;
                if (apq != 0.0 && fabs(apq) > 1e-300) {
                    const double tau = (aqq - app) / (2.0 * apq);
                    const double t = fabs(tau) > 1e150 ? 0.5 / tau
                                                       : (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                    c = 1.0 / sqrt(1.0 + t * t);
                    s = t * c;
                }
                cs[4 * tid + 0] = c;
                cs[4 * tid + 1] = s;
                cs[4 * tid + 2] = p;
                cs[4 * tid + 3] = q;
            }
            __syncthreads();
            const int pr = tid >> 4;
            const double c = cs[4 * pr], s = cs[4 * pr + 1];
            const int p = (int)cs[4 * pr + 2], q = (int)cs[4 * pr + 3];
#pragma unroll
            for (int h = 0; h < 2; ++h) {  // H ← H·J, E ← E·J (columns p, q)
                const int k = (tid & 15) * 2 + h;
                const double hp = H[k][p], hq = H[k][q];
                H[k][p] = c * hp - s * hq;
                H[k][q] = s * hp + c * hq;
                const double ep = E[k][p], eq = E[k][q];
                E[k][p] = c * ep - s * eq;
                E[k][q] = s * ep + c * eq;
            }
            __syncthreads();
#pragma unroll
            for (int h = 0; h < 2; ++h) {  // H ← Jᵀ·H (rows p, q)
                const int k = (tid & 15) * 2 + h;
                const double hp = H[p][k], hq = H[q][k];
                H[p][k] = c * hp - s * hq;
                H[q][k] = s * hp + c * hq;
            }
            __syncthreads();
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Rayleigh–Ritz / orthonormalisation, one workgroup per layer.
//   SIDE 0 (start): V ← V₀ (pseudo-random, keyed by seed and layer index), then V ← V·Ẽ·Λ^{-1/2}.
//   SIDE 1 (left):  H = YᵀY = Ẽ Λ Ẽᵀ (λ descending); Ũ, λ kept; Y ← Y·Ũ·Λ^{-1/2} = U (dropped directions zero).
//   SIDE 2 (right): residual_i = ‖z_i − σ_i·(V·ũ_i)‖ for i < r (z_i = Dᵀu_i), res = max_i / σ_1.  Converged (or `last`):
//                   V ← V·Ũ — column i is v_i, the final `down` row — and the layer is frozen; else V ← Z·Ẽ·Λ^{-1/2}.
template <int SIDE>
__global__ __launch_bounds__(256) void distill_rr_kernel(const int64_t* table, unsigned char* ws, int r, double tol,
                                                        int last, uint64_t seed) {
    const Layer L = load_layer(table, ws, blockIdx.x);
    if (SIDE != 0 && *L.flag() != 0) return;
    const int tid = threadIdx.x;
    const int64_t M = SIDE == 1 ? L.N : L.K;
    float* X = SIDE == 0 ? L.V() : (SIDE == 1 ? L.Y() : L.Z());
    float* dst = SIDE == 1 ? L.Y() : L.V();

    __shared__ double H[kW][kW + 1];
    __shared__ double E[kW][kW + 1];
    __shared__ double T[kW][kW + 1];
    __shared__ float St[kTile][kW + 1];
    __shared__ double red[256];
    __shared__ double cs[64];
    __shared__ double lam_s[kW];
    __shared__ int perm[kW];
    __shared__ int decide;

    if (SIDE == 0) {
        if (tid == 0) {
            *L.flag() = 0;
            *reinterpret_cast<int*>(L.ws + kOffIters) = 0;
            *reinterpret_cast<double*>(L.ws + kOffRes) = 0.0;
        }
        for (int64_t e = tid; e < M * kW; e += 256) X[e] = start_value(seed, L.id, e);
        __syncthreads();
    }

    if (SIDE == 2) {  // residual of the Ritz pairs of the last left step
        const double* ut = L.ut();
        const double* lam = L.lam();
        for (int e = tid; e < kW * kW; e += 256) T[e >> 5][e & 31] = ut[e];
        __syncthreads();
        const int i = tid & 15, g = tid >> 4;
        double acc = 0.0;
        if (i < r) {
            const double sig = sqrt(lam[i]);
            const float* V = L.V();
            for (int64_t k = g; k < L.K; k += 16) {
                double v = 0.0;
                for (int j = 0; j < kW; ++j) v += (double)V[k * kW + j] * T[j][i];
                const double e = (double)X[k * kW + i] - sig * v;
                acc += e * e;
            }
        }
        red[tid] = acc;
        __syncthreads();
        if (tid == 0) {
            double worst = 0.0;
            for (int ii = 0; ii < r; ++ii) {
                double s = 0.0;
                for (int gg = 0; gg < 16; ++gg) s += red[gg * 16 + ii];
                worst = fmax(worst, s);
                if (!isfinite(s)) worst = s;
            }
            const double s1 = sqrt(lam[0]);
            const double res = s1 > 0.0 ? sqrt(worst) / s1 : (worst == 0.0 ? 0.0 : worst);
            *reinterpret_cast<double*>(L.ws + kOffRes) = res;
            *reinterpret_cast<int*>(L.ws + kOffIters) += 1;
            int d = 0;
            if (!isfinite(res)) d = 3;
            else if (res <= tol) d = 1;
            else if (last) d = 2;
            decide = d;
        }
        __syncthreads();
        const int d = decide;
        if (d != 0) {
            if (d != 3) {  // V ← V·Ũ, masked directions zero
                for (int64_t k = tid; k < L.K; k += 256) {
                    float* v = L.V() + k * kW;
                    float x[kW];
#pragma unroll
                    for (int j = 0; j < kW; ++j) x[j] = v[j];
                    for (int c = 0; c < kW; ++c) {
                        double a = 0.0;
#pragma unroll
                        for (int j = 0; j < kW; ++j) a += (double)x[j] * T[j][c];
                        v[c] = lam[c] > 0.0 ? (float)a : 0.f;
                    }
                }
            }
            __syncthreads();
            if (tid == 0) *L.flag() = d;
            return;
        }
    }

    // Gram matrix in fp64, rows staged through LDS in a fixed order
    {
        const int a = tid >> 3, b0 = (tid & 7) * 4;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int64_t m0 = 0; m0 < M; m0 += kTile) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int e = tid + 256 * i, rr = e >> 5, c = e & 31;
                St[rr][c] = (m0 + rr < M) ? X[(m0 + rr) * kW + c] : 0.f;
            }
            __syncthreads();
            for (int rr = 0; rr < kTile; ++rr) {
                const double xa = St[rr][a];
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] += xa * (double)St[rr][b0 + q];
            }
            __syncthreads();
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) H[a][b0 + q] = acc[q];
        double bad = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) bad += isfinite(acc[q]) ? 0.0 : 1.0;
        bad = block_sum(bad, red);
        if (bad != 0.0) {
            if (tid == 0) *L.flag() = 3;
            return;
        }
    }
    jacobi32(H, E, red, cs);

    if (tid == 0) {  // λ descending, ties to the lower index; mask λ ≤ ε·λ_max
        unsigned used = 0;
        for (int i = 0; i < kW; ++i) {
            int best = -1;
            for (int j = 0; j < kW; ++j)
                if (!(used >> j & 1u) && (best < 0 || H[j][j] > H[best][best])) best = j;
            used |= 1u << best;
            perm[i] = best;
            lam_s[i] = H[best][best];
        }
        const double lmax = lam_s[0];
        for (int i = 0; i < kW; ++i)
            if (!(lmax > 0.0) || !(lam_s[i] > kMaskEps * lmax)) lam_s[i] = 0.0;
    }
    __syncthreads();
    for (int e = tid; e < kW * kW; e += 256) {
        const int j = e >> 5, i = e & 31;
        const double u = E[j][perm[i]];
        T[j][i] = lam_s[i] > 0.0 ? u / sqrt(lam_s[i]) : 0.0;
        if (SIDE == 1) L.ut()[e] = u;
    }
    if (SIDE == 1 && tid < kW) L.lam()[tid] = lam_s[tid];
    __syncthreads();
    // dst ← X·T row by row (in place when dst == X: a row is read whole before it is written, by one thread)
    for (int64_t m = tid; m < M; m += 256) {
        const float* xr = X + m * kW;
        float x[kW];
#pragma unroll
        for (int j = 0; j < kW; ++j) x[j] = xr[j];
        float* dr = dst + m * kW;
        for (int c = 0; c < kW; ++c) {
            double a = 0.0;
#pragma unroll
            for (int j = 0; j < kW; ++j) a += (double)x[j] * T[j][c];
            dr[c] = (float)a;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void quantile_clamp_kernel(float* x, int64_t n, float q, float* hi_out) {
    __shared__ int hist[256];
    __shared__ int64_t sh[2];
    const float v = quantile_clamp(x, n, q, true, hist, sh);
    if (threadIdx.x == 0 && hi_out) *hi_out = v;
}

// Final factors of every layer into out[out_off ..] (finalize_layer of distill_common.h at row stride 32).
__global__ __launch_bounds__(256) void distill_finalize_kernel(const int64_t* table, unsigned char* ws, int r, float q,
                                                               int clamp, float* out) {
    const Layer L = load_layer(table, ws, blockIdx.x);
    if (*L.flag() == 3) return;
    finalize_layer<16>(L.Y(), L.V(), L.lam(), L.flag(), L.N, L.K, kW, r, q, clamp, out + L.out_off);
}

bool rank_ok(int r) { return r >= 1 && r <= 16; }

}  // namespace

extern "C" int64_t lora_distill_workspace_bytes(int64_t N, int64_t K) {
    if (N < 1 || K < 1) return 0;
    const int64_t b = kOffBlocks + (N + 2 * K) * kW * 4;
    return (b + 255) / 256 * 256;
}

extern "C" int lora_distill_start(const int64_t* table, int n_layers, int64_t min_nk, int r, int64_t seed, void* workspace,
                                  void* stream) {
    if (!table || !workspace || n_layers < 1 || min_nk < 1) return LORA_E_BADARG;
    if (r < 1 || r > min_nk) return LORA_E_RANK;
    if (r > 16) return LORA_E_UNSUPPORTED;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(distill_rr_kernel<0>, dim3(n_layers), dim3(256), 0, s, table, static_cast<unsigned char*>(workspace),
                       r, 0.0, 0, (uint64_t)seed);
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}

template <bool TRANS>
static int diff_dispatch(const int64_t* table, int n_layers, int64_t max_rows, int dtype, unsigned char* ws, hipStream_t s) {
    const dim3 grid((unsigned)((max_rows + kTile - 1) / kTile), (unsigned)n_layers);
    switch (dtype) {
        case LORA_F32: hipLaunchKernelGGL((distill_diff_kernel<float, TRANS>), grid, dim3(256), 0, s, table, ws); break;
        case LORA_F16: hipLaunchKernelGGL((distill_diff_kernel<half_t, TRANS>), grid, dim3(256), 0, s, table, ws); break;
        case LORA_BF16: hipLaunchKernelGGL((distill_diff_kernel<bf16_t, TRANS>), grid, dim3(256), 0, s, table, ws); break;
        default: return LORA_E_BADARG;
    }
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}

extern "C" int lora_distill_diff(const int64_t* table, int n_layers, int64_t max_rows, int transpose, int dtype,
                                 void* workspace, void* stream) {
    if (!table || !workspace || n_layers < 1 || n_layers > 65535 || max_rows < 1) return LORA_E_BADARG;
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    hipStream_t s = static_cast<hipStream_t>(stream);
    return transpose ? diff_dispatch<true>(table, n_layers, max_rows, dtype, ws, s)
                     : diff_dispatch<false>(table, n_layers, max_rows, dtype, ws, s);
}

extern "C" int lora_distill_rayleigh_ritz(const int64_t* table, int n_layers, int side, int r, double tol, int last,
                                          void* workspace, void* stream) {
    if (!table || !workspace || n_layers < 1 || (side != 1 && side != 2)) return LORA_E_BADARG;
    if (r < 1) return LORA_E_RANK;
    if (!rank_ok(r)) return LORA_E_UNSUPPORTED;
    hipStream_t s = static_cast<hipStream_t>(stream);
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    if (side == 1) hipLaunchKernelGGL(distill_rr_kernel<1>, dim3(n_layers), dim3(256), 0, s, table, ws, r, tol, last, 0ull);
    else hipLaunchKernelGGL(distill_rr_kernel<2>, dim3(n_layers), dim3(256), 0, s, table, ws, r, tol, last, 0ull);
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}

extern "C" int lora_distill_finalize(const int64_t* table, int n_layers, int r, float q, int clamp, void* workspace,
                                     float* out, void* stream) {
    if (!table || !workspace || !out || n_layers < 1) return LORA_E_BADARG;
    if (clamp && !(q >= 0.f && q <= 1.f)) return LORA_E_BADARG;
    if (r < 1) return LORA_E_RANK;
    if (!rank_ok(r)) return LORA_E_UNSUPPORTED;
    hipLaunchKernelGGL(distill_finalize_kernel, dim3(n_layers), dim3(256), 0, static_cast<hipStream_t>(stream), table,
                       static_cast<unsigned char*>(workspace), r, q, clamp, out);
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}

extern "C" int lora_quantile_clamp(float* x, int64_t n, float q, float* hi_out, void* stream) {
    if (!x || n < 1 || !(q >= 0.f && q <= 1.f)) return LORA_E_BADARG;
    hipLaunchKernelGGL(quantile_clamp_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), x, n, q, hi_out);
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}

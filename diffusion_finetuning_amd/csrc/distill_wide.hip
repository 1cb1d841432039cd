// svd_distill (lora_diffusion/cli_svd.py:29-111) at ranks up to 64: the algorithm of distill.hip — batched block subspace
// iteration with Rayleigh–Ritz, one launch per phase over the int64 layer table (DESIGN.md "svd_distill") — at a block width W
// chosen from the rank: W = 48 for r ≤ 32, 64 for r ≤ 48, 80 for r ≤ 64 (W ≥ r + 16 extra directions, as width 32 gives rank 16).
//
// Per-layer workspace (lora_distill_wide_workspace_bytes): the state header of distill.hip (flag, iterations, residual, λ at
// +64), Ũ [W][W] in fp64 at +1280, then three fp32 blocks of width W: Y/U [N,W], Z [K,W], V [K,W].  Columns beyond min(N,K)
// carry zero eigenvalues and are masked, so W > min(N,K) needs no special case.
//
// LDS of the Rayleigh–Ritz kernel: two fp64 W×W arrays, not three.  `A` is the Gram matrix H while it is built and
// diagonalised, and the transform T before (side 2: T = Ũ read back from the workspace for the residual) and after (T = Ẽ·Λ^-½
// once H's diagonal has been copied out); `E` holds the eigenvectors.  At W = 80 that is 2·80·81·8 = 103,680 B, with the row
// staging tile and the small arrays 129,736 B of the 160 KiB.  Ũ and λ live in the layer's workspace between launches.
#include "distill_common.h"

namespace {

constexpr int kMaxRank = 64;

// workspace layout of one layer (bytes); the header fields are those of distill.hip.  Twin: distill.hip holds the width-32
// forms of these offsets, of Layer, load_layer and the Jacobi body; a fix to any of them here is carried there.
constexpr int64_t kOffFlag = 0;      // int32: 0 running, 1 converged, 2 hit max_iters, 3 non-finite
constexpr int64_t kOffIters = 4;     // int32: iterations done
constexpr int64_t kOffRes = 8;       // double: last residual max_i ‖Dᵀu_i − σ_i v_i‖ / σ_1
constexpr int64_t kOffLam = 64;      // double[W]: λ of the last left step, descending, masked ones 0
constexpr int64_t kOffUt = 1280;     // double[W][W]: the matching eigenvectors Ũ (columns); room for λ up to W = 128
__host__ __device__ constexpr int64_t blocks_offset(int W) { return kOffUt + 8 * (int64_t)W * W; }
static_assert(kOffLam + 8 * 80 <= kOffUt, "λ of the widest block (80) overlaps Ũ");

// Jacobi sweep cap for a W×W matrix.  Cyclic Jacobi converges quadratically once the off-diagonal mass is small, and the
// sweeps before that grow like log W: 6–9 at W = 32 (distill.hip caps at 24), 8–12 at W = 80.  24 + W/8 (30, 32, 34) keeps the
// same factor of about three over what a full-rank Gram matrix needs.  A matrix still not diagonal at the cap is used as it
// is: the residual test then keeps the layer running, and `last` ends it in flag 2.
__host__ __device__ constexpr int max_sweeps(int W) { return 24 + W / 8; }

int width_of(int r) { return r <= 32 ? 48 : (r <= 48 ? 64 : 80); }

template <int W> struct Layer {
    const void* w1;
    const void* w0;
    int64_t N, K;
    unsigned char* ws;
    int64_t out_off, id;
    __device__ int* flag() const { return reinterpret_cast<int*>(ws + kOffFlag); }
    __device__ double* lam() const { return reinterpret_cast<double*>(ws + kOffLam); }
    __device__ double* ut() const { return reinterpret_cast<double*>(ws + kOffUt); }
    __device__ float* Y() const { return reinterpret_cast<float*>(ws + blocks_offset(W)); }
    __device__ float* Z() const { return Y() + N * W; }
    __device__ float* V() const { return Z() + K * W; }
};

template <int W> __device__ __forceinline__ Layer<W> load_layer(const int64_t* table, unsigned char* ws, int64_t index) {
    const int64_t* row = table + 8 * index;
    Layer<W> L;
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
// Diff-GEMM.  TRANS = false: Y[N,W] = D·V (V [K,W]).  TRANS = true: Z[K,W] = Dᵀ·U (U = the Y block [N,W]).
// One workgroup per 64 output rows of one layer (grid.y = layer), four waves of 16 rows × W columns each: W/16 independent
// accumulators on v_mfma_f32_16x16x4_f32 (exact f32 products, k-ordered fp32 accumulation).  A 64×64 tile of D is formed on
// load, staged ONCE per contraction step and used for all W columns; D is never stored.
// LDS strides: Ds rows of 66 floats put the 16 rows × 2 k of a half-wave's A read on 32 distinct banks; Bs rows of a stride
// ≡ 16 (mod 32) do the same for the 2 k × 16 columns of its B read.
template <typename T, bool TRANS, int W>
__global__ __launch_bounds__(256) void distill_wide_diff_kernel(const int64_t* table, unsigned char* ws) {
    const Layer<W> L = load_layer<W>(table, ws, blockIdx.y);
    const int64_t M = TRANS ? L.K : L.N, Lr = TRANS ? L.N : L.K;
    const int64_t m0 = (int64_t)blockIdx.x * kTile;
    if (m0 >= M || *L.flag() != 0) return;
    const T* w1 = static_cast<const T*>(L.w1);
    const T* w0 = static_cast<const T*>(L.w0);
    const float* src = TRANS ? L.Y() : L.V();
    float* dst = TRANS ? L.Z() : L.Y();

    constexpr int NB = W / 16;
    constexpr int BS = (W % 32 == 16) ? W : W + 16;
    __shared__ float Ds[kTile][kTile + 2];  // Ds[output row][contraction index]
    __shared__ float Bs[kTile][BS];         // Bs[contraction index][column]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    f32x4 acc[NB];
#pragma unroll
    for (int c = 0; c < NB; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
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
#pragma unroll 4
        for (int i = 0; i < W / 4; ++i) {  // kTile·W / 256 values per thread
            const int e = tid + 256 * i, t = e / W, j = e % W;
            Bs[t][j] = (t0 + t < Lr) ? src[(t0 + t) * W + j] : 0.f;
        }
        __syncthreads();
        const int ar = wave * 16 + (lane & 15), kq = lane >> 4;
#pragma unroll 4
        for (int kk = 0; kk < kTile; kk += 4) {
            const float a = Ds[ar][kk + kq];
#pragma unroll
            for (int c = 0; c < NB; ++c)
                acc[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Bs[kk + kq][16 * c + (lane & 15)], acc[c], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const int64_t m = m0 + wave * 16 + (lane >> 4) * 4 + v;
        if (m < M) {
#pragma unroll
            for (int c = 0; c < NB; ++c) dst[m * W + 16 * c + (lane & 15)] = acc[c][v];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// H (W×W, symmetric, LDS) → eigenvalues on its diagonal, eigenvectors in the columns of E: cyclic Jacobi in parallel
// (round-robin) order, W/2 disjoint rotations per round, W − 1 rounds per sweep, at most max_sweeps(W) sweeps.
template <int W> __device__ void jacobi(double (*H)[W + 1], double (*E)[W + 1], double* red, double* cs) {
    const int tid = threadIdx.x;
    for (int e = tid; e < W * W; e += 256) E[e / W][e % W] = (e / W) == (e % W) ? 1.0 : 0.0;
    __syncthreads();
    for (int sweep = 0; sweep < max_sweeps(W); ++sweep) {
        double off = 0.0, dia = 0.0;
        for (int e = tid; e < W * W; e += 256) {
            const double h = H[e / W][e % W];
            if ((e / W) == (e % W)) dia += h * h;
            else off += h * h;
        }
        off = block_sum(off, red);
        dia = block_sum(dia, red);
        if (!(off > 1e-30 * dia)) break;  // also ends on a zero matrix
        for (int round = 0; round < W - 1; ++round) {
            if (tid < W / 2) {
                // circle method: player 0 fixed, players 1..W−1 rotate
                const int p0 = tid == 0 ? 0 : ((tid - 1 + round) % (W - 1)) + 1;
                const int q0 = ((W - 2 - tid + round) % (W - 1)) + 1;
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
            for (int e = tid; e < (W / 2) * W; e += 256) {  // H ← H·J, E ← E·J (columns p, q of rotation e / W, row e % W)
                const int pr = e / W, k = e % W;
                const double c = cs[4 * pr], s = cs[4 * pr + 1];
                const int p = (int)cs[4 * pr + 2], q = (int)cs[4 * pr + 3];
                const double hp = H[k][p], hq = H[k][q];
                H[k][p] = c * hp - s * hq;
                H[k][q] = s * hp + c * hq;
                const double ep = E[k][p], eq = E[k][q];
                E[k][p] = c * ep - s * eq;
                E[k][q] = s * ep + c * eq;
            }
            __syncthreads();
            for (int e = tid; e < (W / 2) * W; e += 256) {  // H ← Jᵀ·H (rows p, q)
                const int pr = e / W, k = e % W;
                const double c = cs[4 * pr], s = cs[4 * pr + 1];
                const int p = (int)cs[4 * pr + 2], q = (int)cs[4 * pr + 3];
                const double hp = H[p][k], hq = H[q][k];
                H[p][k] = c * hp - s * hq;
                H[q][k] = s * hp + c * hq;
            }
            __syncthreads();
        }
    }
}

// dst ← X·T row by row, fp64 accumulation (in place when dst == X: a row is read whole before it is written, by one
// thread).  With `keep`, column c is written as zero unless keep[c] > 0.
template <int W>
__device__ void rows_times(const float* X, float* dst, int64_t M, const double (*T)[W + 1], const double* keep) {
    for (int64_t m = threadIdx.x; m < M; m += 256) {
        const float* xr = X + m * W;
        float x[W];
#pragma unroll
        for (int j = 0; j < W; ++j) x[j] = xr[j];
        float* dr = dst + m * W;
        for (int c = 0; c < W; ++c) {
            double a = 0.0;
#pragma unroll
            for (int j = 0; j < W; ++j) a += (double)x[j] * T[j][c];
            dr[c] = (!keep || keep[c] > 0.0) ? (float)a : 0.f;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Rayleigh–Ritz / orthonormalisation, one workgroup per layer.
//   SIDE 0 (start): V ← V₀ (pseudo-random, keyed by seed and layer index), then V ← V·Ẽ·Λ^{-1/2}.
//   SIDE 1 (left):  H = YᵀY = Ẽ Λ Ẽᵀ (λ descending); Ũ, λ kept; Y ← Y·Ũ·Λ^{-1/2} = U (dropped directions zero).
//   SIDE 2 (right): residual_i = ‖z_i − σ_i·(V·ũ_i)‖ for i < r (z_i = Dᵀu_i), res = max_i / σ_1.  Converged (or `last`):
//                   V ← V·Ũ — column i is v_i, the final `down` row — and the layer is frozen; else V ← Z·Ẽ·Λ^{-1/2}.
template <int W, int SIDE>
__global__ __launch_bounds__(256) void distill_wide_rr_kernel(const int64_t* table, unsigned char* ws, int r, double tol,
                                                             int last, uint64_t seed) {
    const Layer<W> L = load_layer<W>(table, ws, blockIdx.x);
    if (SIDE != 0 && *L.flag() != 0) return;
    const int tid = threadIdx.x;
    const int64_t M = SIDE == 1 ? L.N : L.K;
    float* X = SIDE == 0 ? L.V() : (SIDE == 1 ? L.Y() : L.Z());
    float* dst = SIDE == 1 ? L.Y() : L.V();

    __shared__ double A[W][W + 1];  // T = Ũ (side 2 residual), then H, then T = Ẽ·Λ^-½
    __shared__ double E[W][W + 1];
    __shared__ float St[kTile][W + 1];
    __shared__ double red[256];
    __shared__ double cs[2 * W];
    __shared__ double lam_d[W];
    __shared__ double lam_s[W];
    __shared__ int perm[W];
    __shared__ int decide;

    if (SIDE == 0) {
        if (tid == 0) {
            *L.flag() = 0;
            *reinterpret_cast<int*>(L.ws + kOffIters) = 0;
            *reinterpret_cast<double*>(L.ws + kOffRes) = 0.0;
        }
        for (int64_t e = tid; e < M * W; e += 256) X[e] = start_value(seed, L.id, e);
        __syncthreads();
    }

    if (SIDE == 2) {  // residual of the Ritz pairs of the last left step
        const double* ut = L.ut();
        const double* lam = L.lam();
        for (int e = tid; e < W * W; e += 256) A[e / W][e % W] = ut[e];
        __syncthreads();
        // thread (g, i): column i of the first r, rows k ≡ g (mod groups); rc = r rounded up to 16, groups = 256 / rc ≥ 4
        const int rc = (r + 15) & ~15, groups = 256 / rc;
        const int i = tid % rc, g = tid / rc;
        double acc = 0.0;
        if (i < r && g < groups) {
            const double sig = sqrt(lam[i]);
            const float* V = L.V();
            for (int64_t k = g; k < L.K; k += groups) {
                double v = 0.0;
                for (int j = 0; j < W; ++j) v += (double)V[k * W + j] * A[j][i];
                const double e = (double)X[k * W + i] - sig * v;
                acc += e * e;
            }
        }
        red[tid] = acc;
        __syncthreads();
        if (tid == 0) {
            double worst = 0.0;
            for (int ii = 0; ii < r; ++ii) {
                double s = 0.0;
                for (int gg = 0; gg < groups; ++gg) s += red[gg * rc + ii];
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
            if (d != 3) rows_times<W>(L.V(), L.V(), L.K, A, lam);  // V ← V·Ũ, masked directions zero
            __syncthreads();
            if (tid == 0) *L.flag() = d;
            return;
        }
    }

    // Gram matrix in fp64, rows staged through LDS in a fixed order: thread (ta, tb) owns H[ta + 16i][tb + 16j]
    {
        constexpr int NB = W / 16;
        const int ta = tid >> 4, tb = tid & 15;
        double acc[NB][NB];
#pragma unroll
        for (int i = 0; i < NB; ++i)
#pragma unroll
            for (int j = 0; j < NB; ++j) acc[i][j] = 0.0;
        for (int64_t m0 = 0; m0 < M; m0 += kTile) {
            for (int e = tid; e < kTile * W; e += 256) {
                const int rr = e / W, c = e % W;
                St[rr][c] = (m0 + rr < M) ? X[(m0 + rr) * W + c] : 0.f;
            }
            __syncthreads();
            for (int rr = 0; rr < kTile; ++rr) {
                double xa[NB], xb[NB];
#pragma unroll
                for (int i = 0; i < NB; ++i) {
                    xa[i] = St[rr][ta + 16 * i];
                    xb[i] = St[rr][tb + 16 * i];
                }
#pragma unroll
                for (int i = 0; i < NB; ++i)
#pragma unroll
                    for (int j = 0; j < NB; ++j) acc[i][j] += xa[i] * xb[j];
            }
            __syncthreads();
        }
        double bad = 0.0;
#pragma unroll
        for (int i = 0; i < NB; ++i)
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                A[ta + 16 * i][tb + 16 * j] = acc[i][j];
                bad += isfinite(acc[i][j]) ? 0.0 : 1.0;
            }
        bad = block_sum(bad, red);
        if (bad != 0.0) {
            if (tid == 0) *L.flag() = 3;
            return;
        }
    }
    jacobi<W>(A, E, red, cs);

    // λ descending, ties to the lower index: λ_i goes to the position given by the number of entries that precede it
    if (tid < W) {
        lam_d[tid] = A[tid][tid];
        perm[tid] = tid;
        lam_s[tid] = 0.0;
    }
    __syncthreads();
    if (tid < W) {
        const double mine = lam_d[tid];
        int before = 0;
        for (int j = 0; j < W; ++j) before += (lam_d[j] > mine || (lam_d[j] == mine && j < tid)) ? 1 : 0;
        perm[before] = tid;
        lam_s[before] = mine;
    }
    __syncthreads();
    const double lmax = lam_s[0];
    __syncthreads();
    if (tid < W && (!(lmax > 0.0) || !(lam_s[tid] > kMaskEps * lmax))) lam_s[tid] = 0.0;  // mask λ ≤ ε·λ_max
    __syncthreads();
    for (int e = tid; e < W * W; e += 256) {
        const int j = e / W, i = e % W;
        const double u = E[j][perm[i]];
        A[j][i] = lam_s[i] > 0.0 ? u / sqrt(lam_s[i]) : 0.0;
        if (SIDE == 1) L.ut()[e] = u;
    }
    if (SIDE == 1 && tid < W) L.lam()[tid] = lam_s[tid];
    __syncthreads();
    rows_times<W>(X, dst, M, A, nullptr);
}

// Final factors of every layer into out[out_off ..] (finalize_layer of distill_common.h).  W, the row stride of the blocks,
// is a run-time argument: nothing there is sized by it.
__global__ __launch_bounds__(256) void distill_wide_finalize_kernel(const int64_t* table, unsigned char* ws, int r, int W,
                                                                    float q, int clamp, float* out) {
    const int64_t* row = table + 8 * (int64_t)blockIdx.x;
    const int64_t N = row[2], K = row[3];
    unsigned char* lw = ws + row[4];
    int* flag = reinterpret_cast<int*>(lw + kOffFlag);
    if (*flag == 3) return;
    const float* U = reinterpret_cast<const float*>(lw + blocks_offset(W));
    finalize_layer<kMaxRank>(U, U + (N + K) * W, reinterpret_cast<const double*>(lw + kOffLam), flag, N, K, W, r, q, clamp,
                             out + row[5]);
}

template <int W, int SIDE>
int rr_launch(const int64_t* table, int n_layers, int r, double tol, int last, uint64_t seed, unsigned char* ws, hipStream_t s) {
    hipLaunchKernelGGL((distill_wide_rr_kernel<W, SIDE>), dim3(n_layers), dim3(256), 0, s, table, ws, r, tol, last, seed);
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}

template <int SIDE>
int rr_dispatch(const int64_t* table, int n_layers, int r, double tol, int last, uint64_t seed, void* workspace, void* stream) {
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (width_of(r)) {
        case 48: return rr_launch<48, SIDE>(table, n_layers, r, tol, last, seed, ws, s);
        case 64: return rr_launch<64, SIDE>(table, n_layers, r, tol, last, seed, ws, s);
        default: return rr_launch<80, SIDE>(table, n_layers, r, tol, last, seed, ws, s);
    }
}

template <bool TRANS, int W>
int diff_launch(const int64_t* table, int n_layers, int64_t max_rows, int dtype, unsigned char* ws, hipStream_t s) {
    const dim3 grid((unsigned)((max_rows + kTile - 1) / kTile), (unsigned)n_layers);
    switch (dtype) {
        case LORA_F32: hipLaunchKernelGGL((distill_wide_diff_kernel<float, TRANS, W>), grid, dim3(256), 0, s, table, ws); break;
        case LORA_F16: hipLaunchKernelGGL((distill_wide_diff_kernel<half_t, TRANS, W>), grid, dim3(256), 0, s, table, ws); break;
        case LORA_BF16: hipLaunchKernelGGL((distill_wide_diff_kernel<bf16_t, TRANS, W>), grid, dim3(256), 0, s, table, ws); break;
        default: return LORA_E_BADARG;
    }
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}

template <bool TRANS>
int diff_dispatch(const int64_t* table, int n_layers, int64_t max_rows, int dtype, int r, unsigned char* ws, hipStream_t s) {
    switch (width_of(r)) {
        case 48: return diff_launch<TRANS, 48>(table, n_layers, max_rows, dtype, ws, s);
        case 64: return diff_launch<TRANS, 64>(table, n_layers, max_rows, dtype, ws, s);
        default: return diff_launch<TRANS, 80>(table, n_layers, max_rows, dtype, ws, s);
    }
}

// r < 1 is a rank error, r > 64 unsupported; 0 when the wide kernels take r
int rank_status(int r) { return r < 1 ? LORA_E_RANK : (r > kMaxRank ? LORA_E_UNSUPPORTED : LORA_OK); }

}  // namespace

extern "C" int lora_distill_wide_width(int r) { return rank_status(r) != LORA_OK ? rank_status(r) : width_of(r); }

extern "C" int64_t lora_distill_wide_workspace_bytes(int64_t N, int64_t K, int r) {
    if (N < 1 || K < 1 || rank_status(r) != LORA_OK) return 0;
    const int W = width_of(r);
    const int64_t b = blocks_offset(W) + (N + 2 * K) * W * 4;
    return (b + 255) / 256 * 256;
}

extern "C" int lora_distill_wide_start(const int64_t* table, int n_layers, int64_t min_nk, int r, int64_t seed,
                                       void* workspace, void* stream) {
    if (!table || !workspace || n_layers < 1 || min_nk < 1) return LORA_E_BADARG;
    if (rank_status(r) != LORA_OK) return rank_status(r);  // r < 1: rank error; r > 64: unsupported, whatever min_nk
    if (r > min_nk) return LORA_E_RANK;
    return rr_dispatch<0>(table, n_layers, r, 0.0, 0, (uint64_t)seed, workspace, stream);
}

extern "C" int lora_distill_wide_diff(const int64_t* table, int n_layers, int64_t max_rows, int transpose, int dtype, int r,
                                      void* workspace, void* stream) {
    if (!table || !workspace || n_layers < 1 || n_layers > 65535 || max_rows < 1) return LORA_E_BADARG;
    if (dtype != LORA_F32 && dtype != LORA_F16 && dtype != LORA_BF16) return LORA_E_BADARG;
    if (rank_status(r) != LORA_OK) return rank_status(r);
    unsigned char* ws = static_cast<unsigned char*>(workspace);
    hipStream_t s = static_cast<hipStream_t>(stream);
    return transpose ? diff_dispatch<true>(table, n_layers, max_rows, dtype, r, ws, s)
                     : diff_dispatch<false>(table, n_layers, max_rows, dtype, r, ws, s);
}

extern "C" int lora_distill_wide_rayleigh_ritz(const int64_t* table, int n_layers, int side, int r, double tol, int last,
                                               void* workspace, void* stream) {
    if (!table || !workspace || n_layers < 1 || (side != 1 && side != 2)) return LORA_E_BADARG;
    if (rank_status(r) != LORA_OK) return rank_status(r);
    return side == 1 ? rr_dispatch<1>(table, n_layers, r, tol, last, 0ull, workspace, stream)
                     : rr_dispatch<2>(table, n_layers, r, tol, last, 0ull, workspace, stream);
}

extern "C" int lora_distill_wide_finalize(const int64_t* table, int n_layers, int r, float q, int clamp, void* workspace,
                                          float* out, void* stream) {
    if (!table || !workspace || !out || n_layers < 1) return LORA_E_BADARG;
    if (clamp && !(q >= 0.f && q <= 1.f)) return LORA_E_BADARG;
    if (rank_status(r) != LORA_OK) return rank_status(r);
    hipLaunchKernelGGL(distill_wide_finalize_kernel, dim3(n_layers), dim3(256), 0, static_cast<hipStream_t>(stream), table,
                       static_cast<unsigned char*>(workspace), r, width_of(r), q, clamp, out);
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}

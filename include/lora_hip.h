/*
 * lora_hip.h — C-ABI of liblora_hip.so, the gfx950 (MI355X) implementation of the
 * LoRA fine-tuning hot path of levayz/diffusion_finetuning (`lora_diffusion`).
 *
 * The reference has no native code: every entry point below replaces a group of
 * stock-PyTorch calls made by the reference's Python.  Each declaration cites the
 * reference lines it stands in for (paths relative to the reference repo root).
 *
 * Conventions (all entry points)
 *   - plain C: raw DEVICE pointers, sizes, a `void* stream` (hipStream_t; NULL = null stream).
 *   - row-major, densely packed tensors unless a leading dimension is given.
 *   - nothing is allocated, retained or freed by the library; kernels are enqueued on
 *     `stream` and the call returns without synchronising.  Re-entrant, no mutable globals
 *     (the optional launch profiler below is the one exception and is off by default).
 *   - return value: LORA_OK (0) or a negative LORA_E_* code; never throws, never aborts.
 *   - `dtype` selects the storage/compute type of the big operands (X, W, Y, dY, dX, pred ...):
 *     LORA_F32 / LORA_F16 / LORA_BF16.  Accumulation is always fp32.  The rank-r factors,
 *     their gradients and the saved rank-r activations are ALWAYS fp32 ("master" precision).
 *
 * Notation: X[M,K] input rows, W[N,K] frozen base weight, b[N] bias, A[r,K] = lora_down.weight,
 * B[N,r] = lora_up.weight, s = LoraInjectedLinear.scale, T[M,r] = X·Aᵀ.
 */
#ifndef LORA_HIP_H
#define LORA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LORA_HIP_ABI_VERSION 9

enum lora_dtype { LORA_F32 = 0, LORA_F16 = 1, LORA_BF16 = 2 };

enum lora_status {
    LORA_OK = 0,
    LORA_E_BADARG = -1,      /* null pointer / non-positive size / unknown dtype            */
    LORA_E_RANK = -2,        /* r < 1 or r > min(K,N)  (reference: ValueError, lora.py:36-39) */
    LORA_E_ALIGN = -3,       /* pointer not 16-byte aligned where the kernel needs it        */
    LORA_E_LAUNCH = -4,      /* hipLaunch / hipGetLastError reported a failure               */
    LORA_E_UNSUPPORTED = -5  /* combination not implemented                                  */
};

/* ABI version of the loaded library (== LORA_HIP_ABI_VERSION it was built with). */
int lora_version(void);

/* Static, human-readable text for a lora_status code. */
const char* lora_status_string(int status);

/*
 * Packed rank-r factors: the compute-dtype copies of lora_down / lora_up the fused kernels stream, rank padded
 * to 16 with zeros, BOTH orientations per factor so that each is a plain row-major operand tile:
 *     Apack (32·K elements) = [ A16 [16,K] : A16[j,k]  = A[j,k] | At16[K,16] : At16[k,j] = A[j,k] ]
 *     Bpack (32·N elements) = [ Bt16[16,N] : Bt16[j,n] = B[n,j] | B16 [N,16] : B16[n,j]  = B[n,j] ]
 * The [16,len] halves are the main-loop factors (forward T = X·Aᵀ uses A16, backward U = dY·B uses Bt16), the
 * [len,16] halves the epilogue factors (forward B16, backward At16).  This is the same cast of
 * lora_down / lora_up to the compute dtype that autocast applies on lora.py:50 in the reference.  Re-pack
 * whenever A or B changed (once per optimizer step).  The batched form packs every layer of a flat parameter
 * slab in ONE launch: table[l] = {a_off, b_off, K, N, r, apack_off, bpack_off, 0} (int64, device memory;
 * element offsets into `params` resp. `packed`), max_len = max over layers of max(K,N).
 * For r > 16 nothing is packed (those ranks run on the shape-agnostic kernels that read the fp32 masters).
 */
int lora_pack_factors(const float* A, const float* B, void* Apack, void* Bpack, int K, int N, int r,
                      int dtype, void* stream);
int lora_pack_factors_batched(const int64_t* table, int n_layers, int max_len, const float* params,
                              void* packed, int dtype, void* stream);

/* Packing with explicit destinations, one table row per FACTOR (grouped layers place several layers' factors in one
 * operand): table[i] = {src_off, which (0: A [r,len], 1: B [len,r]), len, r, d16_off, d16_ld, dT_off, rows} (int64,
 * device).  Rows j < rows of the [16,len] form go to packed[d16_off + j·d16_ld + c], columns j < rows of the [len,16]
 * form to packed[dT_off + c·16 + j]; an offset of -1 skips a form; rows = 16 zero-fills unused rank slots, rows = r
 * leaves them alone (block-diagonal groups write only their own slots of a buffer zeroed once). */
int lora_pack_items(const int64_t* table, int n_items, int max_len, const float* params, void* packed, int dtype,
                    void* stream);

/*
 * Forward of LoraInjectedLinear.forward — lora_diffusion/lora.py:49-50
 *     Y = X·Wᵀ + b + s·((X·Aᵀ)·Bᵀ)
 * replaces F.linear ×3 + mul + add (5 launches + the [M,N] LoRA temporary) with one kernel.
 * A, B: fp32 masters; Apack, Bpack: their packed forms (both nullable → shape-agnostic slow path).
 * T_out receives T = X·Aᵀ [M,r] fp32 for the backward.
 */
int lora_linear_fwd(const void* X, const void* W, const void* bias /* nullable */,
                    const float* A, const float* B, const void* Apack, const void* Bpack, void* Y,
                    float* T_out, int64_t M, int K, int N, int r, float scale, int dtype,
                    void* stream);
/* The same with optional split-K scratch (see lora_linear_bwd_input_ws / lora_gemm_workspace_bytes(M, K, N, dtype)):
 * the 1280-wide projections at 1024 and 256 rows leave a third of the chip idle unless their contraction is cut. */
int lora_linear_fwd_ws(const void* X, const void* W, const void* bias /* nullable */,
                       const float* A, const float* B, const void* Apack, const void* Bpack, void* Y,
                       float* T_out, int64_t M, int K, int N, int r, float scale, int dtype,
                       void* workspace /* nullable */, int64_t ws_bytes, void* stream);

/*
 * The same forward with the GEGLU gate of its caller folded into the epilogue — diffusers GEGLU.forward
 *     hidden, gate = proj(x).chunk(2, dim=-1);  return hidden * gelu(gate)
 * where `proj` is a LoraInjectedLinear (target class "GEGLU", lora_diffusion/lora.py:53):
 *     Y = X·Wᵀ + b + s·((X·Aᵀ)·Bᵀ)  [M,N],   Out = Y[:, :N/2] · gelu(Y[:, N/2:])  [M,N/2]   (exact gelu, fp32 math on the
 *     values of Y rounded to `dtype`, exactly what geglu_gate_fwd computes from a stored Y)
 * in ONE launch: a column tile owns 64 hidden columns and the 64 gate columns behind them.  Y may be NULL (inference /
 * the no-grad pass of gradient checkpointing): then the [M,N] activation is never written.  16-bit dtypes, packed factors,
 * K % 64 == 0 and N % 128 == 0 only — anything else returns LORA_E_UNSUPPORTED and the caller runs lora_linear_fwd followed
 * by geglu_gate_fwd.
 */
int lora_linear_geglu_fwd(const void* X, const void* W, const void* bias /* nullable */, const void* Apack,
                          const void* Bpack, void* Y /* nullable */, void* Out, float* T_out, int64_t M, int K, int N,
                          int r, float scale, int dtype, void* stream);

/*
 * The two forwards above with a PER-SAMPLE, PER-RANK-SLOT factor in front of the rank-r term (inference only: there is no
 * backward form):
 *     Y[m,:] = X[m,:]·Wᵀ + b + Σ_j (s · G[m / rps, j]) · T[m,j] · B[:,j] ,   T = X·Aᵀ ,   rps = M / n_samples
 * row_scale = G: fp32 [n_samples, ld_scale] in device memory, columns [0, r) are read; a sample is rps consecutive rows of
 * X.  The factor is formed in fp32 as (s·G) first and then multiplied into T wherever a kernel builds s·T per row (every MFMA
 * form); the shape-agnostic kernels, whose ungated form scales the sum, compute the same arithmetic at slot 0's factor plus the
 * other slots' deviations from it — so on EVERY path a table filled with g at scale 1, or a table of ones at scale g, gives bit
 * for bit what lora_linear_fwd_ws gives at scale g, and a row of zeros what it gives at scale 0.  T_out receives T un-gated and unscaled, as above.  One launch then serves what the reference
 * does one sample at a time:
 *   - G[b, :] = s_b: `tune_lora_scale(unet, s_b)` (lora.py:597-600 setting `scale` of lora.py:49-50) per sample of a batch —
 *     the 0.0 / 0.7 / 1.0 sweeps at equal seed;
 *   - K checkpoints of rank r_k stacked along the rank (A = [A_0; A_1; …], B = [B_0 | B_1 | …], Σ r_k slots) with G[b, :]
 *     open on the slots of checkpoint k_b only: `visualize_progress` (utils.py:191-211: patch_pipe, tune_lora_scale, one
 *     sample per checkpoint) as one batch.  Σ r_k <= 16 rides on the same single extra MFMA K-step as one checkpoint.
 * LORA_E_BADARG for n_samples < 1, M % n_samples != 0, ld_scale < r or a null table (nothing is launched or written);
 * everything else as the entry it mirrors, lora_linear_geglu_fwd_rows including the LORA_E_UNSUPPORTED envelope.
 */
int lora_linear_fwd_rows(const void* X, const void* W, const void* bias /* nullable */, const float* A, const float* B,
                         const void* Apack, const void* Bpack, void* Y, float* T_out, int64_t M, int K, int N, int r,
                         float scale, const float* row_scale, int n_samples, int ld_scale, int dtype,
                         void* workspace /* nullable */, int64_t ws_bytes, void* stream);
int lora_linear_geglu_fwd_rows(const void* X, const void* W, const void* bias /* nullable */, const void* Apack,
                               const void* Bpack, void* Y /* nullable */, void* Out, float* T_out, int64_t M, int K, int N,
                               int r, float scale, const float* row_scale, int n_samples, int ld_scale, int dtype,
                               void* stream);

/*
 * Backward of the same gate, in the epilogue of the GEMM that produces its incoming gradient.  In a transformer block the
 * gated activation feeds a frozen linear layer (diffusers FeedForward: net = [GEGLU, Dropout, Linear]); autograd of
 *     z = (hidden * gelu(gate)) @ W2ᵀ + b2 ,   [hidden | gate] = Y = proj(x)      (proj: the LoraInjectedLinear above)
 * needs  dout = dZ·W2  [M,F]  and then  dY[:, :F] = dout·gelu(gate),  dY[:, F:] = dout·hidden·gelu'(gate).
 * geglu_linear_bwd does both in ONE launch: dout never goes to memory (it is rounded to `dtype` in the tile, exactly as the
 * separate tensor would be) and dY [M,2F] is what lora_linear_bwd_input / lora_grad_batched of `proj` consume.
 * W2t = W2ᵀ [F, Nz] row-major in `dtype` (lora_cast_matrix, transpose); zeros: at least 32·max(Nz, F) zero bytes (the launch
 * has no rank-r term).  16-bit dtypes, Nz % 64 == 0, F % 128 == 0; otherwise LORA_E_UNSUPPORTED (caller: a GEMM of its own
 * followed by geglu_gate_bwd).
 */
int geglu_linear_bwd(const void* dZ, const void* W2t, const void* Y, void* dY, const void* zeros, int64_t M, int Nz,
                     int F, int dtype, void* stream);

/*
 * Backward w.r.t. the input — autograd of lora.py:49-50 as driven by
 * training_scripts/train_lora_dreambooth.py:877 (accelerator.backward), base W frozen (:595):
 *     U  = dY·B                         [M,r]  (written to U_out, fp32, unscaled)
 *     dX = dY·W + s·U·A                 [M,K]  (skipped when dX == NULL: attn2 to_k/to_v with a
 *                                               frozen text encoder need no input gradient)
 * Wt is the frozen weight stored TRANSPOSED, Wt[K,N] = Wᵀ, so that the contraction index n is
 * contiguous for both operands (the caller caches Wt once per frozen layer).  Apack, Bpack as above.
 */
int lora_linear_bwd_input(const void* dY, const void* Wt, const float* A, const float* B,
                          const void* Apack, const void* Bpack, void* dX /* nullable */, float* U_out,
                          int64_t M, int K, int N, int r, float scale, int dtype, void* stream);
/*
 * The same with caller-provided scratch for split-K: a contraction on a grid too small for the chip (the GEGLU `proj`
 * backward: dX[1024,1280] = dY[1024,10240]·W — 80 output tiles, 160 K-steps; the 1280-wide projections at 1024 and 256
 * rows) is cut into K-slices inside ONE launch: a slice stores its fp32 partial tile, takes a ticket of the tile, and the
 * workgroup that draws the last ticket adds the slices in index order (deterministic whoever arrives last) and runs the
 * usual epilogue (rank-r term, bias, store).
 * lora_gemm_workspace_bytes(M, Kc, Nc, dtype) says how much scratch the contraction [M,Kc]·[Nc,Kc]ᵀ wants (0: the
 * library would not split it).  Layout: the first LORA_GEMM_WS_TICKET_BYTES bytes are the tiles' tickets — they must be
 * ZERO when the call is made and are zero again when its launch has finished (so one buffer, zeroed once, serves every
 * later call on the same stream) — the rest is uninitialised scratch.  16-byte aligned; used only by the call's launch
 * (stream-ordered); two launches that may run concurrently need a workspace each.
 */
#define LORA_GEMM_WS_TICKET_BYTES 4096
int64_t lora_gemm_workspace_bytes(int64_t M, int Kc, int Nc, int dtype);
int lora_linear_bwd_input_ws(const void* dY, const void* Wt, const float* A, const float* B,
                             const void* Apack, const void* Bpack, void* dX /* nullable */, float* U_out,
                             int64_t M, int K, int N, int r, float scale, int dtype, void* workspace,
                             int64_t ws_bytes, void* stream);

/*
 * The fused kernel's own contract, for callers that hold PACKED factors only — grouped layers that share an input:
 *     C[M,Nc] = Am·Bmᵀ + bias + s·P·Qᵀ ,   P[M,r] = Am·Fᵀ                       (P stored unscaled, fp32)
 * Am [M,Kc] with row stride lda (elements; 0 = Kc), Bm [Nc,Kc], Fp [16,Kc] and Qp [Nc,16] in `dtype` with the
 * unused rank rows / columns zero.  C == NULL computes P only (backward of a layer whose input needs no gradient).
 * Uses in the product (lora_diffusion/lora.py:49-50 and its autograd, several LoraInjectedLinear at once):
 *   - attn1 to_q/to_k/to_v, one launch each way: Bm = [Wq;Wk;Wv] (forward) or its transpose (backward), rank 3r with
 *     block-diagonal factors — X is read once instead of three times, dX needs no accumulation;
 *   - the attn2 to_k/to_v of ALL transformer blocks, which multiply the same encoder_hidden_states: forward as one
 *     launch over the concatenated weights with per-part factors (tile_part[column tile of 64] = part | first<<16,
 *     Fp = [n_parts·16, Kc], P_out = [n_parts][M][r]); backward (no dX: the text encoder output is frozen) as one
 *     P-only launch with part_table[g] = {column offset into Am, contraction length, offset into Fp, offset into P_out}.
 * work_cols: Σ contraction lengths of a part_table launch (profiler accounting only; 0 = Kc).
 * workspace / ws_bytes: optional split-K scratch (lora_gemm_workspace_bytes; NULL / 0 = never split).
 * Returns LORA_E_UNSUPPORTED when the operands are not 16-byte aligned / not a multiple of one K-step (grouping is
 * then simply not used by the caller).
 */
int lora_gemm_packed(const void* Am, int64_t lda, const void* Bm /* nullable with C */, const void* bias /* nullable */,
                     const void* Fp, const void* Qp, const int* tile_part /* nullable, device */,
                     const int64_t* part_table /* nullable, device */, int n_parts, void* C /* nullable */,
                     float* P_out, int64_t M, int Kc, int Nc, int r, float scale, int64_t work_cols,
                     void* workspace /* nullable */, int64_t ws_bytes, int dtype, void* stream);

/*
 * The same contract for n_parts (2..4) LoraInjectedLinear layers of EQUAL shape that share an input, at any rank r <= 16 —
 * attn1 to_q/to_k/to_v (and CLIPAttention q_proj/k_proj/v_proj) when 3r no longer fits one 16-slot factor, i.e. the ranks of
 * BASELINE configs 3 (r = 8, train_lora_dreambooth.py:596-613) and 5 (r = 16, cli_lora_pti.py:693): three
 * lora_diffusion/lora.py:49-50 forwards, or their three backward-input products summed, in ONE launch.  f16 / bf16.
 *   parts_on_k == 0 (forward):  C[M,Nc] = Am·Bmᵀ + bias + s·P_g·Q_gᵀ on column run g = [g·Nc/n, (g+1)·Nc/n),
 *       Am = X [M,Kc], Bm = [W_0; …] [Nc,Kc], Fp = [n_parts][16,Kc] (part g: rows j < r = A_g), Qp = [Nc,16] (row of part
 *       g: columns j < r = B_g); P_out[m, g·r + j] = (X·A_gᵀ)[m, j], row stride ldp floats (>= n_parts·r).
 *   parts_on_k == 1 (backward-input, n_parts == 3):  C[M,Nc] = Am·Bmᵀ + s·Σ_g P_g·Q_gᵀ with the CONTRACTION cut into runs,
 *       Am = [dY_0 | …] [M,Kc], Bm = [W_0; …]ᵀ [Nc,Kc], Fp = [16,Kc] (column run g, rows j < r = B_gᵀ), Qp = [n_parts][Nc,16]
 *       (part g: columns j < r = A_gᵀ); P_out[m, g·r + j] = (dY_g·B_g)[m, j].  No accumulation of three dX tensors.
 * Unused rank rows / columns of Fp / Qp are zero.  LORA_E_UNSUPPORTED: f32, part width or Kc not a multiple of 64, operands
 * not 16-byte aligned, parts_on_k with n_parts != 3 (the caller then runs the layers one by one).
 */
int lora_gemm_parts(const void* Am, const void* Bm, const void* bias /* nullable */, const void* Fp, const void* Qp,
                    void* C, float* P_out, int64_t ldp, int64_t M, int Kc, int Nc, int r, int n_parts, int parts_on_k,
                    float scale, int dtype, void* stream);

/*
 * Backward w.r.t. the LoRA factors (no grad for W or b: lora.py:179-180 set requires_grad only on
 * lora_up / lora_down; train_lora_dreambooth.py:595 freezes the rest):
 *     gB = s·dYᵀ·T      [N,r]
 *     gA = s·Uᵀ·X       [r,K]
 * The M rows are cut into `n_blocks` row blocks; block b STORES its partial sums at
 * gA_part + b·part_stride and gB_part + b·part_stride (fp32; every block is written, zeros included).
 * No global atomics: the outputs are a few KB wide and hundreds of workgroups adding onto so few cache
 * lines serialise at the memory side.  lora_reduce_partials then sums the blocks in index order
 * (deterministic): grads[i] (+)= Σ_b partials[b·part_stride + i] for i < n.  A trainer lays the partials
 * of all layers out as [n_blocks][slab] and reduces the whole slab — the RCCL all-reduce buffer — in
 * one launch per step.
 */
int lora_linear_bwd_params(const void* dY, const void* X, const float* T, const float* U,
                           float* gA_part, float* gB_part, int64_t part_stride, int n_blocks,
                           int64_t M, int K, int N, int r, float scale, int dtype, void* stream);
int lora_reduce_partials(const float* partials, int64_t part_stride, int n_blocks, float* grads,
                         int64_t n, int accumulate, void* stream);

/*
 * The same two reductions for MANY layers at once — what a training step calls once, after backward, with all
 * 2×144 problems of an SD1.5 UNet (MI355X-first: 288 GB of HBM keep every layer's dY and X alive until then, and a
 * few chip-filling launches replace 144 latency-bound ones).  One problem is  G[c,j] = s·Σ_m S[m,c]·P[m,j]:
 *     S  : streamed operand [M, C] (dtype), row stride s_stride elements — dY for gB, X for gA; may be a strided
 *          slice of a wider buffer (grouped projections);
 *     P  : [M, r] fp32, row stride p_stride floats — T for gB, U for gA;
 *     out: partial output of row block 0; rank columns j are split into groups of `rg`
 *          (out[j / rg], local column j % rg): one group normally (rg = r); a grouped q/k/v layer hands U as
 *          [M, 3r] and receives three gA outputs;  out_kn = 1 → out[g] is [rg, C] (gA), 0 → [C, rg] (gB);
 *     row block b of the problem stores at out[g] + b·part_stride; n_blocks = 0 lets the library choose
 *          (lora_grad_row_blocks(M), at most LORA_GRAD_MAX_BLOCKS) — the caller folds that many.
 * `problems` is HOST memory and is consumed during the call (the tables travel as kernel arguments, ≤ 28 problems
 * per launch; nothing is uploaded, so the call may be recorded into a hipGraph).  lora_fold_partials then sums the
 * row blocks of a table of slab ranges, each with its own block count:
 *     grads[off+i] (+)= Σ_{b < blocks} partials[b·part_stride + off + i],  ranges[k] = {off, len, blocks, 0}
 * (int64, DEVICE memory), max_len = the largest len.  Deterministic like lora_reduce_partials.
 * Arithmetic: fp32 sums.  16-bit operands are multiplied on the matrix cores with the row index as the contraction; P
 * enters as an exact hi + lo pair of 16-bit values (fp16: 22 significant bits of P, bf16: 16).  fp32 operands: VALU FMAs.
 */
#define LORA_GRAD_MAX_BLOCKS 64
typedef struct lora_grad_problem {
    const void* S;
    const float* P;
    float* out[4];
    int64_t s_stride, p_stride, part_stride, M;
    int C, r, rg, out_kn, n_blocks;
    float scale;
} lora_grad_problem;
int lora_grad_row_blocks(int64_t M);
int lora_grad_batched(const lora_grad_problem* problems, int n, int dtype, void* stream);
/*
 * The same problems in ONE launch (16-bit operands, ranks <= 16): lora_grad_batched's launches of <= 28 problems each end on a
 * tail, and the last few of a step hold a few dozen workgroups.  Here the table is a PLAN in device memory:
 *     lora_grad_plan_bytes(problems, n)  upper bound of the plan's size in bytes;
 *     lora_grad_plan(...)                writes the plan — [items: 128 bytes per problem | one int per workgroup] — into HOST
 *                                        memory `plan_host` and returns the counts; the first
 *                                        n_items·128 + n_blocks·4 bytes are what the device needs.  LORA_E_UNSUPPORTED (fp32
 *                                        operands, an unaligned operand, a rank above 16): use lora_grad_batched;
 *     lora_grad_planned(plan_dev, ...)   launches on a DEVICE copy of those bytes.  The caller makes that copy with its own
 *                                        stream-ordered transfer (inside a recording it is a memcpy node whose host source the
 *                                        caller keeps alive and unchanged for as long as the recording is replayed) — the
 *                                        library still allocates and retains nothing.  bytes / flops: what lora_prof_* charge.
 * Same arithmetic, same row-block partial layout, same fold as lora_grad_batched: bit-identical results.
 */
int64_t lora_grad_plan_bytes(const lora_grad_problem* problems, int n);
int lora_grad_plan(const lora_grad_problem* problems, int n, int dtype, void* plan_host, int64_t plan_bytes, int* n_items,
                   int* n_blocks);
int lora_grad_planned(const void* plan_dev, int n_items, int n_blocks, int dtype, double bytes, double flops, void* stream);
int lora_fold_partials(const int64_t* ranges, int n_ranges, int64_t max_len, const float* partials,
                       int64_t part_stride, float* grads, int accumulate, void* stream);

/*
 * DDPM noise-prediction loss, forward + gradient in one pass —
 * training_scripts/train_lora_dreambooth.py:855-875 and lora_diffusion/cli_lora_pti.py:222-247.
 *   rows [0, n_inst)            instance part : mean_b(mean_chw((p-t)²))
 *   rows [n_inst, n_inst+n_prior) prior part  : prior_weight · mean((p-t)²)     (n_prior may be 0)
 *   mask (nullable, fp32 [rows, 1, H, W] broadcast over `channels`, already normalised by
 *   lora_mask_prepare): p and t are multiplied by it first (cli_lora_pti.py:243-247).
 * loss_out[0] = loss (fp32).  dpred (nullable, same dtype as pred) = grad_scale · dloss/dpred.
 * workspace: at least lora_mse_workspace_bytes() bytes, 16-byte aligned; the call zeroes what it uses.
 */
int ddpm_mse_fwd_bwd(const void* pred, const void* target, const float* mask /* nullable */,
                     int n_inst, int n_prior, int64_t per_row /* C·H·W */, int64_t hw /* H·W */,
                     float prior_weight, float grad_scale, float* loss_out, void* dpred /* nullable */,
                     void* workspace, int dtype, void* stream);
int64_t lora_mse_workspace_bytes(void);

/*
 * The same loss with one weight per row, looked up on the device by the row's timestep: w_b = weights[t[b]].
 *   instance part : (1/n_inst) Σ_b w_b · mean_chw((m·p − m·t)²)
 *   prior part    : prior_weight · (1/n_prior) Σ_b w_b · mean_chw((m·p − m·t)²)       each row by its own timestep
 * and dpred follows from them.  The table is the caller's: Min-SNR-γ weighting — T. Hang et al., "Efficient Diffusion
 * Training via Min-SNR Weighting Strategy", ICCV 2023: min(SNR(t), γ)/SNR(t) for ε-prediction, min(SNR(t), γ)/(SNR(t) + 1)
 * for v-prediction (`--snr_gamma` of the diffusers and kohya trainers; Python: step.min_snr_weights) — or any other.  An
 * extension beyond the reference, whose objective is the plain mean; it lives here because the timesteps of a replayed step
 * exist on the device only.  t int64 [n_inst + n_prior] and weights fp32 [n_weights], both device memory.
 * The weight is folded into the row's coefficient (coef·w_b, read once per 16-byte chunk); everything else is
 * ddpm_mse_fwd_bwd's arithmetic, fold, workspace and capturability: with a table of ones loss and dpred are bit-identical to
 * its.  A t[b] outside [0, n_weights) is never used as an index: that row's weight is NaN (so are the loss and the row's
 * dpred; the other rows' dpred is unaffected), the convention for token ids outside the embedding table.
 */
int ddpm_mse_weighted_fwd_bwd(const void* pred, const void* target, const float* mask /* nullable */, const int64_t* t,
                              const float* weights, int n_weights, int n_inst, int n_prior, int64_t per_row /* C·H·W */,
                              int64_t hw /* H·W */, float prior_weight, float grad_scale, float* loss_out,
                              void* dpred /* nullable */, void* workspace, int dtype, void* stream);

/*
 * Mask preparation of cli_lora_pti.py:222-241:
 *   out = nearest_resize(mask[B,1,Hin,Win] -> [B,1,H,W]) + 0.05 ;  out /= mean(out)
 * mask_in / mask_out fp32.  Single launch, deterministic.
 */
int lora_mask_prepare(const float* mask_in, float* mask_out, int B, int Hin, int Win, int H, int W,
                      void* stream);

/*
 * weight_apply_lora — lora_diffusion/lora.py:410-424:   W ← W + α·(B @ A).type(W.dtype)
 * In place on W[N,K] (dtype); A[r,K], B[N,r] passed as fp32.  The reference forms B @ A in the dtype the
 * factors are held in (fp16 when they come from a `.pt` file): `factor_dtype` names it, and the product
 * is rounded to it before the cast to W's dtype, the multiply by α and the add — op-by-op as the reference.
 */
int lora_merge_weight(void* W, const float* A, const float* B, int K, int N, int r, float alpha,
                      int dtype, int factor_dtype, void* stream);

/* The same merge for every layer of a model in ONE launch (cli_lora_add.py:72-88 `upl`: 192.6 M base weights of an
 * SD1.5 UNet, one HBM pass).  table: device memory, int64 [n_layers][8] =
 * {W ptr, A ptr (fp32 [r,K]), B ptr (fp32 [N,r]), K, N, r, dtype of W, factor_dtype}; max_elems = max N·K. */
int lora_merge_weight_batched(const int64_t* table, int n_layers, int64_t max_elems, float alpha, void* stream);

/*
 * LoRA (+) LoRA interpolation — lora_diffusion/cli_lora_add.py:52-55 (mode `lpl`), op by op in the tensors' dtype:
 *     x1 ← T( T(a·x1) + T(b·x2) )        with a = alpha, b = 1 − alpha
 * over n elements (the caller concatenates a whole `[up0, down0, …]` list into one buffer).
 */
int lora_lerp(void* x1, const void* x2, int64_t n, float a, float b, int dtype, void* stream);

/* Out-of-place transpose+cast helper used to build the cached operands:
 * dst[cols,rows] (dst_dtype) = src[rows,cols] (src_dtype)ᵀ ; transpose=0 gives a plain cast. */
int lora_cast_matrix(const void* src, void* dst, int64_t rows, int64_t cols, int src_dtype,
                     int dst_dtype, int transpose, void* stream);

/*
 * Fused clip_grad_norm_ + AdamW over the flat LoRA slab —
 * training_scripts/train_lora_dreambooth.py:878-888 (clip_grad_norm_(…, max_grad_norm); optimizer.step())
 * and lora_diffusion/cli_lora_pti.py:448-451.
 *   lora_grad_sqnorm : norm_out (4 floats, device; zero it once before the first step):
 *                      [0] = Σ (grad_mul·g)² over n elements (deterministic two-level sum),
 *                      [1] = 1.0f if any element is non-finite else 0.0f,
 *                      [2] += 1 when [1] == 0: the number of APPLIED optimizer steps including this one,
 *                      [3] += 1 when [1] != 0: the number of skipped steps.
 *   lora_adamw_step  : g' = grad_mul·g·min(1, max_norm/(sqrt(norm_in[0])+1e-6))   (max_norm<=0: no clip)
 *                      torch.optim.AdamW update (decoupled weight decay, bias correction with `step`, or with
 *                      the device counter norm_in[2] when step == 0), skipped entirely when norm_in[1] != 0 —
 *                      torch.cuda.amp.GradScaler semantics: an overflowed step neither moves the parameters nor
 *                      advances the optimizer's step count.
 * `grad_mul` carries 1/world_size (mean all-reduce) and 1/loss_scale.
 */
int lora_grad_sqnorm(const float* grad, int64_t n, float grad_mul, float* norm_out, void* workspace,
                     void* stream);
int64_t lora_sqnorm_workspace_bytes(void);
int lora_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                    const float* norm_in /* nullable: no clip, no skip */, float grad_mul, float max_norm,
                    float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                    void* stream);

/*
 * Exponential moving average (EMA) of the trained parameters, kept inside the optimizer launch.  These two entries replace no
 * line of the reference, which keeps no average: the rule is restated from its published definition ("EMA of
 * parameters").
 *   lora_adamw_ema_step : lora_adamw_step — same arithmetic, same bits in param / exp_avg / exp_avg_sq — and, in the same launch,
 *                         on the parameter value p' just computed:   shadow ← shadow − omd·(shadow − p')   op by op in fp32, with
 *                             t = norm_in[2] (applied steps, this one included), n = max(0, t − ema_update_after − 1),
 *                             d = 0 if n <= 0 else min(ema_max_decay, (1 + n)/(10 + n)) in double, omd = (float)(1 − d).
 *                         `norm_in` is required: the average always follows the device counter, whatever `step` gives the bias
 *                         corrections.  norm_in[1] != 0 (overflow): nothing is written, the shadow included.
 *                         LORA_E_BADARG: a null pointer, n < 1, step < 0, ema_max_decay outside [0, 1], ema_update_after < 0.
 *   lora_slab_swap      : exchanges the fp32 buffers a and b (n elements each, any 4-byte alignment) in place, one launch.
 *                         LORA_E_BADARG, and no launch, when a == b or the two ranges overlap.
 */
int lora_adamw_ema_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* shadow, int64_t n,
                        const float* norm_in, float grad_mul, float max_norm, float lr, float beta1, float beta2, float eps,
                        float weight_decay, int step, float ema_max_decay, int ema_update_after, void* stream);
int lora_slab_swap(float* a, float* b, int64_t n, void* stream);

/*
 * Prodigy (Mishchenko & Defazio, arXiv:2306.06101) over the flat slab: AdamW whose step size is d·lr, with d an on-line estimate
 * of the distance to the solution kept in DEVICE memory.  These entries replace no line of the reference, which has no such
 * optimizer: the rule is restated from its published definition ("Prodigy"; parity with the prodigyopt package is
 * unpinned).  One step = lora_grad_sqnorm, lora_prodigy_moments, lora_prodigy_apply on one stream.
 *   scalars (8 floats, device): [0] d  [1] d_max  [2] numerator  [3] d_prev  [4] d_hat  [5] denom  [6] [7] unused; the caller
 *                      sets [0] = [1] = d0 and the rest to 0 once before the first step.
 *   ranges           : n_ranges (1..4) contiguous ranges of the n elements, range j = [range_end[j-1], range_end[j]) with
 *                      range_end[-1] = 0 and range_end[n_ranges-1] = n, each with γ_j = lr[j] (the group's lr times the schedule
 *                      factor) and weight_decay[j].  HOST arrays, read during the call and passed to the launch by value.
 *   lora_prodigy_moments : with g = grad_mul·grad·clip as lora_adamw_step forms it, t = norm_in[2], bc = sqrt(1−β2^t)/(1−β1^t)
 *                      (in double; 1 unless use_bias_correction), dlr_j = d·γ_j·bc, on every element i of range j
 *                          num_i = (d/d0)·dlr_j·g_i·(param0_i − param_i)
 *                          m_i = β1·m_i + d·(1−β1)·g_i ;  v_i = β2·v_i + d²·(1−β2)·g_i²
 *                          s_i = β3·s_i + (d/d0)·(d if safeguard_warmup else dlr_j)·g_i ;  den_i = |s_i| (the new s)
 *                      then once, in double, in the block that finishes last (fp32 block partials, summed in a fixed order: the
 *                      same bits on every run):  denom = Σ den_i ;  unless denom == 0: numerator = β3·numerator + Σ num_i and,
 *                      if any γ_j > 0:  d_hat = d_coef·numerator/denom ;  d_new = max(d, d_hat) if d == d0 else d ;
 *                      d_max = max(d_max, d_hat) ;  d_new = min(d_max, d_new·growth_rate).  Writes d_prev = d, then d = d_new;
 *                      [4] and [5] are this step's d_hat and denom, d_hat = 0 on a step that forms none.
 *                      `workspace`: lora_prodigy_workspace_bytes() bytes, 16-byte aligned.
 *   lora_prodigy_apply   : dlr_j from d_prev;  param_i = param_i·(1 − weight_decay_j·dlr_j) − dlr_j·m_i/(sqrt(v_i) + d·eps)  with
 *                      the NEW d;  with a non-null `shadow`, in the same launch, lora_adamw_ema_step's average on that param_i.
 * Both skip entirely when norm_in[1] != 0 (overflow): no buffer, no scalar and no shadow element changes.
 * Status, decided before any launch: LORA_E_BADARG for a null pointer (`shadow` excepted), n < 1, n_ranges outside 1..4, range
 * ends that do not increase or do not end at n, a negative lr or weight decay, a beta outside [0, 1), d0 <= 0, d_coef <= 0,
 * growth_rate < 1, eps < 0, and — with a shadow — ema_max_decay outside [0, 1] or ema_update_after < 0; then LORA_E_ALIGN for a
 * device buffer or workspace off a 16-byte boundary (the bodies move 16 bytes per lane; any n >= 1).
 */
int lora_prodigy_moments(const float* param, const float* param0, const float* grad, float* exp_avg, float* exp_avg_sq, float* s,
                         int64_t n, const int64_t* range_end, const float* lr, int n_ranges, const float* norm_in,
                         float* scalars, void* workspace, float grad_mul, float max_norm, float beta1, float beta2, float beta3,
                         float d0, float d_coef, float growth_rate, int use_bias_correction, int safeguard_warmup, void* stream);
int lora_prodigy_apply(float* param, const float* exp_avg, const float* exp_avg_sq, float* shadow /* nullable: no EMA */, int64_t n,
                       const int64_t* range_end, const float* lr, const float* weight_decay, int n_ranges, const float* norm_in,
                       const float* scalars, float beta1, float beta2, float eps, int use_bias_correction, float ema_max_decay,
                       int ema_update_after, void* stream);
int64_t lora_prodigy_workspace_bytes(void);

/*
 * Max-norm constraint on the learned update of every LoRA layer of the flat slab, one launch for any model.  This entry replaces
 * no line of the reference, which has no such control: the rule is restated from its published definition ("Max-norm
 * constraint"; parity with the trainers that call it --scale_weight_norms is unpinned).
 *   table (device, int64, 8 per layer): {up_off, down_off, K, N, r, scale_bits, 0, 0} — up [N,r] and down [r,K], row-major fp32,
 *                      at the ELEMENT offsets up_off / down_off from `params` (any 4-byte alignment; the two need not touch);
 *                      scale_bits = the layer's fp32 `scale`, bit-cast to an integer.
 *   per layer        : GA = down·downᵀ, GB = upᵀ·up (r×r, accumulated in fp32 in an order fixed by (K, N, r): no atomics, the
 *                      same bits on every run);  n² = scale²·Σ_ij GA_ij·GB_ij in double = ‖scale·up·down‖_F²;
 *                      norm = sqrt(max(n², 0));  factor = norm > max_norm ? (float)sqrt((double)max_norm/norm) : 1.0f;
 *                      factor != 1: every element of up and of down is multiplied by factor (one fp32 multiply each), so the
 *                      product shrinks by max_norm/norm;  factor == 1: the layer is not written at all.
 *   stats  (device, [n_layers][2] floats): {(float)norm BEFORE the scaling, factor}.
 *   counters (device, nullable): counters[0] += the number of layers with factor != 1 (an integer sum).
 * max_norm = +inf measures only: stats is all that is written.  A layer with up = 0 has norm 0 and factor 1.  `max_r`: the largest
 * rank in the table, 1..64 (it sizes the launch's LDS); a row with r outside 1..max_r, a size < 1 or a negative offset is left
 * alone and reports {-1, 1}.  Nothing outside the layers of the table is read or written.
 * Status, decided before the launch: LORA_E_BADARG for a null params / table / stats, n_layers < 1, max_norm <= 0 or NaN;
 * LORA_E_RANK for max_r outside 1..64.
 */
int lora_max_norm(float* params, const int64_t* table, int n_layers, int max_r, float max_norm,
                  float* stats /* [n_layers][2]: norm before, factor applied */,
                  int* counters /* nullable: [0] += layers scaled */, void* stream);

/*
 * Step prologue — training_scripts/train_lora_dreambooth.py:824-853 (add_noise / target selection)
 * with the DDPM definitions (diffusers DDPMScheduler, not vendored in the reference):
 *     noisy  = sqrt_acp[t_b]·x0 + sqrt_1macp[t_b]·eps
 *     target = eps                                   (v_prediction == 0)
 *            = sqrt_acp[t_b]·eps − sqrt_1macp[t_b]·x0 (v_prediction != 0)
 * x0, eps fp32 [B, per_row]; t int64 [B]; tables fp32 [T]; noisy/target in `dtype`.
 */
int ddpm_add_noise(const float* x0, const float* eps, const int64_t* t, const float* sqrt_acp,
                   const float* sqrt_1macp, void* noisy, void* target, int B, int64_t per_row,
                   int v_prediction, int dtype, void* stream);

/*
 * Step prologue with build-owned, counter-based randomness: replaces randn_like + randint +
 * add_noise (+ get_velocity) of training_scripts/train_lora_dreambooth.py:824-853 by one launch.
 *     t_b ~ U{0..n_timesteps-1},  eps ~ N(0,1)   from Philox4x32-10 keyed by (seed, step): the same draw on every
 *     rank (set_seed semantics, :509-510) and on the CPU oracle (oracle/philox.py);
 *     noisy / target as in ddpm_add_noise.  eps_out (fp32) and t_out (int64) are optional copies of the draw.
 * Counter layout: element group g = i/4 uses counter (g, 0, 0, 0) → 4 normals by Box–Muller; row b uses
 * counter (b, 0, 1, 0), word 0, mapped to [0, n_timesteps) by the high half of a 32×32-bit product.
 */
int ddpm_noise_prologue(const float* x0, const float* sqrt_acp, const float* sqrt_1macp, void* noisy,
                        void* target /* nullable */, float* eps_out /* nullable */, int64_t* t_out /* nullable */,
                        int B, int64_t per_row, int n_timesteps, uint64_t seed, uint64_t step,
                        int v_prediction, int dtype, void* stream);

/*
 * The prologue one step earlier: the latents are drawn from the VAE encoder's moments instead of being handed in —
 * `vae.encode(pixels).latent_dist.sample() * 0.18215`, training_scripts/train_lora_dreambooth.py:818-821 and
 * lora_diffusion/cli_lora_pti.py:180-184 — so a training set caches the moments and every iteration draws afresh:
 *     lv = clamp(logvar, −30, 20);  x0 = (mean + exp(0.5·lv)·z)·scale,  z ~ N(0,1),  scale = 0.18215 in the reference
 * (DiagonalGaussianDistribution.sample is diffusers', not vendored in the reference: restated from its published
 * definition, parity unpinned).  moments [B, 2·per_row] in `moments_dtype` (f32 / f16 / bf16), row b = mean [per_row] |
 * logvar [per_row] — a contiguous [B, 2C, h, w]; all arithmetic fp32.
 *   ddpm_posterior_prologue : the device-drawn form, ONE launch for chunk + clamp + exp + randn + mul + add + mul and the
 *       whole of ddpm_noise_prologue.  z comes from Philox stream 2 — element group g uses counter (g, g>>32, 2, 0), same
 *       Box–Muller — next to eps (g, g>>32, 0, 0) and t (b, 0, 1, 0): for equal (seed, step) eps and t are bit-identical
 *       to ddpm_noise_prologue's, and z is independent of both.  noisy / target (nullable) in `dtype`; x0_out, z_out,
 *       eps_out (fp32) and t_out (int64) are optional copies.
 *   ddpm_posterior_sample : the caller-drawn form (the reference's route: z from torch's generator), x0 fp32 from an fp32
 *       z [B, per_row]; ddpm_add_noise follows it.
 * 16-byte (fp32) / 8-byte (16-bit) accesses when per_row % 4 == 0 and every pointer is aligned to 4 of its elements,
 * element by element otherwise.  No workspace, nothing retained, capturable.
 */
int ddpm_posterior_prologue(const void* moments, int moments_dtype, const float* sqrt_acp, const float* sqrt_1macp,
                            void* noisy, void* target /* nullable */, float* x0_out /* nullable */,
                            float* z_out /* nullable */, float* eps_out /* nullable */, int64_t* t_out /* nullable */,
                            int B, int64_t per_row, int n_timesteps, float scale, uint64_t seed, uint64_t step,
                            int v_prediction, int dtype, void* stream);
int ddpm_posterior_sample(const void* moments, int moments_dtype, const float* z, float* x0, int B, int64_t per_row,
                          float scale, void* stream);

/*
 * Offset noise inside the two device-drawn prologues — N. Guttenberg, "Diffusion with Offset Noise" (2023), the
 * `--noise_offset` of the diffusers and kohya trainers; an extension beyond the reference.  One more normal ξ per
 * (row, channel) is added to every element of that channel's noise, so the model can learn to move an image's mean:
 *     eps' = fmaf(noise_offset, ξ[b, c], eps)        C = per_row / hw channels per row
 * and eps' is the noise everywhere downstream: noisy, target (ε or velocity) and eps_out.
 * ξ is a fourth Philox stream of the step's key (seed, step): with j = b·C + c, counter (j, j>>32, 3, 0), and
 * ξ = sqrt(−2·ln u(r0))·cos(2π·u(r1)), the first normal of the Box–Muller mapping of the other streams.  t and — before the
 * offset is added — eps and z keep their counters and arithmetic: for equal (seed, step) they are bit-identical to the plain
 * entries'.  With noise_offset == 0 every output is the plain entry's bit for bit.
 * Arguments: those of the plain entry, then hw (per_row % hw != 0 is LORA_E_BADARG, as is a non-finite noise_offset),
 * noise_offset and xi_out (nullable, fp32 [B, C]: a copy of ξ).  Access paths, no workspace, capturable: as the plain entries.
 */
int ddpm_noise_prologue_offset(const float* x0, const float* sqrt_acp, const float* sqrt_1macp, void* noisy,
                               void* target /* nullable */, float* eps_out /* nullable */, int64_t* t_out /* nullable */,
                               int B, int64_t per_row, int n_timesteps, uint64_t seed, uint64_t step, int v_prediction,
                               int dtype, int64_t hw, float noise_offset, float* xi_out /* nullable */, void* stream);
int ddpm_posterior_prologue_offset(const void* moments, int moments_dtype, const float* sqrt_acp, const float* sqrt_1macp,
                                   void* noisy, void* target /* nullable */, float* x0_out /* nullable */,
                                   float* z_out /* nullable */, float* eps_out /* nullable */, int64_t* t_out /* nullable */,
                                   int B, int64_t per_row, int n_timesteps, float scale, uint64_t seed, uint64_t step,
                                   int v_prediction, int dtype, int64_t hw, float noise_offset,
                                   float* xi_out /* nullable */, void* stream);

/*
 * Latent sampler: the loop AROUND the UNet forward when one samples with the model being trained —
 * lora_diffusion/utils.py:112-163 (evaluate_pipe: 50 steps, guidance_scale 5.0) on the pipeline cli_lora_pti.py:370-402
 * builds around the training DDPMScheduler, the class images of training_scripts/train_lora_dreambooth.py:512-558 (the same
 * block in train_lora_w_ti.py:699 and train_lora_pt_caption.py:583) and utils.py:166-214 (visualize_progress).  Stock, that
 * is chunk + classifier-free guidance + scheduler.step + randn + cat + cast: some 25 tiny launches and host work per step;
 * here one launch per step, with no host value in it that changes from step to step.
 * With SD's clip_sample = False every supported scheduler step is linear in the state x and the guided model output o:
 *     o  = u + g·(c − u)             cfg != 0: model_out [2B, per_row] = uncond rows | cond rows;  cfg == 0: o = model_out [B, per_row]
 *     x ← a·x + b·o + σ·z            (a, b, σ) = coef[i], z ~ N(0,1) drawn only where σ != 0
 * coef fp32 [S, 3] and timesteps int64 [S] come from the host (sampling.sampler_schedule: diffusers' DDPMScheduler /
 * DDIMScheduler are not vendored in the reference — restated from their published definitions in float64, parity unpinned,
 * like ddpm_add_noise above).  All arithmetic fp32, every product rounded on its own.
 *   ddpm_sample_init : x = x_T ~ N(0,1) fp32 [B, per_row]; model_in [rows, per_row] in `dtype` = x cast (rows = 2B under cfg:
 *       the same rows twice; else B); t_model int64 [rows] = timesteps[0]; cursor (int32 [2], device) = {0, seed's low word}.
 *   ddpm_sample_step : i = cursor[0] and the seed = cursor[1], read from DEVICE memory — a recorded launch serves every step
 *       and every seed.  i outside [0, S): nothing is read from the tables and nothing
 *       written (one replay too many is a no-op).  Else the update above on x in place, model_in = the NEW x cast (twice
 *       under cfg) and t_model = timesteps[min(i + 1, S − 1)] — the next forward's inputs, so no "prepare" launch exists;
 *       z_out (nullable, fp32 [B, per_row]) gets the draw, zeros where σ == 0.  model_out is read in `dtype`.
 *   ddpm_sample_advance : cursor[0] = i + 1 for i in [0, S), one thread.  A launch of its own BEHIND the step: stream order (an
 *       edge in a captured graph) puts it after every workgroup of that step — all of which have read the cursor — and
 *       before the first of the next.
 * Counter layout (Philox4x32-10, key (seed, i); i = 0 for x_T): element group g = 4 consecutive elements of [B, per_row] uses
 * counter (g, g>>32, 3, 0) for x_T and (g, g>>32, 4, 0) for z — streams of their own next to eps (0), t (1) and the posterior
 * z (2), same Box–Muller.  For equal (seed, i, B, per_row) the draw does not depend on dtype, access path or cfg.
 * 16-byte (fp32) / 8-byte (16-bit) accesses when per_row % 4 == 0 and every pointer is aligned to 4 of its elements, element
 * by element otherwise.  LORA_E_BADARG for a null pointer (z_out excepted), an unknown dtype, B, per_row or S < 1 — before
 * any HIP call.  No workspace, nothing retained, capturable.
 */
int ddpm_sample_init(float* x, void* model_in, int64_t* t_model, int* cursor, const int64_t* timesteps, int B,
                     int64_t per_row, int S, int cfg, uint64_t seed, int dtype, void* stream);
int ddpm_sample_step(float* x, const void* model_out, void* model_in, int64_t* t_model, const int* cursor,
                     const int64_t* timesteps, const float* coef, float* z_out /* nullable */, int B, int64_t per_row,
                     int S, int cfg, float guidance_scale, int dtype, void* stream);
int ddpm_sample_advance(int* cursor, int S, void* stream);

/*
 * Linear multistep step of the latent sampler.  The class images of prior preservation
 * (training_scripts/train_lora_dreambooth.py:512-558, train_lora_w_ti.py:675-699, train_lora_pt_caption.py:559-583) and
 * visualize_progress (lora_diffusion/utils.py:191-211) come from StableDiffusionPipeline.from_pretrained with the model's own
 * scheduler — for SD 1.x PNDM run as PLMS (skip_prk_steps), a fourth-order method over the last four model outputs; a
 * second-order solver at 20 steps (DPM-Solver++(2M)) is the usual preview.  Both are instances of one contract; per iteration
 * i = cursor[0] of I model evaluations, all fp32, every product rounded on its own, summed left to right:
 *     o    = u + g·(c − u)                                         (cfg == 0: o = model_out), as ddpm_sample_step
 *     h    = p·x + q·o                                             what the method keeps history of
 *     base = (flags & USE_SAVED) ? xs : x
 *     x'   = a·base + c0·h + c1·H[s1] + c2·H[s2] + c3·H[s3]
 *     flags & SAVE: xs ← x (the state BEFORE the update);   flags & PUSH: H[w] ← h;   x ← x'
 *     model_in = x' cast (twice under cfg);  t_model = timesteps[min(i + 1, I − 1)]
 * coef fp32 [I, 7] = (p, q, a, c0, c1, c2, c3) and plan int32 [I, 5] = (w, s1, s2, s3, flags), flags = PUSH 1 | SAVE 2 |
 * USE_SAVED 4, come from the host (sampling.multistep_schedule: float64 rounded once; formulas restated from the papers,
 * parity unpinned like ddpm_sample_step's).  The host knows which slot is pushed and which slots hold h of one, two and three
 * pushes ago: the kernel does no ring arithmetic (slot numbers are taken modulo 4).  hist = fp32 [4, B·per_row], xs = fp32
 * [B, per_row]; neither needs clearing: a term whose coefficient is exactly 0.0f is neither loaded nor added (xs likewise
 * unless USE_SAVED with a != 0), so uninitialised history never reaches the state.  No noise term.  Each thread touches its own
 * elements of x, xs and H[*] only and reads before it writes: the pushed slot may be one that is read.  i outside [0, I):
 * nothing is read from the tables and nothing written, hist and xs included.  The cursor is not moved: ddpm_sample_advance
 * with S = I; ddpm_sample_init with S = I starts a run.  4-element accesses when per_row % 4 == 0 and x, xs, hist, model_out
 * and model_in are aligned to 4 of their elements, element by element otherwise — the same bits.  LORA_E_BADARG for a null
 * pointer, an unknown dtype, B, per_row or I < 1 — before any HIP call.  No workspace, nothing retained, capturable.
 */
int ddpm_sample_multistep(float* x, float* xs, float* hist, const void* model_out, void* model_in, int64_t* t_model,
                          const int* cursor, const int64_t* timesteps, const float* coef, const int* plan, int B,
                          int64_t per_row, int I, int cfg, float guidance_scale, int dtype, void* stream);

/*
 * Image-to-image starts and keep-mask steps of the latent sampler — "Making Img2Img Inference with LoRA" (README.md:287-289,
 * scripts/run_img2img.ipynb of the reference: `pipe(image=init_image, strength=0.75)` under tune_lora_scale 0.0 / 0.7 / 1.0).
 * diffusers' img2img / inpaint pipelines are not part of the reference tree: the definitions are restated, parity unpinned
 * beyond this repository's own float64 restatement (tests/partial_reference.py).
 *   ddpm_sample_init_from : the noised start of a run that begins at table row `start`:
 *           x = fp32(k·init) + fp32(n·ε)                       (each product rounded on its own, the sum once: no fma)
 *       ε = the x_T draw of ddpm_sample_init at equal seed (Philox stream 3, key (seed, 0), same counters and Box–Muller),
 *       init fp32 [B, per_row] in model space, (k, n) = (√ᾱ, √(1−ᾱ)) at timesteps[start] — HOST arguments, like `start`: this
 *       launch stays outside a recording, as ddpm_sample_init does.  model_in = x cast (twice under cfg), t_model =
 *       timesteps[start], cursor = {start, seed's low word}; eps_out (nullable, fp32 [B, per_row]) gets ε.
 *   ddpm_sample_step_keep / ddpm_sample_multistep_keep : the contracts of ddpm_sample_step / ddpm_sample_multistep with x' —
 *       the state the method produced, variance noise included — replaced by
 *           x = fp32(m·y) + fp32((1 − m)·x'),      y = fp32(k_i·init) + fp32(n_i·ε)
 *       before model_in is written (model_in is the blended state; SAVE and PUSH read the state before the update, as they
 *       did).  m = mask fp32 [B, hw] in [0, 1] (not checked), broadcast over the per_row / hw channels: 1 holds the original, 0
 *       resamples; (k_i, n_i) = keep_coef[i], fp32 [S, 2] next to coef: (√ᾱ, √(1−ᾱ)) at the model timestep of the NEXT
 *       evaluation, (1, 0) in the last row (sampling.keep_schedule, float64 rounded once); ε regenerated from cursor[1] — no
 *       noise buffer, nothing extra read per step.  Where m == 1 the result is y, where m == 0 it is the bits of the entry
 *       without a mask.  The same kernels as the plain entries, instantiated over a parameter block that carries the three
 *       pointers: the plain instantiations are unchanged.
 * 4-element accesses when per_row % 4 == 0, hw % 4 == 0 (a group of four then lies inside one channel: its mask values are
 * consecutive) and every pointer is aligned to 4 of its elements; element by element, mask index per element, otherwise — the
 * same bits.  A cursor outside [0, S) reads and writes nothing.  LORA_E_BADARG for a null pointer (eps_out, z_out excepted),
 * an unknown dtype, B, per_row, hw or S < 1, per_row % hw != 0, start outside [0, S) — before any HIP call.  No workspace,
 * nothing retained, capturable.
 */
int ddpm_sample_init_from(float* x, void* model_in, int64_t* t_model, int* cursor, const int64_t* timesteps, const float* init,
                          float* eps_out /* nullable */, int B, int64_t per_row, int S, int start, float k, float n, int cfg,
                          uint64_t seed, int dtype, void* stream);
int ddpm_sample_step_keep(float* x, const void* model_out, void* model_in, int64_t* t_model, const int* cursor,
                          const int64_t* timesteps, const float* coef, float* z_out /* nullable */, const float* mask,
                          const float* init, const float* keep_coef, int B, int64_t per_row, int64_t hw, int S, int cfg,
                          float guidance_scale, int dtype, void* stream);
int ddpm_sample_multistep_keep(float* x, float* xs, float* hist, const void* model_out, void* model_in, int64_t* t_model,
                               const int* cursor, const int64_t* timesteps, const float* coef, const int* plan,
                               const float* mask, const float* init, const float* keep_coef, int B, int64_t per_row, int64_t hw,
                               int I, int cfg, float guidance_scale, int dtype, void* stream);

/*
 * Shared noise ("equal seed"): the five entries above that draw — x_T, the start noise ε (drawn, and regenerated by the keep
 * blend) and the variance noise z — with the Philox counter taken from the element's index INSIDE ITS SAMPLE instead of inside
 * the batch: element j of every sample takes lane j mod 4 of counter (j div 4, (j div 4) >> 32, stream, 0) under the same key,
 * which is what the B = 1 run of the same seed gives its element j.  Every sample of the batch therefore starts from, and is
 * perturbed by, the same noise — the reference's comparison loops call torch.manual_seed(seed) before every member
 * (utils.py:191-211: one sample per checkpoint; README.md:287-289: one per tune_lora_scale value).  per_row % 4 != 0 is
 * allowed: a group of four consecutive state elements then straddles counters (and samples) and is assembled element by
 * element; the result is the same B = 1 draw.  A run uses either the plain or the `_shared` entries throughout (the keep blend
 * regenerates the start draw of ddpm_sample_init_from*).  Arguments, statuses and everything else as the entry without the
 * suffix, whose own draws are unchanged.  ddpm_sample_multistep draws nothing and has no such form.
 */
int ddpm_sample_init_shared(float* x, void* model_in, int64_t* t_model, int* cursor, const int64_t* timesteps, int B,
                            int64_t per_row, int S, int cfg, uint64_t seed, int dtype, void* stream);
int ddpm_sample_step_shared(float* x, const void* model_out, void* model_in, int64_t* t_model, const int* cursor,
                            const int64_t* timesteps, const float* coef, float* z_out /* nullable */, int B, int64_t per_row,
                            int S, int cfg, float guidance_scale, int dtype, void* stream);
int ddpm_sample_init_from_shared(float* x, void* model_in, int64_t* t_model, int* cursor, const int64_t* timesteps,
                                 const float* init, float* eps_out /* nullable */, int B, int64_t per_row, int S, int start,
                                 float k, float n, int cfg, uint64_t seed, int dtype, void* stream);
int ddpm_sample_step_keep_shared(float* x, const void* model_out, void* model_in, int64_t* t_model, const int* cursor,
                                 const int64_t* timesteps, const float* coef, float* z_out /* nullable */, const float* mask,
                                 const float* init, const float* keep_coef, int B, int64_t per_row, int64_t hw, int S, int cfg,
                                 float guidance_scale, int dtype, void* stream);
int ddpm_sample_multistep_keep_shared(float* x, float* xs, float* hist, const void* model_out, void* model_in,
                                      int64_t* t_model, const int* cursor, const int64_t* timesteps, const float* coef,
                                      const int* plan, const float* mask, const float* init, const float* keep_coef, int B,
                                      int64_t per_row, int64_t hw, int I, int cfg, float guidance_scale, int dtype,
                                      void* stream);

/*
 * Sigma-space sampling — k-diffusion's Euler, Euler-ancestral and Heun.  Two of the reference's notebooks switch the pipeline
 * to `EulerAncestralDiscreteScheduler` before they sample (scripts/lora_training_process_visualized.ipynb:57, then 40 and 50
 * steps; scripts/merge_lora_with_lora.ipynb:74, then 30 steps), and the equal-seed comparison loop of utils.py:191-211 runs
 * under whichever scheduler the pipeline carries.  diffusers and k-diffusion are not part of the reference tree: the methods
 * are restated from Karras et al. 2022 and k-diffusion's published samplers, parity unpinned beyond this repository's own
 * stateful float64 restatement (tests/sigma_reference.py) and the identity euler == DDIM(η = 0), euler_a == DDIM(η = 1) on a
 * shared integer grid (tests/test_sigma_host.py).
 * The state lives in sigma space (x_T = σ₀·z), the model is fed c_in(σ)·x = x/√(σ²+1) with the σ of the NEXT evaluation, and
 * the timestep grid is fractional: `timesteps` [I] and `t_model` [rows] are FP32 here, int64 everywhere above.
 *   ddpm_sample_sigma_init : x = fp32(k·init) + fp32(nn·ε), or x = fp32(nn·ε) with init == NULL (text-to-image: nn = σ₀; k is
 *       not read); ε the x_T draw of ddpm_sample_init at equal seed (stream 3, key (seed, 0)); model_in = cast(fp32(c_in·x)),
 *       twice under cfg; t_model = timesteps[start]; cursor = {start, seed's low word}; eps_out (nullable) gets ε.  k, nn, c_in
 *       and start are HOST arguments: the launch stays outside a recording.
 *   ddpm_sample_sigma : per iteration i = cursor[0] (seed = cursor[1]), (p, q, a, c0, c1, s, n, σ_eval) = coef[i], fp32 [I, 8],
 *       flags = plan[i][4], int32 [I, 5] with the flag bits of ddpm_sample_multistep (sampling.sigma_schedule):
 *           o    = u + g·(c − u)                              as ddpm_sample_step
 *           h    = p·x + q·o                                  d = (x − denoised)/σ
 *           base = USE_SAVED ? xs : x
 *           x'   = a·base + c0·h + c1·H + s·z                 left to right, every product rounded on its own, no fma;
 *                                                             z (stream 4, key (seed, i)) drawn only where s ≠ 0
 *           SAVE: xs ← x;   PUSH: H ← h                       (hist is ONE slot, fp32 [B, per_row])
 *           keep (mask != NULL): x' ← fp32(m·y) + fp32((1−m)·x'), y = fp32(k_i·init) + fp32(n_i·ε), as ddpm_sample_step_keep
 *           x ← x';   model_in ← cast(fp32(n·x')), twice under cfg;   t_model ← timesteps[min(i+1, I−1)]
 *       A term whose coefficient is exactly 0 is neither loaded nor added: xs and H may be uninitialised until a Heun stage B
 *       reads them.  σ_eval is not read.  z_out (nullable) gets z (zeros where s == 0).  mask == NULL launches the
 *       instantiation without the blend (init and keep_coef are then not read, hw is ignored).  shared != 0: the draws of the
 *       `_shared` entries.  A cursor outside [0, I) reads and writes nothing; the cursor is not moved: ddpm_sample_advance.
 * 4-element accesses under the alignment rule of the entries above (hw % 4 == 0 too with a mask), element by element otherwise —
 * the same bits.  LORA_E_BADARG for a null pointer (init, eps_out, z_out, and the three keep pointers together, excepted), an
 * unknown dtype, B, per_row or I < 1, start outside [0, I), and with a mask a null init / keep_coef, hw < 1 or per_row % hw != 0 —
 * before any HIP call.  No workspace, nothing retained, capturable.
 */
int ddpm_sample_sigma_init(float* x, void* model_in, float* t_model, int* cursor, const float* timesteps,
                           const float* init /* nullable */, float* eps_out /* nullable */, int B, int64_t per_row, int I,
                           int start, float k, float nn, float c_in, int cfg, int shared, uint64_t seed, int dtype, void* stream);
int ddpm_sample_sigma(float* x, float* xs, float* hist, const void* model_out, void* model_in, float* t_model, const int* cursor,
                      const float* timesteps, const float* coef, const int* plan, float* z_out /* nullable */,
                      const float* mask /* nullable */, const float* init /* nullable */, const float* keep_coef /* nullable */,
                      int B, int64_t per_row, int64_t hw, int I, int cfg, int shared, float guidance_scale, int dtype,
                      void* stream);

/*
 * Guidance rescale (Lin et al., "Common Diffusion Noise Schedules and Sample Steps are Flawed", WACV 2024, §3.4, in the
 * model-output form of the pipelines' `rescale_noise_cfg`; restated from the paper and the published behaviour, parity unpinned
 * beyond tests/zero_snr_reference.py).  The one part of a guided iteration that is not linear in the model output, hence a
 * launch of its own IN FRONT of whichever step entry above follows it.  model_out [2B, per_row] in `dtype`, unconditional rows |
 * conditional rows; per sample b, all fp32:
 *     o_e = u_e + g·(c_e − u_e)                  as ddpm_sample_step forms it
 *     σ_c, σ_o                                   standard deviations of c and of o over the row, centred (means first, then the
 *                                                sums of squared deviations); their ratio does not depend on the ddof
 *     k_b = φ·(σ_c/σ_o) + (1 − φ)                φ = rescale; 1 where σ_o == 0, per_row == 1 or the value is not finite (the
 *                                                published function writes NaN there)
 *     c_e ← dtype(k_b·c_e),  u_e ← dtype(k_b·u_e)   in place: one fp32 product each, rounded to nearest even
 * so that the step behind it forms u' + g·(c' − u') = k_b·o up to the storage rounding of the two halves.  k_out (nullable,
 * fp32 [B]) gets k_b.  One workgroup per sample: a row's result depends neither on B nor on the other rows; sums in a fixed
 * order, no atomics — equal input gives equal bits.  Accesses under the alignment rule of ddpm_sample_step.  LORA_E_BADARG for a
 * null model_out, B or per_row < 1, an unknown dtype, a rescale outside [0, 1] or NaN, a guidance_scale that is not finite —
 * before any HIP call.  No workspace, nothing retained, capturable.
 */
int ddpm_cfg_rescale(void* model_out, float* k_out /* nullable */, int B, int64_t per_row, float guidance_scale, float rescale,
                     int dtype, void* stream);

/*
 * The two ops sandwiched by the hot path inside a transformer block, as streaming kernels.
 *   geglu_gate_fwd : out[M,C]  = h · gelu(g)  with [h | g] = y[M,2C], exact (erf) gelu — the body of diffusers'
 *                    GEGLU.forward, the caller of the `proj` LoraInjectedLinear (target class "GEGLU", lora.py:53).
 *   geglu_gate_bwd : dy[M,2C] = [dout·gelu(g) | dout·h·gelu'(g)], contiguous, consumed directly as dY by
 *                    lora_linear_bwd_input / lora_linear_bwd_params of `proj`.
 *   attn_split_heads : [B,N,H·d] → [B,H,N,D], D >= d, columns d..D-1 zero-filled (q/k/v into the attention core).
 *   attn_merge_heads : [B,H,N,D] → [B,N,H·d] (the core's output back, padding dropped).  Each is the other's
 *                    backward.  d and D multiples of 16 bytes.
 */
int geglu_gate_fwd(const void* y, void* out, int64_t M, int C, int dtype, void* stream);
int geglu_gate_bwd(const void* y, const void* dout, void* dy, int64_t M, int C, int dtype, void* stream);
int attn_split_heads(const void* src, void* dst, int B, int N, int H, int d, int D, int dtype, void* stream);
int attn_merge_heads(const void* src, void* dst, int B, int N, int H, int d, int D, int dtype, void* stream);
/* same, reading a [B,H,N,D] VIEW whose (b,h,n) rows start at b·sB + h·sH + n·sN elements (last dim contiguous):
 * the attention core hands back its output and its q/k/v gradients as transposed views; this consumes them in place. */
int attn_merge_heads_strided(const void* src, void* dst, int B, int N, int H, int d, int D, int64_t sB, int64_t sH,
                             int64_t sN, int dtype, void* stream);

/*
 * GroupNorm of the UNet's convolution trunk with its neighbours folded in (csrc/norm.hip):
 *     y = act(GroupNorm(x + a)),   x [N,C,H,W] with HW = H·W,  a [N,C] an optional per-(n,c) addend (nullable),
 *     gamma / beta [C] (same dtype as x),  act = 1: SiLU, 0: identity.
 * channels_last = 0: x, y, dy, dx are NCHW-contiguous (needs HW % 8 == 0); 1: NHWC-contiguous, torch's channels_last
 * (needs C % 8 == 0, C <= 4096).  The group width C/groups may be anything.  groups <= 256.  dtype f16 / bf16 only
 * (LORA_E_UNSUPPORTED for f32 and for the shapes above: the caller keeps the stock composite).
 * Statistics, the normalised value and the activation are fp32 up to the one rounding of y / dx / da.  Two launches each way
 * (statistics, apply), or one where group_norm_act_plan says so; sums folded in a fixed order, no atomics: results are
 * bit-reproducible.
 *   group_norm_act_fwd : writes y and the per-(n,group) mean / rstd [N,groups] fp32 of x + a that the backward takes.
 *   group_norm_act_bwd : recomputes the normalised value and act' from x; writes dx and, when da is not null, da [N,C] (the
 *                        gradient of the addend, a by-product of the per-channel sums).  No gamma / beta gradients.
 * workspace: group_norm_act_workspace_bytes(...) bytes (0: unsupported shape), 16-byte aligned, caller-owned, per call.
 */
int64_t group_norm_act_workspace_bytes(int N, int C, int HW, int groups, int channels_last, int want_da);
/* How many kernels the forward (backward = 0) or the backward (1) launches for this shape: 1 where an NCHW (n,group) slab is
 * small enough for one workgroup to keep it in registers, else 2; 0 for shapes the kernels do not cover.  Host code only, and
 * a function of these arguments alone.  The workspace size does not depend on it (the one-launch form leaves it unused). */
int group_norm_act_plan(int N, int C, int HW, int groups, int channels_last, int backward);
int group_norm_act_fwd(const void* x, const void* addend /* nullable */, const void* gamma, const void* beta, void* y,
                       float* mean, float* rstd, void* workspace, int N, int C, int HW, int groups, float eps, int act,
                       int channels_last, int dtype, void* stream);
int group_norm_act_bwd(const void* dy, const void* x, const void* addend /* nullable */, const void* gamma, const void* beta,
                       const float* mean, const float* rstd, void* dx, void* da /* nullable */, void* workspace, int N, int C,
                       int HW, int groups, int act, int channels_last, int dtype, void* stream);
/* group_norm_act_bwd on NCHW tensors with the gradient that reaches x along a residual path joined in:
 * dx = (GroupNorm's input gradient) + dh in fp32, rounded once.  dh has dx's layout and is nullable (then exactly
 * group_norm_act_bwd with channels_last = 0); da is unaffected by it.  Same workspace, same statuses; dh 16-byte aligned. */
int group_norm_act_bwd_res(const void* dy, const void* dh /* nullable */, const void* x, const void* addend /* nullable */,
                           const void* gamma, const void* beta, const float* mean, const float* rstd, void* dx,
                           void* da /* nullable */, void* workspace, int N, int C, int HW, int groups, int act, int dtype,
                           void* stream);

/*
 * Passes at the edges of the UNet trunk's blocks that only move or add activations (trunk_edges.hip).  f16 / bf16, fp32 sums
 * with one rounding at the store, 16-byte accesses, one launch each, no workspace, no reductions: bit-reproducible.
 *   residual_bias_add  : out[n,c,:] = res[n,c,:] + h[n,c,:] + b1[c] (+ b2[c]) on NCHW-contiguous [N,C,HW] tensors, HW % 8 == 0;
 *                        b1 / b2 [C] of the same dtype, b2 nullable.  out may be h or res.
 *   tokens_to_nchw_add : out[n,c,p] = tok[n,p,c] (+ res[n,c,p]);  tok [N,HW,C] dense, res / out [N,C,HW] dense, res nullable.
 *   nchw_to_tokens     : tok[n,p,c] = x[n,c,p].
 *   The two re-layouts need C % 8 == 0 and HW % 8 == 0 and go through a 64 x 64 tile in LDS; out must not overlap tok / x.
 * *_supported answer 1 / 0 for a shape and dtype without touching a device.  Statuses, decided before any launch:
 * LORA_E_BADARG (null pointer, non-positive size, unknown dtype), LORA_E_UNSUPPORTED (f32, a shape outside the above),
 * LORA_E_ALIGN (h, res, out, tok, x off a 16-byte boundary), in that order.
 */
int residual_bias_add_supported(int N, int C, int HW, int dtype);
int residual_bias_add(const void* h, const void* res, const void* b1, const void* b2 /* nullable */, void* out, int N, int C,
                      int HW, int dtype, void* stream);
int tokens_nchw_supported(int N, int C, int HW, int dtype);
int tokens_to_nchw_add(const void* tok, const void* res /* nullable */, void* out, int N, int C, int HW, int dtype,
                       void* stream);
int nchw_to_tokens(const void* x, void* tok, int N, int C, int HW, int dtype, void* stream);

/*
 * The time-embedding projections of L layers in one launch per 32 layers (time_proj.hip):
 *     out_l[n,c] = sum_e W_l[c,e] * silu(t[n,e]) + b_l[c] + cb_l[c],   t [N,E], W_l [C_l,E] row-major, b_l / cb_l [C_l],
 * f16 / bf16 throughout, silu and all sums in fp32 with one rounding at the store, fixed summation order (bit-reproducible).
 * W, b, cb are host arrays of L device pointers and C a host array of L widths, read during the call; b and cb may be null
 * (no layer has that bias) and so may any of their entries.  out is one buffer of N * sum(C_l) elements: layer l is a dense
 * [N, C_l] block at element offset N * sum_{j<l} C_j.  1 <= N <= 16, E % 8 == 0, any C_l >= 1 (at most 2^31 - 17 rows per 32
 * layers).  Nothing is allocated, uploaded or retained: the descriptors travel in the kernel arguments (capturable).
 * time_proj_supported answers 1 / 0 for (N, E, dtype) without touching a device.  Statuses, decided before any launch, in
 * this order: LORA_E_BADARG (t, W, C, out or a W[l] null, L, N, E or a C[l] < 1, unknown dtype), LORA_E_UNSUPPORTED (f32,
 * N > 16, E % 8 != 0), LORA_E_ALIGN (t or a W[l] off a 16-byte boundary).
 */
int time_proj_supported(int N, int E, int dtype);
int time_proj_all(const void* t, const void* const* W, const void* const* b /* nullable */, const void* const* cb /* nullable */,
                  const int* C, void* out, int L, int N, int E, int dtype, void* stream);

/*
 * 3x3, stride 1, padding 1 convolution with FROZEN weights where the pixels are few and the filters wide (csrc/conv_small.hip):
 *     y[n,k,h,w] = sum_{c,r,s} x[n,c,h+r-1,w+s-1] * w[k,c,r,s] (+ bias[k]),   x [N,C_in,H,W], y [N,C_out,H,W] NCHW-contiguous,
 * f16 / bf16, fp32 accumulation, one rounding at the store.  C_in and C_out multiples of 32; any N, H, W >= 1 whose tiles fit
 * (conv3x3_small_supported: 64 pixels with their halo in 768 padded positions, i.e. W up to about 350; fewer than 2^31 elements
 * per tensor).  An implicit GEMM over K-slices whose fp32 partials a second launch folds in slice order: two launches, no
 * atomics, bit-reproducible.
 *   conv3x3_small_pack : re-lays w [C_out,C_in,3,3] (C_in, C_out as given here, whatever `backward`) into the order the main loop
 *                        fetches (documented in conv_small.hip); packed has C_in*C_out*9 elements, 16-byte aligned.  backward = 1
 *                        packs w'[c,k,r,s] = w[k,c,2-r,2-s], with which dx = conv3x3_small(dy, pack', C_in := C_out, C_out := C_in).
 *                        Run once per weight and direction; the pack is stale once w changes.
 *   conv3x3_small      : bias [C_out] of the same dtype, nullable.  workspace: conv3x3_small_workspace_bytes(...) bytes (0:
 *                        unsupported), 16-byte aligned, caller-owned, per call; y must not overlap x.
 *   conv3x3_small_plan : 1 where this library is the faster way to run a frozen convolution of `pixels` = N*H*W output pixels
 *                        in BOTH directions, 0 where the stock convolution is, or where nothing was measured: host code, a
 *                        function of its arguments alone, and exactly the classes of the committed sweep log
 *                        (tools/conv_small_sweep.py): 256 pixels, 1280 <-> {1280, 2560}; 1024 pixels, 1280 <-> {640, 1280, 1920, 2560}.
 *   conv3x3_small_plan_channels : 1 where conv3x3_small_plan routes these channels at some pixel count (which filters are
 *                        worth packing before the activation's size is known).
 * Statuses, decided before any launch: LORA_E_BADARG (null pointer, non-positive size, unknown dtype, workspace too small),
 * LORA_E_UNSUPPORTED (f32, a shape outside the above), LORA_E_ALIGN (x, pack, y or workspace off a 16-byte boundary).
 */
int conv3x3_small_supported(int N, int C_in, int C_out, int H, int W, int dtype);
int64_t conv3x3_small_workspace_bytes(int N, int C_in, int C_out, int H, int W, int dtype);
int conv3x3_small_plan(int64_t pixels, int C_in, int C_out, int dtype);
int conv3x3_small_plan_channels(int C_in, int C_out, int dtype);
int conv3x3_small_pack(const void* w, void* packed, int C_in, int C_out, int backward, int dtype, void* stream);
int conv3x3_small(const void* x, const void* wpack, const void* bias /* nullable */, void* y, void* workspace,
                  int64_t workspace_bytes, int N, int C_in, int C_out, int H, int W, int dtype, void* stream);
/*
 * conv3x3_small with a named form of the activation staging, for the sweep (tools/conv_small_sweep.py) and the tests.  form 0:
 * positions, 2-byte loads (every supported shape); 1: whole image rows with 16-byte loads, which needs W % 8 == 0, 128-pixel tiles
 * and 128 % (H*W) == 0 or (H*W) % 128 == 0: LORA_E_UNSUPPORTED, with nothing launched, otherwise.  LORA_E_BADARG for any other
 * form.  Both forms give the same bits.  conv3x3_small_form_choice: the form conv3x3_small takes for a shape; -1: not covered.
 */
int conv3x3_small_form_choice(int N, int C_in, int C_out, int H, int W, int dtype);
int conv3x3_small_form(const void* x, const void* wpack, const void* bias /* nullable */, void* y, void* workspace,
                       int64_t workspace_bytes, int N, int C_in, int C_out, int H, int W, int dtype, int form, void* stream);

/*
 * The same convolution, same contract and same packs (conv3x3_small_pack), where the pixels are MANY (csrc/conv_large.hip, the
 * 32x32 and 64x64 levels): one launch, each workgroup owns its outputs over the whole K range and writes NCHW itself, so there
 * are no fp32 partials and no workspace: conv3x3_large_workspace_bytes is 0 and a null workspace is accepted (a non-null one
 * must still be 16-byte aligned).  conv3x3_large_supported: C_in, C_out multiples of 32, fewer than 2^31 elements per tensor,
 * 64 pixels with their halo in 384 padded positions (W up to about 160).  conv3x3_large_plan / _plan_channels: as the small
 * family's, set from profiles/r15_conv_large_sweep.log (tools/conv_large_sweep.py).  Statuses and their order as conv3x3_small.
 */
int conv3x3_large_supported(int N, int C_in, int C_out, int H, int W, int dtype);
int64_t conv3x3_large_workspace_bytes(int N, int C_in, int C_out, int H, int W, int dtype);
int conv3x3_large_plan(int64_t pixels, int C_in, int C_out, int dtype);
int conv3x3_large_plan_channels(int C_in, int C_out, int dtype);
int conv3x3_large(const void* x, const void* wpack, const void* bias /* nullable */, void* y, void* workspace /* nullable */,
                  int64_t workspace_bytes, int N, int C_in, int C_out, int H, int W, int dtype, void* stream);
/*
 * conv3x3_large on a named tile, for the sweep (tools/conv_large_sweep.py) and the tests.  tile 0: the channel-heavy tile the shape
 * rule gives (MT pixels x 160 channels), whatever the measured table of conv3x3_large says; 1: 256 pixels x 80 channels; 2: 128
 * pixels x 80 channels.  Tiles 1 and 2 stage whole image rows with 16-byte loads and need W % 8 == 0, MT % W == 0, H*W % MT == 0
 * and 2*W <= MT: LORA_E_UNSUPPORTED, with nothing launched, otherwise.  LORA_E_BADARG for any other tile.
 */
int conv3x3_large_tile_choice(int N, int C_in, int C_out, int H, int W, int dtype); /* the tile conv3x3_large runs; -1: none */
int conv3x3_large_tile(const void* x, const void* wpack, const void* bias /* nullable */, void* y, void* workspace /* nullable */,
                       int64_t workspace_bytes, int N, int C_in, int C_out, int H, int W, int dtype, int tile, void* stream);

/*
 * LayerNorm of the transformer blocks with the residual add in front of it folded in (csrc/layer_norm.hip), over rows [M, C]
 * with the last dimension contiguous; the caller's `attn(norm(x)) + x` chain, one launch each way:
 *     forward : h = x + delta, rounded to the storage type (bit-equal to the stock sum);  y = (h − mean)·rstd·gamma + beta,
 *               mean and the biased, centred variance of the ROUNDED h in fp32, rstd = rsqrt(var + eps).  Writes h, y and
 *               mean / rstd [M] fp32.  delta and h are null TOGETHER: then it is a plain LayerNorm of x and no h is written.
 *     backward: x̂ = (h − mean)·rstd, g = dy·gamma;  dx = rstd·(g − mean_c(g) − x̂·mean_c(g·x̂)) + dh, fp32 up to the one
 *               rounding of dx.  `h` is the forward's h (x itself where there was no delta); dh, the gradient that reaches h
 *               along the residual path, is nullable.  dx is the gradient of x and of delta alike.  No gamma / beta gradients.
 * Any M >= 1; C % 8 == 0, 8 <= C <= add_layer_norm_max_channels() (2048); dtype f16 / bf16 only (LORA_E_UNSUPPORTED for f32
 * and for other C: the caller keeps the stock composite).  Every tensor pointer 16-byte aligned, gamma / beta [C] of the same
 * dtype included.  One wave per row, reductions inside the wave in a fixed order, no atomics, no workspace: results are
 * bit-reproducible.  The shape is judged before the pointers' alignment, and everything is refused before any launch.
 */
int add_layer_norm_max_channels(void);
int add_layer_norm_fwd(const void* x, const void* delta /* nullable */, const void* gamma, const void* beta,
                       void* h /* null iff delta is null */, void* y, float* mean, float* rstd, int64_t M, int C, float eps,
                       int dtype, void* stream);
int add_layer_norm_bwd(const void* dy, const void* dh /* nullable */, const void* h, const void* gamma, const float* mean,
                       const float* rstd, void* dx, int64_t M, int C, int dtype, void* stream);

/*
 * Token-embedding rows for a text encoder whose INPUT EMBEDDINGS train next to the UNet's LoRA factors: the tuning phase of
 * lora_diffusion/cli_lora_pti.py with continue_inversion (default, :528) puts `text_encoder.get_input_embeddings().parameters()`
 * in the optimizer (:706-722) and runs `text_encoder(batch["input_ids"])[0]` inside loss_step (:199-206) — BASELINE config 5,
 * "+ extended-latent TI".  They replace `torch.nn.Embedding.forward` / its backward for that one table (fp32 master [V, D]).
 *   embed_rows_fwd : out[p, :] = table[ids[p], :] cast to out_dtype, p < n (ids int64; out of range ids are clamped).
 *   embed_rows_bwd : grad_table[t, :] (+)= Σ_{p : ids[p] == t} dE[p, :] for every token t that occurs, the positions added in
 *                    ascending order by ONE owner workgroup (torch's scatter uses atomics: run-to-run sum order).  Rows of tokens
 *                    that do not occur are not touched.  dE in `dtype`; accumulate = 0 overwrites the rows that occur; active[t] = 1
 *                    for every token that occurs (when given).
 */
int embed_rows_fwd(const float* table, const int64_t* ids, void* out, int64_t n, int D, int64_t V, int out_dtype, void* stream);
int embed_rows_bwd(const void* dE, const int64_t* ids, float* grad_table, unsigned char* active /* nullable: [V] */, int64_t n,
                   int D, int64_t V, int dtype, int accumulate, void* stream);
/* torch.optim.AdamW (`lora_adamw_step`'s arithmetic, same norm / skip / step-count inputs) over a [V, D] table of which only the
 * rows flagged in `active` (set by embed_rows_bwd, never cleared) have ever had a gradient: those get the full update, every
 * other row p ← p·(1 − lr·wd) — bit-identical to the dense update (g = m = v = 0 there), at a third of its traffic.
 * Status, decided before any launch: LORA_E_BADARG (null pointer, `norm_in` excepted when step >= 1; V < 1, D < 1, step < 0,
 * step == 0 with a null norm_in), then LORA_E_ALIGN when D % 4 == 0 and `param` is not 16-byte aligned (untouched rows of
 * whole 16-byte chunks are read and written as float4; a table with D % 4 != 0 needs 4-byte alignment only).
 * Reference: the token table as an AdamW group, cli_lora_pti.py:706-738, stepped at :451. */
int lora_adamw_rows(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const unsigned char* active, int64_t V,
                    int D, const float* norm_in, float grad_mul, float max_norm, float lr, float beta1, float beta2, float eps,
                    float weight_decay, int step, void* stream);

/*
 * Placeholder rows of textual inversion — train_inversion of lora_diffusion/cli_lora_pti.py (:290-346), the first phase of
 * train() (:651-687): only the P placeholder rows `slot_ids` [P] (int64, device) of the fp32 token table ever change, because
 * every other row is restored from a clone after each optimizer step (:280,344-346).  P <= LORA_TI_MAX_ROWS.
 *   ti_rows_grad        : grad[s, :] (+)= Σ_{p : ids[p] == slot_ids[s]} dE[p, :], p < n, positions added in ascending order by ONE
 *                         owner workgroup per (slot, column chunk): no atomics, bit-reproducible.  dE [n, D] in `dtype`; grad
 *                         [P, D] fp32; accumulate = 0 writes the sum (zero for a slot whose token does not occur).  Replaces the
 *                         dense backward of `get_input_embeddings()` (:299-307): the [V, D] table gradient is never formed.
 *   ti_rows_adamw_decay : for each slot s, on w = table[slot_ids[s], :] in place — torch.optim.AdamW (lora_adamw_step's
 *                         arithmetic, g = grad_mul·grad[s], bias correction with `step` >= 1; :311-313, created at :651-657),
 *                         then, when decay_lambda >= 0, clip_ti_decay (:318-336):
 *                             pre = ‖w‖ ;  w ← w / max(pre, 1e-12) · (pre + decay_lambda·(target_norm − pre))
 *                         (the reference: target_norm 0.4, decay_lambda = min(1, 100·lr)).  exp_avg / exp_avg_sq [P, D] fp32.
 *                         Rows not named in slot_ids are neither read nor written (the reference's restore of :344-346).
 */
#define LORA_TI_MAX_ROWS 64
int ti_rows_grad(const void* dE, const int64_t* ids, int64_t n, int D, const int64_t* slot_ids, int P, float* grad, int dtype,
                 int accumulate, void* stream);
int ti_rows_adamw_decay(float* table, int64_t V, int D, const int64_t* slot_ids, int P, const float* grad, float* exp_avg,
                        float* exp_avg_sq, float grad_mul, float lr, float beta1, float beta2, float eps, float weight_decay,
                        int step, float decay_lambda, float target_norm, void* stream);

/*
 * Short-context attention core  O = softmax(Q·Kᵀ·scale)·V  per head, for at most 128 keys: the cross-attention
 * (`attn2`) between the to_q/to_k/to_v and to_out LoRA linears (diffusers CrossAttention.forward, the
 * caller of the layers wrapped by lora_diffusion/lora.py:137-183).  Tensors keep the layout those linears produce
 * and consume — Q/O/dO/dQ [B, Tq, H·d], K/V/dK/dV [B, Tk, H·d] — so there are no head split/merge copies.
 *   attn_ctx_supported          : 1 when (shape, dtype) runs here: f16/bf16, d % 8 == 0, d <= 160, Tk <= 128 (<= 96 when d > 96).
 *   attn_ctx_fwd                : O.  Nothing else is saved: backward recomputes the single key tile.
 *   attn_ctx_bwd_workspace_bytes: size of the fp32 partial-sum workspace for dK/dV (-1 when unsupported).
 *   attn_ctx_bwd                : dQ, dK, dV from Q, K, V, dO.  Deterministic (ordered partial sums, no atomics).
 * Unsupported shapes return LORA_E_BADARG; the caller keeps its generic attention for those.
 */
int attn_ctx_supported(int B, int Tq, int Tk, int H, int d, int dtype);
/* _strided forms: K and V (resp. dK and dV) are [B·Tk, ·] column slices of a wider row-major buffer with row stride
 * ldk (ld_dk) elements — the output (gradient) buffer of a grouped to_k/to_v projection (lora_gemm_packed). */
int attn_ctx_fwd_strided(const void* Q, const void* K, const void* V, void* O, int64_t ldk, int B, int Tq, int Tk,
                         int H, int d, float scale, int dtype, void* stream);
int attn_ctx_bwd_strided(const void* Q, const void* K, const void* V, const void* dO, void* dQ, void* dK, void* dV,
                         void* workspace, int64_t ldk, int64_t ld_dk, int B, int Tq, int Tk, int H, int d,
                         float scale, int dtype, void* stream);
int attn_ctx_fwd(const void* Q, const void* K, const void* V, void* O, int B, int Tq, int Tk, int H, int d,
                 float scale, int dtype, void* stream);
int64_t attn_ctx_bwd_workspace_bytes(int B, int Tq, int Tk, int H, int d);
int attn_ctx_bwd(const void* Q, const void* K, const void* V, const void* dO, void* dQ, void* dK, void* dV,
                 void* workspace, int B, int Tq, int Tk, int H, int d, float scale, int dtype, void* stream);

/*
 * Causal short-context attention core  O = softmax(mask(Q·Kᵀ·scale))·V  per head, mask(i, j) = −inf for j > i, self-attention
 * over T <= 128 tokens: the text encoder's attention between the q_proj/k_proj/v_proj and out_proj LoRA linears (transformers
 * CLIPAttention.forward, the caller of the layers wrapped per lora_diffusion/lora.py:54; 77 tokens, heads of 64).  The
 * structure of attn_ctx_* with the triangle used: key fragments above a query block's diagonal are skipped, the diagonal
 * fragment's mask is the initial accumulator of its scores; masked probabilities are exact zeros.  Tensors are [B, T, H·d]:
 * Q, K, V with one row stride ldq (elements; H·d when dense, 3·H·d for the column slices of a grouped q/k/v projection's
 * output), dQ, dK, dV with one row stride ld_dq, O and dO dense.  No head split/merge copies, no [T, T] matrix in memory.
 *   attn_causal_supported          : 1 when (shape, dtype) runs here: f16/bf16, d % 8 == 0, d <= 96, 1 <= T <= 128.
 *   attn_causal_fwd_strided        : O.  Nothing else is saved: backward recomputes the single key tile.
 *   attn_causal_bwd_workspace_bytes: size of the fp32 partial-sum workspace for dK/dV (-1 when unsupported).
 *   attn_causal_bwd_strided        : dQ, dK, dV from Q, K, V, dO.  Deterministic (ordered partial sums, no atomics).
 * Unsupported shapes return LORA_E_BADARG.  Nothing is allocated or retained; all work goes on `stream` (capturable).
 */
int attn_causal_supported(int B, int T, int H, int d, int dtype);
int attn_causal_fwd_strided(const void* Q, const void* K, const void* V, void* O, int64_t ldq, int B, int T, int H, int d,
                            float scale, int dtype, void* stream);
int64_t attn_causal_bwd_workspace_bytes(int B, int T, int H, int d);
int attn_causal_bwd_strided(const void* Q, const void* K, const void* V, const void* dO, void* dQ, void* dK, void* dV,
                            void* workspace, int64_t ldq, int64_t ld_dq, int B, int T, int H, int d, float scale,
                            int dtype, void* stream);

/*
 * Long-context attention core (self-attention: thousands of keys), same tensor layouts as attn_ctx_*: flash-style
 * online softmax over 64-key tiles, no [Tq, Tk] matrix in memory.
 *   attn_flash_supported          : 1 for f16/bf16, d % 8 == 0, d <= 160.
 *   attn_flash_fwd                : O and LSE [B, H, Tq] fp32 = log2-sum-exp2 of the scaled scores (saved for backward;
 *                                   may be NULL when no backward follows).
 *   attn_flash_bwd_workspace_bytes: B·H·Tq·4 (the softmax correction Δ = Σ dO·O per query row).
 *   attn_flash_bwd                : dQ, dK, dV from Q, K, V, O, dO, LSE.  Two launches (query-owned dQ, which also fills the
 *                                   workspace with Δ; key-owned dK/dV), every output element written by one workgroup:
 *                                   deterministic, no atomics.
 */
int attn_flash_supported(int B, int Tq, int Tk, int H, int d, int dtype);
/* _strided forms: Q, K, V share the row stride ldq and dQ, dK, dV the row stride ld_dq (elements): the three column
 * slices of a grouped to_q/to_k/to_v projection's output / gradient buffer.  O, dO, LSE stay dense. */
int attn_flash_fwd_strided(const void* Q, const void* K, const void* V, void* O, float* LSE, int64_t ldq, int B,
                           int Tq, int Tk, int H, int d, float scale, int dtype, void* stream);
int attn_flash_bwd_strided(const void* Q, const void* K, const void* V, const void* O, const void* dO,
                           const float* LSE, void* dQ, void* dK, void* dV, void* workspace, int64_t ldq,
                           int64_t ld_dq, int B, int Tq, int Tk, int H, int d, float scale, int dtype, void* stream);
int attn_flash_fwd(const void* Q, const void* K, const void* V, void* O, float* LSE, int B, int Tq, int Tk, int H,
                   int d, float scale, int dtype, void* stream);
int64_t attn_flash_bwd_workspace_bytes(int B, int Tq, int H);
int attn_flash_bwd(const void* Q, const void* K, const void* V, const void* O, const void* dO, const float* LSE,
                   void* dQ, void* dK, void* dV, void* workspace, int B, int Tq, int Tk, int H, int d, float scale,
                   int dtype, void* stream);

/*
 * fp32 attention core  O = softmax(Q·Kᵀ·scale)·V  per head on fp32 tensors, any Tq >= 1 and Tk >= 1: the attention of the routes
 * the reference runs in fp32 — diffusers CrossAttention.forward under cli_lora_pti.py:685 (mixed_precision=False: PTI's
 * textual-inversion phase) and BASELINE config 1.  Same tensor layouts as attn_flash_* (dense [B, T, H·d], no head split/merge,
 * no [Tq, Tk] matrix in memory); online softmax over 64-key tiles; every product on the exact f32-input MFMA
 * (v_mfma_f32_16x16x4_f32: a k-ordered fmaf chain, no reduced-precision path), softmax in fp32 with exp2.
 *   attn_f32_supported          : 1 for d % 8 == 0, 8 <= d <= 160, B, H, Tq, Tk >= 1.
 *   attn_f32_fwd                : O and LSE [B, H, Tq] = log2-sum-exp2 of the scaled scores (saved for backward; may be NULL
 *                                 when no backward follows).
 *   attn_f32_bwd_workspace_bytes: B·H·Tq·4 (the softmax correction Δ = Σ dO·O per query row); -1 for non-positive sizes.
 *   attn_f32_bwd                : dQ, dK, dV from Q, K, V, O, dO, LSE.  Two launches (query-owned dQ, which also fills the
 *                                 workspace with Δ; key-owned dK/dV), every output element written by one wave: no atomics,
 *                                 bit-identical from run to run.
 * Outside the envelope the entries return LORA_E_BADARG, for an operand off a 16-byte boundary LORA_E_ALIGN.  Nothing is
 * allocated or retained; all work goes on `stream` (capturable).
 */
int attn_f32_supported(int B, int Tq, int Tk, int H, int d);
int attn_f32_fwd(const float* Q, const float* K, const float* V, float* O, float* LSE, int B, int Tq, int Tk, int H, int d,
                 float scale, void* stream);
int64_t attn_f32_bwd_workspace_bytes(int B, int Tq, int H);
int attn_f32_bwd(const float* Q, const float* K, const float* V, const float* O, const float* dO, const float* LSE, float* dQ,
                 float* dK, float* dV, float* workspace, int B, int Tq, int Tk, int H, int d, float scale, void* stream);

/*
 * svd_distill — lora_diffusion/cli_svd.py:29-111: a fully fine-tuned model → rank-r LoRA factors, per target linear
 *     D = float(T(W1 − W0))  (:59-69);  U, S, Vh = svd(D);  up = U_r·diag(S_r) [N,r], down = Vh_r [r,K]  (:71-77)
 *     hi = quantile(cat(up, down), q) (linear interpolation);  up, down ← clamp(·, −hi, hi)  (:79-84)
 * by batched block subspace iteration (width 32) with Rayleigh–Ritz, every phase ONE launch for all layers.
 * table: device memory, int64 [n_layers][8] = {W1 ptr, W0 ptr (dtype, [N,K]), N, K, workspace byte offset (256-aligned),
 * output float offset, layer index (keys the start block), 0}.  Each layer owns lora_distill_workspace_bytes(N, K) bytes of
 * `workspace` from its offset; its factors go to out[off ..] as up [N,r] then down [r,K], fp32.  r <= 16
 * (LORA_E_UNSUPPORTED above: ranks up to 64 run on the lora_distill_wide_* entries below), r <= min(N,K) (LORA_E_RANK).  Sign convention (the SVD fixes none): the largest-magnitude
 * entry of each down row is positive, ties to the lowest index.
 *   lora_distill_start          : resets the per-layer state, V ← orth(V₀), V₀ pseudo-random from (seed, layer index).
 *                                 min_nk = min over the table of min(N,K).
 *   lora_distill_diff           : transpose = 0: Y = D·V [N,32]; 1: Z = Dᵀ·U [K,32].  D formed on load in `dtype`'s
 *                                 rounding and never stored; max_rows = max over the table of N (0) resp. K (1).
 *   lora_distill_rayleigh_ritz  : side 1: Y = U·Σ·Ũᵀ → U (Ritz pairs kept); side 2: residual max_{i<r} ‖Dᵀu_i − σ_i v_i‖/σ_1,
 *                                 converged (<= tol) or `last` → V ← V·Ũ and the layer freezes, else V ← orth(Z).
 *                                 Per-layer int32 state at the layer's workspace offset: [0] = 0 running, 1 converged,
 *                                 2 stopped by `last`, 3 non-finite; [1] = iterations; double at +8 = residual.
 *   lora_distill_finalize       : factors with the sign convention, then (clamp != 0) the quantile clamp at q.
 *   lora_quantile_clamp         : torch.quantile(x, q) (linear) and x ← clamp(x, −hi, hi) in place over n fp32 values, one
 *                                 workgroup; hi_out (nullable, device) receives hi.  Bit-identical to torch on the CPU.
 */
int64_t lora_distill_workspace_bytes(int64_t N, int64_t K);
int lora_distill_start(const int64_t* table, int n_layers, int64_t min_nk, int r, int64_t seed, void* workspace,
                       void* stream);
int lora_distill_diff(const int64_t* table, int n_layers, int64_t max_rows, int transpose, int dtype, void* workspace,
                      void* stream);
int lora_distill_rayleigh_ritz(const int64_t* table, int n_layers, int side, int r, double tol, int last, void* workspace,
                               void* stream);
int lora_distill_finalize(const int64_t* table, int n_layers, int r, float q, int clamp, void* workspace, float* out,
                          void* stream);
int lora_quantile_clamp(float* x, int64_t n, float q, float* hi_out, void* stream);

/*
 * svd_distill at ranks up to 64 — lora_diffusion/cli_svd.py:71-77 slices U[:, :rank] for any rank; a full fine-tune is usually
 * distilled at 32 or 64.  The same algorithm, table row, state header, sign convention and clamp (cli_svd.py:79-84) as the
 * lora_distill_* entries above, at a block width W chosen from the rank: lora_distill_wide_width(r) = 48 for r <= 32,
 * 64 for r <= 48, 80 for r <= 64 (W >= r + 16).  The workspace layout depends on W, so every entry takes r and a layer owns
 * lora_distill_wide_workspace_bytes(N, K, r) bytes: header (λ: double[W] at +64), Ũ double[W][W] at +1280, then
 * Y [N,W], Z [K,W], V [K,W] in fp32.  One r per workspace: the entries of one solve are called with the same r.
 * Status, decided before any launch: LORA_E_BADARG for a null pointer, an unknown side or dtype; LORA_E_RANK for r < 1 or
 * (start) r > min_nk; LORA_E_UNSUPPORTED for r > 64, in every entry and whatever min_nk is (the rank range is checked first).  lora_distill_wide_width returns the same codes for such r;
 * lora_distill_wide_workspace_bytes returns 0 for them and for N < 1 or K < 1.  Ranks 1..16 are accepted here too (W = 48)
 * but distill_lora keeps them on the width-32 entries.
 */
int lora_distill_wide_width(int r);
int64_t lora_distill_wide_workspace_bytes(int64_t N, int64_t K, int r);
int lora_distill_wide_start(const int64_t* table, int n_layers, int64_t min_nk, int r, int64_t seed, void* workspace,
                            void* stream);
int lora_distill_wide_diff(const int64_t* table, int n_layers, int64_t max_rows, int transpose, int dtype, int r,
                           void* workspace, void* stream);
int lora_distill_wide_rayleigh_ritz(const int64_t* table, int n_layers, int side, int r, double tol, int last,
                                    void* workspace, void* stream);
int lora_distill_wide_finalize(const int64_t* table, int n_layers, int r, float q, int clamp, void* workspace, float* out,
                               void* stream);

/*
 * Launch profiler (measurement only; off by default).  When enabled, the hot-path kernels are launched
 * with start/stop events attached to the dispatch itself, so each record is that kernel's own duration on
 * the caller's stream, together with the ALGORITHMIC bytes and flops of the call (formulas: DESIGN.md §5).
 * Records are grouped per kernel instantiation (the names rocprofv3 shows); lora_prof_kernel_name(i)
 * returns a substring of that name.  lora_prof_collect waits for the recorded events, returns the totals
 * and resets the recording.
 */
#define LORA_PROF_KINDS 18
typedef struct lora_prof_totals {
    int64_t launches[LORA_PROF_KINDS];
    double ms[LORA_PROF_KINDS];
    double bytes[LORA_PROF_KINDS];
    double flops[LORA_PROF_KINDS];
} lora_prof_totals;
int lora_prof_enable(int capacity /* max recorded launches; 0 disables and frees */);
int lora_prof_collect(lora_prof_totals* out);
const char* lora_prof_kernel_name(int kind);
/*
 * Launch-floor mode (measurement only; bench.py's `roofline.step_level.launch_floor_ms`): while on, every profiled launch site
 * dispatches an EMPTY kernel of the same signature — same grid, block, dynamic LDS and kernel-argument segment; it reads two
 * argument words and returns — in place of the real one.  With the profiler enabled the recorded durations are then what a
 * launch of that shape costs before it does any work.  Outputs are NOT written while the mode is on: timing only.
 */
int lora_prof_null_mode(int on);

#ifdef __cplusplus
}
#endif
#endif /* LORA_HIP_H */

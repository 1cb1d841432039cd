// Token-embedding rows of a text encoder whose INPUT EMBEDDINGS train next to the UNet's LoRA factors — the tuning phase of
// lora_diffusion/cli_lora_pti.py with continue_inversion (the default, :528): `text_encoder.get_input_embeddings().parameters()`
// joins the optimizer (:706-722) and loss_step runs `text_encoder(batch["input_ids"])[0]` inside the step (:199-206), so the
// step needs the table's forward gather and, in backward, the gradient rows of the tokens that occurred (BASELINE config 5:
// "+ extended-latent TI").  torch's embedding backward scatters with atomics (the sum order of a token that occurs several
// times — every padding position — varies from run to run); here one workgroup OWNS a token: the first position of a token
// sums all its positions in index order.  Deterministic, and the same on every data-parallel rank when the positions of all
// ranks are concatenated in rank order (trainer.TokenTable).
//
// The textual-inversion phase before it (train_inversion, cli_lora_pti.py:290-346) trains only P placeholder rows of the same table:
// ti_rows_grad sums their gradient rows into a [P, D] buffer (one owner workgroup per slot and column chunk), ti_rows_adamw_decay
// runs AdamW + clip_ti_decay on those P rows of the table in place (inversion.InversionTrainer).
#include "common.h"

namespace {

template <typename T>
__global__ __launch_bounds__(256) void embed_rows_fwd_kernel(const float* __restrict__ table, const int64_t* __restrict__ ids,
                                                              T* __restrict__ out, int D, int64_t V) {
    const int64_t id = ids[blockIdx.x];
    T* dst = out + (int64_t)blockIdx.x * D;
    if (id < 0 || id >= V) {
        // An id outside the table (torch.nn.Embedding raises): the row is POISONED with NaN — the loss of the step is NaN, the
        // optimizer's overflow check skips the update and the trainer warns — instead of silently training on another token's
        // row; the backward kernel drops the same positions.  The binding layer validates ids on the host whenever it can.
        const T nan = from_f32<T>(__builtin_nanf(""));
        for (int c = threadIdx.x; c < D; c += 256) dst[c] = nan;
        return;  // (block-uniform)
    }
    const float4* src = reinterpret_cast<const float4*>(table + id * D);
    for (int c = threadIdx.x; c < D / 4; c += 256) {  // (D % 4 == 0: checked by the entry point)
        const float4 v = src[c];
        dst[4 * c + 0] = from_f32<T>(v.x);
        dst[4 * c + 1] = from_f32<T>(v.y);
        dst[4 * c + 2] = from_f32<T>(v.z);
        dst[4 * c + 3] = from_f32<T>(v.w);
    }
}

// grid = positions.  Block p exits unless p is the FIRST position of its token; the owner adds the rows of every position
// of that token in ascending position order (fp32) and stores (or accumulates onto) the table-gradient row.
template <typename T>
__global__ __launch_bounds__(256) void embed_rows_bwd_kernel(const T* __restrict__ dE, const int64_t* __restrict__ ids,
                                                              float* __restrict__ grad, unsigned char* __restrict__ active,
                                                              int64_t n, int D, int64_t V, int accumulate) {
    const int64_t p = blockIdx.x;
    const int64_t id = ids[p];
    if (id < 0 || id >= V) return;  // (block-uniform)
    int earlier = 0;
    for (int64_t q = threadIdx.x; q < p; q += 256) earlier |= ids[q] == id ? 1 : 0;
    if (__syncthreads_or(earlier)) return;
    if (active != nullptr && threadIdx.x == 0) active[id] = 1;  // the row has (had) a gradient: lora_adamw_rows gives it the full update
    for (int c = threadIdx.x; c < D; c += 256) {
        float acc = accumulate ? grad[id * D + c] : 0.f;
        for (int64_t q = p; q < n; ++q)
            if (ids[q] == id) acc += to_f32<T>(dE[q * D + c]);  // (ids[q]: a scalar load, the branch is block-uniform)
        grad[id * D + c] = acc;
    }
}

// grid = (P, column chunks of 256).  Block (s, chunk) OWNS slot s's columns of that chunk: it adds dE[p, c] over the positions p
// whose token is slot_ids[s], in ascending position order, and stores (or accumulates onto) grad[s, c].  No atomics: the same
// sum in the same order on every run.  ids[q] is a block-uniform scalar load; a typical caption has n = 77 positions per image.
template <typename T>
__global__ __launch_bounds__(256) void ti_rows_grad_kernel(const T* __restrict__ dE, const int64_t* __restrict__ ids, int64_t n,
                                                           int D, const int64_t* __restrict__ slot_ids, float* __restrict__ grad,
                                                           int accumulate) {
    const int64_t id = slot_ids[blockIdx.x];
    const int c = blockIdx.y * 256 + threadIdx.x;
    if (c >= D) return;  // (no barrier below)
    float* g = grad + (int64_t)blockIdx.x * D + c;
    float acc = accumulate ? *g : 0.f;
    for (int64_t q = 0; q < n; ++q)
        if (ids[q] == id) acc += to_f32<T>(dE[q * D + c]);
    *g = acc;
}

// grid = P, one workgroup per placeholder row w = table[slot_ids[s]]:
//   AdamW (adamw_element, torch's order) on w with the slot's gradient and moments;
//   then, when decay_lambda >= 0, clip_ti_decay (cli_lora_pti.py:318-336):
//     pre = ‖w‖ ; w ← (w / max(pre, 1e-12)) · (pre + λd·(target − pre))
//   with the square sum in a fixed order (per-lane fmaf chain over the columns, wave butterfly, the 4 wave sums in pairs), and
//   the scale's products and sums rounded one op at a time as the three torch ops give them.  A slot id outside the table is
//   skipped (the host validates ids; the kernel never indexes outside [0, V)).  Each lane re-reads only what it wrote itself.
__global__ __launch_bounds__(256) void ti_rows_adamw_decay_kernel(float* __restrict__ table, int64_t V, int D,
                                                                  const int64_t* __restrict__ slot_ids,
                                                                  const float* __restrict__ grad, float* __restrict__ exp_avg,
                                                                  float* __restrict__ exp_avg_sq, float grad_mul, float lr,
                                                                  float beta1, float beta2, float eps, float wd, float bc1,
                                                                  float bc2_sqrt, float decay_lambda, float target_norm) {
    __shared__ float s_wave[4];
    const float step_size = lr / bc1;  // (on the device, as adamw_kernel forms them)
    const float decay = 1.f - lr * wd;
    const int64_t id = slot_ids[blockIdx.x];
    if (id < 0 || id >= V) return;  // (block-uniform)
    float* w = table + id * D;
    const int64_t base = (int64_t)blockIdx.x * D;
    float sq = 0.f;
    for (int c = threadIdx.x; c < D; c += 256) {
        const float g = grad[base + c] * grad_mul;
        float p = w[c], m = exp_avg[base + c], v = exp_avg_sq[base + c];
        adamw_element(p, m, v, g, decay, step_size, beta1, beta2, bc2_sqrt, eps);
        w[c] = p;
        exp_avg[base + c] = m;
        exp_avg_sq[base + c] = v;
        sq = fmaf(p, p, sq);
    }
    if (decay_lambda < 0.f) return;  // (kernel argument: uniform)
    sq = wave_sum(sq);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = sq;
    __syncthreads();
    const float pre = sqrtf((s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]));
    const float scale = __fadd_rn(pre, __fmul_rn(decay_lambda, __fsub_rn(target_norm, pre)));
    const float den = fmaxf(pre, 1e-12f);
    for (int c = threadIdx.x; c < D; c += 256) w[c] = __fmul_rn(__fdiv_rn(w[c], den), scale);
}

}  // namespace

extern "C" int embed_rows_fwd(const float* table, const int64_t* ids, void* out, int64_t n, int D, int64_t V, int out_dtype,
                              void* stream) {
    if (n < 0 || D < 1 || V < 1) return LORA_E_BADARG;
    if (n == 0) return LORA_OK;
    if (!table || !ids || !out) return LORA_E_BADARG;
    if (!aligned16(table) || (D % 4) != 0) return LORA_E_ALIGN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)n);
    switch (out_dtype) {
        case LORA_F32: hipLaunchKernelGGL(embed_rows_fwd_kernel<float>, grid, dim3(256), 0, s, table, ids, static_cast<float*>(out), D, V); break;
        case LORA_F16: hipLaunchKernelGGL(embed_rows_fwd_kernel<half_t>, grid, dim3(256), 0, s, table, ids, static_cast<half_t*>(out), D, V); break;
        case LORA_BF16: hipLaunchKernelGGL(embed_rows_fwd_kernel<bf16_t>, grid, dim3(256), 0, s, table, ids, static_cast<bf16_t*>(out), D, V); break;
        default: return LORA_E_BADARG;
    }
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}

extern "C" int embed_rows_bwd(const void* dE, const int64_t* ids, float* grad_table, unsigned char* active, int64_t n, int D,
                              int64_t V, int dtype, int accumulate, void* stream) {
    if (n < 0 || D < 1 || V < 1) return LORA_E_BADARG;
    if (n == 0) return LORA_OK;
    if (!dE || !ids || !grad_table) return LORA_E_BADARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)n);
    switch (dtype) {
        case LORA_F32: hipLaunchKernelGGL(embed_rows_bwd_kernel<float>, grid, dim3(256), 0, s, static_cast<const float*>(dE), ids, grad_table, active, n, D, V, accumulate); break;
        case LORA_F16: hipLaunchKernelGGL(embed_rows_bwd_kernel<half_t>, grid, dim3(256), 0, s, static_cast<const half_t*>(dE), ids, grad_table, active, n, D, V, accumulate); break;
        case LORA_BF16: hipLaunchKernelGGL(embed_rows_bwd_kernel<bf16_t>, grid, dim3(256), 0, s, static_cast<const bf16_t*>(dE), ids, grad_table, active, n, D, V, accumulate); break;
        default: return LORA_E_BADARG;
    }
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}

extern "C" int ti_rows_grad(const void* dE, const int64_t* ids, int64_t n, int D, const int64_t* slot_ids, int P, float* grad,
                            int dtype, int accumulate, void* stream) {
    if (n < 0 || D < 1 || P < 1 || P > LORA_TI_MAX_ROWS || !slot_ids || !grad) return LORA_E_BADARG;
    if (n > 0 && (!dE || !ids)) return LORA_E_BADARG;
    if (dtype != LORA_F32 && dtype != LORA_F16 && dtype != LORA_BF16) return LORA_E_BADARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)P, (unsigned)((D + 255) / 256));
    switch (dtype) {
        case LORA_F32: hipLaunchKernelGGL(ti_rows_grad_kernel<float>, grid, dim3(256), 0, s, static_cast<const float*>(dE), ids, n, D, slot_ids, grad, accumulate); break;
        case LORA_F16: hipLaunchKernelGGL(ti_rows_grad_kernel<half_t>, grid, dim3(256), 0, s, static_cast<const half_t*>(dE), ids, n, D, slot_ids, grad, accumulate); break;
        default: hipLaunchKernelGGL(ti_rows_grad_kernel<bf16_t>, grid, dim3(256), 0, s, static_cast<const bf16_t*>(dE), ids, n, D, slot_ids, grad, accumulate); break;
    }
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}

extern "C" int ti_rows_adamw_decay(float* table, int64_t V, int D, const int64_t* slot_ids, int P, const float* grad,
                                   float* exp_avg, float* exp_avg_sq, float grad_mul, float lr, float beta1, float beta2,
                                   float eps, float weight_decay, int step, float decay_lambda, float target_norm,
                                   void* stream) {
    if (!table || !slot_ids || !grad || !exp_avg || !exp_avg_sq) return LORA_E_BADARG;
    if (V < 1 || D < 1 || P < 1 || P > LORA_TI_MAX_ROWS || step < 1) return LORA_E_BADARG;
    // bias corrections in double on the host, as torch does with python floats (lora_adamw_step)
    const float bc1 = (float)(1.0 - pow((double)beta1, (double)step));
    const float bc2_sqrt = (float)sqrt(1.0 - pow((double)beta2, (double)step));
    hipLaunchKernelGGL(ti_rows_adamw_decay_kernel, dim3((unsigned)P), dim3(256), 0, static_cast<hipStream_t>(stream), table, V, D,
                       slot_ids, grad, exp_avg, exp_avg_sq, grad_mul, lr, beta1, beta2, eps, weight_decay, bc1, bc2_sqrt,
                       decay_lambda, target_norm);
    LORA_LAUNCH_CHECK();
    return LORA_OK;
}

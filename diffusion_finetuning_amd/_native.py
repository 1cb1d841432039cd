"""ctypes binding of liblora_hip.so (C-ABI declared in include/lora_hip.h).

Thin by design: tensors in, raw device pointers + sizes + the current HIP stream out.  There is no
fallback: if the library is missing, or a call returns a non-zero status, a RuntimeError is raised.
"""
import ctypes
import os
import threading

import torch

_LIB_PATH = os.environ.get("DFA_LIB_PATH") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "liblora_hip.so")  # (DFA_LIB_PATH: dev A/B builds)
_lib = None
_lock = threading.Lock()

ABI_VERSION = 9
PROF_KINDS = 18

_DTYPE_CODE = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}

_vp, _i64, _i32, _f32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_float


class GradProblem(ctypes.Structure):
    """lora_grad_problem of include/lora_hip.h (host memory, consumed during the call)."""
    _fields_ = [
        ("S", _vp), ("P", _vp), ("out", _vp * 4),
        ("s_stride", _i64), ("p_stride", _i64), ("part_stride", _i64), ("M", _i64),
        ("C", _i32), ("r", _i32), ("rg", _i32), ("out_kn", _i32), ("n_blocks", _i32),
        ("scale", _f32),
    ]


GRAD_MAX_BLOCKS = 64


class ProfTotals(ctypes.Structure):
    _fields_ = [
        ("launches", _i64 * PROF_KINDS),
        ("ms", ctypes.c_double * PROF_KINDS),
        ("bytes", ctypes.c_double * PROF_KINDS),
        ("flops", ctypes.c_double * PROF_KINDS),
    ]


# symbol -> (restype, argtypes); must list every function include/lora_hip.h declares
SIGNATURES = {
    "lora_version": (_i32, []),
    "lora_status_string": (ctypes.c_char_p, [_i32]),
    "lora_pack_factors": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "lora_pack_factors_batched": (_i32, [_vp, _i32, _i32, _vp, _vp, _i32, _vp]),
    "lora_linear_fwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _f32, _i32, _vp]),
    "lora_linear_fwd_ws": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _f32, _i32, _vp, _i64,
                                  _vp]),
    "lora_linear_geglu_fwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _f32, _i32, _vp]),
    "lora_linear_fwd_rows": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _f32, _vp, _i32, _i32,
                                    _i32, _vp, _i64, _vp]),
    "lora_linear_geglu_fwd_rows": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _f32, _vp, _i32,
                                          _i32, _i32, _vp]),
    "lora_linear_bwd_input": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _f32, _i32, _vp]),
    "lora_linear_bwd_params": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i64, _i32, _i32, _i32, _f32, _i32, _vp]),
    "lora_reduce_partials": (_i32, [_vp, _i64, _i32, _vp, _i64, _i32, _vp]),
    "lora_grad_row_blocks": (_i32, [_i64]),
    "lora_grad_batched": (_i32, [ctypes.POINTER(GradProblem), _i32, _i32, _vp]),
    "lora_grad_plan_bytes": (_i64, [ctypes.POINTER(GradProblem), _i32]),
    "lora_grad_plan": (_i32, [ctypes.POINTER(GradProblem), _i32, _i32, _vp, _i64, ctypes.POINTER(_i32), ctypes.POINTER(_i32)]),
    "lora_grad_planned": (_i32, [_vp, _i32, _i32, _i32, ctypes.c_double, ctypes.c_double, _vp]),
    "lora_fold_partials": (_i32, [_vp, _i32, _i64, _vp, _i64, _vp, _i32, _vp]),
    "lora_gemm_packed": (_i32, [_vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _i64, _i32, _i32, _i32, _f32,
                                _i64, _vp, _i64, _i32, _vp]),
    "lora_gemm_parts": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _f32, _i32, _vp]),
    "lora_gemm_workspace_bytes": (_i64, [_i64, _i32, _i32, _i32]),
    "lora_linear_bwd_input_ws": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _f32, _i32, _vp,
                                        _i64, _vp]),
    "lora_pack_items": (_i32, [_vp, _i32, _i32, _vp, _vp, _i32, _vp]),
    "ddpm_mse_fwd_bwd": (_i32, [_vp, _vp, _vp, _i32, _i32, _i64, _i64, _f32, _f32, _vp, _vp, _vp, _i32, _vp]),
    "ddpm_mse_weighted_fwd_bwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i64, _i64, _f32, _f32, _vp, _vp, _vp, _i32,
                                         _vp]),
    "lora_mse_workspace_bytes": (_i64, []),
    "lora_mask_prepare": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "lora_merge_weight": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _f32, _i32, _i32, _vp]),
    "lora_merge_weight_batched": (_i32, [_vp, _i32, _i64, _f32, _vp]),
    "lora_lerp": (_i32, [_vp, _vp, _i64, _f32, _f32, _i32, _vp]),
    "lora_cast_matrix": (_i32, [_vp, _vp, _i64, _i64, _i32, _i32, _i32, _vp]),
    "lora_grad_sqnorm": (_i32, [_vp, _i64, _f32, _vp, _vp, _vp]),
    "lora_sqnorm_workspace_bytes": (_i64, []),
    "lora_adamw_step": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _f32, _f32, _f32, _f32, _f32, _f32, _f32, _i32, _vp]),
    "lora_adamw_ema_step": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _f32, _f32, _f32, _f32, _f32, _f32, _f32, _i32, _f32, _i32,
                                   _vp]),
    "lora_slab_swap": (_i32, [_vp, _vp, _i64, _vp]),
    "lora_prodigy_moments": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _i32, _vp, _vp, _vp, _f32, _f32, _f32, _f32, _f32,
                                    _f32, _f32, _f32, _i32, _i32, _vp]),
    "lora_prodigy_apply": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i32, _vp, _vp, _f32, _f32, _f32, _i32, _f32, _i32, _vp]),
    "lora_prodigy_workspace_bytes": (_i64, []),
    "lora_max_norm": (_i32, [_vp, _vp, _i32, _i32, _f32, _vp, _vp, _vp]),
    "ddpm_add_noise": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i32, _i32, _vp]),
    "ddpm_noise_prologue": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i32, ctypes.c_uint64, ctypes.c_uint64,
                                   _i32, _i32, _vp]),
    "ddpm_posterior_prologue": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i32, _f32,
                                       ctypes.c_uint64, ctypes.c_uint64, _i32, _i32, _vp]),
    "ddpm_posterior_sample": (_i32, [_vp, _i32, _vp, _vp, _i32, _i64, _f32, _vp]),
    "ddpm_noise_prologue_offset": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i32, ctypes.c_uint64, ctypes.c_uint64,
                                          _i32, _i32, _i64, _f32, _vp, _vp]),
    "ddpm_posterior_prologue_offset": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i32, _f32,
                                              ctypes.c_uint64, ctypes.c_uint64, _i32, _i32, _i64, _f32, _vp, _vp]),
    "ddpm_sample_init": (_i32, [_vp, _vp, _vp, _vp, _vp, _i32, _i64, _i32, _i32, ctypes.c_uint64, _i32, _vp]),
    "ddpm_sample_step": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i32, _i32, _f32, _i32, _vp]),
    "ddpm_sample_advance": (_i32, [_vp, _i32, _vp]),
    "ddpm_sample_multistep": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i32, _i32, _f32, _i32, _vp]),
    "ddpm_sample_init_from": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i32, _i32, _f32, _f32, _i32, ctypes.c_uint64,
                                     _i32, _vp]),
    "ddpm_sample_step_keep": (_i32, [_vp] * 11 + [_i32, _i64, _i64, _i32, _i32, _f32, _i32, _vp]),
    "ddpm_sample_multistep_keep": (_i32, [_vp] * 13 + [_i32, _i64, _i64, _i32, _i32, _f32, _i32, _vp]),
    "ddpm_sample_init_shared": (_i32, [_vp, _vp, _vp, _vp, _vp, _i32, _i64, _i32, _i32, ctypes.c_uint64, _i32, _vp]),
    "ddpm_sample_step_shared": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i32, _i32, _f32, _i32, _vp]),
    "ddpm_sample_init_from_shared": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i32, _i32, _f32, _f32, _i32,
                                            ctypes.c_uint64, _i32, _vp]),
    "ddpm_sample_step_keep_shared": (_i32, [_vp] * 11 + [_i32, _i64, _i64, _i32, _i32, _f32, _i32, _vp]),
    "ddpm_sample_multistep_keep_shared": (_i32, [_vp] * 13 + [_i32, _i64, _i64, _i32, _i32, _f32, _i32, _vp]),
    "ddpm_sample_sigma_init": (_i32, [_vp] * 7 + [_i32, _i64, _i32, _i32, _f32, _f32, _f32, _i32, _i32, ctypes.c_uint64, _i32, _vp]),
    "ddpm_sample_sigma": (_i32, [_vp] * 14 + [_i32, _i64, _i64, _i32, _i32, _i32, _f32, _i32, _vp]),
    "ddpm_cfg_rescale": (_i32, [_vp, _vp, _i32, _i64, _f32, _f32, _i32, _vp]),
    "embed_rows_fwd": (_i32, [_vp, _vp, _vp, _i64, _i32, _i64, _i32, _vp]),
    "embed_rows_bwd": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i64, _i32, _i32, _vp]),
    "lora_adamw_rows": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _f32, _f32, _f32, _f32, _f32, _f32, _f32, _i32, _vp]),
    "ti_rows_grad": (_i32, [_vp, _vp, _i64, _i32, _vp, _i32, _vp, _i32, _i32, _vp]),
    "ti_rows_adamw_decay": (_i32, [_vp, _i64, _i32, _vp, _i32, _vp, _vp, _vp, _f32, _f32, _f32, _f32, _f32, _f32, _i32, _f32, _f32,
                                   _vp]),
    "geglu_linear_bwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp]),
    "geglu_gate_fwd": (_i32, [_vp, _vp, _i64, _i32, _i32, _vp]),
    "geglu_gate_bwd": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _vp]),
    "attn_split_heads": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "attn_merge_heads": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "attn_merge_heads_strided": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i64, _i64, _i64, _i32, _vp]),
    "group_norm_act_workspace_bytes": (_i64, [_i32, _i32, _i32, _i32, _i32, _i32]),
    "group_norm_act_plan": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32]),
    "group_norm_act_fwd": (_i32, [_vp] * 8 + [_i32, _i32, _i32, _i32, _f32, _i32, _i32, _i32, _vp]),
    "group_norm_act_bwd": (_i32, [_vp] * 10 + [_i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "group_norm_act_bwd_res": (_i32, [_vp] * 11 + [_i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "residual_bias_add_supported": (_i32, [_i32, _i32, _i32, _i32]),
    "residual_bias_add": (_i32, [_vp] * 5 + [_i32, _i32, _i32, _i32, _vp]),
    "tokens_nchw_supported": (_i32, [_i32, _i32, _i32, _i32]),
    "tokens_to_nchw_add": (_i32, [_vp] * 3 + [_i32, _i32, _i32, _i32, _vp]),
    "nchw_to_tokens": (_i32, [_vp] * 2 + [_i32, _i32, _i32, _i32, _vp]),
    "time_proj_supported": (_i32, [_i32, _i32, _i32]),
    "time_proj_all": (_i32, [_vp] * 6 + [_i32, _i32, _i32, _i32, _vp]),
    "conv3x3_small_supported": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32]),
    "conv3x3_small_workspace_bytes": (_i64, [_i32, _i32, _i32, _i32, _i32, _i32]),
    "conv3x3_small_plan": (_i32, [_i64, _i32, _i32, _i32]),
    "conv3x3_small_plan_channels": (_i32, [_i32, _i32, _i32]),
    "conv3x3_small_pack": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "conv3x3_small": (_i32, [_vp] * 5 + [_i64, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "conv3x3_small_form_choice": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32]),
    "conv3x3_small_form": (_i32, [_vp] * 5 + [_i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "conv3x3_large_supported":(_i32, [_i32, _i32, _i32, _i32, _i32, _i32]),
    "conv3x3_large_workspace_bytes": (_i64, [_i32, _i32, _i32, _i32, _i32, _i32]),
    "conv3x3_large_plan": (_i32, [_i64, _i32, _i32, _i32]),
    "conv3x3_large_plan_channels": (_i32, [_i32, _i32, _i32]),
    "conv3x3_large": (_i32, [_vp] * 5 + [_i64, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "conv3x3_large_tile_choice": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32]),
    "conv3x3_large_tile": (_i32, [_vp] * 5 + [_i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "add_layer_norm_max_channels": (_i32, []),
    "add_layer_norm_fwd": (_i32, [_vp] * 8 + [_i64, _i32, _f32, _i32, _vp]),
    "add_layer_norm_bwd": (_i32, [_vp] * 7 + [_i64, _i32, _i32, _vp]),
    "attn_ctx_supported": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32]),
    "attn_ctx_fwd": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _i32, _vp]),
    "attn_ctx_bwd_workspace_bytes": (_i64, [_i32, _i32, _i32, _i32, _i32]),
    "attn_ctx_fwd_strided": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _f32, _i32, _vp]),
    "attn_ctx_bwd_strided": (_i32, [_vp] * 8 + [_i64, _i64, _i32, _i32, _i32, _i32, _i32, _f32, _i32, _vp]),
    "attn_flash_fwd_strided": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _f32, _i32, _vp]),
    "attn_flash_bwd_strided": (_i32, [_vp] * 10 + [_i64, _i64, _i32, _i32, _i32, _i32, _i32, _f32, _i32, _vp]),
    "attn_ctx_bwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _i32, _vp]),
    "attn_causal_supported": (_i32, [_i32, _i32, _i32, _i32, _i32]),
    "attn_causal_fwd_strided": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _f32, _i32, _vp]),
    "attn_causal_bwd_workspace_bytes": (_i64, [_i32, _i32, _i32, _i32]),
    "attn_causal_bwd_strided": (_i32, [_vp] * 8 + [_i64, _i64, _i32, _i32, _i32, _i32, _f32, _i32, _vp]),
    "attn_flash_supported": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32]),
    "attn_flash_fwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _i32, _vp]),
    "attn_flash_bwd_workspace_bytes": (_i64, [_i32, _i32, _i32]),
    "attn_flash_bwd": (_i32, [_vp] * 10 + [_i32, _i32, _i32, _i32, _i32, _f32, _i32, _vp]),
    "attn_f32_supported": (_i32, [_i32, _i32, _i32, _i32, _i32]),
    "attn_f32_fwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _vp]),
    "attn_f32_bwd_workspace_bytes": (_i64, [_i32, _i32, _i32]),
    "attn_f32_bwd": (_i32, [_vp] * 10 + [_i32, _i32, _i32, _i32, _i32, _f32, _vp]),
    "lora_distill_workspace_bytes": (_i64, [_i64, _i64]),
    "lora_distill_start": (_i32, [_vp, _i32, _i64, _i32, _i64, _vp, _vp]),
    "lora_distill_diff": (_i32, [_vp, _i32, _i64, _i32, _i32, _vp, _vp]),
    "lora_distill_rayleigh_ritz": (_i32, [_vp, _i32, _i32, _i32, ctypes.c_double, _i32, _vp, _vp]),
    "lora_distill_finalize": (_i32, [_vp, _i32, _i32, _f32, _i32, _vp, _vp, _vp]),
    "lora_quantile_clamp": (_i32, [_vp, _i64, _f32, _vp, _vp]),
    "lora_distill_wide_width": (_i32, [_i32]),
    "lora_distill_wide_workspace_bytes": (_i64, [_i64, _i64, _i32]),
    "lora_distill_wide_start": (_i32, [_vp, _i32, _i64, _i32, _i64, _vp, _vp]),
    "lora_distill_wide_diff": (_i32, [_vp, _i32, _i64, _i32, _i32, _i32, _vp, _vp]),
    "lora_distill_wide_rayleigh_ritz": (_i32, [_vp, _i32, _i32, _i32, ctypes.c_double, _i32, _vp, _vp]),
    "lora_distill_wide_finalize": (_i32, [_vp, _i32, _i32, _f32, _i32, _vp, _vp, _vp]),
    "lora_prof_enable": (_i32, [_i32]),
    "lora_prof_collect": (_i32, [ctypes.POINTER(ProfTotals)]),
    "lora_prof_null_mode": (_i32, [_i32]),
    "lora_prof_kernel_name": (ctypes.c_char_p, [_i32]),
}


def library_path() -> str:
    return _LIB_PATH


def lib():
    """Loads the library once.  Raises RuntimeError (never falls back) when it is absent or stale."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(_LIB_PATH):
            raise RuntimeError(
                f"diffusion_finetuning_amd: native library {_LIB_PATH} not found. Build it with "
                "`python -m diffusion_finetuning_amd.build_native` (needs hipcc, targets gfx950). "
                "There is no CPU or PyTorch fallback for the LoRA hot path."
            )
        handle = ctypes.CDLL(_LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        if handle.lora_version() != ABI_VERSION:
            raise RuntimeError(
                f"diffusion_finetuning_amd: {_LIB_PATH} has ABI {handle.lora_version()}, expected {ABI_VERSION}; rebuild it"
            )
        _lib = handle
    return _lib


def _check(status: int, what: str) -> None:
    if status != 0:
        msg = lib().lora_status_string(status).decode()
        if status == -2:
            raise ValueError(f"{what}: {msg}")
        raise RuntimeError(f"{what} failed with status {status}: {msg}")


def dtype_code(dtype: torch.dtype) -> int:
    try:
        return _DTYPE_CODE[dtype]
    except KeyError:
        raise RuntimeError(f"diffusion_finetuning_amd: unsupported dtype {dtype} (float32, float16, bfloat16 only)")


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(t: torch.Tensor) -> int:
    """hipStream_t of the calling thread's current stream on t's device (the raw-handle query when this PyTorch has
    it: building a torch.cuda.Stream object per launch costs ~2 µs of host time, ~700 times per step)."""
    if _raw_stream is not None:
        return _raw_stream(t.device.index)
    return torch.cuda.current_stream(t.device).cuda_stream


def _ptr(t) -> int:
    return 0 if t is None else t.data_ptr()


def _require_device(*tensors) -> None:
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(
                "diffusion_finetuning_amd: the LoRA hot path runs only on a HIP device (MI355X); got a "
                f"{t.device} tensor. Move the model and inputs to 'cuda'. There is no CPU fallback."
            )


def staging_device(*tensors) -> torch.device:
    """The HIP device host-resident operands are staged through: the device of the first device tensor given, else the
    current HIP device.  Raises (never computes on the CPU) when there is none."""
    for t in tensors:
        if t is not None and t.is_cuda:
            return t.device
    if not torch.cuda.is_available():
        raise RuntimeError(
            "diffusion_finetuning_amd: this operation runs as a HIP kernel and no HIP device (MI355X) is visible; "
            "host tensors are staged through the device, there is no CPU implementation."
        )
    return torch.device("cuda", torch.cuda.current_device())


def lora_pack_factors(a, b, dtype: torch.dtype):
    """a [r,K], b [N,r] fp32 → (Apack [2,16·K], Bpack [2,16·N]) in `dtype` (both orientations, see lora_hip.h);
    (None, None) for r > 16."""
    _require_device(a, b)
    r, K = a.shape
    N = b.shape[0]
    if r > 16:
        return None, None
    apack = torch.empty(32 * K, dtype=dtype, device=a.device)
    bpack = torch.empty(32 * N, dtype=dtype, device=a.device)
    _check(lib().lora_pack_factors(_ptr(a), _ptr(b), _ptr(apack), _ptr(bpack), K, N, r, dtype_code(dtype), _stream(a)),
           "lora_pack_factors")
    return apack, bpack


def lora_pack_factors_batched(table, n_layers: int, max_len: int, params, packed) -> None:
    _require_device(table, params, packed)
    _check(lib().lora_pack_factors_batched(_ptr(table), n_layers, max_len, _ptr(params), _ptr(packed),
                                           dtype_code(packed.dtype), _stream(params)), "lora_pack_factors_batched")


def _require_row_scales(table, M: int, r: int, what: str) -> None:
    """The gate table of a `_rows` entry: fp32 [n_samples, R >= r] on the device, rows dense, M a multiple of n_samples."""
    _require_device(table)
    if table.dtype != torch.float32 or table.dim() != 2 or table.stride(1) != 1:
        raise ValueError(f"{what}: the gate table must be a float32 [n_samples, R] tensor with dense rows")
    if table.shape[0] < 1 or M % table.shape[0] != 0 or table.shape[1] < r:
        raise ValueError(f"{what}: a [{table.shape[0]}, {table.shape[1]}] gate table does not fit {M} rows at rank {r}")


def _row_scale_args(table) -> tuple:
    """What a `_rows` entry takes between `scale` and `dtype`."""
    return _ptr(table), table.shape[0], table.stride(0)


def _linear_fwd(what: str, x2, w, bias, a, b, scale: float, row_scales, packs):
    """The one body of lora_linear_fwd (row_scales None: the `_ws` entry) and lora_linear_fwd_rows."""
    _require_device(x2, w, bias, a, b)
    M, K = x2.shape
    N, r = b.shape
    if row_scales is not None:
        _require_row_scales(row_scales, M, r, what)
    if packs is None:
        packs = lora_pack_factors(a, b, x2.dtype)
    y = torch.empty((M, N), dtype=x2.dtype, device=x2.device)
    t = torch.empty((M, r), dtype=torch.float32, device=x2.device)
    ws = _splitk_workspace(M, K, N, x2)
    head = (_ptr(x2), _ptr(w), _ptr(bias), _ptr(a), _ptr(b), _ptr(packs[0]), _ptr(packs[1]), _ptr(y), _ptr(t), M, K, N, r,
            float(scale))
    tail = (dtype_code(x2.dtype), _ptr(ws), 0 if ws is None else ws.numel() * 4, _stream(x2))
    if row_scales is None:
        _check(lib().lora_linear_fwd_ws(*head, *tail), what)
    else:
        _check(lib().lora_linear_fwd_rows(*head, *_row_scale_args(row_scales), *tail), what)
    return y, t


def lora_linear_fwd(x2, w, bias, a, b, scale: float, packs=None):
    """x2 [M,K], w [N,K], bias [N]|None (dtype of x2); a [r,K], b [N,r] fp32 masters; packs = (Apack, Bpack)
    (made here when not given). Returns (y [M,N], T [M,r] fp32)."""
    return _linear_fwd("lora_linear_fwd", x2, w, bias, a, b, scale, None, packs)


def lora_linear_fwd_rows(x2, w, bias, a, b, scale: float, row_scales, packs=None):
    """`lora_linear_fwd` with per-sample, per-rank-slot gates: row_scales fp32 [n_samples, R >= r], sample b = rows
    [b·M/n_samples, (b+1)·M/n_samples) of x2, effective factor scale·row_scales[b, j].  Inference only.  Returns (y, T)."""
    return _linear_fwd("lora_linear_fwd_rows", x2, w, bias, a, b, scale, row_scales, packs)


def _linear_geglu_fwd(what: str, x2, w, bias, r: int, scale: float, row_scales, packs, want_y: bool):
    """The one body of lora_linear_geglu_fwd (row_scales None) and lora_linear_geglu_fwd_rows."""
    _require_device(x2, w, bias)
    M, K = x2.shape
    N = w.shape[0]
    if row_scales is not None:
        _require_row_scales(row_scales, M, r, what)
        if packs is None or packs[0] is None:
            return None
    out = torch.empty((M, N // 2), dtype=x2.dtype, device=x2.device)
    y = torch.empty((M, N), dtype=x2.dtype, device=x2.device) if want_y else None
    t = torch.empty((M, r), dtype=torch.float32, device=x2.device)
    head = (_ptr(x2), _ptr(w), _ptr(bias), _ptr(packs[0]), _ptr(packs[1]), _ptr(y), _ptr(out), _ptr(t), M, K, N, r, float(scale))
    tail = (dtype_code(x2.dtype), _stream(x2))
    if row_scales is None:
        st = lib().lora_linear_geglu_fwd(*head, *tail)
    else:
        st = lib().lora_linear_geglu_fwd_rows(*head, *_row_scale_args(row_scales), *tail)
    if st == -5:
        return None
    _check(st, what)
    return out, y, t


def lora_linear_geglu_fwd(x2, w, bias, r: int, scale: float, packs, want_y: bool):
    """`proj` forward with the GEGLU gate in the epilogue: x2 [M,K], w [2F,K], packs = (Apack, Bpack).
    Returns (out [M,F], y [M,2F] | None, T [M,r] fp32), or None when the library has no fused kernel for the shape/dtype."""
    return _linear_geglu_fwd("lora_linear_geglu_fwd", x2, w, bias, r, scale, None, packs, want_y)


def lora_linear_geglu_fwd_rows(x2, w, bias, r: int, scale: float, row_scales, packs, want_y: bool):
    """`lora_linear_geglu_fwd` with the gates of `lora_linear_fwd_rows`; None when the library has no fused kernel for the
    shape / dtype."""
    return _linear_geglu_fwd("lora_linear_geglu_fwd_rows", x2, w, bias, r, scale, row_scales, packs, want_y)


def lora_linear_bwd_input(dy2, wt, a, b, scale: float, need_dx: bool, packs=None):
    """dy2 [M,N]; wt [K,N] (= Wᵀ) or None when need_dx is False; packs = (Apack, Bpack) (made here when not given).
    Returns (dx [M,K]|None, U [M,r] fp32)."""
    _require_device(dy2, wt, a, b)
    M, N = dy2.shape
    r, K = a.shape
    if packs is None:
        packs = lora_pack_factors(a, b, dy2.dtype)
    dx = torch.empty((M, K), dtype=dy2.dtype, device=dy2.device) if need_dx else None
    u = torch.empty((M, r), dtype=torch.float32, device=dy2.device)
    ws = _splitk_workspace(M, N, K, dy2) if need_dx else None
    _check(
        lib().lora_linear_bwd_input_ws(_ptr(dy2), _ptr(wt), _ptr(a), _ptr(b), _ptr(packs[0]), _ptr(packs[1]), _ptr(dx),
                                       _ptr(u), M, K, N, r, float(scale), dtype_code(dy2.dtype), _ptr(ws),
                                       0 if ws is None else ws.numel() * 4, _stream(dy2)),
        "lora_linear_bwd_input",
    )
    return dx, u


_ws_bytes_cache = {}
_splitk_ws = {}        # device -> persistent workspace (ticket header zeroed ONCE: every launch leaves it zero again)
_splitk_ws_retired = []  # outgrown workspaces stay alive: a recorded hipGraph may still hold their address


def _splitk_workspace(M: int, Kc: int, Nc: int, like):
    """Scratch for a contraction the library wants to split over K (None when it does not): one buffer per device, grown
    on demand, shared by every call on the device — the launches are stream-ordered, and the hot path runs on one stream
    per process (two streams splitting concurrently would need a workspace each: lora_hip.h)."""
    key = (M, Kc, Nc, like.dtype)
    nbytes = _ws_bytes_cache.get(key)
    if nbytes is None:
        nbytes = _ws_bytes_cache[key] = int(lib().lora_gemm_workspace_bytes(M, Kc, Nc, dtype_code(like.dtype)))
    if nbytes <= 0:
        return None
    ws = _splitk_ws.get(like.device)
    if ws is None or ws.numel() * 4 < nbytes:
        if torch.cuda.is_current_stream_capturing():
            return None  # never allocate-and-zero inside a recording: this launch simply runs unsplit
        if ws is not None:
            _splitk_ws_retired.append(ws)
        ws = _splitk_ws[like.device] = torch.zeros(max(nbytes, 32 << 20) // 4, dtype=torch.float32, device=like.device)
    return ws


def grad_blocks_for(M: int) -> int:
    """Row blocks for the factor-gradient kernel when the caller has no fixed layout (plain autograd mode)."""
    return max(1, min(128, M // 32))


def lora_linear_bwd_params_partial(dy2, x2, t, u, ga_part, gb_part, part_stride: int, n_blocks: int, scale: float):
    """Stores per-row-block partial sums: block b at ga_part + b·part_stride ([r,K]) / gb_part + b·part_stride ([N,r])."""
    _require_device(dy2, x2, t, u, ga_part, gb_part)
    M, N = dy2.shape
    K = x2.shape[1]
    r = t.shape[1]
    _check(
        lib().lora_linear_bwd_params(_ptr(dy2), _ptr(x2), _ptr(t), _ptr(u), _ptr(ga_part), _ptr(gb_part),
                                     int(part_stride), int(n_blocks), M, K, N, r, float(scale),
                                     dtype_code(dy2.dtype), _stream(dy2)),
        "lora_linear_bwd_params",
    )


_row_blocks_cache = {}


def grad_row_blocks(M: int) -> int:
    """Row blocks lora_grad_batched uses for a problem of M rows when n_blocks is left to the library."""
    nb = _row_blocks_cache.get(M)
    if nb is None:
        nb = _row_blocks_cache[M] = int(lib().lora_grad_row_blocks(int(M)))
    return nb


def grad_problem(S, s_ptr_off: int, s_stride: int, C: int, P, p_ptr_off: int, p_stride: int, r: int, outs, rg: int,
                 out_kn: bool, part_stride: int, M: int, scale: float, n_blocks: int = 0):
    """One lora_grad_problem: G[c,j] = scale·Σ_m S[m,c]·P[m,j].  S / P are device tensors, *_ptr_off element offsets of
    the slice's first column; outs = device pointers (ints) of the rank groups' row-block-0 partials."""
    q = GradProblem()
    q.S = S.data_ptr() + s_ptr_off * S.element_size()
    q.P = P.data_ptr() + p_ptr_off * 4
    for i, o in enumerate(outs):
        q.out[i] = o
    q.s_stride, q.p_stride, q.part_stride, q.M = s_stride, p_stride, part_stride, M
    q.C, q.r, q.rg, q.out_kn, q.n_blocks, q.scale = C, r, rg, int(out_kn), n_blocks, scale
    return q


def lora_grad_batched(problems, dtype: torch.dtype, device) -> None:
    """Launches every problem of the list (a few launches whatever its length; tables travel as kernel arguments)."""
    n = len(problems)
    if n == 0:
        return
    lora_grad_batched_array((GradProblem * n)(*problems), n, dtype, device)


def lora_grad_batched_array(arr, n: int, dtype: torch.dtype, device) -> None:
    """The same on a `(GradProblem * n)` array the caller keeps (ops._SinkPlan re-uses one from step to step)."""
    stream = _raw_stream(device.index) if _raw_stream is not None else torch.cuda.current_stream(device).cuda_stream
    _check(lib().lora_grad_batched(arr, n, dtype_code(dtype), stream), "lora_grad_batched")


def lora_grad_plan_bytes(problems) -> int:
    n = len(problems)
    return int(lib().lora_grad_plan_bytes((GradProblem * n)(*problems), n)) if n else 0


def lora_grad_one_launch(problems, dtype: torch.dtype, device, host_plan=None):
    """All problems in ONE launch through a plan in device memory (include/lora_hip.h: lora_grad_plan / lora_grad_planned).
    host_plan: a pinned uint8 tensor to write the plan into (a recording hands over a buffer it owns — the copy node reads it
    on every replay); None allocates one (host-launched steps: torch's pinned allocator keeps the block until the copy has
    run).  Returns the (host, device) plan tensors — the caller keeps them alive until the launch has run (a recording: for
    its life) — or None when the library declines (fp32 / unaligned operands / rank > 16: use lora_grad_batched)."""
    n = len(problems)
    if n == 0 or dtype == torch.float32:
        return None
    arr = (GradProblem * n)(*problems)
    need = int(lib().lora_grad_plan_bytes(arr, n))
    if host_plan is None:
        host_plan = torch.empty(need, dtype=torch.uint8, pin_memory=True)
    elif host_plan.numel() < need or not host_plan.is_pinned():
        return None
    n_items, n_blocks = _i32(0), _i32(0)
    st = lib().lora_grad_plan(arr, n, dtype_code(dtype), host_plan.data_ptr(), host_plan.numel(), ctypes.byref(n_items),
                              ctypes.byref(n_blocks))
    if st == -5:
        return None
    _check(st, "lora_grad_plan")
    used = n_items.value * 128 + n_blocks.value * 4
    if used == 0:
        return (host_plan, None)
    dev_plan = torch.empty(used, dtype=torch.uint8, device=device)
    dev_plan.copy_(host_plan[:used], non_blocking=True)
    e = float(torch.empty(0, dtype=dtype).element_size())
    nbytes = sum(e * q.M * q.C + 4.0 * q.M * q.r + 4.0 * q.r * q.C for q in problems)
    flops = sum(2.0 * q.M * q.r * q.C for q in problems)
    stream = _raw_stream(device.index) if _raw_stream is not None else torch.cuda.current_stream(device).cuda_stream
    _check(lib().lora_grad_planned(dev_plan.data_ptr(), n_items.value, n_blocks.value, dtype_code(dtype), nbytes, flops, stream),
           "lora_grad_planned")
    return (host_plan, dev_plan)


def lora_fold_partials(ranges, n_ranges: int, max_len: int, partials, part_stride: int, grads, accumulate: bool) -> None:
    """grads[off:off+len] (+)= Σ_{b<blocks} partials[b·part_stride + off : …] for every row {off, len, blocks, 0} of the
    int64 device table `ranges`."""
    _require_device(ranges, partials, grads)
    _check(lib().lora_fold_partials(_ptr(ranges), int(n_ranges), int(max_len), _ptr(partials), int(part_stride),
                                    _ptr(grads), int(accumulate), _stream(grads)), "lora_fold_partials")


def lora_pack_items(table, n_items: int, max_len: int, params, packed) -> None:
    _require_device(table, params, packed)
    _check(lib().lora_pack_items(_ptr(table), n_items, max_len, _ptr(params), _ptr(packed), dtype_code(packed.dtype),
                                 _stream(params)), "lora_pack_items")


def lora_gemm_packed(am, lda: int, bm, bias, fp, qp, tile_part, part_table, n_parts: int, c, p_out, M: int, Kc: int,
                     Nc: int, r: int, scale: float, work_cols: int = 0) -> None:
    """C = Am·Bmᵀ + bias + s·P·Qᵀ, P = Am·Fᵀ on packed factors (include/lora_hip.h: lora_gemm_packed).  All operands
    are device tensors (or None); nothing is allocated here."""
    _require_device(am, bm, bias, fp, qp, tile_part, part_table, c, p_out)
    ws = _splitk_workspace(M, Kc, Nc, am) if (c is not None and tile_part is None) else None
    _check(lib().lora_gemm_packed(_ptr(am), int(lda), _ptr(bm), _ptr(bias), _ptr(fp), _ptr(qp), _ptr(tile_part),
                                  _ptr(part_table), int(n_parts), _ptr(c), _ptr(p_out), int(M), int(Kc), int(Nc), int(r),
                                  float(scale), int(work_cols), _ptr(ws), 0 if ws is None else ws.numel() * 4,
                                  dtype_code(am.dtype), _stream(am)), "lora_gemm_packed")


def lora_gemm_parts(am, bm, bias, fp, qp, c, p_out, ldp: int, M: int, Kc: int, Nc: int, r: int, n_parts: int,
                    parts_on_k: bool, scale: float) -> bool:
    """n_parts equal LoRA layers that share an input in one launch at any rank <= 16 (include/lora_hip.h: lora_gemm_parts);
    False when the library has no kernel for the shape / dtype (the caller runs the layers one by one)."""
    _require_device(am, bm, bias, fp, qp, c, p_out)
    st = lib().lora_gemm_parts(_ptr(am), _ptr(bm), _ptr(bias), _ptr(fp), _ptr(qp), _ptr(c), _ptr(p_out), int(ldp), int(M),
                               int(Kc), int(Nc), int(r), int(n_parts), int(bool(parts_on_k)), float(scale),
                               dtype_code(am.dtype), _stream(am))
    if st == -5:
        return False
    _check(st, "lora_gemm_parts")
    return True


def lora_reduce_partials(partials, part_stride: int, n_blocks: int, grads, n: int, accumulate: bool) -> None:
    _require_device(partials, grads)
    _check(lib().lora_reduce_partials(_ptr(partials), int(part_stride), int(n_blocks), _ptr(grads), int(n),
                                      int(accumulate), _stream(grads)), "lora_reduce_partials")


def lora_linear_bwd_params(dy2, x2, t, u, ga, gb, scale: float):
    """Accumulates into ga [r,K], gb [N,r] (fp32): partial sums per row block + ordered reduction."""
    _require_device(dy2, x2, t, u, ga, gb)
    M, N = dy2.shape
    r, K = ga.shape
    nb = grad_blocks_for(M)
    size = r * (K + N)
    stride = (size + 3) // 4 * 4
    ws = torch.empty((nb + 1, stride), dtype=torch.float32, device=dy2.device)
    lora_linear_bwd_params_partial(dy2, x2, t, u, ws[0], ws[0, r * K:], stride, nb, scale)
    out = ws[nb]
    lora_reduce_partials(ws, stride, nb, out, size, False)
    ga += out[: r * K].view(r, K)
    gb += out[r * K: size].view(N, r)


_ws_cache = {}


def _workspace(device, nbytes: int, tag: str):
    key = (device, tag, torch.cuda.current_stream(device).cuda_stream)
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        _ws_cache[key] = ws
    return ws


def ddpm_mse_fwd_bwd(pred, target, mask, n_inst: int, n_prior: int, prior_weight: float, grad_scale: float,
                     want_grad: bool = True):
    """pred/target [rows, C, H, W] contiguous, same dtype; mask fp32 [rows,1,H,W] (normalised) or None.
    Returns (loss fp32 scalar tensor, dpred|None)."""
    _require_device(pred, target, mask)
    rows = pred.shape[0]
    assert rows == n_inst + n_prior
    per_row = pred[0].numel()
    hw = pred.shape[-1] * pred.shape[-2]
    loss = torch.empty(1, dtype=torch.float32, device=pred.device)
    dpred = torch.empty_like(pred) if want_grad else None
    ws = _workspace(pred.device, int(lib().lora_mse_workspace_bytes()), "mse")
    _check(
        lib().ddpm_mse_fwd_bwd(_ptr(pred), _ptr(target), _ptr(mask), n_inst, n_prior, per_row, hw,
                               float(prior_weight), float(grad_scale), _ptr(loss), _ptr(dpred), _ptr(ws),
                               dtype_code(pred.dtype), _stream(pred)),
        "ddpm_mse_fwd_bwd",
    )
    return loss, dpred


def ddpm_mse_weighted_fwd_bwd(pred, target, mask, t, weights, n_inst: int, n_prior: int, prior_weight: float,
                              grad_scale: float, want_grad: bool = True):
    """`ddpm_mse_fwd_bwd` with row b weighted by weights[t[b]]: t int64 [rows], weights fp32 [T], both on the device
    (include/lora_hip.h: ddpm_mse_weighted_fwd_bwd).  Returns (loss fp32 scalar tensor, dpred|None)."""
    _require_device(pred, target, mask, t, weights)
    rows = pred.shape[0]
    assert rows == n_inst + n_prior
    if t.dtype != torch.int64 or t.numel() != rows or not t.is_contiguous():
        raise ValueError(f"timesteps must be a contiguous int64 [{rows}] tensor; got {t.dtype} {tuple(t.shape)}")
    if weights.dtype != torch.float32 or weights.dim() != 1 or not weights.numel() or not weights.is_contiguous():
        raise ValueError(f"the weight table must be a contiguous fp32 [T] tensor; got {weights.dtype} {tuple(weights.shape)}")
    per_row = pred[0].numel()
    hw = pred.shape[-1] * pred.shape[-2]
    loss = torch.empty(1, dtype=torch.float32, device=pred.device)
    dpred = torch.empty_like(pred) if want_grad else None
    ws = _workspace(pred.device, int(lib().lora_mse_workspace_bytes()), "mse")
    _check(
        lib().ddpm_mse_weighted_fwd_bwd(_ptr(pred), _ptr(target), _ptr(mask), _ptr(t), _ptr(weights), weights.numel(), n_inst,
                                        n_prior, per_row, hw, float(prior_weight), float(grad_scale), _ptr(loss), _ptr(dpred),
                                        _ptr(ws), dtype_code(pred.dtype), _stream(pred)),
        "ddpm_mse_weighted_fwd_bwd",
    )
    return loss, dpred


def lora_mask_prepare(mask_in, h: int, w: int):
    _require_device(mask_in)
    B, _, hin, win = mask_in.shape
    out = torch.empty((B, 1, h, w), dtype=torch.float32, device=mask_in.device)
    _check(lib().lora_mask_prepare(_ptr(mask_in), _ptr(out), B, hin, win, h, w, _stream(mask_in)), "lora_mask_prepare")
    return out


def lora_merge_weight(w, a, b, alpha: float, factor_dtype: torch.dtype = torch.float32) -> None:
    """In place W += alpha*(b@a); a [r,K], b [N,r] fp32 copies of factors held in `factor_dtype`."""
    _require_device(w, a, b)
    N, K = w.shape
    r = a.shape[0]
    _check(lib().lora_merge_weight(_ptr(w), _ptr(a), _ptr(b), K, N, r, float(alpha), dtype_code(w.dtype),
                                   dtype_code(factor_dtype), _stream(w)),
           "lora_merge_weight")


def lora_merge_weight_batched(entries, alpha: float) -> None:
    """entries: [(W [N,K] device tensor (merged in place), a [r,K] fp32, b [N,r] fp32, factor_dtype), ...] — one launch."""
    if not entries:
        return
    rows, max_elems = [], 1
    for w, a, b, fdt in entries:
        _require_device(w, a, b)
        N, K = w.shape
        rows.append([w.data_ptr(), a.data_ptr(), b.data_ptr(), K, N, a.shape[0], dtype_code(w.dtype), dtype_code(fdt)])
        max_elems = max(max_elems, N * K)
    dev = entries[0][0].device
    table = torch.tensor(rows, dtype=torch.int64).to(dev)
    _check(lib().lora_merge_weight_batched(_ptr(table), len(rows), max_elems, float(alpha), _stream(entries[0][0])),
           "lora_merge_weight_batched")


def lora_lerp_(x1, x2, alpha: float) -> None:
    """In place x1 ← T(T(alpha·x1) + T((1-alpha)·x2)) on flat device tensors of one dtype (cli_lora_add.py:52-55)."""
    _require_device(x1, x2)
    assert x1.dtype == x2.dtype and x1.numel() == x2.numel() and x1.is_contiguous() and x2.is_contiguous()
    _check(lib().lora_lerp(_ptr(x1), _ptr(x2), x1.numel(), float(alpha), float(1 - alpha), dtype_code(x1.dtype),
                           _stream(x1)), "lora_lerp")


def lora_cast_matrix(src, dst_dtype: torch.dtype, transpose: bool):
    _require_device(src)
    rows, cols = src.shape
    dst = torch.empty((cols, rows) if transpose else (rows, cols), dtype=dst_dtype, device=src.device)
    _check(lib().lora_cast_matrix(_ptr(src), _ptr(dst), rows, cols, dtype_code(src.dtype), dtype_code(dst_dtype),
                                  int(transpose), _stream(src)), "lora_cast_matrix")
    return dst


def lora_grad_sqnorm(grad, grad_mul: float, norm_out) -> None:
    _require_device(grad, norm_out)
    ws = _workspace(grad.device, int(lib().lora_sqnorm_workspace_bytes()), "sqnorm")
    _check(lib().lora_grad_sqnorm(_ptr(grad), grad.numel(), float(grad_mul), _ptr(norm_out), _ptr(ws), _stream(grad)),
           "lora_grad_sqnorm")


def lora_adamw_step(param, grad, exp_avg, exp_avg_sq, norm_in, grad_mul, max_norm, lr, beta1, beta2, eps,
                    weight_decay, step: int) -> None:
    _require_device(param, grad, exp_avg, exp_avg_sq, norm_in)
    _check(lib().lora_adamw_step(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), param.numel(),
                                 _ptr(norm_in), float(grad_mul), float(max_norm), float(lr), float(beta1),
                                 float(beta2), float(eps), float(weight_decay), int(step), _stream(param)),
           "lora_adamw_step")


def lora_adamw_ema_step(param, grad, exp_avg, exp_avg_sq, shadow, norm_in, grad_mul, max_norm, lr, beta1, beta2, eps,
                        weight_decay, step: int, ema_max_decay: float, ema_update_after: int) -> None:
    """`lora_adamw_step` plus, in the same launch, the EMA of the parameters in `shadow` (fp32, like param); the decay follows
    the device's applied-step counter norm_in[2], so `norm_in` is required (include/lora_hip.h)."""
    _require_device(param, grad, exp_avg, exp_avg_sq, shadow, norm_in)
    if shadow.dtype != torch.float32 or shadow.numel() != param.numel() or not shadow.is_contiguous():
        raise ValueError("lora_adamw_ema_step: the shadow must be a contiguous fp32 tensor with the parameters' element count")
    _check(lib().lora_adamw_ema_step(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), _ptr(shadow), param.numel(),
                                     _ptr(norm_in), float(grad_mul), float(max_norm), float(lr), float(beta1), float(beta2),
                                     float(eps), float(weight_decay), int(step), float(ema_max_decay), int(ema_update_after),
                                     _stream(param)), "lora_adamw_ema_step")


def lora_slab_swap(a, b) -> None:
    """Exchanges two flat fp32 device tensors of equal length in place (one launch).  The same buffer twice, or two ranges
    that overlap, raise without a launch."""
    _require_device(a, b)
    if a.dtype != torch.float32 or b.dtype != torch.float32 or a.numel() != b.numel() or not (a.is_contiguous()
                                                                                              and b.is_contiguous()):
        raise ValueError("lora_slab_swap: two contiguous fp32 tensors of equal length")
    _check(lib().lora_slab_swap(_ptr(a), _ptr(b), a.numel(), _stream(a)), "lora_slab_swap")


PRODIGY_MAX_RANGES = 4


def prodigy_ranges(ends, lrs, wds=None):
    """The host arrays `lora_prodigy_moments` / `lora_prodigy_apply` read their ranges from: (int64[k], float[k], float[k] or None)."""
    k = len(ends)
    if not (1 <= k <= PRODIGY_MAX_RANGES) or len(lrs) != k or (wds is not None and len(wds) != k):
        raise ValueError(f"prodigy: 1..{PRODIGY_MAX_RANGES} ranges, each with a learning rate and a weight decay")
    return ((_i64 * k)(*[int(e) for e in ends]), (_f32 * k)(*[float(x) for x in lrs]),
            None if wds is None else (_f32 * k)(*[float(x) for x in wds]))


def _require_prodigy_buffers(what: str, n: int, buffers, norm_in, scalars) -> None:
    """The kernels move 16 bytes per lane over n fp32 elements of every buffer: each must be fp32, contiguous and n long."""
    for name, t in buffers:
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n:
            raise ValueError(f"{what}: `{name}` must be a contiguous fp32 tensor of the parameters' {n} elements; got "
                             f"{t.dtype}, {t.numel()} elements, contiguous {t.is_contiguous()}")
    for name, t, k in (("norm_in", norm_in, 4), ("scalars", scalars, 8)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() < k:
            raise ValueError(f"{what}: `{name}` must be a contiguous fp32 tensor of at least {k} elements")


def lora_prodigy_moments(param, param0, grad, exp_avg, exp_avg_sq, s, ends, lrs, norm_in, scalars, grad_mul, max_norm, beta1,
                         beta2, beta3, d0, d_coef, growth_rate, use_bias_correction: bool, safeguard_warmup: bool) -> None:
    """Phase A of a Prodigy step and the scalar step d → d_new on the device (include/lora_hip.h: lora_prodigy_moments).  All
    buffers fp32, contiguous, of param's length; `ends` / `lrs`: the contiguous ranges and their γ (python sequences)."""
    _require_device(param, param0, grad, exp_avg, exp_avg_sq, s, norm_in, scalars)
    _require_prodigy_buffers("lora_prodigy_moments", param.numel(), (("param", param), ("param0", param0), ("grad", grad),
                                                                     ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq), ("s", s)),
                             norm_in, scalars)
    e, l, _ = prodigy_ranges(ends, lrs)
    ws = _workspace(param.device, int(lib().lora_prodigy_workspace_bytes()), "prodigy")
    _check(lib().lora_prodigy_moments(_ptr(param), _ptr(param0), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), _ptr(s), param.numel(),
                                      e, l, len(ends), _ptr(norm_in), _ptr(scalars), _ptr(ws), float(grad_mul), float(max_norm),
                                      float(beta1), float(beta2), float(beta3), float(d0), float(d_coef), float(growth_rate),
                                      int(bool(use_bias_correction)), int(bool(safeguard_warmup)), _stream(param)),
           "lora_prodigy_moments")


def lora_prodigy_apply(param, exp_avg, exp_avg_sq, shadow, ends, lrs, wds, norm_in, scalars, beta1, beta2, eps,
                       use_bias_correction: bool, ema_max_decay: float = 0.0, ema_update_after: int = 0) -> None:
    """Phase B of a Prodigy step; `shadow` (None: no average) as in `lora_adamw_ema_step` (include/lora_hip.h: lora_prodigy_apply)."""
    _require_device(param, exp_avg, exp_avg_sq, shadow, norm_in, scalars)
    _require_prodigy_buffers("lora_prodigy_apply", param.numel(), (("param", param), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)),
                             norm_in, scalars)
    if shadow is not None and (shadow.dtype != torch.float32 or shadow.numel() != param.numel() or not shadow.is_contiguous()):
        raise ValueError("lora_prodigy_apply: the shadow must be a contiguous fp32 tensor with the parameters' element count")
    e, l, w = prodigy_ranges(ends, lrs, wds)
    _check(lib().lora_prodigy_apply(_ptr(param), _ptr(exp_avg), _ptr(exp_avg_sq), _ptr(shadow), param.numel(), e, l, w, len(ends),
                                    _ptr(norm_in), _ptr(scalars), float(beta1), float(beta2), float(eps),
                                    int(bool(use_bias_correction)), float(ema_max_decay), int(ema_update_after), _stream(param)),
           "lora_prodigy_apply")


MAX_NORM_MAX_RANK = 64


def max_norm_table(rows, device):
    """The device table `lora_max_norm` reads: `rows` = [(up_off, down_off, K, N, r, scale), ...] with element offsets into the
    fp32 buffer the launch gets; the scale travels as the bits of its fp32 value."""
    import struct

    out = []
    for up_off, down_off, K, N, r, scale in rows:
        if not (1 <= int(r) <= MAX_NORM_MAX_RANK) or min(int(up_off), int(down_off)) < 0 or min(int(K), int(N)) < 1:
            raise ValueError(f"lora_max_norm: layer (K={K}, N={N}, r={r}) at ({up_off}, {down_off}) is outside ranks 1..64")
        out.append([int(up_off), int(down_off), int(K), int(N), int(r), struct.unpack("<i", struct.pack("<f", float(scale)))[0], 0, 0])
    return torch.tensor(out, dtype=torch.int64).to(device)


def lora_max_norm(params, table, max_r: int, max_norm: float, stats, counters=None) -> None:
    """Per layer of `table` (max_norm_table): stats[l] = (‖scale·up·down‖_F before, factor applied), and the factors of a layer
    above `max_norm` scaled by sqrt(max_norm/norm) in place; math.inf measures only (include/lora_hip.h: lora_max_norm)."""
    _require_device(params, table, stats, counters)
    n_layers = table.shape[0]
    if params.dtype != torch.float32 or not params.is_contiguous():
        raise ValueError("lora_max_norm: `params` must be a contiguous fp32 tensor")
    if table.dtype != torch.int64 or table.dim() != 2 or table.shape[1] != 8 or not table.is_contiguous():
        raise ValueError("lora_max_norm: `table` must be a contiguous int64 [n_layers, 8] tensor")
    if stats.dtype != torch.float32 or stats.numel() != 2 * n_layers or not stats.is_contiguous():
        raise ValueError("lora_max_norm: `stats` must be a contiguous fp32 tensor of 2 values per layer")
    if counters is not None and (counters.dtype != torch.int32 or counters.numel() < 1):
        raise ValueError("lora_max_norm: `counters` must be an int32 tensor")
    _check(lib().lora_max_norm(_ptr(params), _ptr(table), n_layers, int(max_r), float(max_norm), _ptr(stats), _ptr(counters),
                               _stream(params)), "lora_max_norm")


def ddpm_add_noise(x0, eps, t, sqrt_acp, sqrt_1macp, out_dtype: torch.dtype, v_prediction: bool, want_target=True):
    _require_device(x0, eps, t, sqrt_acp, sqrt_1macp)
    B = x0.shape[0]
    per_row = x0[0].numel()
    noisy = torch.empty(x0.shape, dtype=out_dtype, device=x0.device)
    target = torch.empty(x0.shape, dtype=out_dtype, device=x0.device) if want_target else None
    _check(lib().ddpm_add_noise(_ptr(x0), _ptr(eps), _ptr(t), _ptr(sqrt_acp), _ptr(sqrt_1macp), _ptr(noisy),
                                _ptr(target), B, per_row, int(v_prediction), dtype_code(out_dtype), _stream(x0)),
           "ddpm_add_noise")
    return noisy, target


def ddpm_noise_prologue(x0, sqrt_acp, sqrt_1macp, out_dtype: torch.dtype, seed: int, step: int, v_prediction: bool,
                        n_timesteps: int = 1000, want_draw: bool = False):
    """Draws eps/t on the device (Philox keyed by seed, step) and returns (noisy, target, t[, eps])."""
    _require_device(x0, sqrt_acp, sqrt_1macp)
    B = x0.shape[0]
    per_row = x0[0].numel()
    noisy = torch.empty(x0.shape, dtype=out_dtype, device=x0.device)
    target = torch.empty(x0.shape, dtype=out_dtype, device=x0.device)
    t = torch.empty(B, dtype=torch.int64, device=x0.device)
    eps = torch.empty(x0.shape, dtype=torch.float32, device=x0.device) if want_draw else None
    _check(lib().ddpm_noise_prologue(_ptr(x0), _ptr(sqrt_acp), _ptr(sqrt_1macp), _ptr(noisy), _ptr(target), _ptr(eps),
                                     _ptr(t), B, per_row, int(n_timesteps), int(seed) & (2**64 - 1),
                                     int(step) & (2**64 - 1), int(v_prediction), dtype_code(out_dtype), _stream(x0)),
           "ddpm_noise_prologue")
    return (noisy, target, t, eps) if want_draw else (noisy, target, t)


def _moments_rows(moments):
    """(B, per_row, latent shape) of VAE moments [B, 2C, ...]: row b = mean [per_row] | logvar [per_row]."""
    if moments.dim() < 2 or moments.shape[1] % 2 or not moments.is_contiguous():
        raise ValueError(f"moments must be a contiguous [B, 2C, ...] tensor (mean | logvar); got {tuple(moments.shape)}, "
                         f"strides {moments.stride()}")
    shape = (moments.shape[0], moments.shape[1] // 2) + tuple(moments.shape[2:])
    return moments.shape[0], moments[0].numel() // 2, shape


def ddpm_posterior_prologue(moments, sqrt_acp, sqrt_1macp, out_dtype: torch.dtype, seed: int, step: int, v_prediction: bool,
                            n_timesteps: int = 1000, scale: float = 0.18215, want_draw: bool = False, want_target: bool = True):
    """Draws the latents from the VAE moments [B, 2C, h, w] (f32 / f16 / bf16), eps and t on the device (Philox keyed by seed,
    step) in one launch and returns (noisy, target, t[, x0, z, eps]) — include/lora_hip.h: ddpm_posterior_prologue."""
    _require_device(moments, sqrt_acp, sqrt_1macp)
    B, per_row, shape = _moments_rows(moments)
    dev = moments.device
    noisy = torch.empty(shape, dtype=out_dtype, device=dev)
    target = torch.empty(shape, dtype=out_dtype, device=dev) if want_target else None
    t = torch.empty(B, dtype=torch.int64, device=dev)
    x0, z, eps = (torch.empty(shape, dtype=torch.float32, device=dev) for _ in range(3)) if want_draw else (None, None, None)
    _check(lib().ddpm_posterior_prologue(_ptr(moments), dtype_code(moments.dtype), _ptr(sqrt_acp), _ptr(sqrt_1macp), _ptr(noisy),
                                         _ptr(target), _ptr(x0), _ptr(z), _ptr(eps), _ptr(t), B, per_row, int(n_timesteps),
                                         float(scale), int(seed) & (2**64 - 1), int(step) & (2**64 - 1), int(v_prediction),
                                         dtype_code(out_dtype), _stream(moments)),
           "ddpm_posterior_prologue")
    return (noisy, target, t, x0, z, eps) if want_draw else (noisy, target, t)


def _channel_plane(shape) -> int:
    """h·w of a [B, C, h, w] latent shape: what one offset-noise normal covers."""
    if len(shape) != 4:
        raise ValueError(f"offset noise needs [B, C, h, w] latents; got {tuple(shape)}")
    return int(shape[2]) * int(shape[3])


def ddpm_noise_prologue_offset(x0, sqrt_acp, sqrt_1macp, out_dtype: torch.dtype, seed: int, step: int, v_prediction: bool,
                               n_timesteps: int = 1000, noise_offset: float = 0.0, want_draw: bool = False):
    """`ddpm_noise_prologue` with eps' = eps + noise_offset·ξ[b, c], ξ one normal per (row, channel) from Philox stream 3 of
    the same key; returns (noisy, target, t[, eps', ξ [B, C]]) — include/lora_hip.h: ddpm_noise_prologue_offset."""
    _require_device(x0, sqrt_acp, sqrt_1macp)
    B = x0.shape[0]
    per_row = x0[0].numel()
    hw = _channel_plane(x0.shape)
    noisy = torch.empty(x0.shape, dtype=out_dtype, device=x0.device)
    target = torch.empty(x0.shape, dtype=out_dtype, device=x0.device)
    t = torch.empty(B, dtype=torch.int64, device=x0.device)
    eps = torch.empty(x0.shape, dtype=torch.float32, device=x0.device) if want_draw else None
    xi = torch.empty(x0.shape[:2], dtype=torch.float32, device=x0.device) if want_draw else None
    _check(lib().ddpm_noise_prologue_offset(_ptr(x0), _ptr(sqrt_acp), _ptr(sqrt_1macp), _ptr(noisy), _ptr(target), _ptr(eps),
                                            _ptr(t), B, per_row, int(n_timesteps), int(seed) & (2**64 - 1),
                                            int(step) & (2**64 - 1), int(v_prediction), dtype_code(out_dtype), hw,
                                            float(noise_offset), _ptr(xi), _stream(x0)),
           "ddpm_noise_prologue_offset")
    return (noisy, target, t, eps, xi) if want_draw else (noisy, target, t)


def ddpm_posterior_prologue_offset(moments, sqrt_acp, sqrt_1macp, out_dtype: torch.dtype, seed: int, step: int,
                                   v_prediction: bool, n_timesteps: int = 1000, scale: float = 0.18215,
                                   noise_offset: float = 0.0, want_draw: bool = False, want_target: bool = True):
    """`ddpm_posterior_prologue` with the offset noise of `ddpm_noise_prologue_offset`; returns (noisy, target, t[, x0, z,
    eps', ξ [B, C]]) — include/lora_hip.h: ddpm_posterior_prologue_offset."""
    _require_device(moments, sqrt_acp, sqrt_1macp)
    B, per_row, shape = _moments_rows(moments)
    hw = _channel_plane(shape)
    dev = moments.device
    noisy = torch.empty(shape, dtype=out_dtype, device=dev)
    target = torch.empty(shape, dtype=out_dtype, device=dev) if want_target else None
    t = torch.empty(B, dtype=torch.int64, device=dev)
    x0, z, eps = (torch.empty(shape, dtype=torch.float32, device=dev) for _ in range(3)) if want_draw else (None, None, None)
    xi = torch.empty(shape[:2], dtype=torch.float32, device=dev) if want_draw else None
    _check(lib().ddpm_posterior_prologue_offset(_ptr(moments), dtype_code(moments.dtype), _ptr(sqrt_acp), _ptr(sqrt_1macp),
                                                _ptr(noisy), _ptr(target), _ptr(x0), _ptr(z), _ptr(eps), _ptr(t), B, per_row,
                                                int(n_timesteps), float(scale), int(seed) & (2**64 - 1),
                                                int(step) & (2**64 - 1), int(v_prediction), dtype_code(out_dtype), hw,
                                                float(noise_offset), _ptr(xi), _stream(moments)),
           "ddpm_posterior_prologue_offset")
    return (noisy, target, t, x0, z, eps, xi) if want_draw else (noisy, target, t)


def ddpm_posterior_sample(moments, z, scale: float = 0.18215):
    """x0 = (mean + exp(0.5·clamp(logvar, −30, 20))·z)·scale, fp32, from the caller's fp32 z (shaped like the latents)."""
    _require_device(moments, z)
    B, per_row, shape = _moments_rows(moments)
    if z.dtype != torch.float32 or tuple(z.shape) != shape or not z.is_contiguous():
        raise ValueError(f"the posterior noise must be a contiguous fp32 {shape} tensor; got {z.dtype} {tuple(z.shape)}")
    x0 = torch.empty(shape, dtype=torch.float32, device=moments.device)
    _check(lib().ddpm_posterior_sample(_ptr(moments), dtype_code(moments.dtype), _ptr(z), _ptr(x0), B, per_row, float(scale),
                                       _stream(moments)),
           "ddpm_posterior_sample")
    return x0


class SampleState:
    """The device buffers of one sampling run (include/lora_hip.h: ddpm_sample_*): the fp32 state `x` [B, ...], the model
    input [rows, ...] in `dtype` and its timestep tensor [rows] (rows = 2B under guidance: the same rows twice), the cursor
    (int32 [2]: the denoising-step index and the seed's low word, both read by the step launch from device memory), and the
    schedule's tables.  `alloc` makes them; a caller may also hand in views of its own (tests: odd offsets).
    Optional, for image-to-image runs (ddpm_sample_init_from, ddpm_sample_*_keep): `init` fp32 like x, the start image's latents
    in model space; `mask` fp32 [B, 1, h, w] (any [B, ...] of hw elements with per_row % hw == 0) and `keep_coef` fp32 [S, 2] =
    (k, n) per table row (sampling.keep_schedule) — a mask needs both others."""

    init = mask = keep_coef = None
    shared_noise = False  # True: the `_shared` entries — every sample takes the draws of the B = 1 run of the same seed

    def _entry(self, name: str):
        """The library entry `name`, or its `_shared` form when the state draws shared noise."""
        return getattr(lib(), name + "_shared" if self.shared_noise else name)

    def _set_keep(self, x, S, init, mask, keep_coef):
        B, per_row = x.shape[0], x[0].numel()
        if init is not None and (init.dtype != torch.float32 or init.shape != x.shape or not init.is_contiguous()):
            raise ValueError(f"sampler buffers: init must be a contiguous fp32 {tuple(x.shape)} tensor; got {init.dtype} "
                             f"{tuple(init.shape)}")
        if mask is not None:
            if init is None or keep_coef is None:
                raise ValueError("sampler buffers: a keep mask needs init and keep_coef")
            if (mask.dtype != torch.float32 or mask.dim() < 2 or mask.shape[0] != B or not mask.is_contiguous() or
                    per_row % mask[0].numel() != 0):
                raise ValueError(f"sampler buffers: mask must be a contiguous fp32 [B, 1, h, w] tensor for the state "
                                 f"{tuple(x.shape)}; got {mask.dtype} {tuple(mask.shape)}")
        if keep_coef is not None and (keep_coef.dtype != torch.float32 or tuple(keep_coef.shape) != (S, 2) or
                                      not keep_coef.is_contiguous()):
            raise ValueError(f"sampler buffers: keep_coef must be a contiguous fp32 [{S}, 2] tensor")
        _require_device(init, mask, keep_coef)
        self.init, self.mask, self.keep_coef = init, mask, keep_coef
        self.hw = None if mask is None else mask[0].numel()

    # What a subclass changes: the dtype of t_model / timesteps, the width of a coef row, what the dtype error says, and the
    # buffers it adds (_HistoryState below).
    T_DTYPE, COEF_WIDTH = torch.int64, 3
    KINDS = "x fp32, t_model / timesteps int64, cursor int32 [2], coef fp32 [S, 3]"
    _own = ()

    def _own_shapes_ok(self, x) -> bool:
        return True

    def _own_kinds_ok(self, S, timesteps) -> bool:
        return True

    def _own_shapes(self) -> str:
        return ""

    def __init__(self, x, model_in, t_model, cursor, timesteps, coef, cfg: bool, init=None, mask=None, keep_coef=None):
        B, rows, S = x.shape[0], model_in.shape[0], timesteps.shape[0]
        if (rows != (2 * B if cfg else B) or model_in.shape[1:] != x.shape[1:] or t_model.shape != (rows,) or
                not self._own_shapes_ok(x)):
            raise ValueError(f"sampler buffers disagree: state {tuple(x.shape)}, {self._own_shapes()}model input "
                             f"{tuple(model_in.shape)}, timesteps {tuple(t_model.shape)}, guidance {cfg}")
        if (x.dtype != torch.float32 or t_model.dtype != self.T_DTYPE or cursor.dtype != torch.int32 or cursor.numel() != 2 or
                timesteps.dtype != self.T_DTYPE or coef.dtype != torch.float32 or tuple(coef.shape) != (S, self.COEF_WIDTH) or
                S < 1 or not self._own_kinds_ok(S, timesteps)):
            raise ValueError("sampler buffers: " + self.KINDS)
        for t in (x, model_in, t_model, timesteps, coef, *self._own):
            if not t.is_contiguous():
                raise ValueError("sampler buffers must be contiguous")
        self._set_keep(x, S, init, mask, keep_coef)
        _require_device(x, model_in, t_model, cursor, timesteps, coef, *self._own)
        self.x, self.model_in, self.t_model, self.cursor, self.timesteps, self.coef = x, model_in, t_model, cursor, timesteps, coef
        self.cfg, self.B, self.per_row, self.S = bool(cfg), B, x[0].numel(), S

    @classmethod
    def _alloc_run(cls, shape, dtype, cfg, device):
        """(x, model_in, t_model, cursor) of a run."""
        rows = (2 if cfg else 1) * shape[0]
        return (torch.empty(shape, dtype=torch.float32, device=device),
                torch.empty((rows, *shape[1:]), dtype=dtype, device=device),
                torch.empty(rows, dtype=cls.T_DTYPE, device=device), torch.zeros(2, dtype=torch.int32, device=device))

    @staticmethod
    def _alloc_keep(shape, n_rows, device, with_init, with_mask):
        """(init, mask, keep_coef) buffers of an image-to-image run, None where not asked for."""
        if with_mask and not with_init:
            raise ValueError("sampler buffers: a keep mask needs init")
        return (torch.empty(shape, dtype=torch.float32, device=device) if with_init else None,
                torch.empty((shape[0], 1, *shape[2:]), dtype=torch.float32, device=device) if with_mask else None,
                torch.zeros((n_rows, 2), dtype=torch.float32, device=device) if with_mask else None)

    @classmethod
    def alloc(cls, shape, dtype: torch.dtype, cfg: bool, timesteps, coef, device, with_init: bool = False,
              with_mask: bool = False):
        """`shape`: of the state, [B, C, h, w]; `timesteps` / `coef`: host or device tensors of sampler_schedule."""
        return cls(*cls._alloc_run(shape, dtype, cfg, device), timesteps.to(device).contiguous(), coef.to(device).contiguous(),
                   cfg, *cls._alloc_keep(shape, timesteps.shape[0], device, with_init, with_mask))


def _require_model_out(st, model_out) -> None:
    if model_out.dtype != st.model_in.dtype or model_out.shape != st.model_in.shape or not model_out.is_contiguous():
        raise ValueError(f"the model output must be a contiguous {st.model_in.dtype} {tuple(st.model_in.shape)} tensor; got "
                         f"{model_out.dtype} {tuple(model_out.shape)}, strides {model_out.stride()}")


def _require_like_state(st, name: str, t) -> None:
    """`t` (z_out, eps_out: optional outputs shaped like the state) is None or a contiguous fp32 tensor of the state's shape."""
    if t is not None and (t.dtype != torch.float32 or t.shape != st.x.shape or not t.is_contiguous()):
        raise ValueError(f"{name} must be a contiguous fp32 {tuple(st.x.shape)} tensor")


def ddpm_sample_init(st: SampleState, seed: int) -> None:
    """x_T ~ N(0,1) (Philox stream 3, key (seed, 0)) into the state, the first model input and timestep tensor, cursor = 0."""
    _check(st._entry("ddpm_sample_init")(_ptr(st.x), _ptr(st.model_in), _ptr(st.t_model), _ptr(st.cursor), _ptr(st.timesteps), st.B,
                                  st.per_row, st.S, int(st.cfg), int(seed) & (2**64 - 1), dtype_code(st.model_in.dtype),
                                  _stream(st.x)),
           "ddpm_sample_init")


def ddpm_sample_step(st: SampleState, model_out, guidance_scale: float, z_out=None) -> None:
    """One denoising step at the device-resident cursor (and seed): guidance, x ← a·x + b·o + σ·z in place, the next model input and
    timestep tensor.  `model_out` [rows, ...] in the model input's dtype.  Does not move the cursor: ddpm_sample_advance."""
    _require_device(model_out, z_out)
    _require_model_out(st, model_out)
    _require_like_state(st, "z_out", z_out)
    _check(st._entry("ddpm_sample_step")(_ptr(st.x), _ptr(model_out), _ptr(st.model_in), _ptr(st.t_model), _ptr(st.cursor),
                                  _ptr(st.timesteps), _ptr(st.coef), _ptr(z_out), st.B, st.per_row, st.S, int(st.cfg),
                                  float(guidance_scale), dtype_code(model_out.dtype), _stream(st.x)),
           "ddpm_sample_step")


def ddpm_sample_init_from(st: SampleState, seed: int, start: int, k: float, n: float, eps_out=None) -> None:
    """x = fp32(k·init) + fp32(n·ε) with ε the x_T draw of `ddpm_sample_init` at equal seed, from `st.init`; the first model input,
    t_model = timesteps[start], cursor = {start, seed}.  `eps_out` (fp32 like x) gets ε."""
    if st.init is None:
        raise ValueError("ddpm_sample_init_from: the state has no init buffer")
    _require_device(eps_out)
    _require_like_state(st, "eps_out", eps_out)
    _check(st._entry("ddpm_sample_init_from")(_ptr(st.x), _ptr(st.model_in), _ptr(st.t_model), _ptr(st.cursor), _ptr(st.timesteps),
                                       _ptr(st.init), _ptr(eps_out), st.B, st.per_row, st.S, int(start), float(k), float(n),
                                       int(st.cfg), int(seed) & (2**64 - 1), dtype_code(st.model_in.dtype), _stream(st.x)),
           "ddpm_sample_init_from")


def _require_mask(st, what: str) -> None:
    if st.mask is None:
        raise ValueError(f"{what}: the state has no keep mask")


def ddpm_sample_step_keep(st: SampleState, model_out, guidance_scale: float, z_out=None) -> None:
    """`ddpm_sample_step`, then x ← fp32(m·y) + fp32((1−m)·x') with y = fp32(k_i·init) + fp32(n_i·ε) from `st.mask`, `st.init`,
    `st.keep_coef` and the run's start draw; the model input is the blended state."""
    _require_mask(st, "ddpm_sample_step_keep")
    _require_device(model_out, z_out)
    _require_model_out(st, model_out)
    _require_like_state(st, "z_out", z_out)
    _check(st._entry("ddpm_sample_step_keep")(_ptr(st.x), _ptr(model_out), _ptr(st.model_in), _ptr(st.t_model), _ptr(st.cursor),
                                       _ptr(st.timesteps), _ptr(st.coef), _ptr(z_out), _ptr(st.mask), _ptr(st.init),
                                       _ptr(st.keep_coef), st.B, st.per_row, st.hw, st.S, int(st.cfg), float(guidance_scale),
                                       dtype_code(model_out.dtype), _stream(st.x)),
           "ddpm_sample_step_keep")


def ddpm_sample_advance(st: SampleState) -> None:
    """cursor += 1 (up to S), a one-thread launch behind the step that read it."""
    _check(lib().ddpm_sample_advance(_ptr(st.cursor), st.S, _stream(st.x)), "ddpm_sample_advance")


class _HistoryState(SampleState):
    """What MultistepState and SigmaState add to SampleState alike: the saved state `xs` (fp32, like x), the history `hist`
    (fp32, HIST_SLOTS + the state's shape) and `plan` int32 [I, 5], checked inside SampleState's constructor."""

    HIST_SLOTS = ()

    def __init__(self, x, xs, hist, model_in, t_model, cursor, timesteps, coef, plan, cfg: bool, init=None, mask=None,
                 keep_coef=None):
        self.xs, self.hist, self.plan = self._own = xs, hist, plan
        super().__init__(x, model_in, t_model, cursor, timesteps, coef, cfg, init, mask, keep_coef)

    def _own_shapes_ok(self, x) -> bool:
        return self.xs.shape == x.shape and tuple(self.hist.shape) == (*self.HIST_SLOTS, *x.shape)

    def _own_kinds_ok(self, S, timesteps) -> bool:
        return (self.xs.dtype == torch.float32 and self.hist.dtype == torch.float32 and self.plan.dtype == torch.int32 and
                tuple(self.plan.shape) == (S, 5))

    def _own_shapes(self) -> str:
        return f"saved state {tuple(self.xs.shape)}, history {tuple(self.hist.shape)}, "

    @classmethod
    def alloc(cls, shape, dtype: torch.dtype, cfg: bool, timesteps, coef, plan, device, with_init: bool = False,
              with_mask: bool = False):
        """`shape`: of the state, [B, C, h, w]; `timesteps` / `coef` / `plan`: host or device tensors of the class's schedule
        (sampling.multistep_schedule, sampling.sigma_schedule)."""
        x, *run = cls._alloc_run(shape, dtype, cfg, device)
        return cls(x, torch.empty_like(x), torch.empty((*cls.HIST_SLOTS, *shape), dtype=torch.float32, device=device), *run,
                   timesteps.to(device).contiguous(), coef.to(device).contiguous(), plan.to(device).contiguous(), cfg,
                   *cls._alloc_keep(shape, timesteps.shape[0], device, with_init, with_mask))


class MultistepState(_HistoryState):
    """SampleState for the linear multistep methods (include/lora_hip.h: ddpm_sample_multistep): next to its buffers the saved
    state `xs` (fp32, like x), the history ring `hist` (fp32 [4, B, ...]), `coef` fp32 [I, 7] = (p, q, a, c0..c3) and `plan`
    int32 [I, 5] = (w, s1, s2, s3, flags) of sampling.multistep_schedule.  `S` is I, the number of model evaluations, so
    ddpm_sample_init and ddpm_sample_advance serve it as they are.  `xs` and `hist` need no clearing."""

    COEF_WIDTH, HIST_SLOTS = 7, (4,)
    KINDS = "x / xs / hist fp32, t_model / timesteps int64, cursor int32 [2], coef fp32 [I, 7], plan int32 [I, 5]"


def ddpm_sample_multistep(st: MultistepState, model_out, guidance_scale: float) -> None:
    """One multistep iteration at the device-resident cursor: guidance, h = p·x + q·o, x ← a·base + c0·h + Σ c_k·H[s_k] in
    place, the saved state and the pushed history slot as plan[i] says, the next model input and timestep tensor.  `model_out`
    [rows, ...] in the model input's dtype.  Does not move the cursor: ddpm_sample_advance."""
    _require_device(model_out)
    _require_model_out(st, model_out)
    _check(lib().ddpm_sample_multistep(_ptr(st.x), _ptr(st.xs), _ptr(st.hist), _ptr(model_out), _ptr(st.model_in),
                                       _ptr(st.t_model), _ptr(st.cursor), _ptr(st.timesteps), _ptr(st.coef), _ptr(st.plan),
                                       st.B, st.per_row, st.S, int(st.cfg), float(guidance_scale),
                                       dtype_code(model_out.dtype), _stream(st.x)),
           "ddpm_sample_multistep")


def ddpm_sample_multistep_keep(st: MultistepState, model_out, guidance_scale: float) -> None:
    """`ddpm_sample_multistep`, then the keep blend of `ddpm_sample_step_keep` on the state it produced (SAVE and PUSH read the
    state before the update, as they do without a mask)."""
    _require_mask(st, "ddpm_sample_multistep_keep")
    _require_device(model_out)
    _require_model_out(st, model_out)
    _check(st._entry("ddpm_sample_multistep_keep")(_ptr(st.x), _ptr(st.xs), _ptr(st.hist), _ptr(model_out), _ptr(st.model_in),
                                            _ptr(st.t_model), _ptr(st.cursor), _ptr(st.timesteps), _ptr(st.coef),
                                            _ptr(st.plan), _ptr(st.mask), _ptr(st.init), _ptr(st.keep_coef), st.B, st.per_row,
                                            st.hw, st.S, int(st.cfg), float(guidance_scale), dtype_code(model_out.dtype),
                                            _stream(st.x)),
           "ddpm_sample_multistep_keep")


class SigmaState(_HistoryState):
    """SampleState for the sigma-space methods (include/lora_hip.h: ddpm_sample_sigma): the saved state `xs` and the ONE history
    slot `hist` (fp32, like x), `t_model` [rows] and `timesteps` [I] in FP32 — the grid is fractional — `coef` fp32 [I, 8] = (p, q,
    a, c0, c1, s, n, σ_eval) and `plan` int32 [I, 5] of sampling.sigma_schedule.  `S` is I, the number of model evaluations, so
    ddpm_sample_advance serves it as it is.  `xs` and `hist` need no clearing."""

    T_DTYPE, COEF_WIDTH = torch.float32, 8
    KINDS = "x / xs / hist fp32, t_model / timesteps fp32, cursor int32 [2], coef fp32 [I, 8], plan int32 [I, 5]"

    def _own_kinds_ok(self, S, timesteps) -> bool:
        return super()._own_kinds_ok(S, timesteps) and timesteps.dim() == 1

    @classmethod
    def alloc(cls, shape, dtype: torch.dtype, cfg: bool, timesteps, coef, plan, device, with_init: bool = False,
              with_mask: bool = False):
        """As _HistoryState.alloc, with sigma_schedule's float64 timesteps rounded to fp32 here."""
        return super().alloc(shape, dtype, cfg, timesteps.to(torch.float32), coef, plan, device, with_init, with_mask)


def ddpm_sample_sigma_init(st: SigmaState, seed: int, start: int, k: float, nn: float, c_in: float, from_init: bool = False,
                           eps_out=None) -> None:
    """The start of a sigma-space run at table row `start`: x = fp32(nn·ε), or fp32(k·init) + fp32(nn·ε) from `st.init` with
    `from_init`; ε the x_T draw of `ddpm_sample_init` at equal seed; model input cast(fp32(c_in·x)), t_model = timesteps[start],
    cursor = {start, seed}.  `eps_out` (fp32 like x) gets ε."""
    if from_init and st.init is None:
        raise ValueError("ddpm_sample_sigma_init: the state has no init buffer")
    _require_device(eps_out)
    _require_like_state(st, "eps_out", eps_out)
    _check(lib().ddpm_sample_sigma_init(_ptr(st.x), _ptr(st.model_in), _ptr(st.t_model), _ptr(st.cursor), _ptr(st.timesteps),
                                        _ptr(st.init) if from_init else 0, _ptr(eps_out), st.B, st.per_row, st.S, int(start),
                                        float(k), float(nn), float(c_in), int(st.cfg), int(st.shared_noise),
                                        int(seed) & (2**64 - 1), dtype_code(st.model_in.dtype), _stream(st.x)),
           "ddpm_sample_sigma_init")


def ddpm_sample_sigma(st: SigmaState, model_out, guidance_scale: float, z_out=None, keep: bool = False) -> None:
    """One sigma-space iteration at the device-resident cursor (and seed): guidance, h = p·x + q·o, x ← a·base + c0·h + c1·H +
    s·z in place, the saved state and the history slot as plan[i] says, with `keep` the blend of `ddpm_sample_step_keep` on the
    state produced, then the next model input cast(fp32(n·x)) and the fp32 timestep tensor.  `model_out` [rows, ...] in the
    model input's dtype.  Does not move the cursor: ddpm_sample_advance."""
    if keep:
        _require_mask(st, "ddpm_sample_sigma")
    _require_device(model_out, z_out)
    _require_model_out(st, model_out)
    _require_like_state(st, "z_out", z_out)
    _check(lib().ddpm_sample_sigma(_ptr(st.x), _ptr(st.xs), _ptr(st.hist), _ptr(model_out), _ptr(st.model_in), _ptr(st.t_model),
                                   _ptr(st.cursor), _ptr(st.timesteps), _ptr(st.coef), _ptr(st.plan), _ptr(z_out),
                                   _ptr(st.mask) if keep else 0, _ptr(st.init) if keep else 0,
                                   _ptr(st.keep_coef) if keep else 0, st.B, st.per_row, st.hw if keep else 1, st.S, int(st.cfg),
                                   int(st.shared_noise), float(guidance_scale), dtype_code(model_out.dtype), _stream(st.x)),
           "ddpm_sample_sigma")


def ddpm_cfg_rescale(st: SampleState, model_out, guidance_scale: float, rescale: float, k_out=None) -> None:
    """The guidance rescale of a guided iteration, in front of its step launch: both halves of `model_out` [2B, ...] (the model
    input's dtype, unconditional rows first) are multiplied in place by k_b = rescale·σ(c)/σ(o) + (1 − rescale), o the guided
    output of sample b (include/lora_hip.h: ddpm_cfg_rescale).  `k_out` (fp32 [B]) gets k.  Serves every state class."""
    if not st.cfg:
        raise ValueError("ddpm_cfg_rescale: the state has no guidance rows (a single pass has nothing to rescale)")
    _require_device(model_out, k_out)
    _require_model_out(st, model_out)
    if k_out is not None and (k_out.dtype != torch.float32 or tuple(k_out.shape) != (st.B,) or not k_out.is_contiguous()):
        raise ValueError(f"k_out must be a contiguous fp32 [{st.B}] tensor")
    _check(lib().ddpm_cfg_rescale(_ptr(model_out), _ptr(k_out), st.B, st.per_row, float(guidance_scale), float(rescale),
                                  dtype_code(model_out.dtype), _stream(st.x)),
           "ddpm_cfg_rescale")


def embed_rows_fwd(table, ids, out_dtype: torch.dtype):
    """table [V,D] fp32, ids int64 (any shape) → rows [*ids.shape, D] in out_dtype (include/lora_hip.h: embed_rows_fwd)."""
    _require_device(table, ids)
    V, D = table.shape
    flat = ids.reshape(-1)
    flat = flat if flat.is_contiguous() else flat.contiguous()
    out = torch.empty((flat.numel(), D), dtype=out_dtype, device=table.device)
    _check(lib().embed_rows_fwd(_ptr(table), _ptr(flat), _ptr(out), flat.numel(), D, V, dtype_code(out_dtype), _stream(table)),
           "embed_rows_fwd")
    return out.view(*ids.shape, D)


def embed_rows_bwd(d_rows, ids, grad_table, accumulate: bool = False, active=None) -> None:
    """grad_table[t] (+)= Σ of the rows d_rows[p] with ids[p] == t, positions in ascending order (deterministic);
    active [V] uint8 (optional): set to 1 for every token that occurs."""
    _require_device(d_rows, ids, grad_table, active)
    V, D = grad_table.shape
    assert d_rows.is_contiguous() and ids.is_contiguous() and d_rows.numel() == ids.numel() * D
    assert active is None or (active.dtype == torch.uint8 and active.numel() == V)
    _check(lib().embed_rows_bwd(_ptr(d_rows), _ptr(ids), _ptr(grad_table), _ptr(active), ids.numel(), D, V,
                                dtype_code(d_rows.dtype), int(accumulate), _stream(d_rows)), "embed_rows_bwd")


def lora_adamw_rows(param, grad, exp_avg, exp_avg_sq, active, norm_in, grad_mul, max_norm, lr, beta1, beta2, eps,
                    weight_decay, step: int) -> None:
    """AdamW over a [V, D] table whose rows outside `active` never had a gradient (include/lora_hip.h: lora_adamw_rows)."""
    _require_device(param, grad, exp_avg, exp_avg_sq, active, norm_in)
    V, D = param.shape
    _check(lib().lora_adamw_rows(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), _ptr(active), V, D, _ptr(norm_in),
                                 float(grad_mul), float(max_norm), float(lr), float(beta1), float(beta2), float(eps),
                                 float(weight_decay), int(step), _stream(param)), "lora_adamw_rows")


TI_MAX_ROWS = 64  # LORA_TI_MAX_ROWS


def ti_rows_grad(d_rows, ids, slot_ids, grad, accumulate: bool = True) -> None:
    """grad [P, D] fp32 (+)= for each slot s the sum of the rows d_rows[p] with ids[p] == slot_ids[s], positions in ascending
    order (include/lora_hip.h: ti_rows_grad)."""
    _require_device(d_rows, ids, slot_ids, grad)
    P, D = grad.shape
    assert grad.dtype == torch.float32 and grad.is_contiguous() and slot_ids.dtype == torch.int64 and slot_ids.numel() == P
    assert d_rows.is_contiguous() and ids.is_contiguous() and ids.dtype == torch.int64 and d_rows.numel() == ids.numel() * D
    _check(lib().ti_rows_grad(_ptr(d_rows), _ptr(ids), ids.numel(), D, _ptr(slot_ids), P, _ptr(grad), dtype_code(d_rows.dtype),
                              int(accumulate), _stream(grad)), "ti_rows_grad")


def ti_rows_adamw_decay(table, slot_ids, grad, exp_avg, exp_avg_sq, grad_mul, lr, beta1, beta2, eps, weight_decay, step: int,
                        decay_lambda: float, target_norm: float = 0.4) -> None:
    """AdamW + clip_ti_decay (decay_lambda < 0: no decay) on the rows table[slot_ids] in place (include/lora_hip.h:
    ti_rows_adamw_decay)."""
    _require_device(table, slot_ids, grad, exp_avg, exp_avg_sq)
    V, D = table.shape
    P = slot_ids.numel()
    assert table.dtype == torch.float32 and table.is_contiguous() and slot_ids.dtype == torch.int64
    for t in (grad, exp_avg, exp_avg_sq):
        assert t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (P, D)
    _check(lib().ti_rows_adamw_decay(_ptr(table), V, D, _ptr(slot_ids), P, _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq),
                                     float(grad_mul), float(lr), float(beta1), float(beta2), float(eps), float(weight_decay),
                                     int(step), float(decay_lambda), float(target_norm), _stream(table)), "ti_rows_adamw_decay")


DISTILL_NARROW_MAX_RANK = 16  # the width-32 kernels (lora_distill_*); above it the lora_distill_wide_* entries
DISTILL_MAX_RANK = 64


def distill_width(r: int) -> int:
    """Block width (columns of the Y, Z, V blocks) the svd_distill kernels run rank r at."""
    if r <= DISTILL_NARROW_MAX_RANK:
        return 32
    w = lib().lora_distill_wide_width(r)
    if w < 0:
        _check(w, "lora_distill_wide_width")
    return w


class DistillKernels:
    """The svd_distill kernel set that solves rank r (include/lora_hip.h: lora_distill_* for r <= 16, lora_distill_wide_*
    above, whose layout depends on r).  The C entries are resolved here, once per solve, so that a launch costs what a direct
    call of the entry costs."""

    def __init__(self, r: int):
        self.r = r = int(r)
        wide = r > DISTILL_NARROW_MAX_RANK
        self._prefix = "lora_distill_wide_" if wide else "lora_distill_"
        self._r = (r,) if wide else ()  # the rank, where only the wide entry takes it
        handle = lib()
        self._ws_bytes, self._start, self._diff, self._rr, self._finalize = (
            getattr(handle, self._prefix + n) for n in ("workspace_bytes", "start", "diff", "rayleigh_ritz", "finalize"))

    def workspace_bytes(self, N: int, K: int) -> int:
        """Bytes of the per-layer workspace."""
        return int(self._ws_bytes(N, K, *self._r))

    def start(self, table, n_layers: int, min_nk: int, seed: int, ws) -> None:
        _check(self._start(_ptr(table), n_layers, min_nk, self.r, seed, _ptr(ws), _stream(ws)), self._prefix + "start")

    def diff(self, table, n_layers: int, max_rows: int, transpose: bool, dtype: torch.dtype, ws) -> None:
        _check(self._diff(_ptr(table), n_layers, max_rows, int(transpose), dtype_code(dtype), *self._r, _ptr(ws), _stream(ws)),
               self._prefix + "diff")

    def rayleigh_ritz(self, table, n_layers: int, side: int, tol: float, last: bool, ws) -> None:
        _check(self._rr(_ptr(table), n_layers, side, self.r, float(tol), int(last), _ptr(ws), _stream(ws)),
               self._prefix + "rayleigh_ritz")

    def finalize(self, table, n_layers: int, q, ws, out) -> None:
        """q = None: no quantile clamp."""
        _check(self._finalize(_ptr(table), n_layers, self.r, 0.0 if q is None else float(q), int(q is not None), _ptr(ws),
                              _ptr(out), _stream(ws)), self._prefix + "finalize")


def distill_workspace_bytes(N: int, K: int, r: int) -> int:
    """Bytes of the per-layer workspace of the svd_distill kernels at rank r."""
    return DistillKernels(r).workspace_bytes(N, K)


def quantile_clamp_(x, q: float, hi_out=None) -> None:
    """x (fp32, contiguous, device) ← clamp(x, −hi, hi) with hi = torch.quantile(x, q); hi_out [1] fp32 receives hi."""
    _require_device(x, hi_out)
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise RuntimeError("quantile_clamp_: x must be a contiguous float32 tensor")
    _check(lib().lora_quantile_clamp(_ptr(x), x.numel(), float(q), _ptr(hi_out), _stream(x)), "lora_quantile_clamp")


def geglu_gate_fwd(y2):
    """y2 [M, 2C] contiguous → h·gelu(g) [M, C]."""
    _require_device(y2)
    M, C2 = y2.shape
    out = torch.empty((M, C2 // 2), dtype=y2.dtype, device=y2.device)
    _check(lib().geglu_gate_fwd(_ptr(y2), _ptr(out), M, C2 // 2, dtype_code(y2.dtype), _stream(y2)), "geglu_gate_fwd")
    return out


def geglu_gate_bwd(y2, dout2):
    _require_device(y2, dout2)
    M, C2 = y2.shape
    dy = torch.empty_like(y2)
    _check(lib().geglu_gate_bwd(_ptr(y2), _ptr(dout2), _ptr(dy), M, C2 // 2, dtype_code(y2.dtype), _stream(y2)),
           "geglu_gate_bwd")
    return dy


_zero_factors = {}
_zero_factors_retired = []


def zero_factor_buffer(n_elems: int, dtype: torch.dtype, device):
    """A zeroed buffer of >= n_elems elements for launches without a rank-r term (a zero [16, Kc] factor tile and a zero
    [Nc, 16] epilogue factor); one per (device, dtype), grown on demand.  None inside a recording when it would have to be
    allocated (never allocate-and-zero under capture); an outgrown buffer stays alive — a recorded hipGraph may still read it."""
    key = (device, dtype)
    z = _zero_factors.get(key)
    if z is None or z.numel() < n_elems:
        if torch.cuda.is_current_stream_capturing():
            return None
        if z is not None:
            _zero_factors_retired.append(z)
        z = _zero_factors[key] = torch.zeros(max(n_elems, 16 * 10240), dtype=dtype, device=device)
    return z


def geglu_linear_bwd(dz2, w2t, y2):
    """Backward of `z = (h·gelu(g)) @ W2ᵀ + b2` w.r.t. y = [h | g] in ONE launch (the gate's backward rides in the epilogue
    of dout = dz·W2): dz2 [M,Nz], w2t = W2ᵀ [F,Nz], y2 [M,2F] → dY [M,2F]; None when the library has no fused kernel."""
    _require_device(dz2, w2t, y2)
    M, Nz = dz2.shape
    F = w2t.shape[0]
    z = zero_factor_buffer(16 * max(Nz, F), dz2.dtype, dz2.device)
    if z is None:
        return None  # (the caller runs the two-launch form)
    dy = torch.empty_like(y2)
    st = lib().geglu_linear_bwd(_ptr(dz2), _ptr(w2t), _ptr(y2), _ptr(dy), _ptr(z), M, Nz, F, dtype_code(dz2.dtype) if dz2.dtype != torch.float32 else 0,
                                _stream(dz2))
    if st == -5:
        return None
    _check(st, "geglu_linear_bwd")
    return dy


def attn_split_heads(x3, heads: int, D: int):
    """x3 [B, N, H·d] contiguous → [B, H, N, D] (zero-padded columns)."""
    _require_device(x3)
    B, N, HD = x3.shape
    d = HD // heads
    out = torch.empty((B, heads, N, D), dtype=x3.dtype, device=x3.device)
    _check(lib().attn_split_heads(_ptr(x3), _ptr(out), B, N, heads, d, D, dtype_code(x3.dtype), _stream(x3)),
           "attn_split_heads")
    return out


def attn_merge_heads(x4, d: int):
    """x4 [B, H, N, D] → [B, N, H·d].  x4 may be a strided view with a contiguous last dim (what the attention core
    returns); anything else is made contiguous first."""
    _require_device(x4)
    B, H, N, D = x4.shape
    vec = 16 // x4.element_size()
    sB, sH, sN, sD = x4.stride()
    if sD != 1 or sB % vec or sH % vec or sN % vec or x4.data_ptr() % 16:
        x4 = x4.contiguous()
        sB, sH, sN, sD = x4.stride()
    out = torch.empty((B, N, H * d), dtype=x4.dtype, device=x4.device)
    _check(lib().attn_merge_heads_strided(_ptr(x4), _ptr(out), B, N, H, d, D, sB, sH, sN, dtype_code(x4.dtype),
                                          _stream(x4)), "attn_merge_heads_strided")
    return out


_attn_supported = {}  # (core, shape, dtype) → bool: a pure function of the library, asked 2–3 times per attention call


def group_norm_act_layout(x):
    """0 for an NCHW-contiguous [N,C,H,W] tensor, 1 for a channels-last one, None for any other strides (a tensor that is
    both, C == 1 or H·W == 1, counts as NCHW)."""
    if x.dim() != 4:
        return None
    if x.is_contiguous():
        return 0
    return 1 if x.is_contiguous(memory_format=torch.channels_last) else None


def group_norm_act_supported(x, groups: int, layout) -> bool:
    """Whether the kernels take x: a dense layout, a shape they cover, and storage that starts on a 16-byte boundary (a dense
    view at an odd offset into its buffer does not; the entry points answer LORA_E_ALIGN to it)."""
    N, C, H, W = x.shape
    return (layout is not None and C % groups == 0 and x.data_ptr() % 16 == 0 and
            lib().group_norm_act_workspace_bytes(N, C, H * W, groups, layout, 0) > 0)


def _norm_workspace(x, groups: int, layout: int, want_da: bool):
    N, C, H, W = x.shape
    nbytes = lib().group_norm_act_workspace_bytes(N, C, H * W, groups, layout, int(want_da))
    return torch.empty(nbytes // 4, dtype=torch.float32, device=x.device)


def group_norm_act_fwd(x, addend, gamma, beta, groups: int, eps: float, act: bool, layout: int):
    """y (x's layout), mean, rstd ([N, groups] fp32) of act(GroupNorm(x + addend[:, :, None, None]))."""
    _require_device(x, addend, gamma, beta)
    N, C, H, W = x.shape
    y = torch.empty_like(x)  # preserve_format: dense NCHW / channels-last strides are kept
    mean = torch.empty((N, groups), dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    ws = _norm_workspace(x, groups, layout, False)
    _check(lib().group_norm_act_fwd(_ptr(x), _ptr(addend), _ptr(gamma), _ptr(beta), _ptr(y), _ptr(mean), _ptr(rstd), _ptr(ws),
                                    N, C, H * W, groups, float(eps), int(act), layout, dtype_code(x.dtype), _stream(x)),
           "group_norm_act_fwd")
    return y, mean, rstd


def group_norm_act_bwd(dy, x, addend, gamma, beta, mean, rstd, groups: int, act: bool, layout: int, want_da: bool):
    """dx (x's layout) and da [N, C] (None unless want_da); dy must have x's layout."""
    N, C, H, W = x.shape
    dx = torch.empty_like(x)
    da = torch.empty((N, C), dtype=x.dtype, device=x.device) if want_da else None
    ws = _norm_workspace(x, groups, layout, want_da)
    _check(lib().group_norm_act_bwd(_ptr(dy), _ptr(x), _ptr(addend), _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(rstd), _ptr(dx),
                                    _ptr(da), _ptr(ws), N, C, H * W, groups, int(act), layout, dtype_code(x.dtype), _stream(x)),
           "group_norm_act_bwd")
    return dx, da


def group_norm_act_bwd_res(dy, dh, x, addend, gamma, beta, mean, rstd, groups: int, act: bool, want_da: bool):
    """group_norm_act_bwd for an NCHW-contiguous x with dh, the gradient that reaches x along a residual path, added into dx
    before its one rounding; dy and dh dense like x and 16-byte aligned, dh may be None."""
    N, C, H, W = x.shape
    dx = torch.empty_like(x)
    da = torch.empty((N, C), dtype=x.dtype, device=x.device) if want_da else None
    ws = _norm_workspace(x, groups, 0, want_da)
    _check(lib().group_norm_act_bwd_res(_ptr(dy), _ptr(dh), _ptr(x), _ptr(addend), _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(rstd),
                                        _ptr(dx), _ptr(da), _ptr(ws), N, C, H * W, groups, int(act), dtype_code(x.dtype),
                                        _stream(x)), "group_norm_act_bwd_res")
    return dx, da


def _is_dense16(t) -> bool:
    return t.is_contiguous() and t.data_ptr() % 16 == 0


def residual_bias_add_supported(h, res, b1, b2) -> bool:
    """Whether csrc/trunk_edges.hip adds these: 16-bit NCHW-contiguous h and res of one shape from a 16-byte boundary, H·W a
    multiple of 8, dense [C] biases of their type."""
    if h.dim() != 4 or h.dtype not in (torch.float16, torch.bfloat16) or res.shape != h.shape or res.dtype != h.dtype:
        return False
    for b in (b1, b2):
        if b is not None and (b.dtype != h.dtype or b.shape != h.shape[1:2] or not b.is_contiguous()):
            return False
    N, C, H, W = h.shape
    return (h.numel() > 0 and _is_dense16(h) and _is_dense16(res) and
            bool(lib().residual_bias_add_supported(N, C, H * W, dtype_code(h.dtype))))


def residual_bias_add(h, res, b1, b2):
    """res + h + b1[None, :, None, None] (+ b2 likewise), one pass, fp32 sum with one rounding."""
    _require_device(h, res, b1, b2)
    N, C, H, W = h.shape
    out = torch.empty_like(h)
    _check(lib().residual_bias_add(_ptr(h), _ptr(res), _ptr(b1), _ptr(b2), _ptr(out), N, C, H * W, dtype_code(h.dtype),
                                   _stream(h)), "residual_bias_add")
    return out


def time_proj_supported(N: int, E: int, dtype) -> bool:
    """Whether csrc/time_proj.hip takes a [N, E] time embedding of this dtype (no launch)."""
    return dtype in (torch.float16, torch.bfloat16) and bool(lib().time_proj_supported(N, E, dtype_code(dtype)))


def time_proj_all(temb, weights, biases, extra_biases):
    """silu(temb) @ W_l.T + b_l + cb_l for every layer in one launch per 32 layers: temb [N, E], W_l [C_l, E], b_l / cb_l [C_l] or
    None, all dense and of temb's 16-bit dtype.  Returns the [N, C_l] results, views of one allocation."""
    _require_device(temb, *weights)
    N, E = temb.shape
    L = len(weights)
    widths = [w.shape[0] for w in weights]
    out = torch.empty(N * sum(widths), dtype=temb.dtype, device=temb.device)
    ptrs = lambda ts: (_vp * L)(*[None if t is None else t.data_ptr() for t in ts])
    _check(lib().time_proj_all(_ptr(temb), ptrs(weights), ptrs(biases), ptrs(extra_biases), (_i32 * L)(*widths), _ptr(out), L, N, E,
                               dtype_code(temb.dtype), _stream(temb)), "time_proj_all")
    outs, off = [], 0
    for c in widths:
        outs.append(out[off:off + N * c].view(N, c))
        off += N * c
    return outs


def conv3x3_small_supported(N: int, Cin: int, Cout: int, H: int, W: int, dtype) -> bool:
    """Whether csrc/conv_small.hip covers a 3×3 / stride 1 / padding 1 convolution of this shape and dtype (no launch)."""
    return dtype in (torch.float16, torch.bfloat16) and bool(lib().conv3x3_small_supported(N, Cin, Cout, H, W, dtype_code(dtype)))


def conv3x3_small_plan(pixels: int, Cin: int, Cout: int, dtype) -> bool:
    """Whether the library's planner routes a frozen convolution of this class to csrc/conv_small.hip (no launch)."""
    return dtype in (torch.float16, torch.bfloat16) and bool(lib().conv3x3_small_plan(int(pixels), Cin, Cout, dtype_code(dtype)))


def conv3x3_small_plan_channels(Cin: int, Cout: int, dtype) -> bool:
    """Whether the planner routes these channels at some pixel count: the filters worth packing up front (no launch)."""
    return dtype in (torch.float16, torch.bfloat16) and bool(lib().conv3x3_small_plan_channels(Cin, Cout, dtype_code(dtype)))


def conv3x3_small_pack(weight, backward: bool):
    """The pack of weight [C_out, C_in, 3, 3] (dense) for the forward, or of its flipped and swapped form for backward-data."""
    _require_device(weight)
    Cout, Cin = weight.shape[:2]
    packed = torch.empty(weight.numel(), dtype=weight.dtype, device=weight.device)
    _check(lib().conv3x3_small_pack(_ptr(weight), _ptr(packed), Cin, Cout, int(backward), dtype_code(weight.dtype),
                                    _stream(weight)), "conv3x3_small_pack")
    return packed


def conv3x3_small(x, pack, bias, Cout: int):
    """y [N, Cout, H, W] of the 3×3 convolution of the NCHW-contiguous x with a pack of conv3x3_small_pack."""
    _require_device(x, pack, bias)
    N, Cin, H, W = x.shape
    code = dtype_code(x.dtype)
    nbytes = int(lib().conv3x3_small_workspace_bytes(N, Cin, Cout, H, W, code))
    ws = torch.empty(max(nbytes, 16) // 4, dtype=torch.float32, device=x.device)
    y = torch.empty((N, Cout, H, W), dtype=x.dtype, device=x.device)
    _check(lib().conv3x3_small(_ptr(x), _ptr(pack), _ptr(bias), _ptr(y), _ptr(ws), nbytes, N, Cin, Cout, H, W, code, _stream(x)),
           "conv3x3_small")
    return y


def conv3x3_small_form_choice(N: int, Cin: int, Cout: int, H: int, W: int, dtype) -> int:
    """The staging form conv3x3_small takes for this shape (0: positions, 1: rows; -1: not covered).  No launch."""
    if dtype not in (torch.float16, torch.bfloat16):
        return -1
    return int(lib().conv3x3_small_form_choice(N, Cin, Cout, H, W, dtype_code(dtype)))


def conv3x3_small_form(x, pack, bias, Cout: int, form: int):
    """conv3x3_small with a named staging form (0: positions, 1: rows); raises where the form does not cover the shape.  For
    tools/conv_small_sweep.py and the tests."""
    _require_device(x, pack, bias)
    N, Cin, H, W = x.shape
    code = dtype_code(x.dtype)
    nbytes = int(lib().conv3x3_small_workspace_bytes(N, Cin, Cout, H, W, code))
    ws = torch.empty(max(nbytes, 16) // 4, dtype=torch.float32, device=x.device)
    y = torch.empty((N, Cout, H, W), dtype=x.dtype, device=x.device)
    _check(lib().conv3x3_small_form(_ptr(x), _ptr(pack), _ptr(bias), _ptr(y), _ptr(ws), nbytes, N, Cin, Cout, H, W, code, int(form),
                                    _stream(x)), "conv3x3_small_form")
    return y


def conv3x3_large_supported(N: int, Cin: int, Cout: int, H: int, W: int, dtype) -> bool:
    """Whether csrc/conv_large.hip covers a 3×3 / stride 1 / padding 1 convolution of this shape and dtype (no launch)."""
    return dtype in (torch.float16, torch.bfloat16) and bool(lib().conv3x3_large_supported(N, Cin, Cout, H, W, dtype_code(dtype)))


def conv3x3_large_plan(pixels: int, Cin: int, Cout: int, dtype) -> bool:
    """Whether the library's planner routes a frozen convolution of this class to csrc/conv_large.hip (no launch)."""
    return dtype in (torch.float16, torch.bfloat16) and bool(lib().conv3x3_large_plan(int(pixels), Cin, Cout, dtype_code(dtype)))


def conv3x3_large_plan_channels(Cin: int, Cout: int, dtype) -> bool:
    """Whether conv3x3_large_plan routes these channels at some pixel count (no launch)."""
    return dtype in (torch.float16, torch.bfloat16) and bool(lib().conv3x3_large_plan_channels(Cin, Cout, dtype_code(dtype)))


def conv3x3_large(x, pack, bias, Cout: int):
    """y [N, Cout, H, W] of the 3×3 convolution of the NCHW-contiguous x with a pack of conv3x3_small_pack, on the many-pixel
    kernel: one launch, no workspace."""
    _require_device(x, pack, bias)
    N, Cin, H, W = x.shape
    y = torch.empty((N, Cout, H, W), dtype=x.dtype, device=x.device)
    _check(lib().conv3x3_large(_ptr(x), _ptr(pack), _ptr(bias), _ptr(y), None, 0, N, Cin, Cout, H, W, dtype_code(x.dtype),
                               _stream(x)), "conv3x3_large")
    return y


def conv3x3_large_tile_choice(N: int, Cin: int, Cout: int, H: int, W: int, dtype) -> int:
    """The tile conv3x3_large runs this shape on (0: the shape rule's, 1: 256 × 80, 2: 128 × 80; -1: not covered).  No launch."""
    if dtype not in (torch.float16, torch.bfloat16):
        return -1
    return int(lib().conv3x3_large_tile_choice(N, Cin, Cout, H, W, dtype_code(dtype)))


def conv3x3_large_tile(x, pack, bias, Cout: int, tile: int):
    """conv3x3_large on a named tile (0: the shape rule's, 1: 256 pixels × 80 channels, 2: 128 × 80); raises where the tile's
    conditions fail.  For tools/conv_large_sweep.py and the tests."""
    _require_device(x, pack, bias)
    N, Cin, H, W = x.shape
    y = torch.empty((N, Cout, H, W), dtype=x.dtype, device=x.device)
    _check(lib().conv3x3_large_tile(_ptr(x), _ptr(pack), _ptr(bias), _ptr(y), None, 0, N, Cin, Cout, H, W, dtype_code(x.dtype),
                                    int(tile), _stream(x)), "conv3x3_large_tile")
    return y


def tokens_nchw_supported(N: int, C: int, HW: int, dtype) -> bool:
    """Whether the transposing kernels of csrc/trunk_edges.hip cover [N, HW, C] ↔ [N, C, HW] in this dtype (no launch)."""
    return dtype in (torch.float16, torch.bfloat16) and bool(lib().tokens_nchw_supported(N, C, HW, dtype_code(dtype)))


def tokens_to_nchw_add(tok, res, shape):
    """out [N,C,H,W] = tok [N, H·W, C] re-laid out (+ res, NCHW, when given); tok and res dense and 16-byte aligned."""
    _require_device(tok, res)
    N, C, H, W = shape
    out = torch.empty(shape, dtype=tok.dtype, device=tok.device)
    _check(lib().tokens_to_nchw_add(_ptr(tok), _ptr(res), _ptr(out), N, C, H * W, dtype_code(tok.dtype), _stream(tok)),
           "tokens_to_nchw_add")
    return out


def nchw_to_tokens(x):
    """tok [N, H·W, C] = x [N,C,H,W] (NCHW-contiguous, 16-byte aligned) re-laid out."""
    _require_device(x)
    N, C, H, W = x.shape
    tok = torch.empty((N, H * W, C), dtype=x.dtype, device=x.device)
    _check(lib().nchw_to_tokens(_ptr(x), _ptr(tok), N, C, H * W, dtype_code(x.dtype), _stream(x)), "nchw_to_tokens")
    return tok


def add_layer_norm_supported(x) -> bool:
    """Whether the kernels of csrc/layer_norm.hip take x as rows [M, C]: dense, a width they cover, a 16-byte-aligned start."""
    C = x.shape[-1] if x.dim() else 0
    return (x.numel() > 0 and x.is_contiguous() and C % 8 == 0 and C <= lib().add_layer_norm_max_channels() and
            x.data_ptr() % 16 == 0)


def add_layer_norm_fwd(x, delta, gamma, beta, eps: float):
    """(h, y, mean, rstd): h = x + delta (None when delta is None), y = LayerNorm(h)·gamma + beta over the last dimension,
    mean / rstd [M] fp32 of the rounded h."""
    _require_device(x, delta, gamma, beta)
    C = x.shape[-1]
    M = x.numel() // C
    h = None if delta is None else torch.empty_like(x)
    y = torch.empty_like(x)
    mean = torch.empty(M, dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    _check(lib().add_layer_norm_fwd(_ptr(x), _ptr(delta), _ptr(gamma), _ptr(beta), _ptr(h), _ptr(y), _ptr(mean), _ptr(rstd), M, C,
                                    float(eps), dtype_code(x.dtype), _stream(x)), "add_layer_norm_fwd")
    return h, y, mean, rstd


def add_layer_norm_bwd(dy, dh, h, gamma, mean, rstd):
    """dx = LayerNorm's input gradient + dh (dh None: without it); dy / dh dense like h and 16-byte aligned."""
    C = h.shape[-1]
    dx = torch.empty_like(h)
    _check(lib().add_layer_norm_bwd(_ptr(dy), _ptr(dh), _ptr(h), _ptr(gamma), _ptr(mean), _ptr(rstd), _ptr(dx), h.numel() // C, C,
                                    dtype_code(h.dtype), _stream(h)), "add_layer_norm_bwd")
    return dx


def attn_ctx_supported(B: int, Tq: int, Tk: int, H: int, d: int, dtype) -> bool:
    key = (0, B, Tq, Tk, H, d, dtype)
    ok = _attn_supported.get(key)
    if ok is None:
        ok = _attn_supported[key] = (dtype in (torch.float16, torch.bfloat16) and
                                     bool(lib().attn_ctx_supported(B, Tq, Tk, H, d, dtype_code(dtype))))
    return ok


def attn_ctx_fwd(q, k, v, heads: int, scale: float):
    """q [B,Tq,H·d], k/v [B,Tk,H·d] contiguous → softmax(q·kᵀ·scale)·v per head, [B,Tq,H·d]."""
    _require_device(q, k, v)
    B, Tq, HD = q.shape
    Tk = k.shape[1]
    out = torch.empty_like(q)
    _check(lib().attn_ctx_fwd(_ptr(q), _ptr(k), _ptr(v), _ptr(out), B, Tq, Tk, heads, HD // heads, float(scale),
                              dtype_code(q.dtype), _stream(q)), "attn_ctx_fwd")
    return out


def attn_ctx_bwd(q, k, v, dout, heads: int, scale: float):
    """→ (dq, dk, dv), same layouts as the inputs."""
    _require_device(q, k, v, dout)
    B, Tq, HD = q.shape
    Tk = k.shape[1]
    d = HD // heads
    nbytes = lib().attn_ctx_bwd_workspace_bytes(B, Tq, Tk, heads, d)
    if nbytes < 0:
        raise RuntimeError("attn_ctx_bwd: unsupported shape")
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=q.device)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    _check(lib().attn_ctx_bwd(_ptr(q), _ptr(k), _ptr(v), _ptr(dout), _ptr(dq), _ptr(dk), _ptr(dv), _ptr(ws), B, Tq, Tk,
                              heads, d, float(scale), dtype_code(q.dtype), _stream(q)), "attn_ctx_bwd")
    return dq, dk, dv


def attn_ctx_fwd_kv(q, kv, off_k: int, off_v: int, heads: int, scale: float):
    """Cross-attention whose K and V are the column slices [off_k, off_k+H·d) / [off_v, …) of `kv` [B·Tk, ld] (the output
    of a grouped to_k/to_v projection); q [B,Tq,H·d] contiguous → out [B,Tq,H·d]."""
    _require_device(q, kv)
    B, Tq, HD = q.shape
    ld = kv.shape[-1]
    Tk = kv.shape[0] // B
    es = kv.element_size()
    out = torch.empty_like(q)
    _check(lib().attn_ctx_fwd_strided(_ptr(q), kv.data_ptr() + off_k * es, kv.data_ptr() + off_v * es, _ptr(out), ld, B,
                                      Tq, Tk, heads, HD // heads, float(scale), dtype_code(q.dtype), _stream(q)),
           "attn_ctx_fwd_strided")
    return out


def attn_ctx_bwd_kv(q, kv, dkv, off_k: int, off_v: int, dout, heads: int, scale: float):
    """Backward of attn_ctx_fwd_kv: returns dq; dK / dV are WRITTEN into the same column slices of `dkv` [B·Tk, ld]."""
    _require_device(q, kv, dkv, dout)
    B, Tq, HD = q.shape
    ld = kv.shape[-1]
    Tk = kv.shape[0] // B
    d = HD // heads
    es = kv.element_size()
    nbytes = lib().attn_ctx_bwd_workspace_bytes(B, Tq, Tk, heads, d)
    if nbytes < 0:
        raise RuntimeError("attn_ctx_bwd: unsupported shape")
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=q.device)
    dq = torch.empty_like(q)
    _check(lib().attn_ctx_bwd_strided(_ptr(q), kv.data_ptr() + off_k * es, kv.data_ptr() + off_v * es, _ptr(dout),
                                      _ptr(dq), dkv.data_ptr() + off_k * es, dkv.data_ptr() + off_v * es, _ptr(ws), ld,
                                      dkv.shape[-1], B, Tq, Tk, heads, d, float(scale), dtype_code(q.dtype), _stream(q)),
           "attn_ctx_bwd_strided")
    return dq


def attn_causal_supported(B: int, T: int, H: int, d: int, dtype) -> bool:
    key = (2, B, T, H, d, dtype)
    ok = _attn_supported.get(key)
    if ok is None:
        ok = _attn_supported[key] = (dtype in (torch.float16, torch.bfloat16) and
                                     bool(lib().attn_causal_supported(B, T, H, d, dtype_code(dtype))))
    return ok


def shared_row_stride(*tensors):
    """The one row stride (elements) of [B, T, W] tensors that are dense or column slices of row-major [B·T, ld] buffers —
    unit stride along W, batches T rows apart — or None when they have no such common stride.  The strides of size-1
    dimensions say nothing (PyTorch leaves them arbitrary): with T == 1 the batch stride is the row stride, with B == 1 and
    T == 1 any stride ≥ W serves."""
    ld = None
    for t in tensors:
        if t.dim() != 3 or (t.shape[2] > 1 and t.stride(2) != 1):
            return None
        B, T, W = t.shape
        if T > 1:
            mine = t.stride(1)
            if B > 1 and t.stride(0) != T * mine:
                return None
        elif B > 1:
            mine = t.stride(0)
        else:
            continue
        if mine < W or (ld is not None and mine != ld):
            return None
        ld = mine
    return tensors[0].shape[2] if ld is None else ld


def attn_causal_fwd(q, k, v, heads: int, scale: float):
    """Causal self-attention: q, k, v [B,T,H·d] with one row stride (dense, or the column slices of one [B·T, 3·H·d]
    buffer) → softmax(mask(q·kᵀ·scale))·v per head, [B,T,H·d] dense."""
    _require_device(q, k, v)
    B, T, HD = q.shape
    ld = shared_row_stride(q, k, v)
    if ld is None:
        raise RuntimeError("attn_causal_fwd: q, k, v must share one row stride")
    out = torch.empty((B, T, HD), dtype=q.dtype, device=q.device)
    _check(lib().attn_causal_fwd_strided(_ptr(q), _ptr(k), _ptr(v), _ptr(out), ld, B, T, heads, HD // heads, float(scale),
                                         dtype_code(q.dtype), _stream(q)), "attn_causal_fwd_strided")
    return out


def attn_causal_bwd(q, k, v, dout, heads: int, scale: float, out=None):
    """→ (dq, dk, dv) [B,T,H·d]: new dense tensors, or `out` — three tensors with one row stride of their own (the column
    slices of one gradient buffer), written in place.  dout dense."""
    _require_device(q, k, v, dout)
    B, T, HD = q.shape
    d = HD // heads
    ld = shared_row_stride(q, k, v)
    if ld is None:
        raise RuntimeError("attn_causal_bwd: q, k, v must share one row stride")
    nbytes = lib().attn_causal_bwd_workspace_bytes(B, T, heads, d)
    if nbytes < 0:
        raise RuntimeError("attn_causal_bwd: unsupported shape")
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=q.device)
    if out is None:
        out = tuple(torch.empty((B, T, HD), dtype=q.dtype, device=q.device) for _ in range(3))
    dq, dk, dv = out
    ld_dq = shared_row_stride(dq, dk, dv)
    if ld_dq is None or any(t.shape != q.shape or t.dtype != q.dtype for t in out):
        raise RuntimeError("attn_causal_bwd: dq, dk, dv must be [B,T,H·d] tensors of q's dtype sharing one row stride")
    _check(lib().attn_causal_bwd_strided(_ptr(q), _ptr(k), _ptr(v), _ptr(dout), _ptr(dq), _ptr(dk), _ptr(dv), _ptr(ws), ld,
                                         ld_dq, B, T, heads, d, float(scale), dtype_code(q.dtype), _stream(q)),
           "attn_causal_bwd_strided")
    return dq, dk, dv


def attn_flash_fwd_qkv(qkv, heads: int, scale: float, want_lse: bool = True):
    """Self-attention on a grouped projection's output qkv [B, T, 3·H·d] (q | k | v column slices) → (o [B,T,H·d], lse)."""
    _require_device(qkv)
    B, T, W = qkv.shape
    HD = W // 3
    es = qkv.element_size()
    out = torch.empty((B, T, HD), dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty((B, heads, T), dtype=torch.float32, device=qkv.device) if want_lse else None
    base = qkv.data_ptr()
    _check(lib().attn_flash_fwd_strided(base, base + HD * es, base + 2 * HD * es, _ptr(out), _ptr(lse), W, B, T, T, heads,
                                        HD // heads, float(scale), dtype_code(qkv.dtype), _stream(qkv)),
           "attn_flash_fwd_strided")
    return out, lse


def attn_flash_bwd_qkv(qkv, out, dout, lse, heads: int, scale: float):
    """→ dqkv [B, T, 3·H·d] (dq | dk | dv written as column slices of one buffer: the dY of the grouped projection)."""
    _require_device(qkv, out, dout, lse)
    B, T, W = qkv.shape
    HD = W // 3
    es = qkv.element_size()
    ws = torch.empty(lib().attn_flash_bwd_workspace_bytes(B, T, heads) // 4, dtype=torch.float32, device=qkv.device)
    dqkv = torch.empty_like(qkv)
    base, dbase = qkv.data_ptr(), dqkv.data_ptr()
    _check(lib().attn_flash_bwd_strided(base, base + HD * es, base + 2 * HD * es, _ptr(out), _ptr(dout), _ptr(lse), dbase,
                                        dbase + HD * es, dbase + 2 * HD * es, _ptr(ws), W, W, B, T, T, heads, HD // heads,
                                        float(scale), dtype_code(qkv.dtype), _stream(qkv)), "attn_flash_bwd_strided")
    return dqkv


def attn_flash_supported(B: int, Tq: int, Tk: int, H: int, d: int, dtype) -> bool:
    key = (1, B, Tq, Tk, H, d, dtype)
    ok = _attn_supported.get(key)
    if ok is None:
        ok = _attn_supported[key] = (dtype in (torch.float16, torch.bfloat16) and
                                     bool(lib().attn_flash_supported(B, Tq, Tk, H, d, dtype_code(dtype))))
    return ok


def attn_flash_fwd(q, k, v, heads: int, scale: float, want_lse: bool = True):
    """q [B,Tq,H·d], k/v [B,Tk,H·d] contiguous → (o [B,Tq,H·d], lse [B,H,Tq] fp32 | None)."""
    _require_device(q, k, v)
    B, Tq, HD = q.shape
    Tk = k.shape[1]
    out = torch.empty_like(q)
    lse = torch.empty((B, heads, Tq), dtype=torch.float32, device=q.device) if want_lse else None
    _check(lib().attn_flash_fwd(_ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(lse), B, Tq, Tk, heads, HD // heads,
                                float(scale), dtype_code(q.dtype), _stream(q)), "attn_flash_fwd")
    return out, lse


def attn_flash_bwd(q, k, v, out, dout, lse, heads: int, scale: float):
    """→ (dq, dk, dv), same layouts as the inputs."""
    _require_device(q, k, v, out, dout, lse)
    B, Tq, HD = q.shape
    Tk = k.shape[1]
    ws = torch.empty(lib().attn_flash_bwd_workspace_bytes(B, Tq, heads) // 4, dtype=torch.float32, device=q.device)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    _check(lib().attn_flash_bwd(_ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(dout), _ptr(lse), _ptr(dq), _ptr(dk),
                                _ptr(dv), _ptr(ws), B, Tq, Tk, heads, HD // heads, float(scale), dtype_code(q.dtype),
                                _stream(q)), "attn_flash_bwd")
    return dq, dk, dv


def attn_f32_supported(B: int, Tq: int, Tk: int, H: int, d: int) -> bool:
    key = (3, B, Tq, Tk, H, d)
    ok = _attn_supported.get(key)
    if ok is None:
        ok = _attn_supported[key] = bool(lib().attn_f32_supported(B, Tq, Tk, H, d))
    return ok


def _require_f32_dense(name: str, *tensors) -> None:
    for t in tensors:
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError(f"{name}: operands must be contiguous float32 tensors (got {t.dtype}, strides {t.stride()})")


def attn_f32_fwd(q, k, v, heads: int, scale: float, want_lse: bool = True):
    """fp32 q [B,Tq,H·d], k/v [B,Tk,H·d] contiguous → (o [B,Tq,H·d], lse [B,H,Tq] | None)  (csrc/attn_f32.hip)."""
    _require_device(q, k, v)
    _require_f32_dense("attn_f32_fwd", q, k, v)
    B, Tq, HD = q.shape
    Tk = k.shape[1]
    if HD % heads or k.shape != (B, Tk, HD) or v.shape != k.shape:
        raise RuntimeError(f"attn_f32_fwd: shapes {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)} with {heads} heads")
    out = torch.empty_like(q)
    lse = torch.empty((B, heads, Tq), dtype=torch.float32, device=q.device) if want_lse else None
    _check(lib().attn_f32_fwd(_ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(lse), B, Tq, Tk, heads, HD // heads, float(scale),
                              _stream(q)), "attn_f32_fwd")
    return out, lse


def attn_f32_bwd(q, k, v, out, dout, lse, heads: int, scale: float):
    """→ (dq, dk, dv), same layouts as the inputs."""
    _require_device(q, k, v, out, dout, lse)
    _require_f32_dense("attn_f32_bwd", q, k, v, out, dout, lse)
    B, Tq, HD = q.shape
    Tk = k.shape[1]
    ws = torch.empty(lib().attn_f32_bwd_workspace_bytes(B, Tq, heads) // 4, dtype=torch.float32, device=q.device)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    _check(lib().attn_f32_bwd(_ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(dout), _ptr(lse), _ptr(dq), _ptr(dk), _ptr(dv),
                              _ptr(ws), B, Tq, Tk, heads, HD // heads, float(scale), _stream(q)), "attn_f32_bwd")
    return dq, dk, dv


def prof_enable(capacity: int) -> None:
    _check(lib().lora_prof_enable(int(capacity)), "lora_prof_enable")


def prof_null_mode(on: bool) -> None:
    """Launch-floor mode: every profiled launch site dispatches an empty kernel of the same shape (timing only)."""
    _check(lib().lora_prof_null_mode(1 if on else 0), "lora_prof_null_mode")


def prof_collect():
    tot = ProfTotals()
    _check(lib().lora_prof_collect(ctypes.byref(tot)), "lora_prof_collect")
    return {
        lib().lora_prof_kernel_name(k).decode(): {"launches": int(tot.launches[k]), "ms": float(tot.ms[k]),
                                                  "bytes": float(tot.bytes[k]), "flops": float(tot.flops[k])}
        for k in range(PROF_KINDS) if tot.launches[k] > 0
    }

"""ctypes binding of libzigma_hip.so (include/zigma_hip.h).

The product path has NO fallback: if the shared library is missing or a kernel reports an error,
the calling op raises.  torch is used for device memory and streams only — every pointer crossing
the boundary is a raw device address (`Tensor.data_ptr()`), every launch goes to torch's current
HIP stream so that stream semantics (and graph capture) match the reference's extensions
(`at::cuda::getCurrentCUDAStream()`, selective_scan.cpp:326-327).
"""
import ctypes as C
import math
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ZIGMA_AMD_LIB") or os.path.join(_HERE, "lib", "libzigma_hip.so")   # env: A/B builds in tools/

F32, F16, BF16 = 0, 1, 2
_DT = {torch.float32: F32, torch.float16: F16, torch.bfloat16: BF16}

i32, i64, vp, f32, f64 = C.c_int32, C.c_int64, C.c_void_p, C.c_float, C.c_double


class ScanParams(C.Structure):
    _fields_ = (
        [(n, i32) for n in ("batch", "dim", "seqlen", "dstate", "n_groups", "is_variable_B", "is_variable_C",
                            "delta_softplus", "io_dtype", "bc_dtype", "chunk_len", "flags")]
        + [(n, i64) for n in (
            "u_batch_stride", "u_d_stride", "u_l_stride",
            "delta_batch_stride", "delta_d_stride", "delta_l_stride",
            "z_batch_stride", "z_d_stride", "z_l_stride",
            "out_batch_stride", "out_d_stride", "out_l_stride",
            "out_z_batch_stride", "out_z_d_stride", "out_z_l_stride",
            "A_d_stride", "A_dstate_stride",
            "B_batch_stride", "B_group_stride", "B_d_stride", "B_dstate_stride", "B_l_stride",
            "C_batch_stride", "C_group_stride", "C_d_stride", "C_dstate_stride", "C_l_stride")]
        + [(n, vp) for n in ("u", "delta", "A", "B", "C", "D", "delta_bias", "z", "out", "out_z", "x",
                             "z_row_index", "out_row_index", "checkpoints")]
        + [("reset_period", i32), ("pad2_", i32), ("info", C.POINTER(C.c_int32))]
        + [("dt_x", vp), ("dt_w", vp), ("dt_x_batch_stride", i64), ("dt_x_l_stride", i64), ("dt_w_row_stride", i64),
           ("dt_rank", i32), ("pad3_", i32)]
    )


SCAN_Z_PREACTIVATED, SCAN_ACCUMULATE = 2, 4                # zigma_scan_params_t.flags
SCAN_PROBE_V1, SCAN_PROBE_PRIO_SHIFT, SCAN_PROBE_R5_SHIFT = 0x100, 9, 10           # A/B probes (tools/scan_ab.py, tools/r05_scan_ab.py)
SCAN_KERNEL_GENERIC, SCAN_KERNEL_TOK, SCAN_KERNEL_TOK2 = 1, 2, 3   # zigma_scan_params_t.info[0]


class ConvParams(C.Structure):
    _fields_ = (
        [(n, i32) for n in ("batch", "dim", "seqlen", "width", "silu_activation", "io_dtype", "w_dtype", "flags")]
        + [(n, i64) for n in ("x_batch_stride", "x_c_stride", "x_l_stride", "weight_c_stride", "weight_width_stride",
                              "out_batch_stride", "out_c_stride", "out_l_stride")]
        + [(n, vp) for n in ("x", "weight", "bias", "out", "x_row_index")]
        + [("reset_period", i32), ("pad2_", i32)]
    )


class NormParams(C.Structure):
    _fields_ = (
        [(n, i32) for n in ("rows", "cols", "rows_per_batch", "is_rms", "x_dtype", "res_dtype", "w_dtype", "mod_dtype")]
        + [("eps", f32), ("flags", i32)]
        + [(n, i64) for n in ("x_row_stride", "branch_row_stride", "x_out_row_stride", "res_row_stride",
                              "res_out_row_stride", "y_row_stride", "y_mod_row_stride", "mod_batch_stride")]
        + [(n, vp) for n in ("x", "branch", "gate", "x_out", "residual", "residual_out", "weight", "bias", "y_out",
                             "shift", "scale", "y_mod")]
    )


class DtProjParams(C.Structure):
    _fields_ = ([("m", i64), ("n", i32), ("k", i32), ("dtype", i32), ("softplus", i32), ("flags", i32), ("pad_", i32)]
                + [(n, i64) for n in ("x_row_stride", "w_row_stride", "out_row_stride")]
                + [(n, vp) for n in ("x", "w", "bias", "out")])


class ScanBwdParams(C.Structure):
    _fields_ = ([(n, i32) for n in ("batch", "dim", "seqlen", "dstate", "delta_softplus", "io_dtype", "flags", "reset_period")]
                + [(n, i64) for n in (
                    "u_batch_stride", "u_l_stride", "delta_batch_stride", "delta_l_stride", "z_batch_stride", "z_l_stride",
                    "out_batch_stride", "out_l_stride", "dout_batch_stride", "dout_l_stride", "du_batch_stride",
                    "du_l_stride", "ddelta_batch_stride", "ddelta_l_stride", "dz_batch_stride", "dz_l_stride",
                    "A_d_stride", "A_dstate_stride", "B_batch_stride", "B_dstate_stride", "B_l_stride",
                    "C_batch_stride", "C_dstate_stride", "C_l_stride", "dB_batch_stride", "dB_dstate_stride",
                    "dB_l_stride", "dC_batch_stride", "dC_dstate_stride", "dC_l_stride")]
                + [(n, vp) for n in ("u", "delta", "A", "B", "C", "D", "delta_bias", "z", "out", "dout", "du", "ddelta",
                                     "dz", "dA", "dB", "dC", "dD", "ddelta_bias", "workspace")]
                + [("workspace_bytes", i64), ("z_row_index", vp), ("out_row_index", vp), ("checkpoints", vp)])


class ConvBwdParams(C.Structure):
    _fields_ = ([(n, i32) for n in ("batch", "dim", "seqlen", "width", "silu_activation", "io_dtype", "w_dtype", "flags")]
                + [(n, i64) for n in ("x_batch_stride", "x_l_stride", "dout_batch_stride", "dout_l_stride", "dx_batch_stride",
                                      "dx_l_stride", "weight_c_stride", "weight_width_stride")]
                + [(n, vp) for n in ("x", "weight", "bias", "dout", "dx", "dweight", "dbias", "x_row_index", "workspace")]
                + [("workspace_bytes", i64), ("reset_period", i32), ("pad_", i32)])


class NormBwdParams(C.Structure):
    _fields_ = ([(n, i32) for n in ("rows", "cols", "is_rms", "x_dtype", "res_dtype", "w_dtype")]
                + [("eps", f32), ("flags", i32)]
                + [(n, i64) for n in ("xsum_row_stride", "dy_row_stride", "dres_out_row_stride", "dx_row_stride",
                                      "dres_row_stride")]
                + [(n, vp) for n in ("xsum", "weight", "dy", "dresidual_out", "dx", "dresidual", "dweight", "dbias",
                                     "workspace")]
                + [("workspace_bytes", i64)])


class XAttnParams(C.Structure):
    _fields_ = ([(n, i32) for n in ("batch", "seqlen", "n_ctx", "heads", "head_dim", "dtype", "flags")] + [("scale", f32)]
                + [(n, i64) for n in ("q_batch_stride", "q_row_stride", "k_batch_stride", "k_row_stride", "v_batch_stride",
                                      "v_row_stride", "o_batch_stride", "o_row_stride")]
                + [(n, vp) for n in ("q", "k", "v", "out")])


class XAttnBwdParams(C.Structure):
    _fields_ = ([(n, i32) for n in ("batch", "seqlen", "n_ctx", "heads", "head_dim", "dtype", "flags")] + [("scale", f32)]
                + [("chunks", i32), ("pad_", i32)]
                + [(n, i64) for n in ("q_batch_stride", "q_row_stride", "k_batch_stride", "k_row_stride", "v_batch_stride",
                                      "v_row_stride", "do_batch_stride", "do_row_stride", "dq_batch_stride", "dq_row_stride")]
                + [(n, vp) for n in ("q", "k", "v", "dout", "dq", "dk_part", "dv_part")])


class PatchEmbedParams(C.Structure):
    _fields_ = ([(n, i32) for n in ("batch", "in_chans", "height", "width", "patch", "embed_dim", "dtype", "flags")]
                + [(n, i64) for n in ("x_batch_stride", "x_chan_stride", "x_row_stride", "pos_row_stride", "out_batch_stride", "out_row_stride")]
                + [(n, vp) for n in ("x", "weight", "bias", "pos", "out")])


class TimestepEmbedParams(C.Structure):
    _fields_ = [("batch", i32), ("dim", i32), ("dtype", i32), ("flags", i32), ("out_row_stride", i64), ("t", vp), ("freqs", vp), ("out", vp)]


class FinalLayerParams(C.Structure):
    _fields_ = ([("rows", i64), ("cols", i32), ("n_out", i32), ("dtype", i32), ("flags", i32), ("eps", f32), ("pad_", i32),
                 ("x_row_stride", i64), ("out_row_stride", i64)] + [(n, vp) for n in ("x", "weight", "bias", "out")])


class FinalLayerCfgParams(C.Structure):
    _fields_ = ([("rows", i64), ("cols", i32), ("n_out", i32), ("dtype", i32), ("out_dtype", i32), ("flags", i32), ("eps", f32)]
                + [(n, i32) for n in ("rows_per_sample", "tokens_per_frame", "grid_w", "patch", "chans", "pad_")]
                + [(n, i64) for n in ("x_row_stride", "out_sample_stride", "out_frame_stride", "out_chan_stride", "out_row_stride")]
                + [(n, vp) for n in ("x_cond", "x_uncond", "weight", "bias", "scale", "out", "y_out")])


class SkinnyParams(C.Structure):
    _fields_ = ([(n, i32) for n in ("m", "n", "k", "dtype", "flags", "pad_")] + [(n, i64) for n in ("x_row_stride", "w_row_stride", "out_row_stride")]
                + [(n, vp) for n in ("x", "w", "bias", "out")])


class GlueBwdParams(C.Structure):
    _fields_ = ([("rows", i64), ("cols", i32), ("rows_per_batch", i32), ("dtype", i32), ("flags", i32), ("s_add", f32), ("pad_", i32)]
                + [(n, i64) for n in ("dy_row_stride", "a_row_stride", "out_row_stride", "s_batch_stride")]
                + [(n, vp) for n in ("dy", "a", "s", "out", "r1", "r2")])


class CalibParams(C.Structure):
    _fields_ = [("mode", i32), ("iters", i32), ("bytes", i64), ("src", vp), ("dst", vp)]


class XProjParams(C.Structure):
    _fields_ = ([("m", i64), ("n", i32), ("k", i32), ("dtype", i32), ("flags", i32)]
                + [(n, i64) for n in ("x_row_stride", "w_row_stride", "out_row_stride")] + [(n, vp) for n in ("x", "w", "out")])


class ConvXProjParams(C.Structure):
    _fields_ = ([(n, i32) for n in ("batch", "seqlen", "dim", "n", "dtype", "flags")]
                + [(n, i64) for n in ("x_batch_stride", "x_l_stride", "u_batch_stride", "u_l_stride", "w_row_stride", "out_row_stride")]
                + [(n, vp) for n in ("x", "conv_weight", "conv_bias", "w", "u", "out", "x_row_index")])


class LinearParams(C.Structure):
    _fields_ = ([("m", i64), ("n", i32), ("k", i32), ("dtype", i32), ("flags", i32), ("silu_from_col", i32), ("pad_", i32)]
                + [(n, i64) for n in ("x_row_stride", "w_row_stride", "out_row_stride")] + [(n, vp) for n in ("x", "w", "bias", "out")]
                + [("residual", vp), ("gate", vp), ("res_row_stride", i64), ("gate_batch_stride", i64), ("rows_per_batch", i32), ("pad2_", i32)])


LINEAR_WS, LINEAR_SM = 0x4000, 0x8000            # zigma_linear_params_t.flags: ZIGMA_LINEAR_WS (csrc/linear_ws.hip), ZIGMA_LINEAR_SM (csrc/linear_sm.hip)


class LinearWgradParams(C.Structure):
    _fields_ = ([("m", i64), ("n", i32), ("k", i32), ("dtype", i32), ("out_dtype", i32), ("slabs", i32), ("flags", i32)]
                + [(n, i64) for n in ("dy_row_stride", "x_row_stride", "out_row_stride")] + [(n, vp) for n in ("dy", "x", "out", "workspace")]
                + [("workspace_bytes", i64)])


class LinearSplitParams(C.Structure):
    _fields_ = ([("m", i64), ("n", i32), ("k", i32), ("passes", i32), ("flags", i32)]
                + [(n, i64) for n in ("x_row_stride", "w_hi_row_stride", "w_lo_row_stride", "out_row_stride")]
                + [(n, vp) for n in ("x", "w_hi", "w_lo", "bias", "out")])


class NormLinearParams(C.Structure):
    _fields_ = ([("m", i64), ("n", i32), ("k", i32), ("dtype", i32), ("flags", i32), ("rows_per_batch", i32), ("eps", f32)]
                + [(n, i64) for n in ("x_row_stride", "w_row_stride", "out_row_stride", "mod_batch_stride")]
                + [(n, vp) for n in ("x", "w", "shift", "scale", "out")])


class MultiCastParams(C.Structure):
    _fields_ = [("table", vp), ("chunk_map", vp), ("n_entries", i64), ("n_chunks", i64), ("out_dtype", i32), ("chunk", i32), ("flags", i32), ("pad_", i32)]


class OptimRow(C.Structure):            # one row of the device table (zigma_amd/optim.py writes the rows as eight int64)
    _fields_ = [(n, vp) for n in ("p", "g", "m", "v", "ema", "shadow")] + [("numel", i64), ("pad_", i64)]


class OptimState(C.Structure):          # the device state block (eight 4-byte words)
    _fields_ = [("step", f32), ("skipped", i32), ("grad_norm", f32), ("grad_mult", f32), ("step_size", f32), ("bc2_sqrt", f32), ("pad_", i32 * 2)]


class OptimParams(C.Structure):
    _fields_ = ([("table", vp), ("chunk_map", vp), ("n_entries", i64), ("n_chunks", i64), ("partials", vp), ("state", vp), ("grad_scale", vp), ("found_inf", vp)]
                + [(n, f64) for n in ("lr", "beta1", "beta2", "eps", "weight_decay", "max_grad_norm", "ema_decay")]
                + [("shadow_dtype", i32), ("chunk", i32), ("flags", i32), ("pad_", i32)])


class Optim16Row(C.Structure):          # one row of the 16-bit step's device table (zigma_amd/optim.py writes the rows as ten int64)
    _fields_ = [(n, vp) for n in ("p", "g", "m", "v", "ema")] + [("numel", i64), ("pid", i64), ("dbg_x32", vp), ("dbg_bits", vp), ("pad_", i64)]


class Optim16Params(C.Structure):
    _fields_ = ([("table", vp), ("chunk_map", vp), ("n_entries", i64), ("n_chunks", i64), ("max_numel", i64), ("partials", vp), ("state", vp)]
                + [(n, f64) for n in ("lr", "beta1", "beta2", "eps", "weight_decay", "max_grad_norm", "ema_decay")]
                + [(n, C.c_uint32) for n in ("seed_lo", "seed_hi", "stream")] + [("chunk", i32), ("flags", i32), ("pad_", i32)])


OPTIM16_NEAREST = 1                     # zigma_optim16_params_t.flags


class SdeState(C.Structure):            # the device state block of a trajectory's noise (four 4-byte words)
    _fields_ = [(n, C.c_uint32) for n in ("seed_lo", "seed_hi", "stream", "step")]


class SdeStepParams(C.Structure):
    _fields_ = ([(n, i64) for n in ("n", "elem_offset", "coef_rows")] + [(n, i32) for n in ("dtype", "flags", "rows_per_step", "row")]
                + [(n, vp) for n in ("a", "b", "c", "out", "coef", "state", "bits_out")])


class SdeAdvanceParams(C.Structure):
    _fields_ = [("state", vp), ("times", vp), ("t_out", vp), ("n_rows", i64), ("n_t", i32), ("batch", i32), ("flags", i32), ("pad_", i32)]


SDE_ROW_ABSOLUTE = 1                    # zigma_sde_step_params_t.flags

EXPORTS = ("zigma_sde_step_fwd", "zigma_sde_advance", "zigma_optim_grad_sumsq", "zigma_optim_prepare", "zigma_optim_adamw", "zigma_optim16_grad_sumsq", "zigma_optim16_adamw", "zigma_multi_cast_fwd", "zigma_linear_fwd", "zigma_norm_linear_fwd", "zigma_linear_f32_split", "zigma_linear_wgrad","zigma_linear_wgrad_workspace_bytes", "zigma_conv_x_proj_fwd", "zigma_scale_reduce_bwd", "zigma_selective_scan_fwd", "zigma_causal_conv1d_fwd", "zigma_add_norm_fwd", "zigma_dt_proj_softplus_fwd", "zigma_cross_attn_fwd", "zigma_x_proj_fwd", "zigma_selective_scan_bwd",
           "zigma_selective_scan_bwd_workspace_bytes", "zigma_causal_conv1d_bwd",
           "zigma_causal_conv1d_bwd_workspace_bytes", "zigma_add_norm_bwd", "zigma_add_norm_bwd_workspace_bytes",
           "zigma_strerror",
           "zigma_cross_attn_bwd", "zigma_cross_attn_bwd_chunks", "zigma_patch_embed_fwd", "zigma_timestep_embed_fwd", "zigma_final_layer_fwd",
           "zigma_final_layer_cfg_fwd", "zigma_skinny_linear_fwd", "zigma_calib_launch", "zigma_abi_version", "zigma_last_kernel",
           "zigma_selective_scan_fwd_plan", "zigma_causal_conv1d_fwd_plan", "zigma_conv_x_proj_fwd_plan", "zigma_x_proj_fwd_plan",
           "zigma_dt_proj_softplus_fwd_plan", "zigma_linear_fwd_plan", "zigma_norm_linear_fwd_plan", "zigma_linear_f32_split_plan",
           "zigma_patch_embed_fwd_plan", "zigma_timestep_embed_fwd_plan", "zigma_skinny_linear_fwd_plan", "zigma_final_layer_fwd_plan", "zigma_final_layer_cfg_fwd_plan",
           "zigma_cross_attn_fwd_plan", "zigma_cross_attn_bwd_plan", "zigma_scale_reduce_bwd_plan", "zigma_linear_wgrad_plan",
           "zigma_add_norm_fwd_plan", "zigma_add_norm_bwd_plan", "zigma_selective_scan_bwd_plan", "zigma_causal_conv1d_bwd_plan")

_lib = None


def lib():
    """Load the shared library once; raise (never fall back) if it is not there."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"zigma_amd: {LIB_PATH} not built — run `python -m zigma_amd.build` (hipcc, gfx950). "
                "There is no CPU or eager fallback for the HIP ops.")
        L = C.CDLL(LIB_PATH)
        for name, st in (("zigma_selective_scan_fwd", ScanParams), ("zigma_causal_conv1d_fwd", ConvParams),
                         ("zigma_add_norm_fwd", NormParams), ("zigma_dt_proj_softplus_fwd", DtProjParams),
                         ("zigma_selective_scan_bwd", ScanBwdParams), ("zigma_causal_conv1d_bwd", ConvBwdParams),
                         ("zigma_add_norm_bwd", NormBwdParams), ("zigma_cross_attn_fwd", XAttnParams), ("zigma_cross_attn_bwd", XAttnBwdParams), ("zigma_patch_embed_fwd", PatchEmbedParams),
                         ("zigma_timestep_embed_fwd", TimestepEmbedParams), ("zigma_final_layer_fwd", FinalLayerParams), ("zigma_final_layer_cfg_fwd", FinalLayerCfgParams), ("zigma_skinny_linear_fwd", SkinnyParams), ("zigma_x_proj_fwd", XProjParams),
                         ("zigma_linear_fwd", LinearParams), ("zigma_conv_x_proj_fwd", ConvXProjParams), ("zigma_scale_reduce_bwd", GlueBwdParams), ("zigma_calib_launch", CalibParams),
                         ("zigma_linear_wgrad", LinearWgradParams), ("zigma_linear_f32_split", LinearSplitParams), ("zigma_norm_linear_fwd", NormLinearParams),
                         ("zigma_multi_cast_fwd", MultiCastParams), ("zigma_optim_grad_sumsq", OptimParams), ("zigma_optim_prepare", OptimParams),
                         ("zigma_optim_adamw", OptimParams), ("zigma_optim16_grad_sumsq", Optim16Params), ("zigma_optim16_adamw", Optim16Params), ("zigma_sde_step_fwd", SdeStepParams), ("zigma_sde_advance", SdeAdvanceParams)):
            fn = getattr(L, name)
            fn.argtypes = [C.POINTER(st), vp]
            fn.restype = C.c_int
        for name, st in (("zigma_selective_scan_bwd_workspace_bytes", ScanBwdParams),
                         ("zigma_causal_conv1d_bwd_workspace_bytes", ConvBwdParams),
                         ("zigma_add_norm_bwd_workspace_bytes", NormBwdParams),
                         ("zigma_linear_wgrad_workspace_bytes", LinearWgradParams)):
            fn = getattr(L, name)
            fn.argtypes = [C.POINTER(st)]
            fn.restype = C.c_int64
        for name, st in (("zigma_selective_scan_fwd", ScanParams), ("zigma_causal_conv1d_fwd", ConvParams), ("zigma_conv_x_proj_fwd", ConvXProjParams),
                         ("zigma_x_proj_fwd", XProjParams), ("zigma_dt_proj_softplus_fwd", DtProjParams), ("zigma_linear_fwd", LinearParams),
                         ("zigma_norm_linear_fwd", NormLinearParams), ("zigma_linear_f32_split", LinearSplitParams),
                         ("zigma_patch_embed_fwd", PatchEmbedParams), ("zigma_timestep_embed_fwd", TimestepEmbedParams), ("zigma_skinny_linear_fwd", SkinnyParams),
                         ("zigma_final_layer_fwd", FinalLayerParams), ("zigma_final_layer_cfg_fwd", FinalLayerCfgParams), ("zigma_cross_attn_fwd", XAttnParams),
                         ("zigma_cross_attn_bwd", XAttnBwdParams), ("zigma_scale_reduce_bwd", GlueBwdParams), ("zigma_linear_wgrad", LinearWgradParams),
                         ("zigma_add_norm_fwd", NormParams), ("zigma_add_norm_bwd", NormBwdParams), ("zigma_selective_scan_bwd", ScanBwdParams),
                         ("zigma_causal_conv1d_bwd", ConvBwdParams)):
            fn = getattr(L, name + "_plan")
            fn.argtypes = [C.POINTER(st), C.POINTER(C.c_char_p)]
            fn.restype = C.c_int
        L.zigma_cross_attn_bwd_chunks.argtypes = [C.c_int]
        L.zigma_cross_attn_bwd_chunks.restype = C.c_int
        L.zigma_strerror.argtypes = [C.c_int]
        L.zigma_strerror.restype = C.c_char_p
        L.zigma_abi_version.restype = C.c_int
        L.zigma_last_kernel.restype = C.c_char_p
        if L.zigma_abi_version() != 11:
            raise RuntimeError("zigma_amd: libzigma_hip.so ABI version mismatch")
        _lib = L
    return _lib


def last_kernel():
    return lib().zigma_last_kernel().decode()


def dtype_id(t):
    try:
        return _DT[t.dtype]
    except KeyError:
        raise RuntimeError(f"zigma_amd: unsupported dtype {t.dtype}")


def ptr(t):
    return None if t is None else t.data_ptr()


def require_device(*tensors):
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("zigma_amd: HIP kernels need tensors on a GPU device (no CPU fallback); got a "
                               f"{t.device} tensor")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError("zigma_amd: all tensors must be on the same device")
    return dev


FRESH_ADDRESS = 1 << 40     # placeholder address of a tensor that is yet to be allocated (the k-th stand-in of a block: k times this)


class Desc:
    """What the block builders read of a tensor (shape, strides, dtype, address), for the plan queries: of a tensor that exists (`of`), or of
    contiguous rows the front is yet to allocate (`fresh`), with the views mamba_inner_tok takes of u and x_dbl.  A fresh tensor's address is a
    placeholder — non-zero, on a page boundary (the caching allocator hands out blocks on 512-byte boundaries, the plans ask for 16 bytes at
    most) and 1 TiB from the next one, so no two overlap.  A block built on placeholders is asked about; before one is launched, every address
    in it is set from the real tensors (scan_planned, linear_planned).  The ONE stand-in type of the package: the shadows of amp.py (amp.Like) and the
    transposed weight of wgrad.py are `fresh` descriptors too, and read like a tensor that requires no grad."""
    __slots__ = ("dtype", "shape", "strides", "address", "is_cuda", "requires_grad")

    def __init__(self, dtype, shape, strides, address, is_cuda=True, requires_grad=False):
        self.dtype, self.shape, self.strides, self.address, self.is_cuda, self.requires_grad = dtype, shape, strides, address, is_cuda, requires_grad

    @classmethod
    def of(cls, t):
        if isinstance(t, cls):
            return t
        return cls(t.dtype, tuple(t.shape), tuple([t.stride(i) for i in range(t.dim())]), t.data_ptr(), t.is_cuda)

    @classmethod
    def fresh(cls, like, shape, k, dtype=None):
        """contiguous rows of this shape in like's dtype and on its device (like None: dtype, on the device) at the k-th placeholder address"""
        strides, n = [], 1
        for d in reversed(shape):
            strides.append(n)
            n *= d
        return cls(dtype or like.dtype, tuple(shape), tuple(reversed(strides)), k * FRESH_ADDRESS, like is None or like.is_cuda)

    def stride(self, i=None):
        return self.strides if i is None else self.strides[i]

    def dim(self):
        return len(self.shape)

    def data_ptr(self):
        return self.address

    def numel(self):
        return math.prod(self.shape)

    def is_contiguous(self):
        n = 1
        for d, st in zip(reversed(self.shape), reversed(self.strides)):
            if d != 1 and st != n:
                return False
            n *= d
        return True

    def scan_view(self):
        """(B, L, C) rows as the scan's (batch, dim, seqlen) operand: t.transpose(1, 2)"""
        (B, L, C), (sb, sl, sc) = self.shape, self.strides
        return Desc(self.dtype, (B, C, L), (sb, sc, sl), self.address, self.is_cuda)

    def columns(self, first, n):
        """columns [first, first + n) of (B, L, C) rows as the scan's (batch, 1, dstate, seqlen) B / C operand:
        t[:, :, first:first + n].transpose(1, 2).unsqueeze(1)"""
        (B, L, _), (sb, sl, sc) = self.shape, self.strides
        return Desc(self.dtype, (B, 1, n, L), (sb, n * sc, sc, sl), self.address + first * sc * self.dtype.itemsize, self.is_cuda)


def workspace(fn_name, params, device):
    """Allocate the caller-owned scratch buffer a backward entry point asks for and attach it to the parameter block."""
    nbytes = getattr(lib(), fn_name + "_workspace_bytes")(C.byref(params))
    ws = torch.empty(max(int(nbytes), 16), device=device, dtype=torch.uint8)
    params.workspace, params.workspace_bytes = ws.data_ptr(), nbytes
    return ws


GRID_DIM_MAX = 65535        # a 16-bit grid dimension: the batch of one zigma_selective_scan_bwd / zigma_causal_conv1d_bwd launch (kBwdMaxBatch of csrc/bwd_plan.h)
                            # and of the scan's single grid (csrc/scan_plan.h)


def sum_over_batch_slices(batch, run):
    """A batch past GRID_DIM_MAX goes to the backward kernels in slices: run(a, b) launches on samples [a, b) — per-sample outputs land in views of one
    allocation — and returns its parameter gradients (a tuple; None where there is none) -> their sums over the slices"""
    total = None
    for a in range(0, batch, GRID_DIM_MAX):
        part = run(a, min(a + GRID_DIM_MAX, batch))
        total = part if total is None else tuple(None if t is None or q is None else t + q for t, q in zip(total, part))
    return total


def checkpoint_shape(batch, dim, seqlen, dstate):
    """[batch][dim / 64][ceil(seqlen / 16)][dstate][64] fp32: the states before every 16-step tile, which the token-major forward scan writes for
    zigma_selective_scan_bwd; None where that backward does not take the shape (plan_scan_bwd() of csrc/bwd_plan.h: dim % 64, dstate 8 or 16)"""
    return (batch, dim // 64, (seqlen + 15) // 16, dstate, 64) if dim % 64 == 0 and dstate in (8, 16) else None


_PLAN_FNS = {}


def plan(fn_name, params):
    """Ask the library what the entry point `fn_name` would do with this parameter block -> (status, kernel name or None): the status the launch
    would return and what zigma_last_kernel() would report after it (None: a refusal or an empty call).  The five forward entry points of the Mamba
    inner answer (plan_scan() of csrc/scan_plan.h, the plans of csrc/front_plan.h) and the three of the dense projections (plan_linear() and
    plan_linear_split() of csrc/linear_plan.h, plan_norm_linear() of csrc/norm_linear_plan.h), the operators around the blocks (csrc/outer_plan.h),
    cross-attention in both directions and the glue backward (csrc/attn_plan.h), the weight gradient (csrc/wgrad_plan.h), add-norm in both directions
    (csrc/norm_plan.h) and the scan and conv backward (csrc/bwd_plan.h).  Host only: nothing is launched or
    dereferenced, so the block may describe tensors that are yet to be allocated."""
    fn = _PLAN_FNS.get(fn_name)
    if fn is None:
        fn = _PLAN_FNS[fn_name] = getattr(lib(), fn_name + "_plan")
    kernel = C.c_char_p()
    rc = fn(C.byref(params), C.byref(kernel))
    name = kernel.value
    return rc, name.decode() if name else None


def served(fn_name, params):
    """the entry point would launch a kernel for this block (not a refusal, not an empty call)"""
    status, kernel = plan(fn_name, params)
    return status == 0 and kernel is not None


TRACE = None        # tests / tools: set to a list to receive (entry point, kernel that served it, parameter block) per call


def call(fn_name, params, device):
    L = lib()
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device).cuda_stream
        rc = getattr(L, fn_name)(C.byref(params), C.c_void_p(stream))
    if rc != 0:
        raise RuntimeError(f"{fn_name}: {L.zigma_strerror(rc).decode()} (status {rc})")
    if TRACE is not None:
        TRACE.append((fn_name, L.zigma_last_kernel().decode(), params))

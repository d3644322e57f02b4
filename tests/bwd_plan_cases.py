"""The dispatch tables of the four entry points of the training path that answer a plan query last: plan_add_norm(), plan_add_norm_bwd()
(zigma_amd/csrc/norm_plan.h), plan_scan_bwd() and plan_conv_bwd() (csrc/bwd_plan.h) — one case per leaf of the plans: every refusal clause, the empty
calls, every serving leaf at the smallest shape that tells it from its neighbour.

Each case is a small call of the product's own block builder (layernorm.norm_block / norm_bwd_block, selective_scan_interface.scan_bwd_block,
causal_conv1d_interface.conv_bwd_block) on real operands and outputs, with the workspace the library asks for attached, and what the library reports
for it: status and zigma_last_kernel().  A refusal case breaks its check AND a later one where it can, so that two checks in the wrong order change its
status.  test_host_cpu.py checks the table against the plans compiled with g++ and the built library's queries, test_gpu_bwd_plan_query.py against the
launches on the GPU.
"""
from collections import namedtuple

import torch

from zigma_amd import _lib

Expect = namedtuple("Expect", "status kernel")      # kernel None: nothing launched, nothing reported
OK, NULL, SHAPE, DTYPE, STRIDE, UNSUPPORTED = 0, -1, -2, -3, -4, -6
BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
NO_DTYPE = 7                                        # no zigma_dtype_t


def _ok(kernel):
    return Expect(OK, kernel)


def _no(status):
    return Expect(status, None)


def _plus(field, n):
    """patch value: what the builder wrote (a pointer, a size), moved by n"""
    return lambda P: getattr(P, field) + n


V8X4, V4, V1, NB, SB, CB = "add_norm_v8x4", "add_norm_v4", "add_norm_v1", "add_norm_bwd", "scan_bwd_tok", "conv_bwd_tok"
# name: (entry, case, expected).  patch: parameter-block fields set after the builder has filled the block; only refused and empty cases carry one, so
# nothing is ever launched on a block that does not describe its tensors.  set: fields of a SERVED case the builders have no argument for (they still
# describe the tensors).  Defaults of the entries: see their builders below.
CASES = {
    # -- zigma_add_norm_fwd: bf16, 4 rows of 128, weight, y only ("full": gated branch, x_out, residual in and out, bias, y and modulated y)
    "an_null_x": ("add_norm_fwd", dict(patch=dict(x=None, cols=0)), _no(NULL)),
    "an_null_gate_without_branch": ("add_norm_fwd", dict(full=True, patch=dict(gate=None, cols=0)), _no(NULL)),
    "an_null_branch_without_gate": ("add_norm_fwd", dict(full=True, patch=dict(branch=None, cols=0)), _no(NULL)),
    "an_null_scale_without_shift": ("add_norm_fwd", dict(full=True, patch=dict(shift=None, cols=0)), _no(NULL)),
    "an_null_y_mod_with_shift": ("add_norm_fwd", dict(full=True, patch=dict(y_mod=None, cols=0)), _no(NULL)),
    "an_null_no_output": ("add_norm_fwd", dict(patch=dict(y_out=None, cols=0)), _no(NULL)),
    "an_shape_negative_rows": ("add_norm_fwd", dict(patch=dict(rows=-1, flags=2)), _no(SHAPE)),
    "an_shape_cols_0": ("add_norm_fwd", dict(patch=dict(cols=0, flags=2)), _no(SHAPE)),
    "an_shape_rows_per_batch_0": ("add_norm_fwd", dict(patch=dict(rows_per_batch=0, flags=2)), _no(SHAPE)),
    "an_unsupported_flag_2_on_empty": ("add_norm_fwd", dict(patch=dict(rows=0, flags=2, x_dtype=NO_DTYPE)), _no(UNSUPPORTED)),
    "an_empty": ("add_norm_fwd", dict(patch=dict(rows=0, x_dtype=NO_DTYPE)), Expect(OK, None)),
    "an_dtype_x_none": ("add_norm_fwd", dict(patch=dict(x_dtype=NO_DTYPE, cols=4100)), _no(DTYPE)),
    "an_dtype_mod_f16_of_bf16": ("add_norm_fwd", dict(full=True, patch=dict(mod_dtype=_lib.F16, cols=4100)), _no(DTYPE)),
    "an_dtype_res_f16_of_bf16": ("add_norm_fwd", dict(patch=dict(res_dtype=_lib.F16, cols=4100)), _no(DTYPE)),
    "an_dtype_w_f16_of_bf16": ("add_norm_fwd", dict(patch=dict(w_dtype=_lib.F16, cols=4100)), _no(DTYPE)),
    "an_shape_cols_4100": ("add_norm_fwd", dict(cols=4100), _no(SHAPE)),
    "an_shape_cols_4097_unaligned": ("add_norm_fwd", dict(cols=4097), _no(SHAPE)),
    **{f"an_served_rows_4_cols_{c}": ("add_norm_fwd", dict(cols=c), _ok(k)) for c, k in ((8, V4), (128, V8X4), (1024, V8X4), (1028, V4), (4096, V4))},
    **{f"an_served_rows_5_cols_{c}": ("add_norm_fwd", dict(rows=5, cols=c), _ok(V4)) for c in (128, 1024)},
    "an_served_one_row_per_wave_flag": ("add_norm_fwd", dict(set=dict(flags=1)), _ok(V4)),
    "an_served_mod_dtype_unread_without_modulation": ("add_norm_fwd", dict(set=dict(mod_dtype=_lib.F16)), _ok(V8X4)),
    "an_served_full_16_bit_residual": ("add_norm_fwd", dict(full=True, res=BF), _ok(V8X4)),
    "an_served_full_fp32_residual": ("add_norm_fwd", dict(full=True, res=F32), _ok(V4)),
    "an_served_full_fp32_residual_fp32_weight_f16": ("add_norm_fwd", dict(dtype=F16, full=True, res=F32, wdt=F32, cols=1024), _ok(V4)),
    "an_served_fp32_residual_16_bytes_in": ("add_norm_fwd", dict(full=True, res=F32, res_off=4), _ok(V4)),
    "an_served_fp32_weight_16_bytes_in": ("add_norm_fwd", dict(wdt=F32, w_off=4), _ok(V4)),
    "an_served_f32": ("add_norm_fwd", dict(dtype=F32), _ok(V4)),
    "an_served_f32_plus_1_element": ("add_norm_fwd", dict(dtype=F32, off=1), _ok(V1)),
    **{f"an_served_plus_1_element_cols_{c}": ("add_norm_fwd", dict(off=1, cols=c), _ok(V1)) for c in (128, 1028, 4096)},
    **{f"an_served_plus_4_elements_cols_{c}": ("add_norm_fwd", dict(off=4, cols=c), _ok(V4)) for c in (128, 1028)},
    "an_served_plus_8_elements": ("add_norm_fwd", dict(off=8, full=True), _ok(V8X4)),
    # -- zigma_add_norm_bwd: bf16 x with the fp32 residual stream, 5 rows of 768, weight and bias, incoming residual gradient, dx and dresidual
    "nb_shape_negative_rows": ("add_norm_bwd", dict(patch=dict(rows=-1, flags=1)), _no(SHAPE)),
    "nb_shape_cols_0": ("add_norm_bwd", dict(patch=dict(cols=0, flags=1)), _no(SHAPE)),
    "nb_unsupported_flag_on_empty": ("add_norm_bwd", dict(patch=dict(rows=0, flags=1, xsum=None)), _no(UNSUPPORTED)),
    "nb_empty": ("add_norm_bwd", dict(patch=dict(rows=0, xsum=None)), Expect(OK, None)),
    "nb_null_xsum": ("add_norm_bwd", dict(patch=dict(xsum=None, x_dtype=NO_DTYPE)), _no(NULL)),
    "nb_null_dy": ("add_norm_bwd", dict(patch=dict(dy=None, x_dtype=NO_DTYPE)), _no(NULL)),
    "nb_null_neither_dx_nor_dresidual": ("add_norm_bwd", dict(patch=dict(dx=None, dresidual=None, x_dtype=NO_DTYPE)), _no(NULL)),
    "nb_null_workspace": ("add_norm_bwd", dict(patch=dict(workspace=None, x_dtype=NO_DTYPE)), _no(NULL)),
    "nb_null_workspace_4_bytes_short": ("add_norm_bwd", dict(patch=dict(workspace_bytes=_plus("workspace_bytes", -4), x_dtype=NO_DTYPE)), _no(NULL)),
    "nb_dtype_x_none": ("add_norm_bwd", dict(patch=dict(x_dtype=NO_DTYPE, cols=2052, workspace_bytes=1 << 30)), _no(DTYPE)),
    "nb_dtype_res_f16_of_bf16": ("add_norm_bwd", dict(patch=dict(res_dtype=_lib.F16, cols=2052, workspace_bytes=1 << 30)), _no(DTYPE)),
    "nb_dtype_w_f16_of_bf16": ("add_norm_bwd", dict(patch=dict(w_dtype=_lib.F16, cols=2052, workspace_bytes=1 << 30)), _no(DTYPE)),      # (the size a block of 2052 columns would claim: nothing is launched)
    "nb_shape_cols_2052": ("add_norm_bwd", dict(cols=2052), _no(SHAPE)),
    "nb_shape_cols_2049_unaligned": ("add_norm_bwd", dict(cols=2049), _no(SHAPE)),
    **{f"nb_served_cols_{c}": ("add_norm_bwd", dict(cols=c), _ok(NB)) for c in (768, 772, 2048)},
    **{f"nb_served_pitch_plus_1_cols_{c}": ("add_norm_bwd", dict(cols=c, pad=1), _ok(NB)) for c in (256, 260, 768, 772, 2048)},
    "nb_served_plus_1_element_cols_256": ("add_norm_bwd", dict(cols=256, off=1), _ok(NB)),
    "nb_served_2049_rows_of_8_f16_no_weight_dx_only": ("add_norm_bwd", dict(dtype=F16, res=F16, rows=2049, cols=8, weight=False, dres_out=False, want_dres=False), _ok(NB)),
    "nb_served_f32_dresidual_only": ("add_norm_bwd", dict(dtype=F32, cols=772, want_dx=False), _ok(NB)),
    # -- zigma_selective_scan_bwd: bf16, batch 2, dim 64, 32 steps (two tiles), 16 states, z, D, delta_bias, own checkpoints
    "sb_shape_negative_seqlen": ("selective_scan_bwd", dict(patch=dict(seqlen=-1, flags=1)), _no(SHAPE)),
    "sb_shape_negative_batch": ("selective_scan_bwd", dict(patch=dict(batch=-1, flags=1)), _no(SHAPE)),
    "sb_unsupported_flag_on_empty": ("selective_scan_bwd", dict(patch=dict(flags=1, batch=0, dim=96)), _no(UNSUPPORTED)),
    "sb_shape_dim_96": ("selective_scan_bwd", dict(patch=dict(dim=96, u=None)), _no(SHAPE)),
    "sb_shape_dstate_4": ("selective_scan_bwd", dict(patch=dict(dstate=4, u=None)), _no(SHAPE)),
    "sb_shape_batch_65536": ("selective_scan_bwd", dict(patch=dict(batch=65536, u=None)), _no(SHAPE)),
    "sb_shape_reset_period_8": ("selective_scan_bwd", dict(patch=dict(reset_period=8, u=None)), _no(SHAPE)),
    "sb_shape_negative_reset_period": ("selective_scan_bwd", dict(patch=dict(reset_period=-16, u=None)), _no(SHAPE)),
    "sb_empty_no_samples": ("selective_scan_bwd", dict(patch=dict(batch=0, u=None)), Expect(OK, None)),
    "sb_empty_no_steps": ("selective_scan_bwd", dict(patch=dict(seqlen=0, u=None)), Expect(OK, None)),
    "sb_null_u": ("selective_scan_bwd", dict(patch=dict(u=None, workspace=_plus("workspace", 8))), _no(NULL)),
    "sb_null_dC": ("selective_scan_bwd", dict(patch=dict(dC=None, workspace=_plus("workspace", 8))), _no(NULL)),
    "sb_null_out_with_z": ("selective_scan_bwd", dict(patch=dict(out=None, workspace=_plus("workspace", 8))), _no(NULL)),
    "sb_null_dz_with_z": ("selective_scan_bwd", dict(patch=dict(dz=None, workspace=_plus("workspace", 8))), _no(NULL)),
    "sb_null_dD_with_D": ("selective_scan_bwd", dict(patch=dict(dD=None, workspace=_plus("workspace", 8))), _no(NULL)),
    "sb_null_ddelta_bias_with_delta_bias": ("selective_scan_bwd", dict(patch=dict(ddelta_bias=None, workspace=_plus("workspace", 8))), _no(NULL)),
    "sb_null_workspace": ("selective_scan_bwd", dict(patch=dict(workspace=None, u_l_stride=-64)), _no(NULL)),
    "sb_null_workspace_4_bytes_short": ("selective_scan_bwd", dict(patch=dict(workspace_bytes=_plus("workspace_bytes", -4), workspace=_plus("workspace", 8))), _no(NULL)),
    "sb_stride_workspace_plus_8_bytes": ("selective_scan_bwd", dict(patch=dict(workspace=_plus("workspace", 8), io_dtype=NO_DTYPE)), _no(STRIDE)),
    "sb_stride_negative_pitch": ("selective_scan_bwd", dict(patch=dict(u_l_stride=-64, io_dtype=NO_DTYPE)), _no(STRIDE)),
    "sb_stride_pitch_past_2_31_bytes": ("selective_scan_bwd", dict(patch=dict(C_l_stride=1 << 26, io_dtype=NO_DTYPE)), _no(STRIDE)),      # 31 x 2^26 x 2 bytes
    "sb_dtype_none": ("selective_scan_bwd", dict(patch=dict(io_dtype=NO_DTYPE)), _no(DTYPE)),
    "sb_served_16_states": ("selective_scan_bwd", dict(), _ok(SB)),
    "sb_served_8_states": ("selective_scan_bwd", dict(N=8), _ok(SB)),
    "sb_served_16_states_no_z_no_D_no_delta_bias": ("selective_scan_bwd", dict(z=False, D=False, bias=False), _ok(SB)),
    "sb_served_8_states_forward_checkpoints": ("selective_scan_bwd", dict(N=8, ck=True), _ok(SB)),
    "sb_served_f16_reset_period_16": ("selective_scan_bwd", dict(dtype=F16, reset=16, ck=True), _ok(SB)),
    "sb_served_f32_33_steps": ("selective_scan_bwd", dict(dtype=F32, L=33), _ok(SB)),
    # -- zigma_causal_conv1d_bwd: bf16, batch 2, 16 positions, dim 8, width 4, SiLU, bias, taps in bf16
    "cb_shape_width_5": ("causal_conv1d_bwd", dict(patch=dict(width=5, flags=1)), _no(SHAPE)),
    "cb_shape_width_1": ("causal_conv1d_bwd", dict(patch=dict(width=1, flags=1)), _no(SHAPE)),
    "cb_shape_negative_dim": ("causal_conv1d_bwd", dict(patch=dict(dim=-8, flags=1)), _no(SHAPE)),
    "cb_shape_batch_65536": ("causal_conv1d_bwd", dict(patch=dict(batch=65536, flags=1)), _no(SHAPE)),
    "cb_unsupported_flag_on_empty": ("causal_conv1d_bwd", dict(patch=dict(flags=1, seqlen=0, reset_period=8)), _no(UNSUPPORTED)),
    "cb_shape_reset_period_8": ("causal_conv1d_bwd", dict(patch=dict(reset_period=8, x=None)), _no(SHAPE)),
    "cb_empty_no_positions": ("causal_conv1d_bwd", dict(patch=dict(seqlen=0, x=None)), Expect(OK, None)),
    "cb_null_x": ("causal_conv1d_bwd", dict(patch=dict(x=None, x_l_stride=6)), _no(NULL)),
    "cb_null_dweight": ("causal_conv1d_bwd", dict(patch=dict(dweight=None, x_l_stride=6)), _no(NULL)),
    "cb_null_dbias_with_bias": ("causal_conv1d_bwd", dict(patch=dict(dbias=None, x_l_stride=6)), _no(NULL)),
    "cb_null_workspace": ("causal_conv1d_bwd", dict(patch=dict(workspace=None, x_l_stride=6)), _no(NULL)),
    "cb_null_workspace_4_bytes_short": ("causal_conv1d_bwd", dict(patch=dict(workspace_bytes=_plus("workspace_bytes", -4), x_l_stride=6)), _no(NULL)),
    "cb_stride_dim_6": ("causal_conv1d_bwd", dict(patch=dict(dim=6, io_dtype=NO_DTYPE)), _no(STRIDE)),
    "cb_stride_pitch_6": ("causal_conv1d_bwd", dict(patch=dict(x_l_stride=6, io_dtype=NO_DTYPE)), _no(STRIDE)),
    "cb_stride_dout_batch_stride_130": ("causal_conv1d_bwd", dict(patch=dict(dout_batch_stride=130, io_dtype=NO_DTYPE)), _no(STRIDE)),
    "cb_stride_negative_pitch": ("causal_conv1d_bwd", dict(patch=dict(dout_l_stride=-8, io_dtype=NO_DTYPE)), _no(STRIDE)),
    "cb_stride_pitch_past_2_31_bytes": ("causal_conv1d_bwd", dict(patch=dict(dx_l_stride=1 << 27, w_dtype=NO_DTYPE)), _no(STRIDE)),        # 16 x 2^27 x 2 bytes
    "cb_stride_x_plus_4_bytes": ("causal_conv1d_bwd", dict(patch=dict(x=_plus("x", 4), w_dtype=NO_DTYPE)), _no(STRIDE)),
    "cb_stride_f32_dx_plus_8_bytes": ("causal_conv1d_bwd", dict(dtype=F32, patch=dict(dx=_plus("dx", 8), w_dtype=NO_DTYPE)), _no(STRIDE)),
    "cb_dtype_io_none": ("causal_conv1d_bwd", dict(patch=dict(io_dtype=NO_DTYPE)), _no(DTYPE)),
    "cb_dtype_taps_none": ("causal_conv1d_bwd", dict(patch=dict(w_dtype=NO_DTYPE)), _no(DTYPE)),
    "cb_served_width_4_silu_bias": ("causal_conv1d_bwd", dict(), _ok(CB)),
    "cb_served_width_3_no_silu": ("causal_conv1d_bwd", dict(width=3, silu=False), _ok(CB)),
    "cb_served_width_2_no_bias_fp32_taps": ("causal_conv1d_bwd", dict(width=2, bias=False, wdt=F32), _ok(CB)),
    "cb_served_f16_width_4_no_silu_fp32_taps": ("causal_conv1d_bwd", dict(dtype=F16, silu=False, wdt=F32), _ok(CB)),
    "cb_served_f32_width_3": ("causal_conv1d_bwd", dict(dtype=F32, width=3), _ok(CB)),
    "cb_served_129_positions_row_table": ("causal_conv1d_bwd", dict(L=129, perm=True), _ok(CB)),
    "cb_served_reset_period_16": ("causal_conv1d_bwd", dict(L=32, reset=16), _ok(CB)),
}
ENTRY = {e: "zigma_" + e for e in {c[0] for c in CASES.values()}}
# the fields of each block that hold the addresses of tensors the wrapper allocates itself: what a launched block may differ in from the one asked about
ALLOCATED = {"add_norm_fwd": ("y_out", "residual_out", "y_mod"), "add_norm_bwd": ("dx", "dresidual", "dweight", "dbias", "workspace"),
             "selective_scan_bwd": ("du", "ddelta", "dz", "dA", "dB", "dC", "dD", "ddelta_bias", "workspace"),
             "causal_conv1d_bwd": ("dx", "dweight", "dbias", "workspace")}
OWN_LAYOUT = ("off", "res_off", "w_off", "set")      # cases whose outputs have a layout the wrappers do not allocate, or fields they do not set: launched on the case's own block
# (VEC, ITERS, LPR) of the add-norm cases that are served
INSTANTIATION = {
    "an_served_rows_4_cols_8": (8, 2, 64), "an_served_rows_4_cols_128": (8, 1, 16), "an_served_rows_4_cols_1024": (8, 8, 16), "an_served_rows_4_cols_1028": (4, 16, 64),
    "an_served_rows_4_cols_4096": (4, 16, 64), "an_served_rows_5_cols_128": (8, 2, 64), "an_served_rows_5_cols_1024": (8, 2, 64),
    "an_served_one_row_per_wave_flag": (8, 2, 64), "an_served_mod_dtype_unread_without_modulation": (8, 1, 16), "an_served_full_16_bit_residual": (8, 1, 16),
    "an_served_full_fp32_residual": (8, 2, 64), "an_served_full_fp32_residual_fp32_weight_f16": (8, 2, 64), "an_served_fp32_residual_16_bytes_in": (8, 2, 64),
    "an_served_fp32_weight_16_bytes_in": (4, 4, 64), "an_served_f32": (4, 4, 64), "an_served_f32_plus_1_element": (1, 16, 64),
    "an_served_plus_1_element_cols_128": (1, 16, 64), "an_served_plus_1_element_cols_1028": (1, 64, 64), "an_served_plus_1_element_cols_4096": (1, 64, 64),
    "an_served_plus_4_elements_cols_128": (4, 4, 64), "an_served_plus_4_elements_cols_1028": (4, 16, 64), "an_served_plus_8_elements": (8, 1, 16),
    "nb_served_cols_768": (4, 3, 64), "nb_served_cols_772": (4, 8, 64), "nb_served_cols_2048": (4, 8, 64), "nb_served_pitch_plus_1_cols_256": (1, 4, 64),
    "nb_served_pitch_plus_1_cols_260": (1, 12, 64), "nb_served_pitch_plus_1_cols_768": (1, 12, 64), "nb_served_pitch_plus_1_cols_772": (1, 32, 64),
    "nb_served_pitch_plus_1_cols_2048": (1, 32, 64), "nb_served_plus_1_element_cols_256": (1, 4, 64), "nb_served_2049_rows_of_8_f16_no_weight_dx_only": (4, 3, 64),
    "nb_served_f32_dresidual_only": (4, 8, 64),
}


def _rand(g, device, dtype, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(device=device, dtype=dtype)


def _rows(g, device, dtype, rows, cols, off=0, pad=0, fill=True):
    """(rows, cols) rows cols + pad elements apart, `off` elements into their allocation: random, or uninitialised (an output)"""
    n = rows * (cols + pad) + off
    wide = _rand(g, device, dtype, n) if fill else torch.empty(n, device=device, dtype=dtype)
    return wide[off:].view(rows, cols + pad)[:, :cols]


# Every builder below returns (args, kwargs, outs, call): the operands of the product's block builder in their order, its keywords, the outputs the block
# points to as keywords of the block builder, and the wrapper's call on the same operands (it allocates the outputs itself).
def _add_norm_fwd(c, dev, g):
    from zigma_amd import layernorm
    c = {**dict(dtype=BF, rows=4, cols=128, full=False, res=None, wdt=None, off=0, res_off=None, w_off=None), **c}
    dt, rows, cols, off = c["dtype"], c["rows"], c["cols"], c["off"]
    res_off, w_off, wdt = (c["res_off"] if c["res_off"] is not None else off), (c["w_off"] if c["w_off"] is not None else off), c["wdt"] or dt
    row = lambda d=dt, o=off, fill=True: _rows(g, dev, d, rows, cols, o, fill=fill)
    vec = lambda d, o: _rows(g, dev, d, 1, cols, o)[0]
    full, mod = c["full"], _rows(g, dev, dt, 2, 3 * cols, off) if c["full"] else None
    residual = row(c["res"], res_off) if c["res"] is not None else None
    args = (row(), vec(wdt, w_off), vec(wdt, w_off) if full else None, residual, 1e-5, True, c["res"])
    kwargs = dict(rows_per_batch=rows // 2 if full else None)
    if full:
        kwargs.update(branch=row(), gate=mod[:, :cols], shift=mod[:, cols:2 * cols], scale=mod[:, 2 * cols:])
    outs = dict(x_out=row(fill=False) if full else None, y=row(fill=False), res_out=row(c["res"], res_off, fill=False) if c["res"] is not None else None, y_mod=row(fill=False) if full else None)
    return args, kwargs, outs, lambda: layernorm._norm_call(*args, **kwargs, x_out=outs["x_out"], want_y=True, want_res=c["res"] is not None)


def _add_norm_bwd(c, dev, g):
    from zigma_amd import layernorm
    c = {**dict(dtype=BF, res=F32, wdt=None, rows=5, cols=768, weight=True, bias=True, dres_out=True, want_dx=True, want_dres=True, off=0, pad=0), **c}
    dt, rdt, rows, cols, off, pad = c["dtype"], c["res"], c["rows"], c["cols"], c["off"], c["pad"]
    row = lambda d, fill=True, p=pad: _rows(g, dev, d, rows, cols, off, p, fill)
    weight = _rows(g, dev, c["wdt"] or dt, 1, cols, 0)[0] if c["weight"] else None
    args = (row(rdt), weight, row(dt), row(rdt) if c["dres_out"] else None, 1e-5, False)
    f32 = lambda: torch.empty(cols, device=dev, dtype=F32)
    outs = dict(dx=row(dt, False, 0) if c["want_dx"] else None, dres=row(rdt, False, 0) if c["want_dres"] else None, dw=f32() if c["weight"] else None,
                db=f32() if c["bias"] else None)
    return args, dict(x_dtype=dt), outs, lambda: layernorm.norm_bwd(*args, x_dtype=dt, want_dx=c["want_dx"], want_dres=c["want_dres"], has_bias=c["bias"])


def _selective_scan_bwd(c, dev, g):
    from zigma_amd import selective_scan_interface as ssi
    c = {**dict(dtype=BF, B=2, dim=64, L=32, N=16, z=True, D=True, bias=True, ck=False, reset=0), **c}
    dt, B, dim, L, N = c["dtype"], c["B"], c["dim"], c["L"], c["N"]
    tok = lambda fill=True: _rand(g, dev, dt, B, L, dim, scale=0.5) if fill else torch.empty(B, L, dim, device=dev, dtype=dt)
    f32 = lambda *shape: torch.empty(*shape, device=dev, dtype=F32)
    x_dbl = _rand(g, dev, dt, B, L, 2 * N)         # B and C: the column halves of one projection, as the block produces them
    D, bias = _rand(g, dev, F32, dim) if c["D"] else None, _rand(g, dev, F32, dim) if c["bias"] else None
    z, out = (tok(), tok()) if c["z"] else (None, None)
    args = (tok(), _rand(g, dev, dt, B, L, dim, scale=0.1), -torch.rand(dim, N, generator=g).to(dev) - 0.5, x_dbl[:, :, :N], x_dbl[:, :, N:], D, z, bias, tok(), out, True)
    kwargs = dict(reset_period=c["reset"], checkpoints=_rand(g, dev, F32, *_lib.checkpoint_shape(B, dim, L, N)) if c["ck"] else None)
    outs = dict(du=tok(False), ddelta=tok(False), dA=f32(dim, N), dB=f32(B, L, N), dC=f32(B, L, N), dD=f32(dim) if c["D"] else None,
                dz=tok(False) if c["z"] else None, dbias=f32(dim) if c["bias"] else None)
    return args, kwargs, outs, lambda: ssi.scan_bwd_tok(*args, **kwargs)


def _causal_conv1d_bwd(c, dev, g):
    from zigma_amd import causal_conv1d_interface as cci
    c = {**dict(dtype=BF, wdt=None, B=2, L=16, dim=8, width=4, silu=True, bias=True, perm=False, reset=0), **c}
    dt, wdt, B, L, dim, W = c["dtype"], c["wdt"] or c["dtype"], c["B"], c["L"], c["dim"], c["width"]
    perm = torch.randperm(L, generator=g).to(device=dev, dtype=torch.int32) if c["perm"] else None
    args = (_rand(g, dev, dt, B, L, dim), _rand(g, dev, wdt, dim, W, scale=0.5), _rand(g, dev, wdt, dim) if c["bias"] else None, _rand(g, dev, dt, B, L, dim),
            c["silu"], perm)
    outs = dict(dx=torch.empty(B, L, dim, device=dev, dtype=dt), dw=torch.empty(dim, W, device=dev, dtype=F32),
                db=torch.empty(dim, device=dev, dtype=F32) if c["bias"] else None)
    return args, dict(reset_period=c["reset"]), outs, lambda: cci.conv_bwd_tok(*args, reset_period=c["reset"])


_BUILD = {"add_norm_fwd": _add_norm_fwd, "add_norm_bwd": _add_norm_bwd, "selective_scan_bwd": _selective_scan_bwd, "causal_conv1d_bwd": _causal_conv1d_bwd}


def builder(entry):
    """the product's block builder of the entry point"""
    from zigma_amd import causal_conv1d_interface, layernorm, selective_scan_interface
    return {"add_norm_fwd": layernorm.norm_block, "add_norm_bwd": layernorm.norm_bwd_block, "selective_scan_bwd": selective_scan_interface.scan_bwd_block,
            "causal_conv1d_bwd": causal_conv1d_interface.conv_bwd_block}[entry]


def operands(name, device):
    entry, case, _ = CASES[name]
    case = {k: v for k, v in case.items() if k not in ("patch", "set")}
    return _BUILD[entry](case, device, torch.Generator().manual_seed(len(name)))


def block(name, device):
    """Build the case's operands and outputs on `device`, let the product's block builder fill the parameter block on them, attach the workspace the
    library asks for (the backward entry points), fill every output with NaN and apply the case's `set` and `patch`
    -> (entry point, block, outputs, the wrapper's call)"""
    entry, case, _ = CASES[name]
    args, kwargs, outs, call = operands(name, device)
    P = builder(entry)(*args, **kwargs, **outs)
    if hasattr(P, "workspace"):
        outs = dict(outs, workspace=_lib.workspace(ENTRY[entry], P, torch.device(device)))
    for t in outs.values():
        if t is not None and t.dtype != torch.uint8:
            t.fill_(float("nan"))
    for k, v in {**case.get("set", {}), **case.get("patch", {})}.items():
        setattr(P, k, v(P) if callable(v) else v)
    return ENTRY[entry], P, outs, call

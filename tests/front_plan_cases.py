"""The dispatch tables of the four entry points of the Mamba inner's front (plan_conv1d(), plan_conv_x_proj(), plan_x_proj(), plan_dt_proj() in
zigma_amd/csrc/front_plan.h), one case per leaf of the plans: every refusal clause, the empty calls, every serving leaf.

Each case is a small call of the product's own binding (causal_conv1d_raw, conv_x_proj, x_proj, dt_proj_softplus) and what the library reports for it:
status and zigma_last_kernel().  A refusal case breaks its check AND a later one where it can, so that two checks in the wrong order change its status.
test_host_cpu.py checks the table against the plans compiled with g++, test_gpu_front_plan.py against the library on the GPU (and every served case's
result against float64).
"""
from collections import namedtuple

import torch

from zigma_amd import _lib

Expect = namedtuple("Expect", "status kernel")      # kernel None: nothing launched, nothing reported
OK, NULL, SHAPE, DTYPE, STRIDE, UNSUPPORTED = 0, -1, -2, -3, -4, -6
BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
ENTRY = {"conv": "zigma_causal_conv1d_fwd", "conv_x_proj": "zigma_conv_x_proj_fwd", "x_proj": "zigma_x_proj_fwd", "dt_proj": "zigma_dt_proj_softplus_fwd"}


def _ok(kernel):
    return Expect(OK, kernel)


def _no(status):
    return Expect(status, None)


def _plus(field, nbytes):
    """patch value: the pointer the binding wrote, moved by nbytes"""
    return lambda P: getattr(P, field) + nbytes


TOK, GEN, CX = "conv_tok", "conv_generic", "conv_x_proj_mfma"
# name: (entry point, case, expected).  patch: parameter-block fields set after the binding has filled the block (what the binding refuses itself or
# cannot express); only refused and empty cases carry one, so nothing is ever launched on a block that does not describe its tensors.
# conv defaults: bf16, B=2, dim=4, L=17, width 4, SiLU, a bias, token-major rows (layout "tok"; "cf": the reference's channel-first tensor).
# conv_x_proj defaults: bf16, B=1, L=256, dim=64, n=8.  x_proj: bf16, m=32, n=8, k=256.  dt_proj: bf16, m=1, n=64, k=8, bias, softplus.
# *_pitch: the operand's rows are that many elements apart; *_gap: that many unused elements between samples; *_off: the operand starts that many
# elements into its allocation.
CASES = {
    # -- zigma_causal_conv1d_fwd
    "conv_shape_width_5": ("conv", dict(patch=dict(width=5, flags=1)), _no(SHAPE)),
    "conv_shape_width_1": ("conv", dict(patch=dict(width=1)), _no(SHAPE)),
    "conv_shape_negative_batch": ("conv", dict(patch=dict(batch=-1, flags=1)), _no(SHAPE)),
    "conv_shape_negative_dim": ("conv", dict(patch=dict(dim=-4)), _no(SHAPE)),
    "conv_shape_negative_seqlen": ("conv", dict(patch=dict(seqlen=-1)), _no(SHAPE)),
    "conv_unsupported_flag_on_empty": ("conv", dict(B=0, patch=dict(flags=1)), _no(UNSUPPORTED)),
    "conv_empty": ("conv", dict(B=0, patch=dict(x=None, io_dtype=7)), Expect(OK, None)),
    "conv_null_x": ("conv", dict(patch=dict(x=None, io_dtype=7)), _no(NULL)),
    "conv_null_weight": ("conv", dict(patch=dict(weight=None)), _no(NULL)),
    "conv_null_out": ("conv", dict(patch=dict(out=None)), _no(NULL)),
    "conv_dtype_io_7": ("conv", dict(patch=dict(io_dtype=7, reset_period=8)), _no(DTYPE)),
    "conv_dtype_w_7": ("conv", dict(patch=dict(w_dtype=7, reset_period=8)), _no(DTYPE)),
    "conv_shape_reset_period_8_channel_first": ("conv", dict(layout="cf", L=32, rp=8), _no(SHAPE)),
    "conv_shape_reset_period_negative": ("conv", dict(L=32, rp=-16), _no(SHAPE)),
    "conv_stride_reset_period_channel_first": ("conv", dict(layout="cf", L=32, rp=16), _no(STRIDE)),
    "conv_shape_reset_period_8_in_slices": ("conv", dict(B=65536, L=1, bcast=True, rp=8), _no(SHAPE)),
    "conv_tok_L1_w4_silu": ("conv", dict(L=1), _ok(TOK)),
    "conv_tok_L17_w4": ("conv", dict(silu=False), _ok(TOK)),
    "conv_tok_L17_w3_silu": ("conv", dict(W=3), _ok(TOK)),
    "conv_tok_L1_w3": ("conv", dict(L=1, W=3, silu=False), _ok(TOK)),
    "conv_tok_L17_w2": ("conv", dict(W=2, silu=False), _ok(TOK)),
    "conv_tok_L1_w2_silu": ("conv", dict(L=1, W=2), _ok(TOK)),
    "conv_tok_f32_no_bias": ("conv", dict(dtype=F32, bias=False), _ok(TOK)),
    "conv_tok_reset_period_16": ("conv", dict(L=32, rp=16), _ok(TOK)),
    "conv_tok_bf16_x_plus_8_bytes": ("conv", dict(x_off=4), _ok(TOK)),
    "conv_tok_sliced_65536_samples": ("conv", dict(B=65536, L=1, bcast=True), _ok(TOK)),       # what the last slice (1 sample) reports
    "conv_generic_channel_first": ("conv", dict(layout="cf"), _ok(GEN)),                       # x_l_stride == 1
    "conv_generic_dim_6": ("conv", dict(D=6, x_pitch=8, out_pitch=8), _ok(GEN)),
    "conv_generic_x_plus_4_bytes": ("conv", dict(x_off=2), _ok(GEN)),
    "conv_generic_f32_x_plus_8_bytes": ("conv", dict(dtype=F32, x_off=2), _ok(GEN)),
    "conv_generic_out_plus_4_bytes": ("conv", dict(out_off=2), _ok(GEN)),
    "conv_generic_x_pitch_6": ("conv", dict(L=2, x_pitch=6), _ok(GEN)),                        # (L = 2: the batch stride stays a multiple of 4)
    "conv_generic_out_pitch_6": ("conv", dict(L=2, out_pitch=6), _ok(GEN)),
    "conv_generic_x_batch_stride_70": ("conv", dict(x_gap=2), _ok(GEN)),
    "conv_generic_out_batch_stride_70": ("conv", dict(out_gap=2), _ok(GEN)),
    "conv_generic_x_rows_2_pow_30_bytes_apart": ("conv", dict(B=1, L=2, x_pitch=1 << 29), _ok(GEN)),
    "conv_generic_out_rows_2_pow_30_bytes_apart": ("conv", dict(B=1, L=2, out_pitch=1 << 29), _ok(GEN)),
    "conv_tok_rows_just_inside_2_pow_31_bytes": ("conv", dict(B=1, L=2, x_pitch=(1 << 29) - 4), _ok(TOK)),
    # -- zigma_conv_x_proj_fwd
    "cx_shape_negative_batch": ("conv_x_proj", dict(patch=dict(batch=-1, flags=16)), _no(SHAPE)),
    "cx_shape_dim_0": ("conv_x_proj", dict(patch=dict(dim=0)), _no(SHAPE)),
    "cx_shape_n_0": ("conv_x_proj", dict(patch=dict(n=0)), _no(SHAPE)),
    "cx_unsupported_flag_16_on_empty": ("conv_x_proj", dict(B=0, flags=16), _no(UNSUPPORTED)),
    "cx_empty": ("conv_x_proj", dict(B=0, patch=dict(x=None)), Expect(OK, None)),
    "cx_null_conv_bias": ("conv_x_proj", dict(patch=dict(conv_bias=None, dtype=_lib.F32)), _no(NULL)),
    "cx_null_u": ("conv_x_proj", dict(patch=dict(u=None)), _no(NULL)),
    "cx_dtype_f32": ("conv_x_proj", dict(dtype=F32, n=104), _no(DTYPE)),
    "cx_shape_n_104": ("conv_x_proj", dict(n=104, patch=dict(out_row_stride=108)), _no(SHAPE)),
    "cx_shape_n_12": ("conv_x_proj", dict(n=12), _no(SHAPE)),
    "cx_shape_dim_96": ("conv_x_proj", dict(D=96), _no(SHAPE)),
    "cx_shape_seqlen_48": ("conv_x_proj", dict(B=16, L=48), _no(SHAPE)),
    "cx_stride_out_pitch_12": ("conv_x_proj", dict(L=32, patch=dict(out_row_stride=12)), _no(STRIDE)),
    "cx_stride_out_plus_8_bytes": ("conv_x_proj", dict(L=32, patch=dict(out=_plus("out", 8))), _no(STRIDE)),
    "cx_shape_32_positions": ("conv_x_proj", dict(L=32, x_pitch=132), _no(SHAPE)),
    "cx_shape_128_positions": ("conv_x_proj", dict(L=128), _no(SHAPE)),
    "cx_stride_x_pitch_132": ("conv_x_proj", dict(x_pitch=132), _no(STRIDE)),
    "cx_stride_x_batch_stride": ("conv_x_proj", dict(patch=dict(x_batch_stride=4)), _no(STRIDE)),
    "cx_stride_u_pitch": ("conv_x_proj", dict(patch=dict(u_l_stride=68)), _no(STRIDE)),
    "cx_stride_u_batch_stride": ("conv_x_proj", dict(patch=dict(u_batch_stride=4)), _no(STRIDE)),
    "cx_stride_w_pitch_68": ("conv_x_proj", dict(w_pitch=68), _no(STRIDE)),
    "cx_stride_x_plus_8_bytes": ("conv_x_proj", dict(x_off=4), _no(STRIDE)),
    "cx_stride_u_plus_8_bytes": ("conv_x_proj", dict(patch=dict(u=_plus("u", 8))), _no(STRIDE)),
    "cx_stride_w_plus_8_bytes": ("conv_x_proj", dict(w_off=4), _no(STRIDE)),
    "cx_stride_conv_weight_plus_8_bytes": ("conv_x_proj", dict(cw_off=4), _no(STRIDE)),
    "cx_stride_conv_bias_plus_8_bytes": ("conv_x_proj", dict(cb_off=4), _no(STRIDE)),
    "cx_served_flags_0": ("conv_x_proj", dict(), _ok(CX)),
    "cx_served_flags_1": ("conv_x_proj", dict(flags=1), _ok(CX)),
    "cx_served_flags_2": ("conv_x_proj", dict(flags=2), _ok(CX)),
    "cx_served_flags_3_f16": ("conv_x_proj", dict(flags=3, dtype=F16), _ok(CX)),
    # -- zigma_x_proj_fwd
    "xp_shape_negative_m": ("x_proj", dict(patch=dict(m=-1, flags=1)), _no(SHAPE)),
    "xp_shape_n_0": ("x_proj", dict(patch=dict(n=0)), _no(SHAPE)),
    "xp_shape_k_0": ("x_proj", dict(patch=dict(k=0)), _no(SHAPE)),
    "xp_unsupported_flag_on_empty": ("x_proj", dict(m=0, patch=dict(flags=1)), _no(UNSUPPORTED)),
    "xp_empty": ("x_proj", dict(m=0, patch=dict(x=None)), Expect(OK, None)),
    "xp_null_w": ("x_proj", dict(patch=dict(w=None, dtype=_lib.F32)), _no(NULL)),
    "xp_null_out": ("x_proj", dict(patch=dict(out=None)), _no(NULL)),
    "xp_dtype_f32": ("x_proj", dict(dtype=F32, n=104), _no(DTYPE)),
    "xp_shape_n_104": ("x_proj", dict(n=104, x_pitch=260), _no(SHAPE)),
    "xp_shape_k_128": ("x_proj", dict(k=128), _no(SHAPE)),
    "xp_stride_x_pitch_260": ("x_proj", dict(x_pitch=260), _no(STRIDE)),
    "xp_stride_w_pitch_260": ("x_proj", dict(w_pitch=260), _no(STRIDE)),
    "xp_stride_x_plus_8_bytes": ("x_proj", dict(x_off=4), _no(STRIDE)),
    "xp_stride_w_plus_8_bytes": ("x_proj", dict(w_off=4), _no(STRIDE)),
    "xp_splitk": ("x_proj", dict(), _ok("x_proj_splitk")),
    "xp_splitk_k_1536_f16_m_33": ("x_proj", dict(m=33, k=1536, dtype=F16, x_pitch=1544), _ok("x_proj_splitk")),
    "xp_streaming_k_1792": ("x_proj", dict(k=1792), _ok("x_proj_mfma")),
    "xp_streaming_16384_rows": ("x_proj", dict(m=16384), _ok("x_proj_mfma")),
    "xp_splitk_16383_rows": ("x_proj", dict(m=16383), _ok("x_proj_splitk")),
    # -- zigma_dt_proj_softplus_fwd
    "dt_shape_negative_m": ("dt_proj", dict(patch=dict(m=-1, flags=2)), _no(SHAPE)),
    "dt_shape_negative_n": ("dt_proj", dict(patch=dict(n=-64)), _no(SHAPE)),
    "dt_shape_k_0": ("dt_proj", dict(patch=dict(k=0)), _no(SHAPE)),
    "dt_unsupported_flag_2_on_empty": ("dt_proj", dict(m=0, patch=dict(flags=2)), _no(UNSUPPORTED)),
    "dt_empty_no_rows": ("dt_proj", dict(m=0, patch=dict(x=None)), Expect(OK, None)),
    "dt_empty_no_channels": ("dt_proj", dict(n=0, patch=dict(w=None)), Expect(OK, None)),
    "dt_null_x": ("dt_proj", dict(patch=dict(x=None, dtype=_lib.F32)), _no(NULL)),
    "dt_null_w": ("dt_proj", dict(patch=dict(w=None)), _no(NULL)),
    "dt_null_out": ("dt_proj", dict(patch=dict(out=None)), _no(NULL)),
    "dt_dtype_f32": ("dt_proj", dict(dtype=F32, k=56), _no(DTYPE)),
    "dt_shape_k_56": ("dt_proj", dict(k=56, x_pitch=60), _no(SHAPE)),
    "dt_shape_k_12": ("dt_proj", dict(k=12, x_pitch=16), _no(SHAPE)),
    "dt_shape_n_96": ("dt_proj", dict(n=96), _no(SHAPE)),
    "dt_stride_x_pitch_12": ("dt_proj", dict(x_pitch=12), _no(STRIDE)),
    "dt_stride_w_pitch_12": ("dt_proj", dict(w_pitch=12), _no(STRIDE)),
    "dt_stride_out_pitch_65": ("dt_proj", dict(patch=dict(out_row_stride=65)), _no(STRIDE)),
    "dt_stride_x_plus_8_bytes": ("dt_proj", dict(x_off=4, x_pitch=16), _no(STRIDE)),
    "dt_stride_w_plus_8_bytes": ("dt_proj", dict(w_off=4), _no(STRIDE)),
    "dt_stride_out_plus_2_bytes": ("dt_proj", dict(patch=dict(out=_plus("out", 2))), _no(STRIDE)),
    "dt_served_1_row": ("dt_proj", dict(), _ok("dt_proj_softplus_mfma")),
    "dt_served_513_rows_f16": ("dt_proj", dict(m=513, dtype=F16, x_pitch=72), _ok("dt_proj_softplus_mfma")),
    "dt_served_513_rows_k_48_no_bias_no_softplus": ("dt_proj", dict(m=513, k=48, bias=False, softplus=False), _ok("dt_proj_softplus_mfma")),
    "dt_served_flag_1": ("dt_proj", dict(m=513, flags=1), _ok("dt_proj_softplus_mfma")),
}


def _rows(g, device, dtype, r, cols, pitch=0, off=0, scale=1.0, lead=(), gap=0):
    """(*lead, r, cols) random rows `pitch` elements apart, `gap` unused elements behind every (r, cols) block, `off` elements into their allocation (which is
    only touched where the rows lie)"""
    pitch = pitch or cols
    shape, strides, s = (*lead, r, cols), [1, pitch], r * pitch + gap
    for d in reversed(lead):
        strides.append(s)
        s *= d
    last = sum((d - 1) * st for d, st in zip(shape, reversed(strides))) if all(shape) else 0
    flat = torch.empty(off + last + 1, device=device, dtype=dtype)
    v = flat.as_strided(shape, tuple(reversed(strides)), off)
    v.copy_((torch.randn(shape, generator=g) * scale).to(device=device, dtype=dtype))
    return v


def _conv(c, device, g):
    from zigma_amd.causal_conv1d_interface import causal_conv1d_raw
    c = {**dict(dtype=BF, B=2, D=4, L=17, W=4, silu=True, bias=True, layout="tok", rp=0, x_off=0, out_off=0, x_pitch=0, out_pitch=0, x_gap=0, out_gap=0, bcast=False), **c}
    dt, B, D, L = c["dtype"], c["B"], c["D"], c["L"]
    if c["layout"] == "cf":
        x, out = _rows(g, device, dt, D, L, lead=(B,)), _rows(g, device, dt, D, L, lead=(B,))
    else:
        xb = 1 if c["bcast"] else B             # one sample broadcast over the batch (stride 0), so that a batch above 65535 stays small
        x = _rows(g, device, dt, L, D, c["x_pitch"], c["x_off"], lead=(xb,), gap=c["x_gap"]).expand(B, L, D).transpose(1, 2)
        out = _rows(g, device, dt, L, D, c["out_pitch"], c["out_off"], lead=(B,), gap=c["out_gap"]).transpose(1, 2)
    w, b = _rows(g, device, dt, D, c["W"], scale=0.5), (_rows(g, device, dt, 1, D)[0] if c["bias"] else None)
    o = dict(x=x, w=w, b=b, silu=c["silu"], rp=c["rp"], kind=dt, outs=dict(out=out))
    return o, lambda: causal_conv1d_raw(x, w, b, c["silu"], out=out, reset_period=c["rp"])


def _conv_x_proj(c, device, g):
    from zigma_amd.selective_scan_interface import conv_x_proj
    c = {**dict(dtype=BF, B=1, L=256, D=64, n=8, flags=0, x_pitch=0, w_pitch=0, x_off=0, w_off=0, cw_off=0, cb_off=0), **c}
    dt, B, L, D, n = c["dtype"], c["B"], c["L"], c["D"], c["n"]
    x = _rows(g, device, dt, L, D, c["x_pitch"] or 2 * D, c["x_off"], lead=(B,))           # the first half of an in_proj output
    cw, cb = _rows(g, device, dt, D, 4, off=c["cw_off"], scale=0.5), _rows(g, device, dt, 1, D, off=c["cb_off"])[0]
    w = _rows(g, device, dt, n, D, c["w_pitch"], c["w_off"], scale=D ** -0.5)
    perm = torch.randperm(L, generator=g).to(device=device, dtype=torch.int32)
    o = dict(x=x, cw=cw, cb=cb, w=w, perm=perm, kind=dt, outs={})

    def run():
        o["outs"]["u"], o["outs"]["x_dbl"] = conv_x_proj(x, cw, cb, w, perm, _flags=c["flags"])
    return o, run


def _x_proj(c, device, g):
    from zigma_amd.selective_scan_interface import x_proj
    c = {**dict(dtype=BF, m=32, n=8, k=256, x_pitch=0, w_pitch=0, x_off=0, w_off=0), **c}
    dt, k = c["dtype"], c["k"]
    x, w = _rows(g, device, dt, c["m"], k, c["x_pitch"], c["x_off"]), _rows(g, device, dt, c["n"], k, c["w_pitch"], c["w_off"], scale=k ** -0.5)
    o = dict(x=x, w=w, kind=dt, outs={})

    def run():
        o["outs"]["x_dbl"] = x_proj(x, w)
    return o, run


def _dt_proj(c, device, g):
    import zigma_amd.selective_scan_interface as ssi
    c = {**dict(dtype=BF, m=1, n=64, k=8, bias=True, softplus=True, flags=0, x_pitch=0, w_pitch=0, x_off=0, w_off=0), **c}
    dt, k, n = c["dtype"], c["k"], c["n"]
    x = _rows(g, device, dt, c["m"], c["x_pitch"] or k, 0, c["x_off"])                     # x_dbl rows: dt_rank columns, then B | C
    w = _rows(g, device, dt, n, k, c["w_pitch"], c["w_off"], scale=k ** -0.5)
    bias = torch.randn(n, generator=g).to(device) if c["bias"] else None
    o = dict(x=x, w=w, bias=bias, k=k, softplus=c["softplus"], kind=dt, outs={})

    def run():
        knob, ssi.DT_PROJ_FLAGS = ssi.DT_PROJ_FLAGS, c["flags"]
        try:
            o["outs"]["delta"] = ssi.dt_proj_softplus(x, k, w, bias, c["softplus"])
        finally:
            ssi.DT_PROJ_FLAGS = knob
    return o, run


_BUILD = {"conv": _conv, "conv_x_proj": _conv_x_proj, "x_proj": _x_proj, "dt_proj": _dt_proj}


def call(name, device, launch):
    """Build the case's operands on `device`, let the product's binding fill the parameter block, fill every output with NaN, apply the case's patch
    and hand the block to launch(entry point, params).  Returns (what launch returned, the operands; o["outs"]: the output tensors)."""
    entry, case, _ = CASES[name]
    case = dict(case)
    patch = case.pop("patch", {})
    o, run = _BUILD[entry](case, device, torch.Generator().manual_seed(len(name)))
    filled = []
    real_call, real_require = _lib.call, _lib.require_device
    _lib.call = lambda fn, P, dev: filled.append((fn, P))
    _lib.require_device = lambda *t: torch.device(device)
    try:
        run()
    finally:
        _lib.call, _lib.require_device = real_call, real_require
    (fn, P), = filled
    assert fn == ENTRY[entry]
    for t in o["outs"].values():
        t.fill_(float("nan"))
    for k, v in patch.items():
        setattr(P, k, v(P) if callable(v) else v)
    return launch(fn, P), o


def reference(name, o):
    """float64 results of a served case from its operands (on the CPU) -> {output: float64 tensor}; conv_x_proj's x_dbl from the u the kernel wrote,
    as tests/test_gpu_fwd_fuzz.py takes it"""
    entry = CASES[name][0]
    d = lambda t: None if t is None else t.detach().double().cpu()
    act = lambda t: t * torch.sigmoid(t)
    if entry == "conv":
        x, w, b = d(o["x"]), d(o["w"]), d(o["b"])
        B, D, L = x.shape
        W, period = w.shape[1], o["rp"] or L
        y = torch.zeros(B, D, L, dtype=torch.float64) + (0 if b is None else b[:, None])
        for l in range(L):
            for j in range(W):
                k = l - (W - 1 - j)
                if k >= l // period * period:
                    y[:, :, l] += w[:, j] * x[:, :, k]
        return dict(out=act(y) if o["silu"] else y)
    if entry == "conv_x_proj":
        x = d(o["x"]).index_select(1, o["perm"].long().cpu())
        L = x.shape[1]
        xp = torch.nn.functional.pad(x, (0, 0, 3, 0))
        pre = d(o["cb"]) + sum(d(o["cw"])[:, t] * xp[:, t:t + L] for t in range(4))
        return dict(u=act(pre), x_dbl=d(o["outs"]["u"]) @ d(o["w"]).T)
    if entry == "x_proj":
        return dict(x_dbl=d(o["x"]) @ d(o["w"]).T)
    pre = d(o["x"])[:, :o["k"]] @ d(o["w"]).T + (0 if o["bias"] is None else d(o["bias"]))
    return dict(delta=torch.nn.functional.softplus(pre) if o["softplus"] else pre)

"""The dispatch table of zigma_linear_fwd (plan_linear() in zigma_amd/csrc/linear_plan.h), one case per leaf of the plan.

Each case is a small zigma_amd.linear.linear call and what the library reports for it: status and zigma_last_kernel().
test_host_cpu.py checks the table against plan_linear() compiled with g++, test_gpu_parity.py against the library on the GPU
(and every served case's result against float64).
"""
from collections import namedtuple

import torch

from zigma_amd import _lib

Expect = namedtuple("Expect", "status kernel")      # kernel None: nothing launched, nothing reported
OK, NULL, SHAPE, DTYPE, STRIDE, UNSUPPORTED = 0, -1, -2, -3, -4, -6
WS, SM = dict(ws=True), dict(sm=True)


def _ok(kernel):
    return Expect(OK, kernel)


def _no(status):
    return Expect(status, None)


def _c(m, n, k, *more, **kw):
    c = dict(shape=(m, n, k), **kw)
    for d in more:
        c.update(d)
    return c


TN128, TN256, L4W = "linear_tn_256x128", "linear_tn_256x256", "linear4w_256x256"
# name: (case, expected).  Defaults (see operands()): bf16, contiguous 2-D operands, no bias / activation / residual, no flags.
# res = rows per sample of a (m / res, res, k) call with the gated residual; *_off: the operand starts that many elements into its allocation.
CASES = {
    # -- refusals and the empty call
    "empty": (_c(0, 128, 64), Expect(OK, None)),
    "null_x": (_c(8, 128, 64, patch=dict(x=None)), _no(NULL)),
    "dtype_f32": (_c(8, 128, 64, patch=dict(dtype=_lib.F32)), _no(DTYPE)),
    "shape_k_32": (_c(8, 128, 32), _no(SHAPE)),
    "shape_m_4": (_c(4, 128, 64), _no(SHAPE)),
    "shape_n_64": (_c(8, 64, 64), _no(SHAPE)),
    "shape_silu_from_col_16": (_c(8, 128, 64, silu=16), _no(SHAPE)),
    "stride_x_pitch_68": (_c(8, 128, 64, x_pitch=68), _no(STRIDE)),
    "stride_out_plus_4_bytes": (_c(8, 128, 64, out_off=2), _no(STRIDE)),
    "shape_bias_n_4224": (_c(8, 4224, 64, bias=True), _no(SHAPE)),
    "shape_residual_rows_per_batch_128": (_c(256, 256, 64, res=128), _no(SHAPE)),
    "shape_residual_without_gate": (_c(256, 256, 64, res=256, patch=dict(gate=None)), _no(SHAPE)),
    "stride_residual_plus_8_bytes": (_c(256, 256, 64, res=256, res_off=4), _no(STRIDE)),
    "unsupported_flag_bit_0": (_c(8, 128, 64, flags=0x1), _no(UNSUPPORTED)),
    # -- the 8-wave kernel
    "tn_narrow": (_c(8, 128, 64), _ok(TN128)),
    "tn_wide": (_c(8, 256, 64), _ok(TN256)),
    "tn_wide_bias": (_c(8, 256, 64, bias=True), _ok(TN256)),
    "tn_wide_silu": (_c(8, 256, 64, silu=128), _ok(TN256)),
    "tn_residual": (_c(256, 256, 64, res=256), _ok(TN128)),
    # -- the 8-wave kernel on shapes near the 4-wave kernel's limits
    "tn_pinned_by_flag": (_c(32768, 512, 192, flags=0x2000), _ok(TN256)),
    "tn_254_tiles": (_c(32768 - 256, 512, 192), _ok(TN256)),
    "tn_k_128": (_c(32768, 512, 128), _ok(TN256)),
    "tn_bias_alone": (_c(32768, 512, 192, bias=True), _ok(TN256)),
    "tn_out_pitch_516": (_c(32768, 512, 192, out_pitch=516), _ok(TN256)),
    "tn_samples_of_768_rows": (_c(768 * 43, 512, 192, res=768), _ok(TN128)),
    # -- the 4-wave kernel
    "l4w_wide": (_c(32768, 512, 192), _ok(L4W)),
    "l4w_narrow_column": (_c(32768, 384, 192), _ok(L4W + "+128")),
    "l4w_residual": (_c(32768, 512, 192, res=1024), _ok(L4W)),
    "l4w_bias_residual": (_c(32768, 512, 192, res=1024, bias=True), _ok(L4W)),
    # -- the weight-stationary kernel
    "ws_32_panels": (_c(512, 8192, 512, WS), _ok("linear_ws")),
    "ws_one_panel_k640": (_c(16384, 256, 640, WS), _ok("linear_ws")),
    "ws_silu": (_c(512, 8192, 512, WS, silu=4096), _ok("linear_ws_silu")),
    "ws128_k1280": (_c(512, 4096, 1280, WS), _ok("linear_ws_128")),
    "ws128_k1536": (_c(1024, 2048, 1536, WS), _ok("linear_ws_128")),
    "ws_refuses_bias": (_c(16384, 256, 640, WS, bias=True), _no(UNSUPPORTED)),
    "ws_refuses_k_768": (_c(512, 8192, 768, WS), _no(UNSUPPORTED)),
    "ws_refuses_m_256": (_c(256, 8192, 512, WS), _no(UNSUPPORTED)),
    "ws_refuses_too_few_tiles_per_xcd": (_c(512, 4096, 512, WS), _no(UNSUPPORTED)),
    "ws_refuses_33_panels": (_c(512, 33 * 128, 1280, WS), _no(UNSUPPORTED)),
    "ws_refuses_silu_k_1280": (_c(512, 4096, 1280, WS, silu=2048), _no(UNSUPPORTED)),
    "ws_refuses_silu_from_col_64": (_c(512, 8192, 512, WS, silu=64), _no(UNSUPPORTED)),
    "ws_refuses_x_pitch_520": (_c(512, 8192, 512, WS, x_pitch=520), _no(UNSUPPORTED)),
    # -- the few-token kernel
    "sm_128": (_c(128, 128, 128, SM), _ok("linear_sm_128x128")),
    "sm_160": (_c(128, 640, 128, SM), _ok("linear_sm_128x160")),
    "sm_192": (_c(128, 384, 128, SM), _ok("linear_sm_128x192")),
    "sm_bias_residual": (_c(256, 640, 128, SM, res=256, bias=True), _ok("linear_sm_128x160")),
    "sm_refuses_k_64": (_c(128, 128, 64, SM), _no(UNSUPPORTED)),
    "sm_refuses_m_8": (_c(8, 128, 128, SM), _no(UNSUPPORTED)),
    "sm_refuses_silu": (_c(128, 256, 128, SM, silu=128), _no(UNSUPPORTED)),
    "sm_refuses_bias_on_4_bytes": (_c(128, 128, 128, SM, bias=True, bias_off=2), _no(UNSUPPORTED)),
}


def operands(case, device):
    """the case's tensors on `device` (the same values on every device: drawn on the CPU from a fixed seed)"""
    c = {**dict(dtype=torch.bfloat16, bias=False, silu=None, res=0, x_pitch=0, out_pitch=0, out_off=0, res_off=0, bias_off=0), **case}
    m, n, k = c["shape"]
    g = torch.Generator().manual_seed(m + n + k)

    def rows(r, cols, pitch=0, off=0, scale=1.0, zero=False):        # (r, cols) rows of `pitch` elements, `off` elements into their allocation
        pitch = pitch or cols
        flat = torch.zeros(off + r * pitch) if zero else torch.randn(off + r * pitch, generator=g) * scale
        return flat.to(device=device, dtype=c["dtype"])[off:].view(r, pitch)[:, :cols]

    o = dict(x=rows(m, k, c["x_pitch"]), w=rows(n, k, scale=k ** -0.5), out=rows(m, n, c["out_pitch"], c["out_off"], zero=True), bias=None, res=None, gate=None,
             silu=c["silu"], rpb=c["res"])
    if c["bias"]:
        o["bias"] = rows(1, n, off=c["bias_off"], scale=0.3)[0]
    if c["res"]:
        B = m // c["res"]
        o["x"], o["out"] = o["x"].view(B, c["res"], k), o["out"].view(B, c["res"], n)
        o["res"], o["gate"] = rows(m, n, off=c["res_off"]).view(B, c["res"], n), rows(B, n)
    return o


def call(case, device, launch):
    """Build the case's operands on `device` and run zigma_amd.linear.linear with the library call replaced by launch(params) -> anything;
    case["patch"]: parameter-block fields the wrapper would refuse itself.  Returns (what launch returned, the operands)."""
    o = operands(case, device)
    launched = []
    real_call, real_require = _lib.call, _lib.require_device
    _lib.call = lambda name, P, dev: launched.append(launch(_patched(P, case.get("patch", {}))))
    _lib.require_device = lambda *t: torch.device(device)
    try:
        from zigma_amd.linear import linear
        linear(o["x"], o["w"], o["bias"], silu_from_col=o["silu"], out=o["out"], _probe_flags=case.get("flags", 0), residual=o["res"], gate=o["gate"],
               weight_stationary=case.get("ws", False), few_tokens=case.get("sm", False))
    finally:
        _lib.call, _lib.require_device = real_call, real_require
    assert len(launched) == 1
    return launched[0], o


def _patched(P, fields):
    for k, v in fields.items():
        setattr(P, k, v)
    return P

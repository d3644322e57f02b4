"""The dispatch table of zigma_selective_scan_fwd (plan_scan() in zigma_amd/csrc/scan_plan.h), one case per leaf of the plan.

Each case is a small scan_raw call and what the library reports for it: status, kernel family, info and zigma_last_kernel().
test_host_cpu.py checks the table against plan_scan() compiled with g++, test_gpu_parity.py against the library on the GPU.
"""
from collections import namedtuple

import torch

from zigma_amd import _lib

Expect = namedtuple("Expect", "status family info kernel")      # family / info / kernel None: nothing launched, nothing reported
OK, NULL, SHAPE, DTYPE, STRIDE, UNSUPPORTED = 0, -1, -2, -3, -4, -6
GEN, TOK, TOK2 = _lib.SCAN_KERNEL_GENERIC, _lib.SCAN_KERNEL_TOK, _lib.SCAN_KERNEL_TOK2
V1, R5 = _lib.SCAN_PROBE_V1, 1 << _lib.SCAN_PROBE_R5_SHIFT


def _ok(family, kernel, info1=0):
    return Expect(OK, family, (family, info1), kernel)


def _no(status):
    return Expect(status, None, None, None)


DTP, DTP_R6 = "scan_tok2_n16_dtproj", "scan_tok2_n16_dtproj_r6"
# name: (case, expected).  Defaults (see call()): bf16, batch 2, dim 64, seqlen 64, dstate 16, token-major operands, B / C columns of
# x_dbl rows (the model's layout), gate z, delta_bias + softplus, whole sequence.
CASES = {
    "null_split_dtp_without_workspace": (dict(dt=True, chunk=32, delta=False), _no(NULL)),
    "shape_reset_period_not_whole_tiles": (dict(rp=8), _no(SHAPE)),
    "shape_reset_period_with_carries": (dict(rp=16, chunk=32), _no(SHAPE)),
    "dtype_unknown_element_type": (dict(layout="ref", patch=dict(io_dtype=7, bc_dtype=7)), _no(DTYPE)),
    "stride_reset_period_on_reference_layout": (dict(layout="ref", rp=16), _no(STRIDE)),
    "unsupported_unknown_flag": (dict(flags=0x1000), _no(UNSUPPORTED)),
    "unsupported_accumulate_without_dt": (dict(flags=_lib.SCAN_ACCUMULATE), _no(UNSUPPORTED)),
    "unsupported_zact_f32": (dict(dtype="f32", zact=True), _no(UNSUPPORTED)),
    "unsupported_zact_on_v1": (dict(zact=True, flags=V1), _no(UNSUPPORTED)),
    "unsupported_dtp_v1_pin": (dict(dt=True, flags=V1), _no(UNSUPPORTED)),
    "unsupported_dtp_dstate8": (dict(dt=True, N=8), _no(UNSUPPORTED)),
    "unsupported_dtp_dt_rank_24": (dict(dt=True, R=24), _no(UNSUPPORTED)),
    "unsupported_dtp_with_out": (dict(dt=True, out=True), _no(UNSUPPORTED)),
    "unsupported_dtp_split_wide_grid": (dict(dt=True, chunk=32, B=16, D=3072), _no(UNSUPPORTED)),
    "empty": (dict(B=0), Expect(OK, None, None, None)),
    "generic_reference_layout": (dict(layout="ref"), _ok(GEN, "scan_generic")),
    "generic_constant_bc": (dict(bc="const"), _ok(GEN, "scan_generic")),
    "generic_groups2": (dict(bc="ref", groups=2), _ok(GEN, "scan_generic")),
    "generic_dstate32": (dict(N=32), _ok(GEN, "scan_generic")),
    "tok_f32": (dict(dtype="f32"), _ok(TOK, "scan_tok_n16")),
    "tok_dstate8": (dict(N=8), _ok(TOK, "scan_tok_n8")),
    "tok_ragged_length": (dict(L=40), _ok(TOK, "scan_tok_n16")),
    "tok_no_gate": (dict(z=False, out=True), _ok(TOK, "scan_tok_n16")),
    "tok_probe_v1": (dict(flags=V1), _ok(TOK, "scan_tok_n16")),
    "tok_split": (dict(dtype="f32", chunk=32), _ok(TOK, "scan_tok_n16")),
    "tok_carries_without_split": (dict(chunk=32, B=16, D=3072), _ok(TOK, "scan_tok_n16")),
    "tok_training_checkpoints": (dict(dtype="f32", out=True, ckpt=True), _ok(TOK, "scan_tok_n16", 1)),
    "tok2_gated": (dict(), _ok(TOK2, "scan_tok2_n16")),
    "tok2_no_bias_no_softplus": (dict(bias=False, softplus=False), _ok(TOK2, "scan_tok2_n16")),
    "tok2_tables_zact_f16": (dict(dtype="f16", tables=True, zact=True), _ok(TOK2, "scan_tok2_n16")),
    "tok2_training_form": (dict(out=True), _ok(TOK2, "scan_tok2_n16")),
    "tok2_training_checkpoints": (dict(out=True, ckpt=True, tables=True), _ok(TOK2, "scan_tok2_n16", 1)),
    "tok2_split": (dict(chunk=32), _ok(TOK2, "scan_tok2_n16")),
    "tok2_split_tables_zact": (dict(chunk=32, tables=True, zact=True), _ok(TOK2, "scan_tok2_n16")),
    "dtp_r5": (dict(dt=True), _ok(TOK2, DTP)),
    "dtp_r6": (dict(dt=True, B=1536, L=16), _ok(TOK2, DTP_R6)),
    "dtp_r6_pinned_to_r5": (dict(dt=True, B=1536, L=16, flags=R5), _ok(TOK2, DTP)),
    "dtp_acc": (dict(dt=True, acc=True), _ok(TOK2, DTP + "_acc")),
    "dtp_r6_acc": (dict(dt=True, B=1536, L=16, acc=True), _ok(TOK2, DTP_R6 + "_acc")),
    "dtp_zact_tables": (dict(dt=True, zact=True, tables=True), _ok(TOK2, DTP)),
    "dtp_f16_reset_period": (dict(dt=True, dtype="f16", rp=16), _ok(TOK2, DTP)),
    "dtp_split": (dict(dt=True, chunk=32), _ok(TOK2, "scan_tok2_n16_split_dtproj")),
    "slices_above_65535_samples": (dict(B=65536, L=16, bcast=True), _ok(TOK2, "scan_tok2_n16")),   # what the last slice (1 sample) reports
}


def call(case, device, launch):
    """Build the case's operands on `device` and run scan_raw with the library call replaced by launch(params) -> status.
    bcast: the inputs are one sample broadcast over the batch (stride 0), so that a batch above 65535 stays small."""
    c = {**dict(dtype="bf16", B=2, D=64, L=64, N=16, R=40, groups=1, layout="tok", bc="x_dbl", z=True, out=False, bias=True, softplus=True,
                chunk=0, delta=True, ckpt=False, rp=0, zact=False, acc=False, flags=0, dt=False, tables=False, bcast=False, patch={}), **case}
    dt = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[c["dtype"]]
    B, D, L, N, R = c["B"], c["D"], c["L"], c["N"], c["R"]
    g = torch.Generator().manual_seed(0)
    rnd = lambda *s, dtype=dt: (torch.randn(*s, generator=g) * 0.5).to(device=device, dtype=dtype)

    def act(b=B):                   # (batch, dim, seqlen) views: token-major rows or the reference's channel-major layout
        if c["layout"] == "ref":
            return rnd(b, D, L)
        return rnd(b, L, D).transpose(1, 2)

    def inp():
        return act(1).expand(B, D, L) if c["bcast"] else act()

    def new():
        return torch.zeros(B, L, D, device=device, dtype=dt).transpose(1, 2) if c["layout"] == "tok" else torch.zeros(B, D, L, device=device, dtype=dt)

    u, z = inp(), inp() if c["z"] else None
    x_dbl = rnd(1 if c["bcast"] else B, L, R + 2 * N).expand(B, L, R + 2 * N)
    if c["bc"] == "x_dbl":
        Bm, Cm = (x_dbl[:, :, o:o + N].transpose(1, 2).unsqueeze(1) for o in (R, R + N))
    elif c["bc"] == "const":
        Bm, Cm = rnd(D, N, dtype=torch.float32), rnd(D, N, dtype=torch.float32)
    else:
        Bm, Cm = rnd(B, c["groups"], N, L), rnd(B, c["groups"], N, L)
    A = -(torch.rand(D, N, generator=g) + 0.5).to(device)
    delta = None
    if not c["dt"]:
        delta = inp()
    elif c["chunk"] and c["delta"]:
        delta = new()               # the split's workspace: its first pass writes softplus(dt_proj + bias) here
    n_chunks = -(-L // c["chunk"]) if c["chunk"] else 0
    perm = torch.randperm(L, generator=g).to(device=device, dtype=torch.int32) if c["tables"] else None
    launched = []
    real_call, real_require = _lib.call, _lib.require_device
    _lib.call = lambda name, P, dev: launched.append(launch(_patched(P, c["patch"])))
    _lib.require_device = lambda *t: torch.device(device)
    try:
        from zigma_amd.selective_scan_interface import scan_raw
        scan_raw(u, delta, A, Bm, Cm, rnd(D, dtype=torch.float32), z, rnd(D, dtype=torch.float32) if c["bias"] else None, c["softplus"],
                 out=new() if c["out"] else None, out_z=new() if c["z"] else None, want_out=c["out"],
                 x=torch.zeros(B, D, n_chunks, 2 * N, device=device) if c["chunk"] else None, chunk_len=c["chunk"] or 2048,
                 z_row_index=perm, out_row_index=perm,
                 checkpoints=torch.zeros(B * (D // 64) * -(-L // 16) * N * 64, device=device) if c["ckpt"] else None,
                 reset_period=c["rp"], z_preactivated=c["zact"], _probe_flags=c["flags"], accumulate=c["acc"],
                 dt_x=x_dbl if c["dt"] else None, dt_w=rnd(D, R) * 0.2 if c["dt"] else None)
    finally:
        _lib.call, _lib.require_device = real_call, real_require
    assert len(launched) == 1
    return launched[0]


def _patched(P, fields):
    for k, v in fields.items():
        setattr(P, k, v)
    return P

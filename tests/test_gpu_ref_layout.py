"""Sweep of the kernels behind the drop-in call surface — scan_generic_kernel (zigma_selective_scan_fwd through scan_raw, selective_scan_fn and
selective_scan_cuda_fwd) and conv_tok_kernel / conv_generic_kernel (zigma_causal_conv1d_fwd through causal_conv1d_raw and causal_conv1d_fn) —
against float64 row by row, over the case tables of tests/ref_layout_cases.py (coverage, the references' soundness and the rounding model:
tests/test_ref_layout_cases_cpu.py, which also runs every function of this file on the CPU against the float64 stand-ins of
tests/kernel_standins.py).

Every case asserts: the kernel that served it (zigma_last_kernel, `info`) and that the host-only plan query foretells it from the very block that
was launched; finite outputs although every output buffer and the carry tensor were NaN beforehand; not a byte changed outside the output views
(operands, the NaN surroundings of every slice, the guard behind the carry tensor); the norm-wise bound and, for EVERY row, the row-wise limit of
every output (ref_layout_cases: limits); a second launch bit for bit the first; for selective_scan_fn(return_last_state=True) last_state bit for
bit the state row of the last carry.  Each output prints one `ref-layout-sweep` line with its worst ratio of error to bound.
"""
import numpy as np
import pytest
import torch

import ref_layout_cases as rl

pytestmark = pytest.mark.gpu
DEV = "cuda"            # (the CPU test file points this at "cpu" and serves _lib.call with the stand-ins)
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
NAN = float("nan")
SCAN, CONV = rl.scan_generic_cases(), rl.conv_cases()


def _ids(cases):
    return [c["id"] for c in cases]


def _dev(a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def _np(t):
    return None if t is None else t.detach().double().cpu().numpy()


class Slot:
    """a tensor carved out of a NaN-filled buffer (carve: the slicing, applicable to any tensor of the buffer's shape); the buffer as it was before
    the launch is kept, so that afterwards every byte outside an output — every byte of an operand — can be held against it"""
    def __init__(self, shape, dtype, carve=lambda t: t, fill=None, output=False):
        self.buf = torch.full(shape, NAN, dtype=dtype, device=DEV)
        self.carve, self.output, self.t = carve, output, carve(self.buf)
        if fill is not None:
            self.t.copy_(_dev(fill, dtype))
        self.before = self.buf.clone()

    def untouched(self):
        a, b = self.buf.clone(), self.before.clone()
        if self.output:
            self.carve(a).zero_(), self.carve(b).zero_()
        bits = {2: torch.int16, 4: torch.int32}[a.element_size()]
        return torch.equal(a.view(bits), b.view(bits))


def _act(shape, dtype, layout, views, **kw):
    """a logical (B, D, L) activation: `ref` (B, D, L) memory, `tok` token-major (B, L, D) rows; views: a slice of a wider NaN-filled buffer"""
    Bsz, D, L = shape
    pad = 8 if views else 0
    if layout == "ref":
        return Slot((Bsz, D, L + 2 * pad), dtype, lambda t: t[..., pad:pad + L], **kw)
    return Slot((Bsz, L, D + 2 * pad), dtype, lambda t: t[..., pad:pad + D].transpose(1, 2), **kw)


def _report(ident, key, got, ref, bound):
    assert got.shape == ref.shape, (ident, key, got.shape, ref.shape)
    assert np.isfinite(got).all(), (ident, key, "not finite: an element was left unwritten, or a NaN / inf was computed")
    e, r = rl.norm_err(got, ref), rl.row_ratio(key, got, ref, bound)
    print(f"ref-layout-sweep {ident}: {key} norm-wise {e:.3e} (bound {bound:.2e}), row-wise ratio {r:.3g}, worst error / bound {max(e / bound, r / rl.ROW_GUARD):.3f}")
    assert e < bound, (ident, key, e, bound)
    assert r <= rl.ROW_GUARD, (ident, key, r)


def _served(ident, trace, fn_name, kernel):
    """every launch of the call was served by `kernel`, and the plan query says so for the block that was launched"""
    from zigma_amd import _lib
    assert trace and all(t[0] == fn_name and t[1] == kernel for t in trace), (ident, [t[:2] for t in trace])
    for _, _, P in trace:
        assert _lib.plan(fn_name, P) == (0, kernel), (ident, _lib.plan(fn_name, P))


# ---------------------------------------------------------------------------------------------------
# scan_generic_kernel
# ---------------------------------------------------------------------------------------------------
def _bc_slot(c, arr, form, dtype):
    Bsz, G, N, L = c["B"], c["G"], c["N"], c["L"]
    if form == "const":         # fp32 (dim, dstate), contiguous or the transposed view of (dstate, dim)
        if c["const_t"]:
            return Slot((N, c["dim"]), torch.float32, lambda t: t.t(), fill=arr)
        return Slot((c["dim"], N), torch.float32, fill=arr)
    if c["bc_layout"] == "3d":
        return Slot((Bsz, N, L), dtype, fill=arr[:, 0])
    if c["bc_layout"] == "4d_pad":
        return Slot((Bsz, G, N, L + 5), dtype, lambda t: t[..., 2:2 + L], fill=arr)
    return Slot((Bsz, L, G * N + 8), dtype, lambda t: t[..., 4:4 + G * N].unflatten(2, (G, N)).permute(0, 2, 3, 1), fill=arr)     # columns of token-major rows


def scan_run(c, inp, api=None):
    """one call through the case's entry point on fresh buffers laid out as the case says -> dict(outs: the raw output tensors by key, slots, x,
    last, info, trace)"""
    import zigma_amd.selective_scan_interface as ssi
    from zigma_amd import _lib
    api = api or c["api"]
    dt, bdt, shape, N, v = DT[c["kind"]], DT[c["bck"]], (c["B"], c["dim"], c["L"]), c["N"], c["views"]
    f32 = lambda a: _dev(a, torch.float32)
    s = dict(u=_act(shape, dt, c["layout"], v, fill=inp["u"]), delta=_act(shape, dt, c["layout"], v, fill=inp["delta"]),
             B=_bc_slot(c, inp["Bm"], c["bform"], bdt), C=_bc_slot(c, inp["Cm"], c["cform"], bdt))
    if c["z"]:
        s["z"] = _act(shape, dt, c["layout"], v, fill=inp["z"])
    A, D, bias = f32(inp["A"]), f32(inp["D"]), f32(inp["bias"])
    z = s["z"].t if c["z"] else None
    args = (s["u"].t, s["delta"].t, A, s["B"].t, s["C"].t, D, z, bias, c["softplus"])
    outs, x, last, info = {}, None, None, []
    _lib.TRACE = trace = []
    try:
        if api == "raw":
            if c["z"]:
                s["out_z"] = _act(shape, dt, c["olayout"], v, output=True)
            if not c["z"] or c["both"]:
                s["out"] = _act(shape, dt, c["olayout"], v, output=True)
            if c["carries"]:        # contiguous, with a NaN guard of 64 rows behind it
                n_chunks = -(-c["L"] // rl.chunk_len(c))
                n = c["B"] * c["dim"] * n_chunks * 2 * N
                s["x"] = Slot((n + 64 * n_chunks * 2 * N,), torch.float32, lambda t: t[:n].view(c["B"], c["dim"], n_chunks, 2 * N), output=True)
                x = s["x"].t
            i32 = lambda a: None if a is None else torch.from_numpy(a.astype(np.int32)).to(DEV)
            ssi.scan_raw(*args, out=s["out"].t if "out" in s else None, out_z=s["out_z"].t if c["z"] else None, x=x, z_row_index=i32(inp["zi"]) if c["z"] else None,
                         out_row_index=i32(inp["oi"]), want_out="out" in s, chunk_len=rl.chunk_len(c), info=info)
            outs = {k: s[k].t for k in ("out", "out_z") if k in s}
        elif api == "cuda_fwd":
            res = ssi.selective_scan_cuda_fwd(*args)
            x = res[1]
            outs = dict(out=res[0], out_z=res[2]) if c["z"] else dict(out=res[0])
        else:
            res = ssi.selective_scan_fn(*args, return_last_state=api == "fn_last")
            res, last = res if api == "fn_last" else (res, None)
            outs = {"out_z" if c["z"] else "out": res}
    finally:
        _lib.TRACE = None
    return dict(outs=outs, slots=s, x=x, last=last, info=info, trace=trace, kernel=_lib.last_kernel())


def check_scan_case(c, inp=None):
    from zigma_amd import _lib
    inp = rl.scan_inputs(c) if inp is None else inp
    run = scan_run(c, inp)
    again = scan_run(c, inp, "raw" if c["api"] == "fn_last" else None)      # (return_last_state hands out one row of the carries: the raw call shows them all)
    for r in (run, again):
        assert r["kernel"] == c["kernel_name"], (c["id"], r["kernel"])
        _served(c["id"], r["trace"], "zigma_selective_scan_fwd", c["kernel_name"])
        assert not r["info"] or r["info"] == [_lib.SCAN_KERNEL_GENERIC, 0], (c["id"], r["info"])
        for name, sl in r["slots"].items():
            assert sl.untouched(), (c["id"], name, "bytes outside the output views have changed")
    ref = rl.scan_reference(c, inp)
    got = {k: _np(t) for k, t in run["outs"].items()}
    x = run["x"] if run["x"] is not None else again["x"]
    if c["carries"]:
        got["x_prod"], got["x_state"] = _np(x[..., 0::2]), _np(x[..., 1::2])
    assert set(got) == set(ref), (c["id"], sorted(got), sorted(ref))
    for key, want in ref.items():
        _report(c["id"], key, got[key], want, rl.bound_of(c, key))
    for key, t in run["outs"].items():
        assert torch.equal(t, again["outs"][key]), (c["id"], key, "two launches differ")
    if run["x"] is not None:
        assert torch.equal(run["x"], again["x"]), (c["id"], "carries: two launches differ")
    if c["api"] == "fn_last":
        assert run["last"].shape == (c["B"], c["dim"], c["N"]) and torch.equal(run["last"], again["x"][:, :, -1, 1::2]), (c["id"], "last_state is not the last carry's state")
    return run


@pytest.mark.parametrize("c", SCAN, ids=_ids(SCAN))
def test_scan_generic_sweep(c):
    check_scan_case(c)


# ---------------------------------------------------------------------------------------------------
# conv_tok_kernel, conv_generic_kernel
# ---------------------------------------------------------------------------------------------------
def _conv_slots(c, x):
    """x and out of a conv case as its layout says (ref_layout_cases.conv_tok_ok)"""
    dt, (Bsz, D, L), lay = DT[c["kind"]], x.shape, c["layout"]
    n = Bsz * L * D
    tok = lambda **kw: Slot((Bsz, L, D + 16), dt, lambda t: t[..., 8:8 + D].transpose(1, 2), **kw)
    off = lambda **kw: Slot((n + 4,), dt, lambda t: t[2:2 + n].view(Bsz, L, D).transpose(1, 2), **kw)       # starts 2 elements into its allocation
    if lay == "cf":             # the reference's (B, D, L), positions contiguous; `fn` takes the plain contiguous tensor
        pad = 0 if c["api"] == "fn" else 3
        mk = lambda **kw: Slot((Bsz, D, L + 2 * pad), dt, lambda t: t[..., pad:pad + L], **kw)
        return mk(fill=x), mk(output=True)
    if lay == "half":           # x: the first half of (B, L, 2 dim) rows; out: rows of pitch dim + 8
        return (Slot((Bsz, L, 2 * D), dt, lambda t: t[..., :D].transpose(1, 2), fill=x),
                Slot((Bsz, L, D + 8), dt, lambda t: t[..., :D].transpose(1, 2), output=True))
    if lay == "cl":             # channel-last rows of a dim that is no multiple of 4
        mk = lambda **kw: Slot((Bsz, L, D + 2), dt, lambda t: t[..., 1:1 + D].transpose(1, 2), **kw)
        return mk(fill=x), mk(output=True)
    if lay == "pitch":          # rows dim + 2 elements apart
        return Slot((Bsz, L, D + 2), dt, lambda t: t[..., :D].transpose(1, 2), fill=x), tok(output=True)
    return (off if lay == "x_off" else tok)(fill=x), (off if lay == "out_off" else tok)(output=True)


def conv_run(c, inp):
    from zigma_amd import _lib
    from zigma_amd.causal_conv1d_interface import causal_conv1d_fn, causal_conv1d_raw
    xs, os_ = _conv_slots(c, inp["x"])
    w, b = _dev(inp["w"], DT[c["wkind"]]), _dev(inp["b"], DT[c["wkind"]])
    rows = None if inp["rows"] is None else torch.from_numpy(inp["rows"].astype(np.int32)).to(DEV)
    _lib.TRACE = trace = []
    try:
        if c["api"] == "fn":
            out = causal_conv1d_fn(xs.t, w, b, "silu" if c["silu"] else None)
        else:
            out = causal_conv1d_raw(xs.t, w, b, c["silu"], out=os_.t, x_row_index=rows, reset_period=c["reset"])
    finally:
        _lib.TRACE = None
    return dict(out=out, slots=dict(x=xs, **({} if c["api"] == "fn" else dict(out=os_))), trace=trace, kernel=_lib.last_kernel())


def check_conv_case(c, inp=None):
    inp = rl.conv_inputs(c) if inp is None else inp
    run, again = conv_run(c, inp), conv_run(c, inp)
    for r in (run, again):
        assert r["kernel"] == c["kernel_name"], (c["id"], r["kernel"])
        _served(c["id"], r["trace"], "zigma_causal_conv1d_fwd", c["kernel_name"])
        for name, sl in r["slots"].items():
            assert sl.untouched(), (c["id"], name, "bytes outside the output view have changed")
    assert run["out"].shape == inp["x"].shape, c["id"]
    _report(c["id"], "conv", _np(run["out"]), rl.conv_reference(c, inp)["conv"], rl.IO_BOUND[c["kind"]])
    assert torch.equal(run["out"], again["out"]), (c["id"], "two launches differ")
    return run


@pytest.mark.parametrize("c", CONV, ids=_ids(CONV))
def test_conv_sweep(c):
    check_conv_case(c)

"""Sweep of the three backward kernels (zigma_selective_scan_bwd, zigma_causal_conv1d_bwd, zigma_add_norm_bwd) against float64 in every I/O
type, over the case tables of tests/bwd_fuzz_cases.py (coverage, oracle soundness and rounding floor: tests/test_bwd_fuzz_cases_cpu.py).

Every case: the kernel the call names really served it (zigma_last_kernel, the parameter block of the call trace); every output is finite
although every buffer it could land in was NaN beforehand, and what lies next to a preallocated output (the other columns of d(x_dbl), the other
half of d(xz), pitch padding) is still NaN; norm-wise distance to the float64 oracle within the bound of the existing tests of that kernel
(bwd_fuzz_cases.*_bounds); and, since a norm hides one wrong row or a wrong tail tile, EVERY row within 4 x that bound of
max(its own norm, the rms row norm) and every element of the reduced gradients within 4 x the bound of max(|ref|, rms(ref)).  The oracle never
sees a kernel result, except the forward's ungated `out` for dz — the kernel's documented contract.  One case per kernel and type runs twice:
bit-identical (fixed summation order).  Production shapes at the end: float64 torch autograd on the device as the reference.

Each case prints `bwd-fuzz <kernel> <type> <output> norm-wise <e> row-wise <r>` (r in units of the bound) for DESIGN.md's parity table.
"""
import numpy as np
import pytest
import torch

import bwd_fuzz_cases as bc
from conftest import rel_err
from oracle import zigma_oracle as zo

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
SCAN, CONV, NORM = bc.scan_cases(), bc.conv_cases(), bc.norm_cases()
NAN = float("nan")


def _ids(cases):
    return [c["id"] for c in cases]


def _dev(a, dtype, pad=0):
    """device tensor in `dtype`; pad > 0: a slice of a NaN-filled buffer whose rows are `pad` elements longer"""
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)
    if not pad:
        return t
    buf = torch.full((*t.shape[:-1], t.shape[-1] + pad), NAN, dtype=dtype, device=DEV)
    buf[..., :t.shape[-1]] = t
    return buf[..., :t.shape[-1]]


def _i32(a):
    return None if a is None else torch.from_numpy(a.astype(np.int32)).to(DEV)


def _np(t):
    return None if t is None else t.detach().double().cpu().numpy()


def _poison(*specs):
    """allocate and free NaN-filled tensors of the shapes / dtypes the wrapper is about to allocate: a recycled block then holds NaN, not
    the previous case's correct answer"""
    keep = [torch.full(shape, NAN, dtype=dtype, device=DEV) for shape, dtype in specs]
    torch.cuda.synchronize()
    del keep


def _traced(fn):
    from zigma_amd import _lib
    _lib.TRACE = []
    try:
        res = fn()
    finally:
        trace, _lib.TRACE = _lib.TRACE, None
    return res, trace


def _compare(kernel, kind, got, ref, bounds, ident):
    """got / ref: dicts of numpy arrays (None where there is no such output)"""
    for key, want in ref.items():
        g = got.get(key)
        if want is None:
            assert g is None, (ident, key)
            continue
        assert g is not None and g.shape == want.shape, (ident, key, None if g is None else g.shape, want.shape)
        assert np.isfinite(g).all(), (ident, key, "not finite: an element was left unwritten, or a NaN / inf was computed")
        e, r = rel_err(g, want), bc.worst_ratio(key, g, want, bounds[key])
        print(f"bwd-fuzz {kernel} {kind} {key} norm-wise {e:.3e} (bound {bounds[key]:.2e}) row-wise {r:.3g} [{ident}]")
        assert e < bounds[key], (ident, key, e, bounds[key])
        assert r <= bc.ROW_GUARD, (ident, key, r)


def _same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------
# scan backward
# ---------------------------------------------------------------------------------------------------
def _scan_device(c, inp):
    """operands on the device as the case lays them out; the forward's ungated out (and the checkpoints) from the forward kernel"""
    from zigma_amd.selective_scan_interface import scan_raw
    dt, Bsz, L, dim, N, R = DT[c["kind"]], c["B"], inp["u"].shape[1], c["dim"], c["N"], bc.R_COLS
    d = dict(u=_dev(inp["u"], dt, c["pad"]), delta=_dev(inp["delta"], dt, c["pad"]), dout=_dev(inp["dout"], dt, c["pad"]), z=_dev(inp["z"], dt),
             A=_dev(inp["A"], torch.float32), D=_dev(inp["D"], torch.float32), bias=_dev(inp["delta_bias"], torch.float32),
             zi=_i32(inp["zi"]), oi=_i32(inp["oi"]), out=None, ck=None)
    if c["bc_slices"]:
        x_dbl = torch.full((Bsz, L, R + 2 * N), NAN, dtype=dt, device=DEV)
        x_dbl[..., :R] = 0
        x_dbl[..., R:R + N], x_dbl[..., R + N:] = _dev(inp["Bm"], dt), _dev(inp["Cm"], dt)
        d["Bm"], d["Cm"] = x_dbl[..., R:R + N], x_dbl[..., R + N:]
    else:
        d["Bm"], d["Cm"] = _dev(inp["Bm"], dt), _dev(inp["Cm"], dt)
    if d["z"] is not None:
        d["out"], oz = torch.empty(Bsz, L, dim, dtype=dt, device=DEV), torch.empty(Bsz, L, dim, dtype=dt, device=DEV)
        if c["ckpt"] == "fwd":
            d["ck"] = torch.full((Bsz, dim // 64, (L + 15) // 16, N, 64), NAN, device=DEV)
        xc = torch.empty(Bsz, dim, (L + 2047) // 2048, 2 * N, device=DEV) if c["carries"] else None
        info = []
        tr = lambda t: t.transpose(1, 2)
        scan_raw(tr(d["u"]), tr(d["delta"]), d["A"], tr(d["Bm"]).unsqueeze(1), tr(d["Cm"]).unsqueeze(1), d["D"], tr(d["z"]), d["bias"],
                 c["softplus"], out=tr(d["out"]), out_z=tr(oz), z_row_index=d["zi"], out_row_index=d["oi"], checkpoints=d["ck"], x=xc,
                 reset_period=c["reset"], info=info)
        if d["ck"] is not None:
            assert info[1] == 1, (c["id"], info)                 # the forward kernel wrote them
            assert torch.isfinite(d["ck"]).all(), c["id"]
    return d


def _scan_call(c, d):
    """one zigma_selective_scan_bwd call with fresh NaN-filled output buffers -> (results, the buffers around them, trace)"""
    from zigma_amd.selective_scan_interface import scan_bwd_tok
    dt, (Bsz, L, dim), N, R = DT[c["kind"]], d["u"].shape, c["N"], bc.R_COLS
    kw, bufs, fresh = {}, {}, [((Bsz, L, dim), dt), ((Bsz, L, dim), dt)]
    if c["dbc_slices"]:
        bufs["dx_dbl"] = torch.full((Bsz, L, R + 2 * N), NAN, device=DEV)
        kw.update(dB=bufs["dx_dbl"][..., R:R + N], dC=bufs["dx_dbl"][..., R + N:])
    else:
        fresh += [((Bsz, L, N), torch.float32)] * 2
    if d["z"] is not None:
        if c["dz_half"]:
            bufs["dxz"] = torch.full((Bsz, L, 2 * dim), NAN, dtype=dt, device=DEV)
            kw["dz"] = bufs["dxz"][..., dim:]
        else:
            fresh.append(((Bsz, L, dim), dt))
    _poison(*fresh)
    res, trace = _traced(lambda: scan_bwd_tok(d["u"], d["delta"], d["A"], d["Bm"], d["Cm"], d["D"], d["z"], d["bias"], d["dout"], d["out"],
                                              c["softplus"], z_row_index=d["zi"], out_row_index=d["oi"], checkpoints=d["ck"],
                                              reset_period=c["reset"], **kw))
    return res, bufs, trace


SCAN_KEYS = ("du", "ddelta", "dA", "dB", "dC", "dD", "dz", "ddelta_bias")


@pytest.mark.parametrize("c", SCAN, ids=_ids(SCAN))
def test_scan_bwd_sweep(c):
    from zigma_amd import _lib
    inp = bc.scan_inputs(c)
    d = _scan_device(c, inp)
    res, bufs, trace = _scan_call(c, d)
    assert _lib.last_kernel() == "scan_bwd_tok" and [t[:2] for t in trace] == [("zigma_selective_scan_bwd", "scan_bwd_tok")]
    P = trace[0][2]
    assert (P.io_dtype, P.dstate, P.seqlen, P.reset_period) == (_lib._DT[DT[c["kind"]]], c["N"], c["L"], c["reset"])
    assert bool(P.checkpoints) == (c["ckpt"] == "fwd") and bool(P.z_row_index) == bool(P.out_row_index) == c["tables"]
    R, N, dim = bc.R_COLS, c["N"], c["dim"]
    if "dx_dbl" in bufs:      # dB / dC are columns of d(x_dbl): its dt_rank columns belong to someone else
        assert torch.isnan(bufs["dx_dbl"][..., :R]).all() and torch.isfinite(bufs["dx_dbl"][..., R:]).all(), c["id"]
        assert res[3].data_ptr() == bufs["dx_dbl"][..., R:].data_ptr() and res[4].data_ptr() == bufs["dx_dbl"][..., R + N:].data_ptr()
    if "dxz" in bufs:         # dz is the upper half of d(xz): the lower half is the conv backward's
        assert torch.isnan(bufs["dxz"][..., :dim]).all() and torch.isfinite(bufs["dxz"][..., dim:]).all(), c["id"]
        assert res[6].data_ptr() == bufs["dxz"][..., dim:].data_ptr()
    ref = bc.scan_reference(c, inp, out=_np(d["out"]))
    _compare("scan", c["kind"], dict(zip(SCAN_KEYS, map(_np, res))), ref, bc.scan_bounds(c["kind"]), c["id"])
    if c["twice"]:
        res2, _, _ = _scan_call(c, d)
        assert _same(res, res2), c["id"]


# ---------------------------------------------------------------------------------------------------
# conv backward
# ---------------------------------------------------------------------------------------------------
def _conv_call(c, d):
    from zigma_amd.causal_conv1d_interface import conv_bwd_tok
    dt, (Bsz, L, dim) = DT[c["kind"]], d["x"].shape
    buf = dx = None
    if c["dx_pad"]:
        buf = torch.full((Bsz, L, dim + c["dx_pad"]), NAN, dtype=dt, device=DEV)
        dx = buf[..., :dim]
    else:
        _poison(((Bsz, L, dim), dt))
    res, trace = _traced(lambda: conv_bwd_tok(d["x"], d["w"], d["b"], d["dout"], c["silu"], d["perm"], dx=dx, reset_period=c["reset"]))
    return res, buf, trace


@pytest.mark.parametrize("c", CONV, ids=_ids(CONV))
def test_conv_bwd_sweep(c):
    from zigma_amd import _lib
    inp = bc.conv_inputs(c)
    dt, wdt = DT[c["kind"]], DT[c["wkind"]]
    d = dict(x=_dev(inp["x"], dt, c["x_pad"]), dout=_dev(inp["dout"], dt), w=_dev(inp["w"], wdt), b=_dev(inp["b"], wdt), perm=_i32(inp["perm"]))
    res, buf, trace = _conv_call(c, d)
    assert _lib.last_kernel() == "conv_bwd_tok" and [t[:2] for t in trace] == [("zigma_causal_conv1d_bwd", "conv_bwd_tok")]
    P = trace[0][2]       # the instantiation asked for is the one launched: <IO, WT, W, SILU>
    assert (P.width, P.io_dtype, P.w_dtype, P.silu_activation) == (c["W"], _lib._DT[dt], _lib._DT[wdt], int(c["silu"])), c["id"]
    assert (P.dim, P.seqlen, P.reset_period, bool(P.x_row_index), bool(P.bias)) == (c["dim"], c["L"], c["reset"], c["table"], c["bias"])
    assert P.x_l_stride == c["dim"] + c["x_pad"] and P.dx_l_stride == c["dim"] + c["dx_pad"]
    if buf is not None:
        assert torch.isnan(buf[..., c["dim"]:]).all() and res[0].data_ptr() == buf.data_ptr(), c["id"]
    ref = bc.conv_reference(c, inp)
    _compare("conv", c["kind"], dict(zip(("dx", "dweight", "dbias"), map(_np, res))), ref, bc.conv_bounds(c["kind"]), c["id"])
    if c["twice"]:
        res2, _, _ = _conv_call(c, d)
        assert _same(res, res2), c["id"]


# ---------------------------------------------------------------------------------------------------
# norm backward
# ---------------------------------------------------------------------------------------------------
def _norm_branch_of(P):
    """launch_norm_bwd's rule (csrc/norm_bwd.hip) applied to the parameter block that went to the library"""
    es = {0: 4, 1: 2, 2: 2}
    xs, rs, ws = es[P.x_dtype], es[P.res_dtype], es[P.w_dtype]
    al = lambda q, a: not q or q % a == 0
    vec = (P.cols % 4 == 0 and all(s % 4 == 0 for s in (P.xsum_row_stride, P.dy_row_stride, P.dres_out_row_stride, P.dx_row_stride, P.dres_row_stride))
           and al(P.xsum, 4 * rs) and al(P.dy, 4 * xs) and al(P.dresidual_out, 4 * rs) and al(P.dx, 4 * xs) and al(P.dresidual, 4 * rs)
           and al(P.weight, 4 * ws))
    if vec and P.cols <= 768:
        return (4, 3)
    if vec and P.cols <= 2048:
        return (4, 8)
    return (1, 4) if P.cols <= 256 else (1, 12) if P.cols <= 768 else (1, 32) if P.cols <= 2048 else None


def _norm_call(c, d):
    from zigma_amd.layernorm import norm_bwd
    xdt, rdt = DT[c["xk"]], DT[c["rk"]]
    _poison(*([((c["rows"], c["cols"]), xdt)] * c["want_dx"] + [((c["rows"], c["cols"]), rdt)] * c["want_dres"]))
    return _traced(lambda: norm_bwd(d["xsum"], d["w"], d["dy"], d["dres_out"], bc.EPS, c["rms"], x_dtype=xdt, want_dx=c["want_dx"],
                                    want_dres=c["want_dres"], has_bias=c["bias"]))


@pytest.mark.parametrize("c", NORM, ids=_ids(NORM))
def test_norm_bwd_sweep(c):
    from zigma_amd import _lib
    inp = bc.norm_inputs(c)
    xdt, rdt = DT[c["xk"]], DT[c["rk"]]
    d = dict(xsum=_dev(inp["xsum"], rdt, c["pitch_pad"]), dy=_dev(inp["dy"], xdt, c["pitch_pad"]), dres_out=_dev(inp["dres_out"], rdt, c["pitch_pad"]),
             w=_dev(inp["w"], DT[c["wk"]]) if c["wk"] else None)
    if c["error"]:
        with pytest.raises(RuntimeError, match="zigma_add_norm_bwd"):
            _norm_call(c, d)
        return
    res, trace = _norm_call(c, d)
    assert _lib.last_kernel() == "add_norm_bwd" and [t[:2] for t in trace] == [("zigma_add_norm_bwd", "add_norm_bwd")]
    P = trace[0][2]
    assert (P.x_dtype, P.res_dtype, P.w_dtype) == (_lib._DT[xdt], _lib._DT[rdt], _lib._DT[DT[c["wk"] or c["xk"]]]), c["id"]
    assert (P.rows, P.cols, P.is_rms, bool(P.weight), bool(P.dbias), bool(P.dresidual_out), bool(P.dx), bool(P.dresidual)) == \
        (c["rows"], c["cols"], int(c["rms"]), c["wk"] is not None, c["bias"], c["dres_out"], c["want_dx"], c["want_dres"]), c["id"]
    assert c["rows"] == 1 or P.xsum_row_stride == c["cols"] + c["pitch_pad"] == P.dy_row_stride      # (one row: torch normalises its stride)
    assert _norm_branch_of(P) == c["branch"], (c["id"], _norm_branch_of(P), c["branch"])       # the launch branch the table expects
    dx, dres, dw, db = res
    assert (dx is None or dx.dtype == xdt) and (dres is None or dres.dtype == rdt)
    ref = bc.norm_reference(c, inp)
    _compare("norm", f"x{c['xk']}/r{c['rk']}", dict(dx=_np(dx), dresidual=_np(dres), dweight=_np(dw), dbias=_np(db)), ref, bc.norm_bounds(c), c["id"])
    if c["twice"]:
        res2, _ = _norm_call(c, d)
        assert _same(res, res2), c["id"]


def test_norm_sweep_takes_every_launch_branch():
    """all five (VEC, ITERS) branches of launch_norm_bwd are in the table (each case asserts its own from its parameter block)"""
    assert {c["branch"] for c in NORM if not c["error"]} == set(bc.NORM_BRANCHES)


# ---------------------------------------------------------------------------------------------------
# production shapes: float64 torch autograd on the device through the plain restatements of bwd_fuzz_cases
# ---------------------------------------------------------------------------------------------------
def _rand(gen, kind, *shape, scale=1.0, f32=False):
    """values representable in the case's type, as float64 leaf (reference) and in the type (kernel)"""
    t = (torch.randn(*shape, generator=gen) * scale).to(DEV)
    lo = t if f32 else t.to(DT[kind])
    return lo, lo.double().requires_grad_(True)


def _zigzag_tables():
    paths = zo.zigzag_paths(32)
    perm, out_rows = paths[1].astype(np.int32), paths[2].astype(np.int32)        # out_rows is not perm: the write-back goes elsewhere
    assert not np.array_equal(perm, out_rows)
    return torch.from_numpy(perm).to(DEV), torch.from_numpy(out_rows).to(DEV)


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_scan_bwd_production_shape(kind):
    """zigma_selective_scan_bwd as MambaInnerTokFn.backward calls it: B = 2, L = 1024, Di = 1280, N = 16, R = 40, zigzag row tables with
    out_rows != perm, dB / dC into the columns of an fp32 d(x_dbl), dz into the z half of d(xz), checkpoints written by the forward kernel."""
    from zigma_amd import _lib
    from zigma_amd.selective_scan_interface import scan_bwd_tok, scan_raw
    Bsz, L, Di, N, R = 2, 1024, 1280, 16, 40
    dt, gen = DT[kind], torch.Generator().manual_seed(41)
    perm, out_rows = _zigzag_tables()
    u, u64 = _rand(gen, kind, Bsz, L, Di)
    delta, delta64 = _rand(gen, kind, Bsz, L, Di, scale=0.3)
    x_dbl, x_dbl64 = _rand(gen, kind, Bsz, L, R + 2 * N)
    xz, xz64 = _rand(gen, kind, Bsz, L, 2 * Di)
    dout, _ = _rand(gen, kind, Bsz, L, Di)
    A = (-0.5 * torch.rand(Di, N, generator=gen) - 0.05).to(DEV)
    D = torch.randn(Di, generator=gen).to(DEV)
    bias = (0.5 * torch.rand(Di, generator=gen)).to(DEV)
    bias[0] = 25.0
    A64, D64, bias64 = (t.double().requires_grad_(True) for t in (A, D, bias))
    Bm, Cm, z = x_dbl[..., R:R + N], x_dbl[..., R + N:], xz[..., Di:]
    out, y = torch.empty(Bsz, L, Di, dtype=dt, device=DEV), torch.empty(Bsz, L, Di, dtype=dt, device=DEV)
    ck = torch.full((Bsz, Di // 64, L // 16, N, 64), NAN, device=DEV)
    info, tr = [], lambda t: t.transpose(1, 2)
    scan_raw(tr(u), tr(delta), A, tr(Bm).unsqueeze(1), tr(Cm).unsqueeze(1), D, tr(z), bias, True, out=tr(out), out_z=tr(y), z_row_index=perm,
             out_row_index=out_rows, checkpoints=ck, info=info)
    assert info[1] == 1 and torch.isfinite(ck).all()
    dx_dbl = torch.full((Bsz, L, R + 2 * N), NAN, device=DEV)
    dxz = torch.full((Bsz, L, 2 * Di), NAN, dtype=dt, device=DEV)
    _poison(((Bsz, L, Di), dt), ((Bsz, L, Di), dt))
    res, trace = _traced(lambda: scan_bwd_tok(u, delta, A, Bm, Cm, D, z, bias, dout, out, True, dB=dx_dbl[..., R:R + N], dC=dx_dbl[..., R + N:],
                                              dz=dxz[..., Di:], z_row_index=perm, out_row_index=out_rows, checkpoints=ck))
    assert [t[:2] for t in trace] == [("zigma_selective_scan_bwd", "scan_bwd_tok")] and trace[0][2].io_dtype == _lib._DT[dt]
    assert torch.isnan(dx_dbl[..., :R]).all() and torch.isnan(dxz[..., :Di]).all()
    zi, oi = perm.long(), out_rows.long()
    y64 = bc.torch_scan(u64, delta64, A64, x_dbl64[..., R:R + N], x_dbl64[..., R + N:], D64, xz64[..., Di:], bias64, True, zi, oi)
    y64.backward(dout.double())
    z_s, dout_s, out_s = z.double().index_select(1, zi), dout.double().index_select(1, oi), out.double().index_select(1, oi)
    sg = torch.sigmoid(z_s)
    dz_ref = torch.empty_like(z_s).index_copy_(1, zi, dout_s * out_s * sg * (1 + z_s * (1 - sg)))       # from the forward kernel's out: the contract
    ref = dict(du=u64.grad, ddelta=delta64.grad, dA=A64.grad, dB=x_dbl64.grad[..., R:R + N], dC=x_dbl64.grad[..., R + N:], dD=D64.grad, dz=dz_ref,
               ddelta_bias=bias64.grad)
    got = dict(zip(SCAN_KEYS, map(_np, res)))
    _compare("scan", kind, got, {k: _np(v) for k, v in ref.items()}, bc.scan_bounds(kind), f"production-{kind}")


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_conv_bwd_production_shape(kind):
    """zigma_causal_conv1d_bwd at B = 2, L = 1024, Di = 1280: x the lower half of xz, the zigzag table, dx into the lower half of d(xz)."""
    from zigma_amd import _lib
    from zigma_amd.causal_conv1d_interface import conv_bwd_tok
    Bsz, L, Di = 2, 1024, 1280
    dt, gen = DT[kind], torch.Generator().manual_seed(43)
    perm, _ = _zigzag_tables()
    xz, xz64 = _rand(gen, kind, Bsz, L, 2 * Di)
    w, w64 = _rand(gen, kind, Di, 4, scale=0.5)
    b, b64 = _rand(gen, kind, Di, scale=0.2)
    dout, _ = _rand(gen, kind, Bsz, L, Di)
    dxz = torch.full((Bsz, L, 2 * Di), NAN, dtype=dt, device=DEV)
    res, trace = _traced(lambda: conv_bwd_tok(xz[..., :Di], w, b, dout, True, perm, dx=dxz[..., :Di]))
    P = trace[0][2]
    assert [t[:2] for t in trace] == [("zigma_causal_conv1d_bwd", "conv_bwd_tok")]
    assert (P.width, P.io_dtype, P.w_dtype, P.silu_activation, P.x_l_stride, P.dx_l_stride) == (4, _lib._DT[dt], _lib._DT[dt], 1, 2 * Di, 2 * Di)
    assert torch.isnan(dxz[..., Di:]).all() and res[0].data_ptr() == dxz.data_ptr()
    bc.torch_conv(xz64[..., :Di], w64, b64, True, perm.long()).backward(dout.double())
    ref = dict(dx=xz64.grad[..., :Di], dweight=w64.grad, dbias=b64.grad)
    _compare("conv", kind, dict(zip(("dx", "dweight", "dbias"), map(_np, res))), {k: _np(v) for k, v in ref.items()}, bc.conv_bounds(kind),
             f"production-{kind}")


@pytest.mark.parametrize("rms", [True, False], ids=["rms-dro", "ln-bias"])
@pytest.mark.parametrize("cols", [640, 768])
@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_norm_bwd_production_shape(kind, cols, rms):
    """zigma_add_norm_bwd as a 16-bit model trains: rows = 2 * 1024, x 16-bit, fp32 residual stream, 16-bit weight; RMSNorm with the residual
    stream's incoming gradient, LayerNorm with a bias."""
    from zigma_amd import _lib
    from zigma_amd.layernorm import norm_bwd
    rows = 2 * 1024
    dt, gen = DT[kind], torch.Generator().manual_seed(47 + cols)
    xsum, x64 = _rand(gen, kind, rows, cols, f32=True)
    dy, _ = _rand(gen, kind, rows, cols)
    w, w64 = _rand(gen, kind, cols, scale=0.2)
    w = (w.float() + 1).to(dt)
    w64 = w.double().requires_grad_(True)
    dro = torch.randn(rows, cols, generator=gen).to(DEV) if rms else None
    b64 = None if rms else torch.zeros(cols, dtype=torch.float64, device=DEV, requires_grad=True)
    _poison(((rows, cols), dt), ((rows, cols), torch.float32))
    res, trace = _traced(lambda: norm_bwd(xsum, w, dy, dro, bc.EPS, rms, x_dtype=dt, want_dx=True, want_dres=True, has_bias=not rms))
    P = trace[0][2]
    assert [t[:2] for t in trace] == [("zigma_add_norm_bwd", "add_norm_bwd")]
    assert (P.x_dtype, P.res_dtype, P.w_dtype) == (_lib._DT[dt], _lib.F32, _lib._DT[dt]) and _norm_branch_of(P) == (4, 3)
    loss = (bc.torch_norm(x64, w64, b64, bc.EPS, rms) * dy.double()).sum()
    if dro is not None:
        loss = loss + (x64 * dro.double()).sum()
    loss.backward()
    ref = dict(dx=_np(x64.grad), dresidual=_np(x64.grad), dweight=_np(w64.grad), dbias=None if rms else _np(b64.grad))
    c = dict(xk=kind, rk="f32", wk=kind)
    _compare("norm", f"x{kind}/rf32", dict(zip(("dx", "dresidual", "dweight", "dbias"), map(_np, res))), ref, bc.norm_bounds(c),
             f"production-{kind}-{cols}-{'rms' if rms else 'ln'}")

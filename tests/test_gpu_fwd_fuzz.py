"""Sweep of the forward Mamba-inner kernels — scan_tok2_kernel and scan_tok_kernel (zigma_selective_scan_fwd), zigma_conv_x_proj_fwd,
zigma_x_proj_fwd, zigma_dt_proj_softplus_fwd — against float64 row by row, over the case tables of tests/fwd_fuzz_cases.py (coverage, the
references' soundness and the rounding model: tests/test_fwd_fuzz_cases_cpu.py, which also runs every function of this file on the CPU against
the float64 stand-ins of tests/kernel_standins.py).

Every case goes through scan_raw / conv_x_proj / x_proj / dt_proj_softplus, never through the model, and asserts: the kernel that served it
(zigma_last_kernel, `info`); finite outputs although every output buffer, the carry tensor, the checkpoints and the split's delta workspace
were NaN beforehand; NaN surroundings of every operand and output still NaN; the norm-wise bound and, for EVERY row, the row-wise limit of
every output (fwd_fuzz_cases: limits); bit-for-bit equality for the known-answer cases, for the cases that run twice and between the six-
resident form and the same case pinned to five resident workgroups.  Each output prints one `fwd-sweep` line for DESIGN.md's parity table.
"""
import numpy as np
import pytest
import torch

import fwd_fuzz_cases as fc

pytestmark = pytest.mark.gpu
DEV = "cuda"            # (the CPU test file points this at "cpu" and serves _lib.call with the stand-ins)
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
NAN = float("nan")
SCAN2, SCAN1, CONVX, XPROJ, DTPROJ = fc.scan2_cases(), fc.scan1_cases(), fc.conv_xproj_cases(), fc.xproj_cases(), fc.dtproj_cases()


def _ids(cases):
    return [c["id"] for c in cases]


def _dev(a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def _np(t):
    return None if t is None else t.detach().double().cpu().numpy()


class Slot:
    """a tensor that is a column slice of a wider NaN-filled buffer (views=False: a plain contiguous tensor)"""
    def __init__(self, shape, dtype, views, lead=8, tail=8, fill=None):
        self.views = views
        if views:
            self.buf = torch.full((*shape[:-1], lead + shape[-1] + tail), NAN, dtype=dtype, device=DEV)
            self.t = self.buf[..., lead:lead + shape[-1]]
        else:
            self.buf = self.t = torch.full(shape, NAN, dtype=dtype, device=DEV)
        if fill is not None:
            self.t.copy_(_dev(fill, dtype))

    def surroundings_nan(self):
        if not self.views:
            return True
        lead, n = self.t.storage_offset() % self.buf.shape[-1], self.t.shape[-1]
        return bool(torch.isnan(self.buf[..., :lead]).all() and torch.isnan(self.buf[..., lead + n:]).all())


def _report(ident, key, got, ref, bound, terms=None, elementwise=False):
    assert got.shape == ref.shape, (ident, key, got.shape, ref.shape)
    assert np.isfinite(got).all(), (ident, key, "not finite: an element was left unwritten, or a NaN / inf was computed")
    e = fc.norm_err(got, ref)
    r = fc.elementwise_worst(got, ref, bound) if elementwise else fc.row_ratio(got, ref, bound, terms)
    print(f"fwd-sweep {ident}: {key} norm-wise {e:.3e} (bound {bound:.2e}), {'element' if elementwise else 'row'}-wise ratio {r:.3g}")
    assert e < bound, (ident, key, e, bound)
    assert r <= fc.ROW_GUARD, (ident, key, r)


# ---------------------------------------------------------------------------------------------------
# the two scan kernels
# ---------------------------------------------------------------------------------------------------
def scan_run(c, inp, r5=False):
    """one scan_raw call on fresh buffers laid out as the case says -> dict of the raw output tensors and the slots around them"""
    from zigma_amd import _lib
    from zigma_amd.selective_scan_interface import scan_raw
    dt, (Bsz, L, dim), N, R, v = DT[c["kind"]], inp["u"].shape, c["N"], c["R"], c["views"]
    tr = lambda t: None if t is None else t.transpose(1, 2)
    s = dict(u=Slot((Bsz, L, dim), dt, v, fill=inp["u"]))
    xd = _dev(inp["xdbl"], dt)                              # B | C (and the dt columns) inside one buffer, NaN elsewhere
    Bv, Cv = (xd[..., o:o + N].transpose(1, 2).unsqueeze(1) for o in (R, R + N))
    if c["z"]:                                              # z: the upper half of a (B, L, 2 dim) buffer
        s["z"] = Slot((Bsz, L, dim), dt, v, lead=dim, tail=0, fill=inp["z"])
        s["out_z"] = Slot((Bsz, L, dim), dt, v, lead=0, tail=16, fill=inp["out_z0"])
    if c["out"]:
        s["out"] = Slot((Bsz, L, dim), dt, v, lead=16, tail=0)
    delta = None
    if inp["delta"] is not None:
        s["delta"] = Slot((Bsz, L, dim), dt, v, lead=0, tail=8, fill=inp["delta"])
        delta = s["delta"].t
    elif c["chunk"]:                                        # the split's workspace: its first pass writes the step sizes there
        s["delta_ws"] = Slot((Bsz, L, dim), dt, v, lead=8, tail=8)
        delta = s["delta_ws"].t
    w = None
    if c["dt"]:
        s["w"] = Slot((dim, R), dt, v, lead=0, tail=8, fill=inp["w"])
        w = s["w"].t
    x = torch.full((Bsz, dim, -(-L // c["chunk"]), 2 * N), NAN, device=DEV) if c["chunk"] else None
    ck = torch.full((Bsz, dim // 64, -(-L // 16), N, 64), NAN, device=DEV) if c["ckpt"] else None
    i32 = lambda a: None if a is None else torch.from_numpy(a.astype(np.int32)).to(DEV)
    info = []
    flags = (_lib.SCAN_PROBE_V1 if c["v1"] else 0) | ((1 << _lib.SCAN_PROBE_R5_SHIFT) if r5 else 0)
    scan_raw(tr(s["u"].t), tr(delta), _dev(inp["A"], torch.float32), Bv, Cv, _dev(inp["D"], torch.float32), tr(s["z"].t) if c["z"] else None,
             _dev(inp["bias"], torch.float32), c["softplus"], out=tr(s["out"].t) if c["out"] else None, out_z=tr(s["out_z"].t) if c["z"] else None,
             x=x, z_row_index=i32(inp["zi"]), out_row_index=i32(inp["oi"]), want_out=c["out"], checkpoints=ck, reset_period=c["reset"],
             chunk_len=c["chunk"] or 2048, z_preactivated=c["zact"], info=info, _probe_flags=flags, dt_x=xd if c["dt"] else None, dt_w=w,
             accumulate=c["acc"])
    return dict(slots=s, x=x, ck=ck, info=info, kernel=_lib.last_kernel())


def scan_outputs(c, run):
    """the raw tensors of a run, in float64 and in the layout of fc.scan_reference"""
    s, got = run["slots"], {}
    for key in ("out_z", "out"):
        if key in s:
            got[key] = _np(s[key].t)
    if "delta_ws" in s:
        got["delta"] = _np(s["delta_ws"].t)
    if run["x"] is not None:
        x = _np(run["x"]).transpose(0, 2, 1, 3)             # (B, dim, chunk, 2N) -> (B, chunk, dim, 2N)
        got["x_prod"], got["x_state"] = x[..., 0::2], x[..., 1::2]
    if run["ck"] is not None:
        ck = _np(run["ck"])                                 # (B, slab, tile, N, 64) -> (B, tile, dim, N)
        got["ckpt"] = ck.transpose(0, 2, 1, 4, 3).reshape(ck.shape[0], ck.shape[2], -1, ck.shape[3])
    return got


def _raw(run):
    return [sl.t for sl in run["slots"].values()] + [t for t in (run["x"], run["ck"]) if t is not None]


def check_scan_case(c, inp=None):
    from zigma_amd import _lib
    inp = fc.scan_inputs(c) if inp is None else inp
    run = scan_run(c, inp)
    family = _lib.SCAN_KERNEL_TOK2 if c["kernel_name"].startswith("scan_tok2") else _lib.SCAN_KERNEL_TOK
    assert run["kernel"] == c["kernel_name"] and run["info"] == [family, c["info1"]], (c["id"], run["kernel"], run["info"])
    for name, sl in run["slots"].items():
        assert sl.surroundings_nan(), (c["id"], name, "the NaN surroundings were written")
    got = scan_outputs(c, run)
    for key, g in got.items():
        assert np.isfinite(g).all(), (c["id"], key, "not finite")
    ref = fc.scan_reference(c, inp)
    if "delta" in got:      # staged: the 16-bit delta the first pass wrote, then the scan on the kernel's own delta
        _report(c["id"], "delta", got["delta"], ref["delta"], fc.bound_of(c, "delta"), elementwise=True)
        flips = fc.flipped_share(got["delta"], ref["delta"], c["kind"])
        print(f"fwd-sweep {c['id']}: delta off the correctly rounded value in {flips:.4f} of its elements")
        assert flips <= fc.DELTA_FLIPS, (c["id"], flips)
        ref = fc.scan_reference(c, inp, step=got["delta"])
    assert {k for k in ref if not k.startswith("_")} == set(got) - {"delta"}, (c["id"], sorted(ref), sorted(got))
    for key, want in ref.items():
        if not key.startswith("_"):
            _report(c["id"], key, got[key], want, fc.bound_of(c, key), terms=ref.get("_acc_terms") if key == "out_z" else None)
    if c["known"]:
        ans = fc.known_answer(c, inp)
        for key, want in ans.items():
            assert np.array_equal(got[key], fc.round_to(want, fc.out_kind(c, key)).astype(np.float64)), (c["id"], key, "known answer: not bit for bit")
    if c["twice"]:
        again = scan_run(c, inp)
        assert all(torch.equal(a, b) for a, b in zip(_raw(run), _raw(again))), (c["id"], "two runs differ")
    if c["r6_twin"]:
        five = scan_run(c, inp, r5=True)
        assert "_r6" in run["kernel"] and five["kernel"] == run["kernel"].replace("_r6", ""), (c["id"], run["kernel"], five["kernel"])
        assert all(torch.equal(a, b) for a, b in zip(_raw(run), _raw(five))), (c["id"], "six and five resident workgroups differ")
    return run


@pytest.mark.parametrize("c", SCAN2, ids=_ids(SCAN2))
def test_scan_tok2_sweep(c):
    check_scan_case(c)


@pytest.mark.parametrize("c", SCAN1, ids=_ids(SCAN1))
def test_scan_tok_sweep(c):
    check_scan_case(c)


# ---------------------------------------------------------------------------------------------------
# conv_x_proj, x_proj, dt_proj
# ---------------------------------------------------------------------------------------------------
def check_conv_xproj_case(c):
    from zigma_amd import _lib
    from zigma_amd.selective_scan_interface import conv_x_proj
    inp, dt, dim = fc.conv_xproj_inputs(c), DT[c["kind"]], c["dim"]
    xz = _dev(inp["xz"], dt)                                # x_half: the lower half; the upper half is NaN
    perm = None if inp["perm"] is None else torch.from_numpy(inp["perm"]).to(DEV)
    u, x_dbl = conv_x_proj(xz[..., :dim], _dev(inp["cw"], dt), _dev(inp["cb"], dt), _dev(inp["w"], dt), perm, _flags=c["flags"])
    assert _lib.last_kernel() == "conv_x_proj_mfma" and u.shape == (c["B"], c["L"], dim) and x_dbl.shape == (c["B"], c["L"], c["n"]), c["id"]
    assert torch.isnan(xz[..., dim:]).all(), c["id"]
    ref = fc.conv_xproj_reference(c, inp, u_own=_np(u))
    for key, got in (("u", u), ("x_dbl", x_dbl)):
        _report(c["id"], key, _np(got), ref[key], fc.IO_BOUND[c["kind"]])


@pytest.mark.parametrize("c", CONVX, ids=_ids(CONVX))
def test_conv_x_proj_sweep(c):
    check_conv_xproj_case(c)


def check_xproj_case(c):
    from zigma_amd import _lib
    from zigma_amd.selective_scan_interface import x_proj
    inp, dt = fc.xproj_inputs(c), DT[c["kind"]]
    u = Slot((c["M"], c["K"]), dt, c["pad"] > 0, lead=0, tail=c["pad"], fill=inp["u"])
    w = Slot((c["n"], c["K"]), dt, c["pad"] > 0, lead=0, tail=c["pad"], fill=inp["w"])
    out = x_proj(u.t, w.t)
    assert _lib.last_kernel() == c["kernel_name"] and out.shape == (c["M"], c["n"]), (c["id"], _lib.last_kernel())
    assert u.surroundings_nan() and w.surroundings_nan(), c["id"]
    _report(c["id"], "x_dbl", _np(out), fc.xproj_reference(c, inp)["x_dbl"], fc.IO_BOUND[c["kind"]])
    assert torch.equal(x_proj(u.t, w.t), out), (c["id"], "two runs differ")         # fixed summation order


@pytest.mark.parametrize("c", XPROJ, ids=_ids(XPROJ))
def test_x_proj_sweep(c):
    check_xproj_case(c)


def check_dtproj_case(c):
    from zigma_amd import _lib
    from zigma_amd.selective_scan_interface import dt_proj_softplus
    inp, dt, R = fc.dtproj_inputs(c), DT[c["kind"]], c["R"]
    x = _dev(inp["x"], dt)                                  # columns beyond R are NaN
    w = Slot((c["dim"], R), dt, c["w_pad"] > 0, lead=0, tail=c["w_pad"], fill=inp["w"])
    out = dt_proj_softplus(x, R, w.t, _dev(inp["bias"], torch.float32), c["softplus"])
    assert _lib.last_kernel() == "dt_proj_softplus_mfma" and out.shape == (c["M"], c["dim"]), c["id"]
    assert w.surroundings_nan(), c["id"]
    ref = fc.dtproj_reference(c, inp)["delta"]
    bound = fc.IO_BOUND[c["kind"]]
    _report(c["id"], "delta", _np(out), ref, bound)
    _report(c["id"], "delta", _np(out), ref, bound, elementwise=True)
    flips = fc.flipped_share(_np(out), ref, c["kind"])
    print(f"fwd-sweep {c['id']}: delta off the correctly rounded value in {flips:.4f} of its elements")
    assert flips <= fc.DELTA_FLIPS, (c["id"], flips)


@pytest.mark.parametrize("c", DTPROJ, ids=_ids(DTPROJ))
def test_dt_proj_sweep(c):
    check_dtproj_case(c)


# ---------------------------------------------------------------------------------------------------
# production shapes: the sweep's metric where the model runs
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", fc.production_cases(), ids=_ids(fc.production_cases()))
def test_scan_production_shape(c):
    check_scan_case(c, fc.production_inputs(c))

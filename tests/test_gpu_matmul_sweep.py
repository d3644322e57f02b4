"""Sweep of the fp32 split projection — linear_split_kernel<3 | 1> behind zigma_linear_f32_split — and of the weight-gradient kernels —
wgrad_kernel<T, 128 | 64> and wgrad_reduce_kernel behind zigma_linear_wgrad — against float64 on EVERY output element, over the case tables of
tests/matmul_sweep_cases.py (coverage, the references' soundness and the fp32 model: tests/test_matmul_sweep_cases_cpu.py, which also runs every
function of this file on the CPU against the float64 stand-ins of tests/kernel_standins.py).

Every case fills the parameter block itself and goes through _lib.call.  Every operand and output is a window of a NaN-filled buffer with its own
lead and pitch and NaN rows below (x of the split: NaN from row m to the end of its 128-row tile; dy and x of wgrad: column windows with NaN
columns to their right and 64 NaN rows below); the two weight planes have different pitches; the wgrad workspace is NaN and 64 elements longer
than workspace_bytes.  Asserted per case: the kernel string (from the passes; from wgrad_bk and wgrad_slabs restated); every byte around every
window and every input operand bit for bit what it was before the call (integer views), the workspace past workspace_bytes still NaN; finite
outputs although they were NaN beforehand; a second launch bit-identical; the limits of the case table's docstring on every element, compared on
the host in float64; the known answers bit for bit — selection weights (FLT_MAX under a unit weight is +inf in "high": hi = 0x7f7f plus
lo = 2^120, by the definition), the three integer kinds, periodic rows; token selection and sparse integers, the latter equal to the one-slab
launch — and the short table of non-finite inputs.  Each case prints one `matmul-sweep` line for DESIGN.md's table.
"""
import time

import numpy as np
import pytest
import torch

import matmul_sweep_cases as mc

pytestmark = pytest.mark.gpu
DEV = "cuda"            # (the CPU test file points this at "cpu" and serves _lib.call with the stand-ins)
DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
INT = {2: torch.int16, 4: torch.int32}
NAN = float("nan")
SPLIT, WGRAD, PRODUCTION = mc.split_cases(), mc.wgrad_cases(), mc.production_cases()
TIMES = {}              # id -> seconds (test_zz_summary prints the counts, the wall time and the slowest case)
WS_TAIL, LEAD_WS = 64, 4 # fp32 elements of the workspace buffer past workspace_bytes, and in front of the workspace


def _ids(cases):
    return [c["id"] for c in cases]


class Win:
    """(rows, cols) window of a flat NaN-filled buffer: `lead` elements in front, rows `pitch` apart, `below` NaN rows after the last one.
    fill: float32 values, or uint16 bit patterns of a 16-bit type"""
    def __init__(self, shape, dtype, fill=None):
        rows, cols, lead, pitch, below = shape
        self.buf = torch.full((lead + (rows + below) * pitch,), NAN, dtype=dtype, device=DEV)
        self.geom = ((rows, cols), (pitch, 1), lead)
        self.t = self.buf.as_strided(*self.geom)
        if fill is not None:
            fill = np.ascontiguousarray(fill)
            src = torch.from_numpy(fill.view(np.int16)).view(dtype) if fill.dtype == np.uint16 else torch.from_numpy(fill)
            self.t.copy_(src.to(DEV).to(dtype))
        self.before = None

    def bits(self):
        return self.buf.view(INT[self.buf.element_size()])

    def snapshot(self):
        self.before = self.bits().clone()

    def unchanged(self, but_window=False):
        """every byte of the buffer (but_window: outside the window) has the bit pattern of the snapshot"""
        diff = self.before != self.bits()
        if but_window:
            diff.as_strided(*self.geom).fill_(False)
        return not bool(diff.any())


def _host(t):
    """on the host as numpy; a 16-bit tensor as the float32 array of the same values (exact, and +-0 stay apart)"""
    t = t.detach()
    return (t if t.dtype == torch.float32 or t.dtype == torch.float64 else t.float()).cpu().numpy()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _call(c, name, P):
    from zigma_amd import _lib
    _lib.call(name, P, torch.device(DEV))
    assert _lib.last_kernel() == c["kernel_name"], (c["id"], _lib.last_kernel(), c["kernel_name"])


def clean(c, w, written):
    for name, win in w.items():
        assert win.unchanged(but_window=name in written), (c["id"], name, "bytes outside the output window were written" if name in written else "an operand changed")


# ---------------------------------------------------------------------------------------------------
# zigma_linear_f32_split
# ---------------------------------------------------------------------------------------------------
def split_windows(c, inp):
    sh, f32, bf = mc.split_fields(c)["shape"], torch.float32, torch.bfloat16
    w = dict(x=Win(sh["x"], f32, inp["x"]), w_hi=Win(sh["w_hi"], bf, inp["w_hi"]), w_lo=Win(sh["w_lo"], bf, inp["w_lo"]), out=Win(sh["out"], f32))
    if c["bias"]:
        w["bias"] = Win(sh["bias"], f32, inp["bias"][None])
    assert _same_bits(_host(w["x"].t), inp["x"]), "the operand on the device holds the case's bit patterns"
    return w


def split_params(c, w, x=None, out=None):
    from zigma_amd import _lib
    x, out = (x or w["x"]).t, (out or w["out"]).t
    P = _lib.LinearSplitParams()
    P.m, P.n, P.k, P.passes, P.flags = c["m"], c["n"], c["k"], c["passes"], 0
    P.x_row_stride, P.w_hi_row_stride, P.w_lo_row_stride, P.out_row_stride = x.stride(0), w["w_hi"].t.stride(0), w["w_lo"].t.stride(0), out.stride(0)
    assert (P.x_row_stride, P.w_hi_row_stride, P.w_lo_row_stride, P.out_row_stride) == (c["k"] + c["x_pad"], c["k"] + 8, c["k"] + 24, c["n"] + c["out_pad"])
    P.x, P.w_hi, P.out = x.data_ptr(), w["w_hi"].t.data_ptr(), out.data_ptr()
    P.w_lo = w["w_lo"].t.data_ptr() if c["passes"] == 3 else None          # ("medium" does not read it)
    if c["bias"]:
        P.bias = w["bias"].t.data_ptr()
        assert P.bias % 16 == 0
    return P


def split_run(c, w, x=None, out=None):
    """the case's call, checked for the kernel string, for stray writes and for a bit-identical second launch -> the output on the host"""
    every = dict(w, **({"x": x} if x else {}), **({"out": out} if out else {}))
    for win in every.values():
        win.snapshot()
    P = split_params(c, w, x, out)
    _call(c, "zigma_linear_f32_split", P)
    clean(c, every, ("out",))
    first = _host(every["out"].t)
    _call(c, "zigma_linear_f32_split", P)
    assert _same_bits(first, _host(every["out"].t)), (c["id"], "the second launch differs from the first")
    return first


def split_limits(c, got, ref, mask=None, tag="out"):
    need = mc.split_need(c, got, ref, mask)
    rows = f", row-wise ratio {need['rows'] * mc.ROW_GUARD:.3g}" if "rows" in need else ""
    print(f"matmul-sweep {c['id']}: {tag} [split{c['passes']}] element-wise {need['true']:.3f} of the limit vs the true product (2^{int(np.log2(mc.TOL_TRUE[c['passes']]))} "
          f"sum|x||w| + 2^-133 sum|w|), {need['planes']:.3f} of the limit vs the planes (2^-16 sum|x||w|){rows}")
    assert all(v <= 1.0 for v in need.values()), (c["id"], tag, need)


def check_split_case(c):
    t0 = time.perf_counter()
    inp = mc.split_inputs(c)
    w = split_windows(c, inp)
    got = split_run(c, w)
    if c["nonfinite"]:
        r0, c0 = mc.nonfinite_at(c)
        inp0 = dict(inp, x=inp["x"].copy())
        inp0["x"][r0, c0] = 0.0
        x0, out0 = Win(mc.split_fields(c)["shape"]["x"], torch.float32, inp0["x"]), Win(mc.split_fields(c)["shape"]["out"], torch.float32)
        got0 = split_run(c, w, x=x0, out=out0)
        others = np.arange(c["m"]) != r0
        assert _same_bits(got[others], got0[others]), (c["id"], "a non-finite element of one token row changed another row")
        want = mc.split_row_reference(c, inp, r0)
        row = got[r0].astype(np.float64)
        for name, kind in (("NaN", np.isnan), ("+inf", np.isposinf), ("-inf", np.isneginf)):
            assert np.array_equal(kind(row), kind(want)), (c["id"], name, "pattern of the row differs from the plane reference's")
        fin = np.isfinite(want)
        assert not fin.any() or np.abs(row[fin] - want[fin]).max() <= mc.TOL_PLANES * mc.split_reference(c, inp0, slice(r0, r0 + 1))["mag"][0][fin].max()
        print(f"matmul-sweep {c['id']}: row {r0} holds {int(np.isnan(want).sum())} NaN, {int(np.isposinf(want).sum())} +inf, {int(np.isneginf(want).sum())} -inf "
              f"as the plane reference; every other row bit-identical to the launch without the element")
        inp, got = inp0, got0
    ref, known = mc.split_reference(c, inp), mc.split_known(c, inp)
    mask = None if known is None else np.isfinite(known)
    assert np.isfinite(got[mask if mask is not None else slice(None)]).all(), (c["id"], "not finite: an element was left unwritten, or a NaN / inf was computed")
    split_limits(c, got, ref, mask)
    if known is not None:
        off = ~(got.view(np.uint32) == known.view(np.uint32))
        if c["known"] == "select":
            top = inp["x"].view(np.uint32) == mc.FLT_MAX_BITS
            if top.any() and c["passes"] == 3:          # named: FLT_MAX under c = +1 is +inf by the definition
                _, col = np.nonzero(inp["w"])
                unit = inp["w"][np.arange(c["n"]), col] == 1.0
                hit = top[:, col] & unit[None, :]
                assert not hit.any() or np.isposinf(known[hit]).all()
        assert not off.any(), (c["id"], f"known answer ({c['known']}): not bit for bit in {int(off.sum())} elements, first at {tuple(np.argwhere(off)[0])}")
    if c["known"] == "periodic":    # rows r mod 8, columns j mod 16: one value per residue pair
        assert _same_bits(got, np.tile(got[:8, :16], (c["m"] // 8, c["n"] // 16))), (c["id"], "rows / columns of one residue differ")
    if c["regime"] == "edges" and not c["known"]:       # zero rows of x: exactly the bias, or +0
        for r0 in mc.edge_blocks(c["m"]):
            r = r0 + mc.EDGE_ROWS["zero"]
            want = inp["bias"] if c["bias"] else np.zeros(c["n"], np.float32)
            assert not inp["x"][r].any() and _same_bits(got[r], want.astype(np.float32)), (c["id"], "zero row of x: not exactly the bias / +0", r)
        assert ref["mag"].max() < mc.FLT_MAX and np.abs(ref["true"]).max() < mc.FLT_MAX
    TIMES[c["id"]] = time.perf_counter() - t0
    return got


# ---------------------------------------------------------------------------------------------------
# zigma_linear_wgrad
# ---------------------------------------------------------------------------------------------------
def wgrad_windows(c, inp):
    f = mc.wgrad_fields(c)
    sh, dt = f["shape"], DT[c["kind"]]
    return dict(dy=Win(sh["dy"], dt, inp["dy"]), x=Win(sh["x"], dt, inp["x"]), out=Win(sh["out"], torch.float32 if c["out32"] else dt),
                ws=Win((1, f["workspace_bytes"] // 4, LEAD_WS, f["workspace_bytes"] // 4 + WS_TAIL, 0), torch.float32))


def wgrad_params(c, w, out=None):
    from zigma_amd import _lib
    out = (out or w["out"]).t
    f = mc.wgrad_fields(c)
    P = _lib.LinearWgradParams()
    P.m, P.n, P.k, P.dtype, P.out_dtype, P.slabs, P.flags = c["m"], c["n"], c["k"], mc.DTYPE_ID[c["kind"]], mc.DTYPE_ID["f32" if c["out32"] else c["kind"]], c["slabs"], 0
    P.dy_row_stride, P.x_row_stride, P.out_row_stride = w["dy"].t.stride(0), w["x"].t.stride(0), out.stride(0)
    assert P.out_row_stride > c["k"] and P.dy_row_stride > c["n"] and P.x_row_stride > c["k"]
    P.dy, P.x, P.out = w["dy"].t.data_ptr(), w["x"].t.data_ptr(), out.data_ptr()
    P.workspace, P.workspace_bytes = w["ws"].buf.data_ptr() + 4 * LEAD_WS, f["workspace_bytes"]
    return P


def wgrad_run(c, w):
    for win in w.values():
        win.snapshot()
    P = wgrad_params(c, w)
    _call(c, "zigma_linear_wgrad", P)
    clean(c, w, ("out", "ws"))      # (ws: the window is workspace_bytes long; its lead and the 64 elements behind it must still be NaN)
    first = _host(w["out"].t)
    _call(c, "zigma_linear_wgrad", P)
    assert _same_bits(first, _host(w["out"].t)), (c["id"], "the second launch differs from the first")
    return first


def wgrad_reference(c, inp, w):
    if not c.get("production"):
        return mc.wgrad_reference(c, inp)
    dy, x = w["dy"].t.double(), w["x"].t.double()                  # (13 GFLOP in float64: formed where the operands are, compared on the host)
    return dict(out=_host(dy.T @ x), mag=_host(dy.abs().T @ x.abs()))


def check_wgrad_case(c):
    t0 = time.perf_counter()
    inp = mc.wgrad_inputs(c)
    w = wgrad_windows(c, inp)
    got = wgrad_run(c, w)
    assert np.isfinite(got.astype(np.float32)).all(), (c["id"], "not finite: an element was left unwritten, a NaN partial or a NaN row / column was read")
    ref = wgrad_reference(c, inp, w)
    g64 = got.astype(np.float32).astype(np.float64)
    need = mc.wgrad_need(c, g64, ref)
    bound, form = mc.wgrad_bound(c), f"{c['kernel_name']} {c['kind']}->{'f32' if c['out32'] else c['kind']}"
    if "cancel" in need:
        print(f"matmul-sweep {c['id']}: out [{form}] element-wise {need['cancel'] * bound:.3e} of sum|dy||x| (limit {bound:.2e})")
    else:
        print(f"matmul-sweep {c['id']}: out [{form}] norm-wise {need['norm'] * bound:.3e} (bound {bound:.2e}), row-wise ratio {need['rows'] * mc.ROW_GUARD:.3g}, "
              f"element-wise ratio {need['elements'] * mc.ROW_GUARD:.3g}")
    assert all(v <= 1.0 for v in need.values()), (c["id"], need)
    known = mc.wgrad_known(c, inp)
    if known is not None:           # token selection / sparse integers: the float64 value is the answer, and an unselected row is +0
        want = _host(torch.from_numpy(known).float().to(torch.float32 if c["out32"] else DT[c["kind"]]))
        assert _same_bits(got, want), (c["id"], f"known answer ({c['known']}): not bit for bit", int((g64 != known).sum()))
    if c["known"] == "ints" and mc.wgrad_fields(c)["S"] > 1:       # equal across all slab counts: each equals the one-slab launch
        one = Win(mc.wgrad_fields(c)["shape"]["out"], w["out"].buf.dtype)
        one.snapshot()
        c1 = dict(c, slabs=1, kernel_name=mc.wgrad_fields(dict(c, slabs=1))["kernel"])
        _call(c1, "zigma_linear_wgrad", wgrad_params(c1, w, out=one))
        assert one.unchanged(but_window=True) and _same_bits(_host(one.t), got), (c["id"], "differs from the one-slab launch")
    if c["regime"] == "edges" and not c["known"]:                  # zero columns of dy: output rows of exactly +0
        rows = mc.wgrad_edges(c["m"], c["n"])["zero_cols"]
        assert not got[rows].view(np.uint8).any(), (c["id"], "zero column of dy: the output row is not +0")
    TIMES[c["id"]] = time.perf_counter() - t0
    return got


@pytest.mark.parametrize("c", SPLIT, ids=_ids(SPLIT))
def test_split_sweep(c):
    check_split_case(c)


@pytest.mark.parametrize("c", WGRAD, ids=_ids(WGRAD))
def test_wgrad_sweep(c):
    check_wgrad_case(c)


@pytest.mark.parametrize("c", PRODUCTION, ids=_ids(PRODUCTION))
def test_production_shape(c):
    (check_split_case if c["kernel"] == "split" else check_wgrad_case)(c)


def test_zz_summary():
    """(runs last in the file) the case counts, the sweep's wall time and the slowest case, for profiles/matmul_sweep_gpu_tests.txt"""
    every = SPLIT + WGRAD + PRODUCTION
    print(f"matmul-sweep cases: split {len(SPLIT)}, wgrad {len(WGRAD)}, production {len(PRODUCTION)}")
    if TIMES:
        slow = max(TIMES, key=TIMES.get)
        print(f"matmul-sweep wall time of {len(TIMES)} cases: {sum(TIMES.values()):.1f} s; slowest {slow}: {TIMES[slow]:.2f} s")
    assert len({c["id"] for c in every}) == len(every)

"""Sweep of the dense projection kernels — linear_tn_kernel, linear4w_kernel, linear_ws_kernel, linear_sm_kernel behind zigma_linear_fwd and
norm_linear_kernel behind zigma_norm_linear_fwd — against float64 on EVERY output row, over the case tables of tests/linear_cases.py (coverage, the
plans, the references' soundness and the rounding model: tests/test_linear_cases_cpu.py, which also runs every function of this file on the CPU
against the float64 stand-ins of tests/kernel_standins.py).

Every case fills the parameter block itself and goes through _lib.call.  x, w, bias, residual and out are windows of NaN-filled buffers with their
own row pitch and lead and a NaN row below; gate, shift and scale are column windows of one (batch, 6 cols) buffer that is NaN everywhere else.
Asserted per case: the kernel string the library reports; every byte around every window and every operand bit for bit what it was before the call
(integer views); finite outputs although they were NaN beforehand; the norm-wise bound and, for every output row, the row-wise limit; a second
launch bit-identical; the known answers and the exactly known rows bit for bit; the gated epilogue's one defined value given the kernel's own
plain output; whole-output equality with the 8-wave kernel where the header promises it (ws, sm, 4w EPI 0 / 1).  The float64 reference is the
numpy one of the case table; outputs above 2^21 elements are compared against its torch restatement (kernel_standins.torch_linear /
torch_norm_linear, pinned to the numpy reference below 1e-12 by the CPU test) formed on the device in row chunks, so that nothing large crosses
to the host.  Each case prints one `linear-sweep` line for DESIGN.md's parity table.
"""
import time

import numpy as np
import pytest
import torch

import kernel_standins as ks
import linear_cases as lc

pytestmark = pytest.mark.gpu
DEV = "cuda"            # (the CPU test file points this at "cpu" and serves _lib.call with the stand-ins)
DT = {"bf16": torch.bfloat16, "f16": torch.float16}
NAN = float("nan")
LIN, NL, PRODUCTION = lc.linear_cases(), lc.norm_linear_cases(), lc.production_cases()
HOST_LIMIT = 1 << 21    # output elements up to which the numpy reference is used
CHUNK = 1 << 22         # output elements per row chunk of a comparison
TIMES = {}              # id -> seconds (test_zz_summary prints the counts, the wall time and the slowest case)


def _ids(cases):
    return [c["id"] for c in cases]


class Win:
    """(rows, cols) window of a NaN-filled (rows + 1, pitch) buffer, `lead` elements into every row; cols: a column range inside the row instead"""
    def __init__(self, shape, dtype, fill=None):
        rows, cols, lead, pitch = shape
        self.buf = torch.full((rows + 1, pitch), NAN, dtype=dtype, device=DEV)
        self.index = (slice(0, rows), slice(lead, lead + cols))
        self.t = self.buf[self.index]
        if fill is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(fill)).to(DEV).to(dtype))
        self.before = None

    def snapshot(self):
        self.before = self.buf.view(torch.int16).clone()

    def unchanged(self, but_window=False):
        """every byte of the buffer (but_window: outside the window) has the bit pattern of the snapshot"""
        diff = self.before != self.buf.view(torch.int16)
        if but_window:
            diff[self.index] = False
        return not bool(diff.any())


def windows(c, inp):
    """the case's operands as windows; `mod`: the (batch, 6 cols) buffer whose column windows are gate, or shift and scale"""
    f, dt = lc.fields(c), DT[c["kind"]]
    sh = f["shape"]
    w = dict(x=Win(sh["x"], dt, inp["x"]), w=Win(sh["w"], dt, inp["w"]), out=Win(sh["out"], dt))
    if c["kernel"] == "nl":
        k, mod = c["k"], np.full((sh["mod"][0], 6 * c["k"]), np.nan, np.float32)
        mod[:, lc.SHIFT_WINDOW * k:(lc.SHIFT_WINDOW + 1) * k], mod[:, lc.SCALE_WINDOW * k:(lc.SCALE_WINDOW + 1) * k] = inp["shift"], inp["scale"]
        w["mod"] = Win(sh["mod"], dt, mod)
        return w
    if c["bias"]:
        w["bias"] = Win(sh["bias"], dt, inp["bias"][None])
    if c["rpb"]:
        n, mod = c["n"], np.full((sh["mod"][0], 6 * c["n"]), np.nan, np.float32)
        mod[:, lc.GATE_WINDOW * n:(lc.GATE_WINDOW + 1) * n] = inp["gate"]
        w["residual"], w["mod"] = Win(sh["residual"], dt, inp["res"]), Win(sh["mod"], dt, mod)
    return w


def mod_window(w, index, cols):
    return w["mod"].t[:, index * cols:(index + 1) * cols]


def params(c, w, out=None, flags=None, plain=False):
    """the parameter block of the case on the windows w; out: another output window; flags: other flags; plain: without the gated residual"""
    from zigma_amd import _lib
    f, out = lc.fields(c), (out or w["out"]).t
    if c["kernel"] == "nl":
        P = _lib.NormLinearParams()
        for key in ("m", "n", "k", "dtype", "flags", "rows_per_batch", "eps", "mod_batch_stride"):
            setattr(P, key, f[key])
        P.x_row_stride, P.w_row_stride, P.out_row_stride = w["x"].t.stride(0), w["w"].t.stride(0), out.stride(0)
        P.x, P.w, P.out = w["x"].t.data_ptr(), w["w"].t.data_ptr(), out.data_ptr()
        P.shift, P.scale = mod_window(w, lc.SHIFT_WINDOW, c["k"]).data_ptr(), mod_window(w, lc.SCALE_WINDOW, c["k"]).data_ptr()
        assert (P.x_row_stride, P.w_row_stride, P.out_row_stride) == (f["x_row_stride"], f["w_row_stride"], f["out_row_stride"])
        assert f["mod_batch_stride"] in (0, w["mod"].t.stride(0))
        return P
    P = _lib.LinearParams()
    P.m, P.n, P.k, P.dtype, P.flags, P.silu_from_col = f["m"], f["n"], f["k"], f["dtype"], f["flags"] if flags is None else flags, f["silu_from_col"]
    P.x_row_stride, P.w_row_stride, P.out_row_stride = w["x"].t.stride(0), w["w"].t.stride(0), out.stride(0)
    P.x, P.w, P.out = w["x"].t.data_ptr(), w["w"].t.data_ptr(), out.data_ptr()
    assert (P.x_row_stride, P.w_row_stride, P.out_row_stride) == (f["x_row_stride"], f["w_row_stride"], f["out_row_stride"])
    if c["bias"]:
        P.bias = w["bias"].t.data_ptr()
    if c["rpb"] and not plain:
        P.residual, P.gate = w["residual"].t.data_ptr(), mod_window(w, lc.GATE_WINDOW, c["n"]).data_ptr()
        P.res_row_stride, P.gate_batch_stride, P.rows_per_batch = w["residual"].t.stride(0), w["mod"].t.stride(0), c["rpb"]
        assert (P.res_row_stride, P.gate_batch_stride) == (f["res_row_stride"], f["gate_batch_stride"])
    for key, off in f["off"].items():           # the alignment the case table planned with
        ptr = getattr(P, key)
        assert (not ptr) == (off is None or (plain and key in ("residual", "gate"))) and (not ptr or ptr % 16 == off % 16), (c["id"], key)
    return P


def _call(c, P, kernel=None):
    from zigma_amd import _lib
    name = "zigma_norm_linear_fwd" if c["kernel"] == "nl" else "zigma_linear_fwd"
    _lib.call(name, P, torch.device(DEV))
    if kernel is not None:
        assert _lib.last_kernel() == kernel, (c["id"], _lib.last_kernel(), kernel)
    return _lib.last_kernel()


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(DEV)


def reference_rows(c, inp, w):
    """-> f(a, b) -> (ref, terms) of the output rows [a, b) as float64 tensors on the device: the numpy reference (evaluated once, whole) for small
    outputs, its torch restatement on the operands in the windows for large ones"""
    if c["m"] * c["n"] <= HOST_LIMIT:
        r = lc.reference(c, inp)
        ref, terms = _t(r["out"]), None if r["terms"] is None or c["kernel"] == "nl" else (_t(r["terms"][0]), _t(r["terms"][1]))
        return lambda a, b: (ref[a:b], None if terms is None else (terms[0][a:b], terms[1][a:b]))
    d, dt = (lambda t: t.double()), DT[c["kind"]]
    if c["kernel"] == "nl":
        def rows(a, b):
            pick = lambda t: t.double()[torch.arange(a, b, device=DEV) // (c["m"] if c["bcast"] else c["rpb"])]
            return ks.torch_norm_linear(d(w["x"].t[a:b]), d(w["w"].t), pick(mod_window(w, lc.SHIFT_WINDOW, c["k"])), pick(mod_window(w, lc.SCALE_WINDOW, c["k"])),
                                        lc.NL_EPS, dt)["out"], None
        return rows

    def rows(a, b):
        res = gate = None
        if c["rpb"]:
            res, gate = d(w["residual"].t[a:b]), d(mod_window(w, lc.GATE_WINDOW, c["n"]))[torch.arange(a, b, device=DEV) // c["rpb"]]
        return ks.torch_linear(d(w["x"].t[a:b]), d(w["w"].t), d(w["bias"].t[0]) if c["bias"] else None, c["silu"], res, gate, dt, c["family"] != "4w")
    return rows


def compare(c, key, got, rows, bound):
    """norm-wise against the unrounded reference and row-wise for EVERY row (fwd_fuzz_cases.norm_err / row_ratio, on the device, in row chunks)"""
    m, n = got.shape
    step, num, den, d_rows, r_rows = max(CHUNK // n, 1), 0.0, 0.0, [], []
    for a in range(0, m, step):
        b = min(a + step, m)
        ref, terms = rows(a, b)
        g = got[a:b].double()
        assert ref.shape == g.shape, (c["id"], key, ref.shape, g.shape)
        assert bool(torch.isfinite(g).all()), (c["id"], key, "not finite: an element was left unwritten, or a NaN / inf was computed")
        diff = g - ref
        num, den = num + float((diff * diff).sum()), den + float((ref * ref).sum())
        d_rows.append(diff.norm(dim=1))
        r_rows.append(ref.norm(dim=1) if terms is None else terms[0].norm(dim=1) + terms[1].norm(dim=1))
    d, rn = torch.cat(d_rows), torch.cat(r_rows)
    e = (num / max(den, 1e-300)) ** 0.5 if den > 0 else num ** 0.5
    floor = torch.sqrt((rn * rn).mean()).clamp_min(1e-300)
    r = float((d / (bound * torch.maximum(rn, floor))).max())
    print(f"linear-sweep {c['id']}: {key} [{c['leaf']}] norm-wise {e:.3e} (bound {bound:.2e}), row-wise ratio {r:.3g}")
    assert e <= bound, (c["id"], key, e, bound)
    assert r <= lc.ROW_GUARD, (c["id"], key, r)


def clean(c, w, written=("out",)):
    for name, win in w.items():
        assert win.unchanged(but_window=name in written), (c["id"], name, "bytes outside the output window were written" if name in written else "an operand changed")


def run(c, inp):
    """the windows after the case's call, checked for the kernel string, for stray writes and for a bit-identical second launch"""
    w = windows(c, inp)
    for win in w.values():
        win.snapshot()
    P = params(c, w)
    _call(c, P, c["kernel_name"])
    clean(c, w)
    first = w["out"].t.clone()
    _call(c, P, c["kernel_name"])
    assert torch.equal(first, w["out"].t), (c["id"], "the second launch differs from the first")
    return w


def second_output(c, w, **how):
    """the case on the same operands into a second NaN-filled output window -> (window, kernel string); how: flags / plain of params()"""
    out = Win(lc.fields(c)["shape"]["out"], DT[c["kind"]])
    out.snapshot()
    kernel = _call(c, params(c, w, out=out, **how))
    assert out.unchanged(but_window=True), (c["id"], how, "bytes outside the output window were written")
    return out, kernel


def check_linear_case(c):
    t0 = time.perf_counter()
    inp = lc.inputs(c)
    w = run(c, inp)
    got, dt, n = w["out"].t, DT[c["kind"]], c["n"]
    rows = reference_rows(c, inp, w)
    compare(c, "out", got, rows, lc.IO_BOUND[c["kind"]])
    plain = slice(0, c["silu"] if c["bias"] or c["known"] else n)            # columns whose exactly known values stay exact: silu(0) = 0
    if c["known"]:           # selection weights / sparse integers: the float64 value is the answer
        for a in range(0, c["m"], max(CHUNK // n, 1)):
            b = min(a + max(CHUNK // n, 1), c["m"])
            assert torch.equal(got[a:b, plain], rows(a, b)[0].float().to(dt)[:, plain]), (c["id"], "known answer: not bit for bit", a)
    elif c["regime"] == "edges":          # zero rows of x: exactly bias, residual + gate * bias, or 0
        for r in lc.edge_rows(c["m"])["zero"]:
            assert not bool(w["x"].t[r].any())
            assert torch.equal(got[r:r + 1, plain], rows(r, r + 1)[0].float().to(dt)[:, plain]), (c["id"], "zero row of x: not exact", r)
    if c["rpb"] and c["family"] in ("tn", "sm"):      # the gated epilogue's ONE value given the kernel's own plain output
        p16, kernel = second_output(c, w, plain=True, flags=c["flags"] | (lc.PIN | lc.NARROW if c["family"] == "tn" else 0))
        assert kernel == c["kernel_name"], (c["id"], kernel)
        gate = mod_window(w, lc.GATE_WINDOW, n).double().repeat_interleave(c["rpb"], 0)
        want = torch.addcmul(w["residual"].t.double(), gate, p16.t.double()).float().to(dt)
        off = float((want != got).double().mean())
        print(f"linear-sweep {c['id']}: gated epilogue off r16(fl32(fma(gate, p16, residual))) in {off:.2e} of the elements")
        assert off == 0.0, (c["id"], "the gated epilogue is not the defined value", off)
    if c["family"] in ("ws", "sm") or c["leaf"] in ("4w<0>", "4w<1>"):            # "same result bit for bit" as the 8-wave kernel
        other, kernel = second_output(c, w, flags=lc.PIN)
        assert kernel.startswith("linear_tn_"), (c["id"], kernel)
        assert torch.equal(other.t, got), (c["id"], "differs from the 8-wave kernel", float((other.t != got).double().mean()))
    TIMES[c["id"]] = time.perf_counter() - t0
    return w


def check_norm_linear_case(c):
    t0 = time.perf_counter()
    inp = lc.inputs(c)
    w = run(c, inp)
    got, kind = w["out"].t, c["kind"]
    compare(c, "out", got, reference_rows(c, inp, w), lc.IO_BOUND[kind])
    if c["known"]:           # selection weights: out[i, j] = xa[i, start + j], the hidden intermediate
        from zigma_amd import _lib
        k, n, start = c["k"], c["n"], c["part"] * (c["k"] - c["n"])
        ref = lc.reference(c, inp)
        seen, want = got.double().cpu().numpy(), ref["xa"][:, start:start + n].astype(np.float64)
        assert np.array_equal(want, ref["out"]), "the selection shows xa exactly"
        off = seen != want
        xa_seen = np.array(ref["xa"], np.float64)
        xa_seen[:, start:start + n] = seen
        allow = lc.xa_allowance(ref, xa_seen, kind)[:, start:start + n]
        worst = float((np.abs(seen - want) / allow).max())
        assert worst <= 1.0, (c["id"], "xa more than one ulp off at one of its two rounding points", worst)
        # ... and zigma_add_norm_fwd's y_mod on the same operands
        ym = Win((c["m"], k, lc.LEAD, lc.LEAD + k + 8), DT[kind])
        P = _lib.NormParams()
        P.rows, P.cols, P.rows_per_batch, P.is_rms, P.eps, P.flags = c["m"], k, c["rpb"], 0, lc.NL_EPS, 0
        P.x_dtype = P.res_dtype = P.w_dtype = P.mod_dtype = lc.DTYPE_ID[kind]
        P.x, P.x_row_stride, P.y_mod, P.y_mod_row_stride = w["x"].t.data_ptr(), w["x"].t.stride(0), ym.t.data_ptr(), ym.t.stride(0)
        P.shift, P.scale = mod_window(w, lc.SHIFT_WINDOW, k).data_ptr(), mod_window(w, lc.SCALE_WINDOW, k).data_ptr()
        P.mod_batch_stride = w["mod"].t.stride(0)
        _lib.call("zigma_add_norm_fwd", P, torch.device(DEV))
        same = float((ym.t[:, start:start + n] == got).double().mean())
        print(f"linear-sweep {c['id']}: xa off the correctly rounded y_mod in {off.mean():.4f} of its elements (limit {lc.DELTA_FLIPS}), worst {worst:.2f} of "
              f"one ulp at each rounding point, bit-equal with add_norm's y_mod in {same:.4f}")
        assert off.mean() <= lc.DELTA_FLIPS, (c["id"], off.mean())
    TIMES[c["id"]] = time.perf_counter() - t0
    return w


@pytest.mark.parametrize("c", LIN, ids=_ids(LIN))
def test_linear_sweep(c):
    check_linear_case(c)


@pytest.mark.parametrize("c", NL, ids=_ids(NL))
def test_norm_linear_sweep(c):
    check_norm_linear_case(c)


@pytest.mark.parametrize("c", PRODUCTION, ids=_ids(PRODUCTION))
def test_production_shape(c):
    (check_norm_linear_case if c["kernel"] == "nl" else check_linear_case)(c)


def test_zz_summary():
    """(runs last in the file) the case counts per family, the sweep's wall time and the slowest case, for profiles/linear_sweep_gpu_tests.txt"""
    every = LIN + NL + PRODUCTION
    print(f"linear-sweep cases per family: {lc.counts(LIN + NL)}, production {len(PRODUCTION)}")
    if TIMES:
        slow = max(TIMES, key=TIMES.get)
        print(f"linear-sweep wall time of {len(TIMES)} cases: {sum(TIMES.values()):.1f} s; slowest {slow}: {TIMES[slow]:.2f} s")
    assert len({c["id"] for c in every}) == len(every)

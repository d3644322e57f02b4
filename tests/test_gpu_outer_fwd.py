"""Sweep of add-norm forward and the operators around the blocks — zigma_add_norm_fwd, zigma_patch_embed_fwd, zigma_timestep_embed_fwd,
zigma_skinny_linear_fwd, zigma_final_layer_fwd — against float64 row by row, over the case tables of tests/outer_fwd_cases.py (coverage, the
references' soundness and the rounding model: tests/test_outer_fwd_cases_cpu.py, which also runs every function of this file on the CPU against
the float64 stand-ins of tests/kernel_standins.py).

Every case fills the entry point's parameter block itself and goes through _lib.call: every tensor the kernel reads or writes is a window of a
NaN-filled buffer with a row pitch (the wrappers cannot express a pitch for the outputs).  Asserted per case: the kernel that served it; finite
outputs although they were NaN beforehand; NaN surroundings of every operand and output still NaN; the norm-wise bound and, for EVERY output
row, the row-wise limit; bit-for-bit equality where the result has one defined value (add_norm's x_out and residual_out, the known-answer
cases); element by element for the timestep features.  Each output prints one `outer-sweep` line for DESIGN.md's parity table.
"""
import numpy as np
import pytest
import torch

import outer_fwd_cases as oc

pytestmark = pytest.mark.gpu
DEV = "cuda"            # (the CPU test file points this at "cpu" and serves _lib.call with the stand-ins)
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
BF = torch.bfloat16
NAN = float("nan")
NORM, PATCH, TIMESTEP, SKINNY, FINAL = oc.norm_cases(), oc.patch_cases(), oc.timestep_cases(), oc.skinny_cases(), oc.final_cases()
PRODUCTION = oc.norm_production_cases() + oc.patch_production_cases() + oc.skinny_production_cases() + oc.final_production_cases()


def _ids(cases):
    return [c["id"] for c in cases]


def _np(t):
    return None if t is None else t.detach().double().cpu().numpy()


class Win:
    """a tensor that is the window `index` of a NaN-filled buffer of shape `shape`"""
    def __init__(self, shape, index, dtype, fill=None):
        self.buf = torch.full(tuple(shape), NAN, dtype=dtype, device=DEV)
        self.index = tuple(index)
        self.t = self.buf[self.index]
        if fill is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(fill)).to(DEV).to(dtype))

    def surroundings_nan(self):
        m = torch.isnan(self.buf)
        m[self.index] = True
        return bool(m.all())


def rows_win(rows, n, dtype, lead, tail, fill=None, extra_rows=0):
    """(rows, n) window, `lead` NaN elements in front of and `tail` behind every row, extra_rows NaN rows below"""
    return Win((rows + extra_rows, lead + n + tail), (slice(0, rows), slice(lead, lead + n)), dtype, fill)


def vec_win(n, dtype, lead, tail, fill=None):
    return Win((lead + n + tail,), (slice(lead, lead + n),), dtype, fill)


def _call(name, P, kernel):
    from zigma_amd import _lib
    _lib.call(name, P, torch.device(DEV))
    assert _lib.last_kernel() == kernel, (name, _lib.last_kernel(), kernel)


def _report(ident, key, got, ref, bound, terms=None):
    assert got.shape == ref.shape, (ident, key, got.shape, ref.shape)
    assert np.isfinite(got).all(), (ident, key, "not finite: an element was left unwritten, or a NaN / inf was computed")
    e = oc.norm_err(got, ref) if np.linalg.norm(ref) > 0 else float(np.linalg.norm(got))
    r = oc.row_ratio(got, ref, bound, terms)
    print(f"outer-sweep {ident}: {key} norm-wise {e:.3e} (bound {bound:.2e}), row-wise ratio {r:.3g}")
    assert e <= bound, (ident, key, e, bound)
    assert r <= oc.ROW_GUARD, (ident, key, r)


def _clean(ident, wins):
    for name, w in wins.items():
        assert w.surroundings_nan(), (ident, name, "the NaN surroundings were written")


# ---------------------------------------------------------------------------------------------------
# add_norm forward
# ---------------------------------------------------------------------------------------------------
def norm_run(c, inp):
    from zigma_amd import _lib
    rows, cols, u, lead = c["rows"], c["cols"], oc.norm_uses(c), oc.LEAD + c["align"]
    xdt, rdt, wdt = DT[c["xk"]], DT[c["rk"]], DT[c["wk"]]
    row = lambda dt, fill=None: rows_win(rows, cols, dt, lead, oc.TAIL, fill)
    w = dict(x=row(xdt, inp["x"]))
    P = _lib.NormParams()
    P.rows, P.cols, P.rows_per_batch, P.is_rms, P.eps, P.flags = rows, cols, c["rpb"], int(c["form"] == "rms"), oc.EPS, c["flags"]
    P.x_dtype, P.res_dtype, P.w_dtype, P.mod_dtype = _lib._DT[xdt], _lib._DT[rdt], _lib._DT[wdt], _lib._DT[xdt]

    def put(field, stride, win):
        setattr(P, field, win.t.data_ptr())
        if stride:
            setattr(P, stride, win.t.stride(0))
    put("x", "x_row_stride", w["x"])
    if u["branch"]:
        w["branch"] = row(xdt, inp["branch"])
        put("branch", "branch_row_stride", w["branch"])
    if u["x_out"]:
        w["x_out"] = row(xdt)
        put("x_out", "x_out_row_stride", w["x_out"])
    if u["res"]:
        w["residual"] = row(rdt, inp["residual"])
        put("residual", "res_row_stride", w["residual"])
    if u["res_out"]:
        w["residual_out"] = row(rdt)
        put("residual_out", "res_out_row_stride", w["residual_out"])
    if inp["weight"] is not None:
        w["weight"] = vec_win(cols, wdt, lead, oc.TAIL, inp["weight"])
        put("weight", None, w["weight"])
    if inp["bias"] is not None:
        w["bias"] = vec_win(cols, wdt, lead, oc.TAIL, inp["bias"])
        put("bias", None, w["bias"])
    if u["y_out"]:
        w["y_out"] = row(xdt)
        put("y_out", "y_row_stride", w["y_out"])
    if inp["mod"] is not None:          # shift | scale | gate: three windows of one (batch, 6 cols) buffer
        w["mod"] = rows_win(inp["mod"].shape[0], 6 * cols, xdt, lead, oc.TAIL, inp["mod"])
        win = lambda k: w["mod"].t[:, oc.MOD_WINDOWS[k] * cols:].data_ptr()
        P.mod_batch_stride = w["mod"].t.stride(0)
        if u["mod"]:
            w["y_mod"] = row(xdt)
            put("y_mod", "y_mod_row_stride", w["y_mod"])
            P.shift, P.scale = win(0), win(1)
        if u["branch"]:
            P.gate = win(2)
    _call("zigma_add_norm_fwd", P, c["kernel_name"])
    return w


def check_norm_case(c):
    inp = oc.norm_inputs(c)
    w = norm_run(c, inp)
    _clean(c["id"], w)
    ref = oc.norm_reference(c, inp)
    keys = [k for k in ("x_out", "residual_out", "y_out", "y_mod") if k in ref]
    assert keys == [k for k in ("x_out", "residual_out", "y_out", "y_mod") if k in w], (c["id"], keys)
    for key in keys:
        _report(c["id"], key, _np(w[key].t), ref[key], oc.IO_BOUND[oc.norm_out_kind(c, key)], terms=ref["_terms"] if key == "y_mod" else None)
    for key, want in oc.norm_exact(c, ref).items():
        assert np.array_equal(_np(w[key].t), want.astype(np.float64)), (c["id"], key, "not the one defined value")
    return w


@pytest.mark.parametrize("c", NORM, ids=_ids(NORM))
def test_add_norm_sweep(c):
    check_norm_case(c)


# ---------------------------------------------------------------------------------------------------
# patch_embed
# ---------------------------------------------------------------------------------------------------
def patch_run(c, inp):
    from zigma_amd import _lib
    B, C, p, E, L = c["B"], c["C"], c["p"], c["E"], c["L"]
    H, W = c["gh"] * p, c["gw"] * p
    w = dict(x=Win((B, C + 2, H + 1, W + 8), (slice(None), slice(1, C + 1), slice(0, H), slice(4, 4 + W)), BF, inp["x"]),
             weight=vec_win(E * c["K"], BF, 8, 8, inp["w"].reshape(-1)),
             out=Win((B, L + 1, 8 + E + 8), (slice(None), slice(0, L), slice(8, 8 + E)), BF))
    P = _lib.PatchEmbedParams()
    P.batch, P.in_chans, P.height, P.width, P.patch, P.embed_dim, P.dtype, P.flags = B, C, H, W, p, E, _lib.BF16, 0
    x, out = w["x"].t, w["out"].t
    P.x_batch_stride, P.x_chan_stride, P.x_row_stride = x.stride(0), x.stride(1), x.stride(2)
    P.out_batch_stride, P.out_row_stride = out.stride(0), out.stride(1)
    P.x, P.weight, P.out = x.data_ptr(), w["weight"].t.data_ptr(), out.data_ptr()
    if inp["bias"] is not None:
        w["bias"] = vec_win(E, BF, 8, 8, inp["bias"])
        P.bias = w["bias"].t.data_ptr()
    if inp["pos"] is not None:
        w["pos"] = rows_win(L, E, BF, 8, 8, inp["pos"]) if c["pos"] == "pitched" else Win((L, E), (slice(None),), BF, inp["pos"])
        P.pos, P.pos_row_stride = w["pos"].t.data_ptr(), w["pos"].t.stride(0)
    _call("zigma_patch_embed_fwd", P, "patch_embed")
    return w


def check_patch_case(c):
    inp = oc.patch_inputs(c)
    w = patch_run(c, inp)
    _clean(c["id"], w)
    ref, got = oc.patch_reference(c, inp)["out"], _np(w["out"].t)
    _report(c["id"], "out", got, ref, oc.IO_BOUND["bf16"])
    if c["known"]:
        assert np.array_equal(got, ref), (c["id"], "known answer: not bit for bit")


@pytest.mark.parametrize("c", PATCH, ids=_ids(PATCH))
def test_patch_embed_sweep(c):
    check_patch_case(c)


# ---------------------------------------------------------------------------------------------------
# timestep_embed
# ---------------------------------------------------------------------------------------------------
def timestep_run(c, inp):
    from zigma_amd import _lib
    B, dim = c["B"], c["dim"]
    w = dict(t=vec_win(B, BF, 3, 2, inp["t"]), freqs=vec_win(dim // 2, BF, 1, 4, inp["freqs"]),
             out=rows_win(B, dim, BF, 0, c["pitch"]) if c["pitch"] else Win((B, dim), (slice(None),), BF))
    P = _lib.TimestepEmbedParams()
    P.batch, P.dim, P.dtype, P.flags, P.out_row_stride = B, dim, _lib.BF16, 0, w["out"].t.stride(0)
    P.t, P.freqs, P.out = w["t"].t.data_ptr(), w["freqs"].t.data_ptr(), w["out"].t.data_ptr()
    _call("zigma_timestep_embed_fwd", P, "timestep_embed")
    return w


def check_timestep_case(c):
    inp = oc.timestep_inputs(c)
    w = timestep_run(c, inp)
    _clean(c["id"], w)
    ref, got = oc.timestep_reference(c, inp)["out"], _np(w["out"].t)
    _report(c["id"], "out", got, ref, oc.IO_BOUND["bf16"])
    worst, flips = oc.timestep_worst(got, ref), oc.flipped_share(got, ref, "bf16")
    print(f"outer-sweep {c['id']}: out element-wise {worst:.3g} of a bf16 ulp, off the correctly rounded value in {flips:.4f} of its elements")
    assert worst <= 1.0, (c["id"], worst)
    assert flips <= oc.DELTA_FLIPS, (c["id"], flips)
    if c["dim"] % 2:
        assert not got[:, -1].any(), (c["id"], "the padding column is not 0")


@pytest.mark.parametrize("c", TIMESTEP, ids=_ids(TIMESTEP))
def test_timestep_embed_sweep(c):
    check_timestep_case(c)


# ---------------------------------------------------------------------------------------------------
# skinny_linear
# ---------------------------------------------------------------------------------------------------
def skinny_run(c, inp):
    from zigma_amd import _lib
    m, k, n, v = c["m"], c["k"], c["n"], c["views"]
    lead = lambda a: a if v else 0
    w = dict(x=rows_win(m, k, BF, lead(8), lead(8), inp["x"], extra_rows=lead(3)), w=rows_win(n, k, BF, lead(8), lead(16), inp["w"]),
             out=rows_win(m, n, BF, lead(4), lead(8), extra_rows=lead(2)))
    P = _lib.SkinnyParams()
    P.m, P.n, P.k, P.dtype, P.flags = m, n, k, _lib.BF16, int(c["silu"])
    P.x_row_stride, P.w_row_stride, P.out_row_stride = w["x"].t.stride(0), w["w"].t.stride(0), w["out"].t.stride(0)
    P.x, P.w, P.out = w["x"].t.data_ptr(), w["w"].t.data_ptr(), w["out"].t.data_ptr()
    if inp["bias"] is not None:
        w["bias"] = vec_win(n, BF, lead(4), lead(3), inp["bias"])
        P.bias = w["bias"].t.data_ptr()
    _call("zigma_skinny_linear_fwd", P, "skinny_linear_mfma")
    return w


def check_skinny_case(c):
    inp = oc.skinny_inputs(c)
    w = skinny_run(c, inp)
    _clean(c["id"], w)
    ref, got = oc.skinny_reference(c, inp)["out"], _np(w["out"].t)
    _report(c["id"], "out", got, ref, oc.IO_BOUND["bf16"])
    if c["known"]:
        assert np.array_equal(got, ref), (c["id"], "known answer: not bit for bit")


@pytest.mark.parametrize("c", SKINNY, ids=_ids(SKINNY))
def test_skinny_linear_sweep(c):
    check_skinny_case(c)


# ---------------------------------------------------------------------------------------------------
# final_layer
# ---------------------------------------------------------------------------------------------------
def final_run(c, inp):
    from zigma_amd import _lib
    rows, cols, n_out = c["rows"], c["cols"], c["n_out"]
    w = dict(x=rows_win(rows, cols, BF, 8, 8, inp["x"], extra_rows=1), weight=vec_win(n_out * cols, BF, 8, 8, inp["w"].reshape(-1)),
             out=rows_win(rows, n_out, BF, 2, 3, extra_rows=1))
    P = _lib.FinalLayerParams()
    P.rows, P.cols, P.n_out, P.dtype, P.flags, P.eps = rows, cols, n_out, _lib.BF16, 0, oc.FL_EPS
    P.x_row_stride, P.out_row_stride = w["x"].t.stride(0), w["out"].t.stride(0)
    P.x, P.weight, P.out = w["x"].t.data_ptr(), w["weight"].t.data_ptr(), w["out"].t.data_ptr()
    if inp["bias"] is not None:
        w["bias"] = vec_win(n_out, BF, 3, 2, inp["bias"])
        P.bias = w["bias"].t.data_ptr()
    _call("zigma_final_layer_fwd", P, "final_layer")
    return w


def check_final_case(c):
    inp = oc.final_inputs(c)
    w = final_run(c, inp)
    _clean(c["id"], w)
    _report(c["id"], "out", _np(w["out"].t), oc.final_reference(c, inp)["out"], oc.IO_BOUND["bf16"])


@pytest.mark.parametrize("c", FINAL, ids=_ids(FINAL))
def test_final_layer_sweep(c):
    check_final_case(c)


# ---------------------------------------------------------------------------------------------------
# production shapes: the sweep's metric where the model runs
# ---------------------------------------------------------------------------------------------------
CHECKS = dict(norm=check_norm_case, patch=check_patch_case, timestep=check_timestep_case, skinny=check_skinny_case, final=check_final_case)


@pytest.mark.parametrize("c", PRODUCTION, ids=[f"{c['kernel']}-{c['id']}" for c in PRODUCTION])
def test_production_shape(c):
    CHECKS[c["kernel"]](c)


# ---------------------------------------------------------------------------------------------------
# refusals: no kernel runs
# ---------------------------------------------------------------------------------------------------
def _valid_call(entry):
    """a small valid parameter block of the entry point and the windows behind it"""
    from zigma_amd import _lib
    bf = lambda *s: torch.zeros(*s, dtype=BF, device=DEV)
    if entry == "zigma_patch_embed_fwd":
        P, t = _lib.PatchEmbedParams(), dict(x=bf(1, 4, 4, 4), w=bf(64, 4, 1, 1), out=bf(1, 16, 64))
        P.batch, P.in_chans, P.height, P.width, P.patch, P.embed_dim, P.dtype = 1, 4, 4, 4, 1, 64, _lib.BF16
        P.x_batch_stride, P.x_chan_stride, P.x_row_stride, P.out_batch_stride, P.out_row_stride = 64, 16, 4, 16 * 64, 64
        P.x, P.weight, P.out = t["x"].data_ptr(), t["w"].data_ptr(), t["out"].data_ptr()
    elif entry == "zigma_timestep_embed_fwd":
        P, t = _lib.TimestepEmbedParams(), dict(t=bf(2), f=bf(4), out=bf(2, 8))
        P.batch, P.dim, P.dtype, P.out_row_stride = 2, 8, _lib.BF16, 8
        P.t, P.freqs, P.out = t["t"].data_ptr(), t["f"].data_ptr(), t["out"].data_ptr()
    elif entry == "zigma_skinny_linear_fwd":
        P, t = _lib.SkinnyParams(), dict(x=bf(65, 1160), w=bf(32, 1160), b=bf(40), out=bf(65, 40))
        P.m, P.n, P.k, P.dtype = 2, 16, 128, _lib.BF16
        P.x_row_stride, P.w_row_stride, P.out_row_stride = 1160, 1160, 40
        P.x, P.w, P.bias, P.out = t["x"].data_ptr(), t["w"].data_ptr(), t["b"].data_ptr(), t["out"].data_ptr()
    elif entry == "zigma_final_layer_fwd":
        P, t = _lib.FinalLayerParams(), dict(x=bf(2, 2056), w=bf(17, 2056), out=bf(2, 17))
        P.rows, P.cols, P.n_out, P.dtype, P.eps, P.x_row_stride, P.out_row_stride = 2, 64, 3, _lib.BF16, 1e-6, 2056, 17
        P.x, P.weight, P.out = t["x"].data_ptr(), t["w"].data_ptr(), t["out"].data_ptr()
    else:
        P, t = _lib.NormParams(), dict(x=bf(4, 4104), br=bf(4, 4104), mod=bf(1, 3 * 4104), y=bf(4, 4104), ym=bf(4, 4104))
        P.rows, P.cols, P.rows_per_batch, P.is_rms, P.eps = 4, 64, 4, 1, 1e-5
        P.x_dtype = P.res_dtype = P.w_dtype = P.mod_dtype = _lib.BF16
        P.x_row_stride = P.branch_row_stride = P.y_row_stride = P.y_mod_row_stride = 4104
        P.mod_batch_stride = 3 * 4104
        P.x, P.y_out = t["x"].data_ptr(), t["y"].data_ptr()
    return P, t


def _break(entry, what, P, t):
    from zigma_amd import _lib
    if what in ("f16", "f32"):
        P.dtype = _lib.F16 if what == "f16" else _lib.F32
    elif what == "above-64KB":
        P.in_chans, P.embed_dim = 16, 1032          # 16 x 1032 x 4 bytes = 66 048
    elif what == "m65":
        P.m = 65
    elif what == "k1152":
        P.k = 1152
    elif what == "n24":
        P.n = 24
    elif what.endswith("-off-by-one"):
        field = {"x": "x", "w": "w", "out": "out", "bias": "bias"}[what.split("-")[0]]
        setattr(P, field, getattr(P, field) + 2)
    elif what == "n_out17":
        P.n_out = 17
    elif what == "cols2056":
        P.cols = 2056
    elif what == "cols4097":
        P.cols = 4097
    elif what == "gate-without-branch":
        P.gate = t["mod"].data_ptr()
    elif what == "shift-without-ymod":
        P.shift, P.scale = t["mod"].data_ptr(), t["mod"][:, 4104:].data_ptr()
    elif what == "mod-dtype":
        P.branch, P.gate, P.mod_dtype = t["br"].data_ptr(), t["mod"].data_ptr(), _lib.F16
    else:
        raise KeyError(what)


@pytest.mark.parametrize("entry,what,status", oc.REFUSALS, ids=[f"{e[6:-4]}-{w}" for e, w, _ in oc.REFUSALS])
def test_refusals(entry, what, status):
    from zigma_amd import _lib
    P, t = _valid_call(entry)
    _lib.call(entry, P, torch.device(DEV))          # the block is valid before it is broken
    _break(entry, what, P, t)
    outs = [v.clone() for v in t.values()]
    with pytest.raises(RuntimeError, match=rf"\(status {status}\)"):
        _lib.call(entry, P, torch.device(DEV))
    assert all(torch.equal(a, b) for a, b in zip(outs, t.values())), (entry, what, "a refused call wrote")

"""CPU checks of the backward sweep's case tables (tests/bwd_fuzz_cases.py): the tables cover every cell they are meant to cover; on exactly
these inputs the float64 oracle agrees with float64 torch autograd through a plain restatement of each operator (< 1e-12 norm-wise); and the
oracle's result ROUNDED to the case's I/O type stays below the case's norm-wise bound and below 1 x the bound row by row — the inputs leave the
reference alone inside every limit, so a failure of tests/test_gpu_bwd_fuzz.py is the kernel's."""
import numpy as np
import pytest
import torch

import bwd_fuzz_cases as bc
from conftest import rel_err

SCAN, CONV, NORM = bc.scan_cases(), bc.conv_cases(), bc.norm_cases()
CPU_LONG = 300          # the two long scan cases are checked at this length here


# ---------------------------------------------------------------------------------------------------
# coverage
# ---------------------------------------------------------------------------------------------------
def test_scan_table_covers_its_cells():
    assert 50 <= len(SCAN) <= 75 and len({c["id"] for c in SCAN}) == len(SCAN)
    assert {(c["kind"], c["N"]) for c in SCAN} == {(k, n) for k in bc.KINDS for n in (16, 8)}
    for k in bc.KINDS:
        mine = [c for c in SCAN if c["kind"] == k]
        for opt in ("z", "D", "bias", "softplus"):
            assert {c[opt] for c in mine} == {True, False}, (k, opt)
        assert any(c["tables"] and c["z"] for c in mine), k
        assert any(c["dbc_slices"] for c in mine) and any(not c["dbc_slices"] for c in mine), k
        assert any(c["dz_half"] for c in mine) and any(c["z"] and not c["dz_half"] for c in mine), k
        assert any(c["bc_slices"] for c in mine) and any(not c["bc_slices"] for c in mine), k
        assert any(c["pad"] for c in mine) and any(not c["pad"] for c in mine), k
        assert {c["ckpt"] for c in mine} == {"fwd", "own"}, k
        assert any(c["twice"] for c in mine), k
    assert {c["L"] for c in SCAN} >= set(bc.SCAN_L) | set(bc.SCAN_LONG)
    for L in bc.SCAN_LONG:
        assert any(c["L"] == L and c["B"] == 1 and c["dim"] == 64 and c["ckpt"] == "fwd" and c["carries"] for c in SCAN), L
    assert {c["dim"] for c in SCAN} == {64, 128, 192} and {c["B"] for c in SCAN} == {1, 2, 3}
    assert {(c["reset"], c["tables"]) for c in SCAN if c["reset"]} == {(r, t) for r in (16, 32) for t in (False, True)}
    for c in SCAN:
        assert c["z"] or not (c["tables"] or c["dz_half"] or c["ckpt"] == "fwd"), c["id"]       # these need the gate
        if c["tables"]:
            inp = bc.scan_inputs(c, min(c["L"], CPU_LONG))
            for t in (inp["zi"], inp["oi"]):
                assert sorted(t.tolist()) == list(range(len(t)))
            assert c["L"] == 1 or not np.array_equal(inp["zi"], inp["oi"]), c["id"]


def test_conv_table_covers_its_cells():
    assert 45 <= len(CONV) <= 75 and len({c["id"] for c in CONV}) == len(CONV)
    assert {(c["kind"], c["W"], c["silu"]) for c in CONV} == {(k, w, s) for k in bc.KINDS for w in (2, 3, 4) for s in (False, True)}
    for k in ("bf16", "f16"):       # the fp32-weight twins of every 16-bit instantiation, and the same-type ones
        for wk in (k, "f32"):
            assert {(c["W"], c["silu"]) for c in CONV if c["kind"] == k and c["wkind"] == wk} == {(w, s) for w in (2, 3, 4) for s in (False, True)}
    assert all(c["wkind"] == "f32" for c in CONV if c["kind"] == "f32")
    for k in bc.KINDS:
        mine = [c for c in CONV if c["kind"] == k]
        for opt in ("bias", "table"):
            assert {c[opt] for c in mine} == {True, False}, (k, opt)
        assert any(c["x_pad"] for c in mine) and any(c["dx_pad"] for c in mine) and any(not c["dx_pad"] for c in mine), k
        assert any(c["reset"] == 16 and c["table"] for c in mine), k
        assert any(c["twice"] for c in mine), k
    assert {c["dim"] for c in CONV} >= set(bc.CONV_DIM) and {c["L"] for c in CONV} >= set(bc.CONV_L)
    assert any(c["L"] < c["W"] for c in CONV)
    for c in CONV:
        if c["reset"]:
            perm = bc.conv_inputs(c)["perm"]
            assert sorted(perm.tolist()) == list(range(c["L"])) and (perm // 16 == np.arange(c["L"]) // 16).all()
            assert not np.array_equal(perm, np.arange(c["L"]))


def test_norm_table_covers_its_cells():
    assert 50 <= len(NORM) <= 75 and len({c["id"] for c in NORM}) == len(NORM)
    ok = [c for c in NORM if not c["error"]]
    assert {c["branch"] for c in ok} == set(bc.NORM_BRANCHES)
    for br in bc.NORM_BRANCHES:
        assert {c["rms"] for c in ok if c["branch"] == br} == {True, False}, br
    assert len(bc.NORM_DTYPES) == 9 and {(c["xk"], c["rk"], c["wk"]) for c in ok if c["wk"]} == set(bc.NORM_DTYPES)
    for k in ("bf16", "f16"):
        for cols in (640, 768):
            assert any((c["xk"], c["rk"], c["wk"], c["cols"]) == (k, "f32", k, cols) and c["want_dx"] and c["want_dres"] for c in ok), (k, cols)
    assert {c["cols"] for c in ok} == set(bc.NORM_COLS) and {c["rows"] for c in ok} == set(bc.NORM_ROWS)
    errs = [c for c in NORM if c["error"]]
    assert [c["cols"] for c in errs] == [2049] and errs[0]["branch"] is None
    assert any(c["wk"] is None for c in ok)
    for opt in ("bias", "dres_out"):
        assert {c[opt] for c in ok} == {True, False}, opt
    assert {(c["want_dx"], c["want_dres"]) for c in ok} == set(bc.NORM_WANTS)
    forced = [c for c in ok if c["cols"] % 4 == 0 and (c["cols"] + c["pitch_pad"]) % 4 != 0]
    assert {c["branch"] for c in forced} == {(1, 12), (1, 32)} and any(not c["rms"] and c["branch"] == (1, 32) for c in forced)
    assert any(c["rows"] > 2048 and c["branch"] == br for c in ok for br in bc.NORM_BRANCHES[:2])
    for k in bc.KINDS:
        assert any(c["twice"] and c["xk"] == k for c in ok), k
    # the rule restated: launch_norm_bwd's thresholds
    assert [bc.norm_branch(c, 0) for c in (768, 772, 2048, 2049, 256, 257, 769)] == [(4, 3), (4, 8), (4, 8), None, (4, 3), (1, 12), (1, 32)]
    assert [bc.norm_branch(c, 1) for c in (256, 260, 768, 772, 2048)] == [(1, 4), (1, 12), (1, 12), (1, 32), (1, 32)]


# ---------------------------------------------------------------------------------------------------
# the oracle against float64 autograd on these inputs, and the rounding floor
# ---------------------------------------------------------------------------------------------------
def _t(a, grad=True):
    return None if a is None else torch.from_numpy(np.asarray(a, np.float64)).requires_grad_(grad)


def _idx(a):
    return None if a is None else torch.from_numpy(a.astype(np.int64))


def _floor(kind_of, bounds, ref, ident):
    """the oracle's result rounded to the type it is stored in: below the norm-wise bound, below 1 x the bound row by row"""
    for key, val in ref.items():
        if val is None:
            continue
        rounded = bc.round_to(val, kind_of(key))
        assert rel_err(rounded, val) < bounds[key], (ident, key, rel_err(rounded, val))
        assert bc.worst_ratio(key, rounded, val, bounds[key]) < 1.0, (ident, key, bc.worst_ratio(key, rounded, val, bounds[key]))


@pytest.mark.parametrize("c", SCAN, ids=[c["id"] for c in SCAN])
def test_scan_oracle_vs_float64_autograd_and_rounding_floor(c):
    inp = bc.scan_inputs(c, min(c["L"], CPU_LONG))
    ref = bc.scan_reference(c, inp)
    u, delta, A, Bm, Cm, D, z, db = (_t(inp[k]) for k in ("u", "delta", "A", "Bm", "Cm", "D", "z", "delta_bias"))
    y = bc.torch_scan(u, delta, A, Bm, Cm, D, z, db, c["softplus"], _idx(inp["zi"]), _idx(inp["oi"]), c["reset"])
    y.backward(_t(inp["dout"], False))
    for key, leaf in (("du", u), ("ddelta", delta), ("dA", A), ("dB", Bm), ("dC", Cm), ("dD", D), ("dz", z), ("ddelta_bias", db)):
        if leaf is None:
            assert ref[key] is None
            continue
        want = leaf.grad.numpy()
        if np.linalg.norm(want) == 0.0:
            assert np.linalg.norm(ref[key]) == 0.0, (c["id"], key)
        else:
            assert rel_err(ref[key], want) < 1e-12, (c["id"], key, rel_err(ref[key], want))
    io = ("du", "ddelta", "dz")
    _floor(lambda key: c["kind"] if key in io else "f32", bc.scan_bounds(c["kind"]), ref, c["id"])


@pytest.mark.parametrize("c", CONV, ids=[c["id"] for c in CONV])
def test_conv_oracle_vs_float64_autograd_and_rounding_floor(c):
    inp = bc.conv_inputs(c)
    ref = bc.conv_reference(c, inp)
    x, w, b = _t(inp["x"]), _t(inp["w"]), _t(inp["b"])
    bc.torch_conv(x, w, b, c["silu"], _idx(inp["perm"]), c["reset"]).backward(_t(inp["dout"], False))
    for key, leaf in (("dx", x), ("dweight", w), ("dbias", b)):
        if leaf is None:
            assert ref[key] is None
            continue
        assert rel_err(ref[key], leaf.grad.numpy()) < 1e-12, (c["id"], key, rel_err(ref[key], leaf.grad.numpy()))
    _floor(lambda key: c["kind"] if key == "dx" else "f32", bc.conv_bounds(c["kind"]), ref, c["id"])


@pytest.mark.parametrize("c", [c for c in NORM if not c["error"]], ids=[c["id"] for c in NORM if not c["error"]])
def test_norm_oracle_vs_float64_autograd_and_rounding_floor(c):
    inp = bc.norm_inputs(c)
    ref = bc.norm_reference(c, inp)
    x, w = _t(inp["xsum"]), _t(inp["w"])
    b = torch.zeros(c["cols"], dtype=torch.float64, requires_grad=True) if c["bias"] else None
    loss = (bc.torch_norm(x, w, b, bc.EPS, c["rms"]) * _t(inp["dy"], False)).sum()
    if inp["dres_out"] is not None:
        loss = loss + (x * _t(inp["dres_out"], False)).sum()            # the gradient flowing into the prenorm form's second output
    loss.backward()
    for key, leaf in (("dx", x), ("dresidual", x), ("dweight", w), ("dbias", b)):
        if ref[key] is None:
            continue
        want = leaf.grad.numpy()
        if np.linalg.norm(want) == 0.0:          # (LayerNorm over one column: xhat = 0 exactly)
            assert np.linalg.norm(ref[key]) == 0.0, (c["id"], key)
        else:
            assert rel_err(ref[key], want) < 1e-12, (c["id"], key, rel_err(ref[key], want))
    assert (ref["dweight"] is None) == (w is None) and (ref["dbias"] is None) == (b is None)
    kind_of = {"dx": c["xk"], "dresidual": c["rk"], "dweight": "f32", "dbias": "f32"}
    _floor(kind_of.get, bc.norm_bounds(c), ref, c["id"])

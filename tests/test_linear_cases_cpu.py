"""CPU checks of the case tables of tests/linear_cases.py (the four kernel families of zigma_linear_fwd and norm_linear_kernel).
Plans: the kernel string and the family every case expects (linear_cases.plan(), a restatement on the case's parameters) against plan_linear() /
plan_norm_linear() compiled with g++ on the parameter block the GPU file builds; every served leaf of both plans reached in bf16 and in fp16.
Coverage: the axis values the tables are meant to hold.  Reference: it agrees to < 1e-12 with an independent float64 torch restatement (F.linear,
F.silu, F.layer_norm, torch.addcmul: tests/kernel_standins.py).  Rounding model: the fp32 numpy model of every case (fp32 accumulation in 64-wide
k-steps, fp32 epilogue, one output rounding) needs less than the bound norm-wise and row-wise — need < 1 — and so does the rounded reference
itself; no case has a raised bound; nothing overflows fp16; the known answers are exact in both types.  And every function of
tests/test_gpu_linear_sweep.py runs here against the float64 stand-ins served at the C ABI.

`python tests/test_linear_cases_cpu.py` prints the worst need of the model per family."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]      # (run as a script)
import kernel_standins as ks  # noqa: E402
import linear_cases as lc  # noqa: E402
from test_host_cpu import _LINEAR_PLAN_DRIVER, _compile_plan, _plan_caller  # noqa: E402

LIN, NL, PROD = lc.linear_cases(), lc.norm_linear_cases(), lc.production_cases()
RAISED = {}             # id -> bound: stays empty
DT = {"bf16": torch.bfloat16, "f16": torch.float16}
_ids = lambda cases: [c["id"] for c in cases]
_t = lambda a: None if a is None else torch.from_numpy(np.asarray(a, np.float64))
_NL_PLAN_DRIVER = r"""
#include "norm_linear_plan.h"
using namespace zigma;
extern "C" int plan(const zigma_norm_linear_params_t *p, int *fields, const char **kernel) {
    const NormLinearPlan s = plan_norm_linear(*p);
    fields[0] = s.status; fields[1] = s.kernel != nullptr; fields[2] = s.ksteps; fields[3] = static_cast<int>(s.grid);
    *kernel = s.kernel;
    return s.status;
}
"""
_PLANS = {}


def plans():
    """plan_linear() and plan_norm_linear() compiled on their own with g++ (no HIP), once per session"""
    if not _PLANS:
        from zigma_amd import _lib
        _PLANS["lin"] = _plan_caller(_compile_plan(_LINEAR_PLAN_DRIVER), _lib.LinearParams, ("status", "family", "pw", "panels", "ranges", "tiles_per_xcd"))
        _PLANS["nl"] = _plan_caller(_compile_plan(_NL_PLAN_DRIVER), _lib.NormLinearParams, ("status", "family", "ksteps", "grid"))
    return _PLANS


def small(c):
    """a production case at 4096 rows' worth"""
    return dict(c, m=22528 if c["family"] == "4w" else 4096) if c.get("production") else c         # (the 4-wave kernel's floor: 256 tiles)


# ---------------------------------------------------------------------------------------------------
# the plans and the coverage
# ---------------------------------------------------------------------------------------------------
def _block(c):
    """the parameter block of fields(c) on 256-byte aligned allocations that do not exist"""
    from zigma_amd import _lib
    f = lc.fields(c)
    P = _lib.NormLinearParams() if c["kernel"] == "nl" else _lib.LinearParams()
    for key, v in f.items():
        if key not in ("off", "shape"):
            setattr(P, key, v)
    for i, (key, off) in enumerate(f["off"].items()):
        setattr(P, key, None if off is None else (i + 1 << 36) + off)
    return P


@pytest.mark.parametrize("c", LIN + NL + PROD, ids=_ids(LIN + NL + PROD))
def test_expected_kernel_is_the_compiled_plans(c):
    got = plans()[c["kernel"]](_block(c))
    assert got["status"] == 0 and got["kernel"] == c["kernel_name"], (c["id"], got)
    if c["kernel"] == "lin":
        p = lc.plan(c)
        assert got["family"] == {"tn": 1, "4w": 2, "ws": 3, "sm": 4}[c["family"]], (c["id"], got)
        if c["family"] == "ws":
            assert (got["panels"], got["ranges"], got["tiles_per_xcd"]) == (p["panels"], p["ranges"], p["tiles_per_xcd"])
    else:
        assert got["ksteps"] == c["k"] // 64 and got["grid"] == c["m"] // 128


def test_ids_are_unique_and_no_bound_is_raised():
    every = LIN + NL + PROD
    assert len({c["id"] for c in every}) == len(every)
    assert RAISED == {} and lc.SEED_MOVED == {}
    assert lc.IO_BOUND["bf16"] == 2.5e-3 and lc.IO_BOUND["f16"] == 2.5e-3 / 8 and (lc.DELTA_FLIPS, lc.ROW_GUARD) == (0.02, 4.0)


def test_every_served_leaf_is_reached_in_both_types():
    assert len(lc.TN_LEAVES) == 8 and len(set(lc.LEAVES)) == 8 + 4 + 6 + 6
    for kind in lc.KINDS:
        assert {c["leaf"] for c in LIN if c["kind"] == kind} == set(lc.LEAVES), kind
        assert {c["leaf"] for c in NL if c["kind"] == kind} == set(lc.NL_LEAVES), kind
    for leaf in lc.LEAVES:
        assert {c["regime"] for c in LIN if c["leaf"] == leaf and not c["known"]} == set(lc.REGIMES), leaf
    for leaf in lc.NL_LEAVES:
        assert {c["regime"] for c in NL if c["leaf"] == leaf and not c["known"]} == set(lc.NL_REGIMES), leaf
    groups = {"tn<4": "tn<4", "tn<2,2": "tn<2,2", "tn<2,3,0,0": "tn<2,3", "tn<2,3,1,0": "tn<2,3", "tn<2,3,0,1": "tn-gated", "tn<2,3,1,1": "tn-gated",
              "4w<0": "4w", "4w<1": "4w", "4w<2": "4w-gated", "4w<3": "4w-gated", "ws<32,0": "ws", "ws<40,0": "ws", "ws<80": "ws128", "ws<96": "ws128",
              "ws<32,1": "ws-silu", "ws<40,1": "ws-silu", "sm<": "sm"}
    group = lambda c: next(g for p, g in groups.items() if c["leaf"].startswith(p))
    for known in ("select", "ints"):      # one known answer of each kind per family and instantiation group (SiLU columns have none with integers)
        have = {group(c) for c in LIN if c["known"] == known}
        assert have >= set(groups.values()) - ({"ws-silu"} if known == "ints" else set()), (known, have)
    assert {(c["k"], c["kind"], c["part"]) for c in NL if c["known"]} == {(k, kind, p) for k in (512, 640, 768) for kind in lc.KINDS for p in (0, 1)}


def test_tables_cover_their_axes():
    fam = lambda f: [c for c in LIN if c["family"] == f]
    tn, w4, ws, sm = fam("tn"), fam("4w"), fam("ws"), fam("sm")
    for lead in ("tn<2,3,0,0>", "tn<2,3,", "tn<4,2", "tn<2,2"):       # k-steps below, at and above the stages of every pipeline form
        pick = [c for c in tn if c["leaf"].startswith(lead) and (lead != "tn<2,3," or c["rpb"])]
        assert {c["k"] for c in pick} >= {64, 128, 192, 256, 320}, lead
    assert {c["m"] for c in tn} >= {8, 16, 248, 256, 264, 504, 1040, 4352, 4344}
    tiles = {lc.plan(c)["tiles"]: lc.plan(c)["grid"] for c in tn}
    assert tiles[1] == 8 and tiles[3] == 8 and tiles[9] == 16 and tiles[272] == 256 and tiles[255] == 256
    assert {(c["n"], c["bias_lead"]) for c in tn if c["bias"]} >= {(128, 8), (128, 2), (4096, 8), (4096, 2)}
    for wide in (True, False):
        assert {c["silu"] for c in tn if c["n"] == 256 and c["leaf"].startswith("tn<4" if wide else "tn<2")} >= {0, 32, 96, 224, 256}
    assert any(c["out_lead"] == 4 and lc.fields(c)["out_row_stride"] % 8 == 4 for c in tn if c["leaf"].startswith("tn<4"))
    assert any(c["out_lead"] == 4 and lc.fields(c)["out_row_stride"] % 8 == 4 for c in tn if c["leaf"].startswith("tn<2"))
    gated = [c for c in tn if c["rpb"]]
    assert {(c["rpb"], c["m"] // c["rpb"]) for c in gated} >= {(256, 5), (256, 3), (512, 2), (768, 1), (512, 4)} and {c["bias"] for c in gated} == {True, False}
    assert all(lc.fields(c)["res_row_stride"] != lc.fields(c)["out_row_stride"] for c in gated if c["m"] < 2048)
    assert {(c["m"], c["n"]) for c in w4} >= {(2048, 8192), (2304, 8192), (2048, 8064), (2304, 8064)} and {c["k"] for c in w4} == {192, 256, 320, 448}
    assert {c["rpb"] for c in w4 if c["rpb"]} == {256, 512, 2048} and any(c["rpb"] == 256 and c["m"] == 2304 for c in w4)
    assert all(lc.fields(c)["out_row_stride"] == c["n"] + 128 for c in w4 if c["rpb"]) and all(c["rpb"] for c in w4 if c["bias"])
    near = [c for c in tn if c["m"] * c["n"] >= 2048 * 4096 and c["k"] >= 128 and not c["flags"]]
    assert {(lc.plan(c)["tiles"] == 255, c["k"] == 128, c["bias"] and not c["rpb"], bool(c["rpb"])) for c in near} >= {
        (True, False, False, False), (False, True, False, False), (False, False, True, False), (False, False, False, True)}
    pr = {(p["panels"], p["ranges"], p["tiles_per_xcd"], c["k"]) for c in ws for p in [lc.plan(c)]}
    assert pr >= {(32, 1, 1, 512), (1, 32, 32, 640), (32, 1, 1, 1280), (1, 32, 32, 1536), (1, 32, 33, 512), (1, 32, 43, 640), (1, 32, 65, 512), (8, 4, 4, 640),
                  (8, 4, 5, 512), (8, 4, 9, 640)}
    assert {c["silu"] for c in ws if c["n"] == 512} >= {0, 128, 384} and {lc.fields(c)["x_row_stride"] - c["k"] for c in ws} == {128, 256}
    assert {(c["n"], c["k"]) for c in sm} >= {(n, k) for n in (128, 384, 640, 768, 1920) for k in (128, 192, 256, 320, 1536)}
    assert {c["m"] for c in sm} >= {128, 256, 384, 768} and {(c["bias"], bool(c["rpb"])) for c in sm} == {(a, b) for a in (True, False) for b in (True, False)}
    assert any(c["bias"] and c["bias_lead"] == 4 for c in sm) and any(c["m"] == 768 and c["rpb"] == 256 for c in sm)
    assert {(c["k"], c["m"]) for c in NL} >= {(k, m) for k in (512, 640, 768) for m in (128, 256, 384)}
    assert {c["rpb"] for c in NL} >= {384, 256, 128, 96, 32, 1} and {c["bcast"] for c in NL} == {True, False}
    assert any(c["x_pad"] > 0 and c["w_pad"] > 0 and c["out_pad"] > 0 for c in NL)
    assert [(c["family"], c["m"], c["n"], c["k"]) for c in PROD] == [("ws", 65536, 2560, 640), ("4w", 65536, 640, 1280), ("4w", 65536, 640, 512),
                                                                      ("sm", 8192, 640, 1280), ("nl", 65536, 512, 640)]
    assert [c["leaf"] for c in PROD] == ["ws<40,1>", "4w<2>", "4w<3>", "sm<5,0>", "nl<10>"]


def test_edges_hold_what_they_are_meant_to():
    for fam in ("tn", "4w", "ws", "sm"):
        assert {c["seed"] % 2 for c in LIN if c["family"] == fam and c["regime"] == "edges" and not c["known"]} == {0, 1}, fam
    pick = lambda v: next(c for c in LIN if c["regime"] == "edges" and c["rpb"] and not c["known"] and c["m"] >= 16 and c["seed"] % 2 == v)
    c = pick(0)
    inp, r = lc.inputs(c), lc.edge_rows(c["m"])
    ref = lc.reference(c, inp)
    assert not inp["x"][r["zero"]].any() and not inp["w"][[2, c["n"] - 3]].any()
    xw = np.linalg.norm(inp["x"][r["cancel"]], axis=1).min() * np.linalg.norm(inp["w"], axis=1).mean()
    assert np.abs(ref["v"][r["cancel"]]).max() < 1e-12 * xw and xw > 1, "rows built to cancel"
    tiny = np.abs(inp["x"][r["tiny"]])
    assert ((tiny > 0) & (tiny < 2.0 ** -14)).any(), "fp16 subnormal operands"
    assert {4.0, -4.0, 0.0} <= set(inp["gate"][0, :4].tolist())
    c = pick(1)
    inp, r = lc.inputs(c), lc.edge_rows(c["m"])
    assert 3.5 < inp["x"][r["mean"]].mean() < 4.5 and inp["w"][20:24].mean() > 0.4
    s = next(c for c in LIN if c["regime"] == "edges" and c["silu"] == 0 and not c["bias"] and c["m"] >= 16)
    v = lc._product(lc.inputs(s)["x"], lc.inputs(s)["w"], np.float64)
    assert {-100.0, -30.0, -12.0, 12.0, 30.0, 100.0} <= set(np.unique(v[[row for row, _ in lc.edge_rows(s["m"])["spike"]]]).tolist())
    out = lc.reference(s, lc.inputs(s))["out"]
    assert np.isfinite(out).all() and (lc.round_to(out[s["m"] - 2][v[s["m"] - 2] == -100.0], s["kind"]) == 0).all()
    m = next(c for c in LIN if c["regime"] == "model" and c["rpb"])
    inp = lc.inputs(m)
    assert 20 < inp["res"].std() < 40 and 0.05 < inp["gate"].mean() < 0.15 and abs(np.sqrt((inp["x"] ** 2).mean(-1)) - 1).max() < 0.01
    e = next(c for c in NL if c["regime"] == "edges")
    inp = lc.inputs(e)
    assert np.ptp(inp["x"][1]) == 0 and abs(inp["x"][2].mean() - 100) < 1 and not inp["x"][3].any() and (inp["scale"][:, :8] == -1).all()
    assert {4.0, -4.0} <= set(inp["scale"][0, 8:12].tolist()) and {4.0, -4.0} <= set(inp["shift"][0, 8:12].tolist())
    assert np.abs(lc.reference(e, inp)["y"][[1, 3]]).max() == 0


# ---------------------------------------------------------------------------------------------------
# reference vs the torch restatement; the rounding model
# ---------------------------------------------------------------------------------------------------
MEASURED = {}           # (family, kind) -> worst need of the fp32 model in units of the bound


def _pin(c, key, ref, again):
    e = lc.norm_err(ref, again.numpy()) if np.linalg.norm(ref) > 0 else float(again.norm())
    assert e < 1e-12, (c["id"], key, e)


def _model(c, model, ref, terms):
    kind = c["kind"]
    bound = lc.IO_BOUND[kind]
    assert np.isfinite(ref).all() and np.abs(ref).max() < lc.F16_LIMIT, (c["id"], "overflows fp16")
    own = lc.need(lc.round_to(ref, kind), ref, terms) / bound
    assert own < 1, (c["id"], own, "the rounded reference itself: another seed (SEED_MOVED), not another bound")
    got = lc.need(lc.round_to(model, kind), ref, terms) / bound
    slot = (c["family"], kind)
    MEASURED[slot] = max(MEASURED.get(slot, 0.0), got)
    assert got < 1, (c["id"], got)


@pytest.mark.parametrize("c", LIN + PROD[:4], ids=_ids(LIN + PROD[:4]))
def test_linear_reference_and_rounding_model(c):
    c = small(c)
    inp, dt = lc.inputs(c), DT[c["kind"]]
    ref = lc.reference(c, inp)
    gate = None if inp["gate"] is None else _t(lc.gate_rows(c, inp))
    again, terms = ks.torch_linear(_t(inp["x"]), _t(inp["w"]), _t(inp["bias"]), c["silu"], _t(inp["res"]), gate, dt, c["family"] != "4w")
    _pin(c, "out", ref["out"], again)
    if terms is not None:
        _pin(c, "gate * v", ref["terms"][1], terms[1])
    m32 = lc.reference(c, inp, np.float32)["out"]
    assert m32.dtype == np.float32
    _model(c, m32, ref["out"], ref["terms"])
    if c["known"]:          # exact in fp32 and in the case's type (SiLU columns aside)
        plain = slice(0, c["silu"])
        exact = ref["out"] if not c["rpb"] else lc.round_to(ref["out"].astype(np.float32), c["kind"]).astype(np.float64)
        assert np.array_equal(lc.round_to(m32, c["kind"]).astype(np.float64)[:, plain], exact[:, plain])
        assert np.array_equal(lc.round_to(ref["v"].astype(np.float32), c["kind"]).astype(np.float64)[:, plain], ref["v"][:, plain]), "x w^T + bias is exact"
        if c["known"] == "select":
            assert len(np.unique(np.nonzero(inp["w"])[1])) == min(c["n"], c["k"]) and (np.count_nonzero(inp["w"], axis=1) == 1).all()
            assert len(np.unique(inp["x"], axis=0)) == c["m"] and np.abs(inp["x"]).max() > 256 and np.abs(inp["x"]).min() < 2.0 ** -7
        else:
            nz = np.count_nonzero(inp["w"], axis=1)
            assert nz.max() <= 8 and nz.min() >= 1 and np.abs(inp["w"][:, :64]).sum(1).min() > 0 and np.abs(inp["w"][:, -64:]).sum(1).min() > 0
            assert np.abs(ref["v"] - (0 if inp["bias"] is None else inp["bias"])).max() <= 64 and np.array_equal(ref["v"], np.rint(ref["v"]))
    if c["rpb"] and c["family"] != "4w":         # the defined value of the gated epilogue, on the reference's own plain output
        p16 = lc.round_to(ref["v"].astype(np.float32), c["kind"])
        assert np.array_equal(lc.gated_defined(c, inp, p16), lc.round_to(ref["out"].astype(np.float32), c["kind"]))


@pytest.mark.parametrize("c", NL + PROD[4:], ids=_ids(NL + PROD[4:]))
def test_norm_linear_reference_and_rounding_model(c):
    c = small(c)
    inp, dt = lc.inputs(c), DT[c["kind"]]
    ref = lc.reference(c, inp)
    rep = c["m"] if c["bcast"] else c["rpb"]
    again = ks.torch_norm_linear(_t(inp["x"]), _t(inp["w"]), _t(inp["shift"]).repeat_interleave(rep, 0), _t(inp["scale"]).repeat_interleave(rep, 0), lc.NL_EPS, dt)
    for key in ("y_mod", "out"):
        _pin(c, key, ref[key], again[key])
    assert np.array_equal(ref["xa"].astype(np.float64), again["xa"].numpy())
    m32 = lc.reference(c, inp, np.float32)
    _model(c, m32["out"], ref["out"], None)
    assert lc.need(lc.round_to(m32["y_mod"], c["kind"]), ref["y_mod"], ref["terms"]) < lc.IO_BOUND[c["kind"]]
    assert lc.flipped_share(lc.round_to(m32["y_mod"], c["kind"]), ref["y_mod"], c["kind"]) < lc.DELTA_FLIPS / 2, "the fp32 model of the hidden intermediate"
    if c["known"]:
        start = c["part"] * (c["k"] - c["n"])
        assert np.array_equal(ref["out"], ref["xa"][:, start:start + c["n"]].astype(np.float64))


def test_worst_need_of_the_model_per_family():
    """(after the parametrised tests above) prints what the model measured; every family was measured in both types"""
    for slot, v in sorted(MEASURED.items()):
        print(f"fp32 model, worst need in units of the bound: {slot[0]:3s} {slot[1]:5s} {v:.3f}")
    assert all(v < 1 for v in MEASURED.values())


# ---------------------------------------------------------------------------------------------------
# tests/test_gpu_linear_sweep.py on the CPU: float64 stand-ins at the C ABI
# ---------------------------------------------------------------------------------------------------
@pytest.fixture
def gpu_file(monkeypatch):
    import test_gpu_linear_sweep as gf
    ks.install_lib_call(monkeypatch, linear_plan=plans()["lin"], norm_linear_plan=plans()["nl"])
    monkeypatch.setattr(gf, "DEV", "cpu")
    return gf


@pytest.mark.parametrize("c", LIN + PROD[:4], ids=_ids(LIN + PROD[:4]))
def test_gpu_linear_checks_pass_on_the_stand_in(c, gpu_file, capsys):
    gpu_file.check_linear_case(small(c))
    assert f"linear-sweep {c['id']}: out " in capsys.readouterr().out


@pytest.mark.parametrize("c", NL + PROD[4:], ids=_ids(NL + PROD[4:]))
def test_gpu_norm_linear_checks_pass_on_the_stand_in(c, gpu_file, capsys):
    gpu_file.check_norm_linear_case(small(c))
    assert f"linear-sweep {c['id']}: out " in capsys.readouterr().out


def test_gpu_checks_turn_red_on_a_wrong_row(gpu_file, monkeypatch):
    """one row of 4344 from its neighbour, a gate row of the wrong sample, a read of the NaN beside x, a write beside the output, a hidden
    intermediate 0.4 % off: each is caught"""
    real_lin, real_nl = ks.torch_linear, ks.torch_norm_linear

    def wrong_row(*a):
        out, terms = real_lin(*a)
        out[4000] = out[3999]
        return out, terms

    def wrong_sample(x, w, bias, s, res, gate, *a):
        return real_lin(x, w, bias, s, res, None if gate is None else gate.roll(256, 0), *a)

    def poisoned(x, *a):
        return real_lin(torch.cat([x[:, :-1], x[:, -1:] + float("nan")], 1), *a)

    def scaled_y(x, w, shift, scale, eps, dt):
        r = real_nl(x, w, shift, scale, eps, dt)
        r["out"] = torch.nn.functional.linear(r["y_mod"] * 1.004, w)
        return r
    big = next(c for c in LIN if c["m"] == 4344 and c["family"] == "tn" and not c["known"])
    gated = next(c for c in LIN if c["family"] == "tn" and c["rpb"] == 256 and c["m"] == 1280 and not c["known"])
    sel = next(c for c in NL if c["known"])
    for name, bad, c, check in (("torch_linear", wrong_row, big, "check_linear_case"), ("torch_linear", wrong_sample, gated, "check_linear_case"),
                                ("torch_linear", poisoned, LIN[0], "check_linear_case"), ("torch_norm_linear", scaled_y, sel, "check_norm_linear_case")):
        with monkeypatch.context() as mp:
            mp.setattr(ks, name, bad)
            mp.setattr(gpu_file, "HOST_LIMIT", 1 << 40)          # (the numpy reference: the restatement is what is broken here)
            with pytest.raises(AssertionError):
                getattr(gpu_file, check)(c)
    real_call = gpu_file._call

    def spill(c, P, kernel=None):
        got = real_call(c, P, kernel)
        ks._view(P.out, (1, 1), (1, 1), DT[c["kind"]])[0, 0] = 1.0
        ks._view(P.out - 2, (1, 1), (1, 1), DT[c["kind"]])[0, 0] = 1.0
        return got
    monkeypatch.setattr(gpu_file, "_call", spill)
    with pytest.raises(AssertionError, match="outside the output window"):
        gpu_file.check_linear_case(LIN[0])


if __name__ == "__main__":
    for fn, cases in ((test_linear_reference_and_rounding_model, LIN + PROD[:4]), (test_norm_linear_reference_and_rounding_model, NL + PROD[4:])):
        for case in cases:
            try:
                fn(case)
            except AssertionError as err:
                print("FAILS", err)
    for slot, v in sorted(MEASURED.items()):
        print(f"fp32 model, worst need in units of the bound: {slot[0]:3s} {slot[1]:5s} {v:.3f}")
    print(f"RAISED = {RAISED!r}, SEED_MOVED = {lc.SEED_MOVED!r}")

"""CPU checks of the forward sweep's case tables (tests/fwd_fuzz_cases.py).  Coverage: every leaf of tests/scan_plan_cases.py that launches a
token-major kernel, every axis value in every I/O type, every value regime per form, different row tables, the chunk counts.  Reference: it
agrees to < 1e-12 with an independent float64 restatement on exactly these inputs (torch, an explicit loop over sequence, chunk and step:
tests/kernel_standins.py), carries and checkpoints included.  Rounding model: the reference rounded to the I/O type needs < 1 x every limit,
the fp32 numpy model <= 1/2 x every limit or the case carries the raised bound of fwd_fuzz_cases.RAISED.  Known answers are exact in float64
and in a step-by-step fp32 recurrence.  And every function of tests/test_gpu_fwd_fuzz.py runs here against float64 stand-ins served at the C
ABI, with plan_scan() and the front's plans compiled with g++ naming the kernel: the kernel each case expects is the one the plan picks.

`python tests/test_fwd_fuzz_cases_cpu.py` prints the RAISED table (2 x d_model of the cases whose fp32 model needs more than half a limit)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]      # (run as a script)
import fwd_fuzz_cases as fc  # noqa: E402
import kernel_standins as ks  # noqa: E402

SCAN2, SCAN1, CONVX, XPROJ, DTPROJ, PROD = (fc.scan2_cases(), fc.scan1_cases(), fc.conv_xproj_cases(), fc.xproj_cases(), fc.dtproj_cases(),
                                            fc.production_cases())
SCAN = SCAN2 + SCAN1
CPU_BATCH = 2           # the wide cases (B >= 24) are modelled on their first two samples here
_ids = lambda cases: [c["id"] for c in cases]


def _cpu_inputs(c):
    return fc.production_inputs(c) if c["form"].startswith("production") else fc.scan_inputs(c, CPU_BATCH if c["B"] >= 24 else None)


# ---------------------------------------------------------------------------------------------------
# coverage
# ---------------------------------------------------------------------------------------------------
def test_every_token_major_leaf_of_the_plan_is_hit():
    import scan_plan_cases as spc
    tok = {name for name, (_, want) in spc.CASES.items() if want.family in (spc.TOK, spc.TOK2)}
    assert tok == set(fc.PLAN_LEAVES) | set(fc.PLAN_LEAVES_ELSEWHERE), tok ^ (set(fc.PLAN_LEAVES) | set(fc.PLAN_LEAVES_ELSEWHERE))
    for name, hit in fc.PLAN_LEAVES.items():
        mine = [c for c in SCAN if hit(c)]
        assert mine, name
        kernel = spc.CASES[name][1].kernel
        assert all(c["kernel_name"] in (kernel, kernel.replace("tok_n16", "tok_n8")) or c["r6_twin"] for c in mine), (name, kernel, {c["kernel_name"] for c in mine})
        assert all(c["info1"] == spc.CASES[name][1].info[1] for c in mine), name


def test_scan2_table_covers_its_axes():
    assert len({c["id"] for c in SCAN}) == len(SCAN) and 140 <= len(SCAN2) <= 180
    assert {c["form"] for c in SCAN2} == set(fc.SCAN2_FORMS)
    for kind in ("bf16", "f16"):
        mine = [c for c in SCAN2 if c["kind"] == kind]
        assert all(c["kernel_name"].startswith("scan_tok2") for c in mine)
        assert {c["L"] for c in mine} >= set(fc.SCAN2_L) and {c["dim"] for c in mine} >= set(fc.SCAN2_DIM) and {c["B"] for c in mine} >= {1, 2, 3}
        for form in fc.SCAN2_FORMS:
            assert {c["regime"] for c in mine if c["form"] == form and not c["known"]} == set(fc.REGIMES), (kind, form)
        assert {c["form"] for c in mine if c["known"]} == set(fc.KNOWN_FORMS)
        assert {(c["bias"], c["softplus"]) for c in mine if c["form"].startswith("whole")} == {(a, b) for a in (True, False) for b in (True, False)}
        split = [c for c in mine if c["chunk"]]
        assert {(c["L"], c["chunk"]) for c in split if not c["known"]} == set(fc.SCAN2_SPLITS), kind
        assert {c["chunk"] for c in split} == {16, 32, 48} and any(c["L"] % c["chunk"] for c in split)
        assert {2, 7} <= {-(-c["L"] // c["chunk"]) for c in split} and max(-(-c["L"] // c["chunk"]) for c in split) >= 7
        assert {c["reset"] for c in mine if c["form"] == "reset"} == {16, 32, 64} == {c["reset"] for c in mine if c["form"] == "dtp-reset"}
        dtp = [c for c in mine if c["dt"]]
        assert {c["R"] for c in dtp} == set(fc.SCAN2_R) and {c["pitch"] - c["R"] for c in dtp if c["pitch"] != 128} == {32, 40} and any(c["pitch"] == 128 for c in dtp)
        assert {(c["B"], c["dim"], c["L"]) for c in mine if c["r6_twin"]} == set(fc.SCAN2_R6)
        assert all("_r6" in c["kernel_name"] and 1281 <= c["B"] * (c["dim"] // 64) <= 1536 for c in mine if c["r6_twin"])
        assert sum(c["twice"] for c in mine) == 2
        assert any(c["views"] for c in mine) and any(not c["views"] for c in mine)
    for c in SCAN + PROD:
        if c["tables"] and c["L"] > 1:
            inp = _cpu_inputs(c)
            period = c["reset"] or c["L"]
            for t in (inp["zi"], inp["oi"]):
                assert sorted(t.tolist()) == list(range(c["L"])) and (t // period == np.arange(c["L"]) // period).all(), c["id"]
            assert not np.array_equal(inp["zi"], inp["oi"]), c["id"]
        if c["chunk"] and c in SCAN:        # every split case has the chunk count it claims
            assert fc.scan_reference(c, fc.scan_inputs(c, 1))["x_state"].shape[1] == -(-c["L"] // c["chunk"]) >= 2, c["id"]
    assert [(c["L"], c["chunk"]) for c in PROD if c["chunk"]] == [(4096, 256)]


def test_scan1_table_covers_its_axes():
    assert all(c["kernel_name"] == f"scan_tok_n{c['N']}" for c in SCAN1)
    base = [c for c in SCAN1 if c["form"] == "tok"]
    assert {(c["kind"], c["N"], c["L"]) for c in base} == {(k, n, L) for k in ("f32", "bf16", "f16") for n in (16, 8) for L in fc.SCAN1_L}
    for kind in ("f32", "bf16", "f16"):
        mine = [c for c in SCAN1 if c["kind"] == kind]
        for opt in ("z", "D", "bias", "softplus", "tables", "views"):
            assert {c[opt] for c in mine} == {True, False}, (kind, opt)
        assert {c["regime"] for c in mine} == set(fc.REGIMES)
        assert any(c["form"] == "tok-carries" for c in mine) and any(c["form"] == "tok-ckpt" and c["info1"] == 1 for c in mine)
    assert {(c["L"], c["N"]) for c in SCAN1 if c["form"] == "tok-split"} == {(L, n) for L in (48, 100, 257) for n in (16, 8)}
    assert all(c["chunk"] == 32 and c["kind"] == "f32" for c in SCAN1 if c["form"] == "tok-split")


def test_feeder_tables_cover_their_axes():
    for kind in ("bf16", "f16"):
        cx = [c for c in CONVX if c["kind"] == kind]
        assert {(c["B"], c["L"]) for c in cx} == set(fc.CX_SHAPES) and {c["dim"] for c in cx} == set(fc.CX_DIM) and {c["n"] for c in cx} == set(fc.CX_N)
        assert {c["table"] for c in cx} == set(fc.CX_TABLES) and {c["flags"] for c in cx} == {0, 1, 2, 3} and {c["regime"] for c in cx} == {"benign", "edges"}
        assert all(c["L"] % 32 == 0 and c["B"] * c["L"] % 256 == 0 and c["dim"] % 64 == 0 and c["n"] % 8 == 0 for c in cx)       # the entry point's limits
        xp = [c for c in XPROJ if c["kind"] == kind]
        sk = [c for c in xp if c["kernel_name"] == "x_proj_splitk"]
        assert {c["M"] for c in sk} == set(fc.XP_M) and {c["K"] for c in sk} == set(fc.XP_K) and {c["n"] for c in sk} == set(fc.XP_N)
        assert {(c["M"], c["K"]) for c in xp if c["kernel_name"] == "x_proj_mfma"} == {(16, 2048), (257, 2048), (512, 2048)}
        assert {c["pad"] > 0 for c in xp} == {True, False}
        dp = [c for c in DTPROJ if c["kind"] == kind]
        assert {c["M"] for c in dp} == set(fc.DT_M) and {c["dim"] for c in dp} == set(fc.DT_DIM) and {c["R"] for c in dp} == set(fc.DT_R)
        assert {c["pitch"] - c["R"] for c in dp if c["pitch"] != 72} >= {0, 32} and any(c["pitch"] == 72 for c in dp)
        assert {(c["softplus"], c["bias"]) for c in dp} == {(a, b) for a in (True, False) for b in (True, False)}
        assert {c["regime"] for c in dp} == set(fc.REGIMES) and {c["w_pad"] > 0 for c in dp} == {True, False}
    assert len({c["id"] for c in CONVX + XPROJ + DTPROJ}) == len(CONVX + XPROJ + DTPROJ)


# ---------------------------------------------------------------------------------------------------
# reference vs an independent restatement; rounding model; known answers; edge values
# ---------------------------------------------------------------------------------------------------
def _restated(c, inp, step):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))
    R, N = c["R"], c["N"]
    r = ks.torch_scan_fwd(t(inp["u"]), t(step), t(inp["A"]), t(inp["xdbl"][..., R:R + N]), t(inp["xdbl"][..., R + N:R + 2 * N]), t(inp["D"]), t(inp["gate"]),
                          t(inp["zi"]), t(inp["oi"]), reset=c["reset"], chunk=c["chunk"], out_z0=t(inp["out_z0"]))
    return {"out_z": r["y_gated"], "out": r["y"], "ckpt": r["ckpt"], "x_prod": r["x_prod"], "x_state": r["x_state"]}


def model_needs(c, inp, ref):
    """the fp32 numpy oracle on the same operands -> per output fc.model_excess: (excess, d_model)"""
    m = fc.scan_reference(c, inp, dt=np.float32)
    return {k: fc.model_excess(v, ref[k], fc.out_kind(c, k), ref.get("_acc_terms") if k == "out_z" else None, k == "delta")
            for k, v in m.items() if not k.startswith("_")}


@pytest.mark.parametrize("c", SCAN + PROD, ids=_ids(SCAN + PROD))
def test_scan_reference_restatement_and_rounding_model(c):
    inp = _cpu_inputs(c)
    ref = fc.scan_reference(c, inp)
    pre = fc.pre_softplus(c, inp)
    step = torch.nn.functional.softplus(torch.from_numpy(pre)).numpy() if c["softplus"] else pre
    again = _restated(c, inp, step) if c in SCAN else {}        # (the production shapes: the same code on 4096 steps; the model only)
    for key, want in ref.items():
        if key.startswith("_") or key == "delta" or not again:
            continue
        assert np.isfinite(want).all(), (c["id"], key)
        e = fc.norm_err(want, again[key].numpy())
        assert e < 1e-12 or np.linalg.norm(want) == 0.0 == float(again[key].norm()), (c["id"], key, e)
    if "delta" in ref:
        assert fc.norm_err(ref["delta"], step) < 1e-12
    # the reference rounded to the type it is stored in: < 1 x every limit
    for key, want in ref.items():
        if key.startswith("_"):
            continue
        rounded = fc.round_to(want, fc.out_kind(c, key))
        n = fc.need(rounded, want, ref.get("_acc_terms") if key == "out_z" else None, elementwise=key == "delta")
        assert n < fc.base_bound(c, key), (c["id"], key, n)
        if c["regime"] == "edges" and c["kind"] == "f16":
            assert np.abs(want).max() < 65504.0, (c["id"], key, "a correct output would overflow fp16")
    # the fp32 model: <= 1/2 x every limit, or the raised bound covers 2 x d_model
    for key, (excess, d_model) in model_needs(c, inp, ref).items():
        assert d_model < fc.bound_of(c, key), (c["id"], key, d_model)
        if key in fc.RAISED.get(c["id"], {}):
            assert 2.0 * d_model <= fc.bound_of(c, key), (c["id"], key, d_model, fc.bound_of(c, key))
        else:
            assert excess <= 0.5 * fc.base_bound(c, key), (c["id"], key, excess, "the case needs an entry in fwd_fuzz_cases.RAISED")
    if "delta" in ref:      # the staged check holds on the model
        m = fc.round_to(fc.step_sizes(c, inp, np.float32), c["kind"])
        assert fc.flipped_share(m, ref["delta"], c["kind"]) < fc.DELTA_FLIPS_MODEL, c["id"]
        own = fc.scan_reference(c, inp if c in SCAN else {k: (v[:, :512] if k in ("u", "z", "gate", "xdbl") else v) for k, v in inp.items()},
                                step=m if c in SCAN else m[:, :512])
        assert "delta" not in own and fc.need(fc.round_to(own["out_z"], c["kind"]), own["out_z"]) < fc.base_bound(c, "out_z")


def test_raised_table_names_only_cases_that_need_it():
    ids = {c["id"] for c in SCAN + PROD}
    assert set(fc.RAISED) <= ids
    for cid, keys in fc.RAISED.items():
        c = next(c for c in SCAN + PROD if c["id"] == cid)
        inp = _cpu_inputs(c)
        needs = model_needs(c, inp, fc.scan_reference(c, inp))
        for key, b in keys.items():
            excess, d_model = needs[key]
            assert excess > 0.5 * fc.base_bound(c, key) and 2.0 * d_model <= b <= 2.5 * d_model, (cid, key, excess, d_model, b)


@pytest.mark.parametrize("c", [c for c in SCAN2 if c["known"]], ids=_ids([c for c in SCAN2 if c["known"]]))
def test_known_answers_are_exact(c):
    inp = fc.scan_inputs(c)
    exact, fp32, ref = fc.known_answer(c, inp), fc.known_answer(c, inp, np.float32), fc.scan_reference(c, inp)
    assert np.float32(fc.A_HALF * np.float32(1.4426950408889634)) == np.float32(-1.0)
    for key, want in exact.items():
        assert fp32[key].dtype == np.float32 and np.array_equal(want, fp32[key].astype(np.float64)), (c["id"], key)
        assert np.abs(want).max() > 0 and fc.norm_err(ref[key], want) < 1e-6, (c["id"], key)      # (the reference takes exp(A_HALF), 0.5 to 1e-8)
        assert np.array_equal(want.astype(np.float32).astype(np.float64), want) and np.abs(want).max() < 65504.0
    assert set(exact) == {k for k in ref if not k.startswith("_")}


@pytest.mark.parametrize("kind", ["bf16", "f16"])
def test_edges_regime_reaches_every_edge(kind):
    bands = dict(below_pass=0, above_pass=0, switch=0, zero=0)
    for c in SCAN2 + SCAN1:
        if c["regime"] != "edges" or c["kind"] != kind:
            continue
        inp = _cpu_inputs(c)
        for k in ("u", "z", "delta", "w"):      # every 16-bit operand survives its round trip
            if inp[k] is not None:
                assert np.array_equal(fc.round_to(inp[k], kind), inp[k], equal_nan=True) and np.abs(np.nan_to_num(inp[k])).max() < 65504.0
        used = inp["xdbl"][..., (0 if c["dt"] else c["R"]):c["R"] + 2 * c["N"]]
        assert np.isfinite(used).all() and np.array_equal(fc.round_to(inp["xdbl"], kind), inp["xdbl"], equal_nan=True)
        if c["z"]:
            zs = set(np.unique(inp["z"][np.abs(inp["z"]) >= 11.0]).tolist()) if not c["zact"] else None
            assert zs is None or zs >= {12.0, -12.0, 30.0, -30.0}, (c["id"], zs)
        R, N = c["R"], c["N"]
        assert (np.abs(inp["u"]).max(-1) == 0).any() and (np.abs(inp["xdbl"][..., R:R + N]).max(-1) == 0).any() and (np.abs(inp["xdbl"][..., R + N:R + 2 * N]).max(-1) == 0).any()
        if kind == "f16":
            assert ((np.abs(inp["u"]) < 6.1e-5) & (inp["u"] != 0)).any(), c["id"]
        if c["softplus"] and c["bias"]:
            pre = fc.pre_softplus(c, inp)
            bands["below_pass"] += int(((pre > 19.5) & (pre <= 20.0)).sum())
            bands["above_pass"] += int(((pre > 20.0) & (pre < 20.5)).sum())
            bands["switch"] += int(((pre > -6.0) & (pre < -3.0)).sum())
            bands["zero"] += int((pre < -17.0).sum())
    assert all(v > 100 for v in bands.values()), bands


def _t64(a):
    return torch.from_numpy(np.asarray(a, np.float64))


@pytest.mark.parametrize("c", CONVX, ids=_ids(CONVX))
def test_conv_xproj_reference_and_rounding_model(c):
    inp, kind, dim, L = fc.conv_xproj_inputs(c), c["kind"], c["dim"], c["L"]
    ref = fc.conv_xproj_reference(c, inp)
    x = _t64(inp["xz"][..., :dim])
    if inp["perm"] is not None:
        x = x.index_select(1, torch.from_numpy(inp["perm"]).long())
    xp = torch.nn.functional.pad(x, (0, 0, 3, 0))
    pre = _t64(inp["cb"]) + sum(_t64(inp["cw"])[:, t] * xp[:, t:t + L] for t in range(4))
    assert fc.norm_err(ref["u"], (pre * torch.sigmoid(pre)).numpy()) < 1e-12
    if c["regime"] == "edges":
        assert {12.0, -12.0, 30.0, -30.0} <= set(np.round(pre.numpy()[0, 5, :4]).tolist())
    u_own = fc.round_to(fc.conv_xproj_reference(c, inp, dt=np.float32)["u"], kind)          # the model's own u
    ref2 = fc.conv_xproj_reference(c, inp, u_own=u_own)
    assert fc.norm_err(ref2["x_dbl"], (_t64(u_own) @ _t64(inp["w"]).T).numpy()) < 1e-12
    m2 = fc.conv_xproj_reference(c, inp, u_own=u_own, dt=np.float32)
    bound = fc.IO_BOUND[kind]
    for key, model in (("u", fc.conv_xproj_reference(c, inp, dt=np.float32)["u"]), ("x_dbl", m2["x_dbl"])):
        excess, d_model = fc.model_excess(model, ref2[key], kind)
        assert fc.need(fc.round_to(ref2[key], kind), ref2[key]) < bound and excess <= 0.5 * bound and d_model < bound, (c["id"], key, excess, d_model)
        assert np.abs(ref2[key]).max() < 65504.0


@pytest.mark.parametrize("c", XPROJ, ids=_ids(XPROJ))
def test_xproj_reference_and_rounding_model(c):
    inp, bound = fc.xproj_inputs(c), fc.IO_BOUND[c["kind"]]
    ref = fc.xproj_reference(c, inp)["x_dbl"]
    assert fc.norm_err(ref, (_t64(inp["u"]) @ _t64(inp["w"]).T).numpy()) < 1e-12
    excess, d_model = fc.model_excess(fc.xproj_reference(c, inp, np.float32)["x_dbl"], ref, c["kind"])
    assert fc.need(fc.round_to(ref, c["kind"]), ref) < bound and excess <= 0.5 * bound and d_model < bound, (c["id"], excess, d_model)


@pytest.mark.parametrize("c", DTPROJ, ids=_ids(DTPROJ))
def test_dtproj_reference_and_rounding_model(c):
    inp, bound, kind = fc.dtproj_inputs(c), fc.IO_BOUND[c["kind"]], c["kind"]
    ref = fc.dtproj_reference(c, inp)
    pre = _t64(inp["x"][:, :c["R"]]) @ _t64(inp["w"]).T + (0 if inp["bias"] is None else _t64(inp["bias"]))
    want = torch.nn.functional.softplus(pre) if c["softplus"] else pre
    assert fc.norm_err(ref["delta"], want.numpy()) < 1e-12 and np.isnan(inp["x"][:, c["R"]:]).all()
    m32 = fc.dtproj_reference(c, inp, np.float32)["delta"]
    model = fc.round_to(m32, kind)
    for ew in (False, True):
        assert fc.need(fc.round_to(ref["delta"], kind), ref["delta"], elementwise=ew) < bound, c["id"]
        excess, d_model = fc.model_excess(m32, ref["delta"], kind, elementwise=ew)
        assert excess <= 0.5 * bound and d_model < bound, (c["id"], ew, excess, d_model)
    assert fc.flipped_share(model, ref["delta"], kind) < fc.DELTA_FLIPS_MODEL, c["id"]
    if c["regime"] == "edges" and c["softplus"] and c["bias"]:
        p = ref["pre"]
        assert ((p > 19.5) & (p < 20.5)).any() and ((p > -6) & (p < -3)).any() and (p < -17).any()


# ---------------------------------------------------------------------------------------------------
# tests/test_gpu_fwd_fuzz.py on the CPU: float64 stand-ins at the C ABI, plan_scan() compiled with g++ names the kernel
# ---------------------------------------------------------------------------------------------------
from test_host_cpu import front_plan, scan_plan  # noqa: E402,F401  (the module-scoped fixtures)


@pytest.fixture
def gpu_file(monkeypatch, scan_plan, front_plan):  # noqa: F811
    import test_gpu_fwd_fuzz as gf
    ks.install_lib_call(monkeypatch, scan_plan, front_plan)
    monkeypatch.setattr(gf, "DEV", "cpu")
    return gf


@pytest.mark.parametrize("c", SCAN, ids=_ids(SCAN))
def test_gpu_scan_checks_pass_on_the_stand_in(c, gpu_file, capsys):
    gpu_file.check_scan_case(c)
    assert f"fwd-sweep {c['id']}: " in capsys.readouterr().out


def test_gpu_feeder_checks_pass_on_the_stand_in(gpu_file):
    for c in CONVX[::5]:
        gpu_file.check_conv_xproj_case(c)
    for c in XPROJ[::3]:
        gpu_file.check_xproj_case(c)
    for c in DTPROJ[::4]:
        gpu_file.check_dtproj_case(c)


def test_gpu_checks_turn_red_on_a_wrong_row(gpu_file, monkeypatch):
    """one output row 3 % off, a carry from the chunk before, a write into the NaN surroundings: each is caught"""
    c = next(c for c in SCAN2 if c["form"] == "split" and c["views"] and c["L"] == 256 and c["kind"] == "bf16")
    real = ks.torch_scan_fwd

    def wrong_row(*a, **kw):
        r = real(*a, **kw)
        r["y_gated"][0, int(r["y_gated"][0].norm(dim=-1).argmax())] *= 1.03         # (a row of at least the rms row norm: the metric's floor)
        return r

    def stale_carry(*a, **kw):
        r = real(*a, **kw)
        r["x_state"][:, 2] = r["x_state"][:, 1]
        return r
    for bad in (wrong_row, stale_carry):
        monkeypatch.setattr(ks, "torch_scan_fwd", bad)
        with pytest.raises(AssertionError):
            gpu_file.check_scan_case(c)
    monkeypatch.setattr(ks, "torch_scan_fwd", real)
    real_run = gpu_file.scan_run

    def spill(c, inp, r5=False):
        run = real_run(c, inp, r5)
        run["slots"]["out_z"].buf[0, 3, -1] = 1.0
        return run
    monkeypatch.setattr(gpu_file, "scan_run", spill)
    with pytest.raises(AssertionError, match="surroundings"):
        gpu_file.check_scan_case(c)


if __name__ == "__main__":
    table = {}
    for case in SCAN + PROD:
        inputs = _cpu_inputs(case)
        needs = model_needs(case, inputs, fc.scan_reference(case, inputs))
        over = {k: float(f"{2.2 * d:.3g}") for k, (excess, d) in needs.items() if excess > 0.5 * fc.base_bound(case, k)}
        if over:
            table[case["id"]] = over
    print("RAISED = {")
    for cid, v in table.items():
        print(f"    {cid!r}: {v!r},")
    print("}")

"""CPU checks of the case tables of the reference-layout sweep (tests/ref_layout_cases.py).  Coverage: every axis the tables claim, per I/O type;
every generic leaf of tests/scan_plan_cases.py is reached by cases plan_scan() (compiled with g++) serves with scan_generic, and no case is
served by a token-major kernel; the conv cases' kernels are the ones plan_conv1d() (compiled) names.  Reference: it agrees to < 1e-12 with an
independent float64 restatement on exactly these inputs (explicit torch loops in tests/kernel_standins.py; F.conv1d for the conv).  Rounding
model: the reference rounded to the I/O type needs < 0.9 x every limit, the fp32 numpy model <= 1/2 x every limit or the case carries the raised
bound of ref_layout_cases.RAISED, which is held to its conditions.  Every function of tests/test_gpu_ref_layout.py runs here against float64
stand-ins served at the C ABI, and four mutated stand-ins each turn some case red.

`python tests/test_ref_layout_cases_cpu.py` prints the RAISED table (2 x d_model of the cases whose fp32 model needs more than half a limit)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]      # (run as a script)
import kernel_standins as ks  # noqa: E402
import ref_layout_cases as rl  # noqa: E402

SCAN, CONV = rl.scan_generic_cases(), rl.conv_cases()
_ids = lambda cases: [c["id"] for c in cases]
PAIRS = {(a, b) for a in (True, False) for b in (True, False)}


# ---------------------------------------------------------------------------------------------------
# coverage
# ---------------------------------------------------------------------------------------------------
def test_instantiation_rule_is_the_launchers():
    for N in range(1, 257):
        i = 0
        while (1 << i) < N:     # launch_generic (csrc/selective_scan.hip): kernels[i], 64 >> min(i, 6) rows per wave
            i += 1
        assert rl.instantiation(N) == rl.INSTANTIATIONS[i], N
        assert 64 // rl.instantiation(N)[0] == 64 >> min(i, 6)
    assert len(rl.INSTANTIATIONS) == 9


def test_scan_table_covers_its_axes():
    assert len({c["id"] for c in SCAN}) == len(SCAN)
    assert all(c["kernel_name"] == "scan_generic" and rl.turned_away(c) for c in SCAN)
    for kind in rl.KINDS:
        mine = [c for c in SCAN if c["kind"] == kind]
        assert {c["bck"] for c in mine} == ({"f32"} if kind == "f32" else {kind, "f32"}), kind
        # every instantiation twice: at its power of two and at a dstate that leaves lanes or states of it unused (n_ok)
        assert {c["N"] for c in mine} >= set(rl.DSTATES)
        for inst in rl.INSTANTIATIONS:
            ns = [c["N"] for c in mine if c["sec"] == "dstate" and c["inst"] == inst]
            assert len(ns) >= 2 and max(ns) == inst[0] * inst[1] and (max(ns) // 2 < min(ns) < max(ns) or max(ns) <= 2), (kind, inst, ns)
        # rows: one row, and a row count that is no multiple of the rows per wave, for every instantiation of fewer than 64 lanes per row
        for lanes in (1, 2, 4, 8, 16, 32):
            rows = {c["B"] * c["dim"] for c in mine if c["inst"][0] == lanes}
            assert 1 in rows and any(r > 1 and r % (64 // lanes) for r in rows), (kind, lanes, rows)
        assert any(c["B"] == 1 and c["dim"] == 1 for c in mine) and any((c["B"], c["dim"]) == (1, 3) for c in mine) and any((c["B"], c["dim"]) == (3, 6) for c in mine)
        # B / C forms, groups, how they are passed
        assert {(c["bform"], c["cform"]) for c in mine} == set(rl.BC_FORMS)
        var = [c for c in mine if "var" in (c["bform"], c["cform"])]
        assert {c["G"] for c in var} >= {1, 2, 3} and any(c["G"] == c["dim"] > 1 for c in var), kind
        assert {c["bc_layout"] for c in var} == {"3d", "4d_pad", "cols"} and any(c["bc_layout"] == "3d" and c["api"].startswith("fn") for c in var)
        const = [c for c in mine if "const" in (c["bform"], c["cform"])]
        assert {c["const_t"] for c in const} == {True, False}
        # layouts
        assert {c["layout"] for c in mine} == {"ref", "tok"} and any(c["layout"] == "ref" and not c["views"] for c in mine)
        tok = [c for c in mine if c["sec"] == "tokview"]
        reasons = {r for c in tok for r in rl.turned_away(c)}
        assert reasons >= {"dim % 64", "groups"} and (kind == "f32" or "bc_dtype" in reasons), (kind, reasons)
        assert {c["dim"] for c in tok} >= {96, 136} and all(c["layout"] == "tok" for c in tok)
        for why in reasons:
            assert {c["tables"] for c in tok if why in rl.turned_away(c)} == {True, False}, (kind, why)
        assert any(c["bck"] == "f32" and c["N"] == 16 and c["dim"] % 64 == 0 and c["G"] == 1 for c in tok) or kind == "f32"
        assert {(c["layout"], c["olayout"]) for c in mine} >= {("ref", "ref"), ("tok", "tok"), ("ref", "tok"), ("tok", "ref")}, kind
        assert {c["views"] for c in mine} == {True, False} and {c["tables"] for c in mine} == {True, False}
        # switches
        assert {(c["bias"], c["softplus"]) for c in mine} == PAIRS and {c["z"] for c in mine} == {True, False} == {c["D"] for c in mine}
        assert any(c["z"] and not c["both"] and c["api"] == "raw" for c in mine) and any(c["both"] and c["api"] == "raw" for c in mine)
        assert {c["api"] for c in mine} == {"raw", "fn", "fn_last", "cuda_fwd"}
        # lengths and carries
        assert {c["L"] for c in mine if not c["chunk"]} >= set(rl.SHORT_L) | set(rl.LONG_L)
        ch = [c for c in mine if c["chunk"]]
        assert {(c["L"], c["chunk"]) for c in ch} == {(L, k) for L in rl.CHUNK_L for k in rl.CHUNKS} and all(c["api"] == "raw" and c["carries"] for c in ch)
        counts = {-(-c["L"] // c["chunk"]) for c in ch}
        assert {1, 2, 7} <= counts and max(counts) == 7 and any(c["L"] % c["chunk"] for c in ch) and any(c["L"] % c["chunk"] == 0 for c in ch)
        long = [c for c in mine if c["sec"] == "long"]
        assert [c["L"] for c in long] == list(rl.LONG_L) and all(c["B"] * c["dim"] <= 8 and c["carries"] and c["api"] in ("cuda_fwd", "fn_last") for c in long)
        assert {c["regime"] for c in mine} == set(rl.REGIMES)
        for sec in ("dstate", "tokview", "chunks"):
            assert {c["regime"] for c in mine if c["sec"] == sec} == set(rl.REGIMES), (kind, sec)
    assert {(c["L"], c["api"]) for c in SCAN if c["sec"] == "long"} == {(L, a) for L in rl.LONG_L for a in ("cuda_fwd", "fn_last")}
    for c in SCAN:
        if c["tables"] and c["L"] > 1:
            inp = rl.scan_inputs(c)
            assert sorted(inp["zi"].tolist()) == list(range(c["L"])) == sorted(inp["oi"].tolist()) and not np.array_equal(inp["zi"], inp["oi"]), c["id"]
        if c["carries"]:
            assert rl.scan_reference(c, rl.scan_inputs(c))["x_state"].shape[2] == -(-c["L"] // rl.chunk_len(c)), c["id"]


@pytest.mark.parametrize("kind", rl.KINDS)
def test_edges_regime_reaches_every_edge(kind):
    bands = dict(below_pass=0, above_pass=0, switch=0, zero=0, u_zero=0, z_neg=0, dead_state=0)
    for c in SCAN:
        if c["regime"] != "edges" or c["kind"] != kind:
            continue
        inp = rl.scan_inputs(c)
        for k in ("u", "delta", "z"):       # every operand survives its round trip
            if inp[k] is not None:
                assert np.array_equal(rl.round_to(inp[k], kind), inp[k]) and np.abs(inp[k]).max() < 65504.0, (c["id"], k)
        if c["softplus"]:
            pre = rl.pre_softplus(c, inp)
            bands["below_pass"] += int(((pre > 19.5) & (pre <= 20.0)).sum())
            bands["above_pass"] += int(((pre > 20.0) & (pre < 20.5)).sum())
            bands["switch"] += int(((pre > -6.0) & (pre < -3.0)).sum())
            bands["zero"] += int((pre < -17.0).sum())
        bands["u_zero"] += int((np.abs(inp["u"]).max(-1) == 0).sum())
        if c["z"]:
            bands["z_neg"] += int((inp["z"] <= -29.0).sum())
        bands["dead_state"] += int((rl.step_sizes(c, inp)[..., None] * inp["A"][None, :, None] < -100.0).sum())     # exp(delta A) = 0 to fp32
    assert bands.pop("u_zero") >= 3 and all(v > 20 for v in bands.values()), bands       # (u_zero: whole channels)


def test_conv_table_covers_its_axes():
    assert len({c["id"] for c in CONV}) == len(CONV)
    for kind in rl.KINDS:
        mine = [c for c in CONV if c["kind"] == kind]
        tok, gen = [c for c in mine if c["kernel_name"] == "conv_tok"], [c for c in mine if c["kernel_name"] == "conv_generic"]
        for part in (tok, gen):
            assert {c["wkind"] for c in part} == ({"f32"} if kind == "f32" else {kind, "f32"}), kind
            assert {c["W"] for c in part} == {2, 3, 4} and {c["silu"] for c in part} == {True, False} == {c["bias"] for c in part}
            assert {c["tab"] for c in part} == {True, False} and {c["api"] for c in part} == {"raw", "fn"}
        assert {c["dim"] for c in tok} == set(rl.CONV_TOK_DIM) and {c["L"] for c in tok if not c["reset"]} == set(rl.CONV_TOK_L)
        assert {c["layout"] for c in tok} == {"tok", "half"}
        rs = [c for c in tok if c["reset"]]
        assert {c["reset"] for c in rs} == set(rl.CONV_RESET) and {c["L"] // c["reset"] for c in rs} == {2, 3, 4} and all(c["L"] % c["reset"] == 0 for c in rs)
        for period in rl.CONV_RESET:
            assert {c["tab"] for c in rs if c["reset"] == period} == {True, False}
        assert {c["layout"] for c in gen} == {"cf", "cl", "x_off", "out_off", "pitch"}
        assert {c["dim"] for c in gen if c["layout"] == "cl"} == {6, 70} and all(c["dim"] % 4 for c in gen if c["layout"] == "cl")
        for lay in ("cf", "cl"):
            assert {c["tab"] for c in gen if c["layout"] == lay} == {True, False}, (kind, lay)
            sizes = [c["B"] * c["dim"] * c["L"] for c in gen if c["layout"] == lay]
            assert min(sizes) < 256 < max(sizes) and any(s % 256 for s in sizes if s > 256)
    for c in CONV:
        if c["tab"]:
            rows, period = rl.conv_inputs(c)["rows"], c["reset"] or c["L"]
            assert sorted(rows.tolist()) == list(range(c["L"])) and (rows // period == np.arange(c["L"]) // period).all(), c["id"]
            assert c["L"] < 2 or not np.array_equal(rows, np.arange(c["L"])), c["id"]


# ---------------------------------------------------------------------------------------------------
# reference vs an independent restatement; rounding model
# ---------------------------------------------------------------------------------------------------
def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def _restated(c, inp):
    pre = rl.pre_softplus(c, inp)
    step = torch.nn.functional.softplus(torch.from_numpy(pre)) if c["softplus"] else torch.from_numpy(pre)
    gate = None if inp["z"] is None else torch.nn.functional.silu(_t(inp["z"]).double())
    r = ks.torch_scan_ref_layout(_t(inp["u"]), step, _t(inp["A"]), _t(inp["Bm"]), _t(inp["Cm"]), _t(inp["D"]), gate, _t(inp["zi"]), _t(inp["oi"]),
                                 chunk=rl.chunk_len(c) if c["carries"] else 0)
    return {"out": r["y"], "out_z": r["y_gated"], "x_prod": r["x_prod"], "x_state": r["x_state"]}


def scan_model_needs(c, inp, ref):
    m = rl.scan_reference(c, inp, dt=np.float32)
    return {k: rl.model_excess(k, v, ref[k], rl.out_kind(c, k)) for k, v in m.items()}


@pytest.mark.parametrize("c", SCAN, ids=_ids(SCAN))
def test_scan_reference_restatement_and_rounding_model(c):
    inp = rl.scan_inputs(c)
    ref, again = rl.scan_reference(c, inp), _restated(c, inp)
    assert set(ref) == ({"out_z"} if c["z"] and not c["both"] else {"out", "out_z"} if c["z"] else {"out"}) | ({"x_prod", "x_state"} if c["carries"] else set())
    for key, want in ref.items():
        assert np.isfinite(want).all() and want.dtype == np.float64, (c["id"], key)
        e = rl.norm_err(want, again[key].numpy())
        assert e < 1e-12 or np.linalg.norm(want) == 0.0 == float(again[key].norm()), (c["id"], key, e)
        n = rl.need(key, rl.round_to(want, rl.out_kind(c, key)), want)     # the reference rounded to the type it is stored in: < 0.9 x every limit
        assert n < 0.9 * rl.base_bound(c, key), (c["id"], key, n, "ref_layout_cases.RESEED")
        assert np.abs(want).max() < 65504.0, (c["id"], key, "a correct output would overflow fp16")
    for key, (excess, d_model) in scan_model_needs(c, inp, ref).items():        # the fp32 model: <= 1/2 x every limit, or the raised bound covers 2 x d_model
        assert d_model < rl.bound_of(c, key), (c["id"], key, d_model)
        if key in rl.RAISED.get(c["id"], {}):
            assert 2.0 * d_model <= rl.bound_of(c, key), (c["id"], key, d_model, rl.bound_of(c, key))
        else:
            assert excess <= 0.5 * rl.base_bound(c, key), (c["id"], key, excess, "the case needs an entry in ref_layout_cases.RAISED")


def test_raised_table_keeps_its_conditions():
    by_id = {c["id"]: c for c in SCAN}
    assert set(rl.RESEED) <= set(by_id) and len(rl.RESEED) <= 0.1 * len(SCAN)
    assert set(rl.RAISED) <= set(by_id) and len(rl.RAISED) <= rl.RAISED_SHARE * len(SCAN)
    for cid, keys in rl.RAISED.items():
        c = by_id[cid]
        assert c["regime"] in rl.RAISED_REGIMES, cid
        inp = rl.scan_inputs(c)
        needs = scan_model_needs(c, inp, rl.scan_reference(c, inp))
        for key, b in keys.items():
            excess, d_model = needs[key]
            assert excess > 0.5 * rl.base_bound(c, key) and 2.0 * d_model <= b <= 2.5 * d_model and b <= rl.RAISED_FACTOR * rl.base_bound(c, key), (cid, key, excess, d_model, b)


@pytest.mark.parametrize("c", CONV, ids=_ids(CONV))
def test_conv_reference_restatement_and_rounding_model(c):
    inp, bound, F = rl.conv_inputs(c), rl.IO_BOUND[c["kind"]], torch.nn.functional
    ref = rl.conv_reference(c, inp)["conv"]
    x, w = _t(inp["x"]).double(), _t(inp["w"]).double()
    if inp["rows"] is not None:
        x = x.index_select(2, _t(inp["rows"]).long())
    period, W = c["reset"] or c["L"], c["W"]
    parts = [F.conv1d(F.pad(x[:, :, a:a + period], (W - 1, 0)), w[:, None], None if inp["b"] is None else _t(inp["b"]).double(), groups=c["dim"])
             for a in range(0, c["L"], period)]
    y = torch.cat(parts, -1)
    assert rl.norm_err(ref, (F.silu(y) if c["silu"] else y).numpy()) < 1e-12, c["id"]
    if c["regime"] == "edges" and c["bias"] and c["silu"] and c["dim"] >= 4:
        assert {12.0, -12.0, 30.0, -30.0} <= set(np.round(y.numpy()[0, :4, 0]).tolist()), c["id"]
    assert rl.need("conv", rl.round_to(ref, c["kind"]), ref) < 0.9 * bound and np.abs(ref).max() < 65504.0, c["id"]
    excess, d_model = rl.model_excess("conv", rl.conv_reference(c, inp, dt=np.float32)["conv"], ref, c["kind"])
    assert excess <= 0.5 * bound and d_model < bound, (c["id"], excess, d_model)


# ---------------------------------------------------------------------------------------------------
# tests/test_gpu_ref_layout.py on the CPU: float64 stand-ins at the C ABI, the plans compiled with g++ name the kernel
# ---------------------------------------------------------------------------------------------------
from test_host_cpu import front_plan, scan_plan  # noqa: E402,F401  (the module-scoped fixtures)


@pytest.fixture
def gpu_file(monkeypatch, scan_plan, front_plan):  # noqa: F811
    import test_gpu_ref_layout as gf
    ks.install_lib_call(monkeypatch, scan_plan, front_plan)
    monkeypatch.setattr(gf, "DEV", "cpu")
    return gf


@pytest.mark.parametrize("c", SCAN, ids=_ids(SCAN))
def test_gpu_scan_checks_pass_on_the_stand_in(c, gpu_file, capsys):
    """... and with them: plan_scan() (compiled) serves every case with scan_generic, none with a token-major kernel"""
    run = gpu_file.check_scan_case(c)
    assert run["kernel"] == "scan_generic" and f"ref-layout-sweep {c['id']}: " in capsys.readouterr().out


@pytest.mark.parametrize("c", CONV, ids=_ids(CONV))
def test_gpu_conv_checks_pass_on_the_stand_in(c, gpu_file, capsys):
    """... and with them: plan_conv1d() (compiled) names the kernel the case states"""
    assert gpu_file.check_conv_case(c)["kernel"] == c["kernel_name"] and f"ref-layout-sweep {c['id']}: conv" in capsys.readouterr().out


# generic leaves of tests/scan_plan_cases.py -> the cases of the table that reach the same leaf of plan_scan
GENERIC_LEAVES = {
    "generic_reference_layout": lambda c: c["layout"] == "ref" and c["L"] > 1 and c["kind"] == "bf16" and (c["bform"], c["cform"]) == ("var", "var"),
    "generic_constant_bc": lambda c: (c["bform"], c["cform"]) == ("const", "const"),
    "generic_groups2": lambda c: c["G"] == 2,
    "generic_dstate32": lambda c: c["N"] == 32,
}


def test_every_generic_leaf_of_the_plan_is_hit(gpu_file):
    import scan_plan_cases as spc
    assert {name for name, (_, want) in spc.CASES.items() if want.family == spc.GEN} == set(GENERIC_LEAVES)
    for name, hit in GENERIC_LEAVES.items():
        mine = [c for c in SCAN if hit(c)]
        assert len(mine) >= 3 and spc.CASES[name][1].kernel == "scan_generic", name
        for c in mine[:3]:          # (every case goes through the compiled plan in test_gpu_scan_checks_pass_on_the_stand_in)
            run = gpu_file.scan_run(c, rl.scan_inputs(c))
            assert run["kernel"] == "scan_generic" and all(t[1] == "scan_generic" for t in run["trace"]), (name, c["id"])


def _fails_some(check, cases):
    for c in cases:
        try:
            check(c)
        except AssertionError:
            return c["id"]
    return None


def test_mutated_scan_stand_ins_turn_a_case_red(gpu_file, monkeypatch, capsys):
    """a stand-in that drops the last state when dstate is no power of two, one that reads group 0 for every channel, one whose surplus lanes of the
    last wave store their carry one row further: the table sees each"""
    real, real_fwd = ks.torch_scan_ref_layout, ks._scan_generic_fwd

    def drops_last_state(u, step, A, Bm, Cm, *a, **kw):
        N = A.shape[1]
        if N & (N - 1):         # B of the last state is zero: the state stays zero and y misses its term
            Bm = Bm.clone()
            Bm.select(-2 if Bm.dim() == 4 else -1, N - 1).zero_()
        return real(u, step, A, Bm, Cm, *a, **kw)

    def group_0(u, step, A, Bm, Cm, *a, **kw):
        Bm, Cm = (M[:, :1] if M.dim() == 4 else M for M in (Bm, Cm))
        return real(u, step, A, Bm, Cm, *a, **kw)
    for bad, cases in ((drops_last_state,[c for c in SCAN if c["N"] & (c["N"] - 1)]), (group_0, [c for c in SCAN if c["G"] > 1])):
        monkeypatch.setattr(ks, "torch_scan_ref_layout", bad)
        assert _fails_some(gpu_file.check_scan_case, cases[:12]), bad.__name__
    monkeypatch.setattr(ks, "torch_scan_ref_layout", real)

    def writes_the_clamped_row(P, got):
        kernel = real_fwd(P, got)
        rows, rpw = P.batch * P.dim, 64 // rl.instantiation(P.dstate)[0]
        if P.x and rows % rpw:
            nc = -(-P.seqlen // (P.chunk_len if P.chunk_len > 0 else 2048))
            x = ks._view(P.x, (rows + 1, nc * 2 * P.dstate), (nc * 2 * P.dstate, 1), torch.float32)
            x[rows] = x[rows - 1]
        return kernel
    monkeypatch.setattr(ks, "_scan_generic_fwd", writes_the_clamped_row)
    spilled = [c for c in SCAN if c["api"] == "raw" and c["carries"] and (c["B"] * c["dim"]) % (64 // c["inst"][0])]
    assert len(spilled) >= 5 and _fails_some(gpu_file.check_scan_case, spilled[:3]) == spilled[0]["id"]
    monkeypatch.setattr(ks, "_scan_generic_fwd", real_fwd)
    gpu_file.check_scan_case(spilled[0])


def test_mutated_conv_stand_in_and_wrong_rows_turn_a_case_red(gpu_file, monkeypatch, capsys):
    """a conv that ignores reset_period; one output row 3 % off in a scan and in a conv; a write into the surroundings of an output"""
    real = ks.torch_conv1d
    monkeypatch.setattr(ks, "torch_conv1d", lambda x, w, b, silu, rows=None, reset=0: real(x, w, b, silu, rows, 0))
    assert _fails_some(gpu_file.check_conv_case, [c for c in CONV if c["reset"]][:3])

    def wrong_row(*a, **kw):
        y = real(*a, **kw)
        y[0, :, int(y[0].norm(dim=0).argmax())] *= 1.03        # (a row of at least the rms row norm: the metric's floor)
        return y
    monkeypatch.setattr(ks, "torch_conv1d", wrong_row)
    with pytest.raises(AssertionError):
        gpu_file.check_conv_case(max((c for c in CONV if c["kind"] == "bf16"), key=lambda c: c["dim"] * c["L"]))
    monkeypatch.setattr(ks, "torch_conv1d", real)
    real_scan = ks.torch_scan_ref_layout

    def wrong_channel_row(*a, **kw):
        r = real_scan(*a, **kw)
        for k in ("y", "y_gated"):
            if r[k] is not None:
                r[k][0, int(r[k][0].norm(dim=1).argmax())] *= 1.03
        return r
    c = max((c for c in SCAN if c["sec"] == "tokview" and c["kind"] == "bf16"), key=lambda c: c["dim"] * c["L"])
    monkeypatch.setattr(ks, "torch_scan_ref_layout", wrong_channel_row)
    with pytest.raises(AssertionError):
        gpu_file.check_scan_case(c)
    monkeypatch.setattr(ks, "torch_scan_ref_layout", real_scan)
    c = next(c for c in CONV if c["layout"] == "half" and c["api"] == "raw")
    real_run = gpu_file.conv_run

    def spill(c, inp):
        run = real_run(c, inp)
        run["slots"]["out"].buf[0, 0, -1] = 1.0
        return run
    monkeypatch.setattr(gpu_file, "conv_run", spill)
    with pytest.raises(AssertionError, match="outside"):
        gpu_file.check_conv_case(c)


if __name__ == "__main__":
    table = {}
    for case in SCAN:
        inputs = rl.scan_inputs(case)
        needs = scan_model_needs(case, inputs, rl.scan_reference(case, inputs))
        over = {k: float(f"{2.2 * d:.3g}") for k, (excess, d) in needs.items() if excess > 0.5 * rl.base_bound(case, k)}
        if over:
            table[case["id"]] = over
            print(f"# {case['id']}: " + ", ".join(f"{k} excess {needs[k][0] / rl.base_bound(case, k):.2f} x base, d_model {needs[k][1] / rl.base_bound(case, k):.2f} x base" for k in over), file=sys.stderr)
    print("RAISED = {")
    for cid, v in table.items():
        print(f"    {cid!r}: {v!r},")
    print("}")

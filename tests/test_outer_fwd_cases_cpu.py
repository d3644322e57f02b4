"""CPU checks of the case tables of tests/outer_fwd_cases.py (add-norm forward, patch_embed, timestep_embed, skinny_linear, final_layer).
Coverage: every axis value the tables are meant to hold, every instantiation of add_norm_kernel in each 16-bit type (launch_norm's selection
restated twice, on the case's parameters and on the parameter block the GPU file builds), every templated form of the other kernels, unique ids.
Reference: it agrees to < 1e-12 with an independent float64 torch restatement (F.layer_norm, F.linear, unfold + matmul, the model's own
timestep_embedding: tests/kernel_standins.py).  Rounding model: the fp32 numpy model of every case, rounded to the I/O type, stays within
HALF of every norm-wise and row-wise limit and within DELTA_FLIPS_MODEL element-wise; no case has a raised bound.  Known answers are exact in
fp32.  And every function of tests/test_gpu_outer_fwd.py runs here against the float64 stand-ins served at the C ABI.

`python tests/test_outer_fwd_cases_cpu.py` prints what the model measured per kernel and the timestep floor (outer_fwd_cases.TS_ABS_FLOOR)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]      # (run as a script)
import kernel_standins as ks  # noqa: E402
import outer_fwd_cases as oc  # noqa: E402

NORM, PATCH, TIMESTEP, SKINNY, FINAL = oc.norm_cases(), oc.patch_cases(), oc.timestep_cases(), oc.skinny_cases(), oc.final_cases()
NORM_P, PATCH_P, SKINNY_P, FINAL_P = oc.norm_production_cases(), oc.patch_production_cases(), oc.skinny_production_cases(), oc.final_production_cases()
RAISED = {}             # id -> bound: stays empty (a case whose model needs more than half a limit gets other inputs, not another limit)
_ids = lambda cases: [c["id"] for c in cases]
_t = lambda a: None if a is None else torch.from_numpy(np.asarray(a, np.float64))


# ---------------------------------------------------------------------------------------------------
# coverage
# ---------------------------------------------------------------------------------------------------
def test_ids_are_unique_and_no_bound_is_raised():
    every = NORM + PATCH + TIMESTEP + SKINNY + FINAL + NORM_P + PATCH_P + SKINNY_P + FINAL_P
    assert len({(c["kernel"], c["id"]) for c in every}) == len(every)
    assert RAISED == {}
    assert oc.IO_BOUND == {"f32": 2e-5, "bf16": 2.5e-3, "f16": 2.5e-3 / 8} and (oc.DELTA_FLIPS, oc.DELTA_FLIPS_MODEL, oc.ROW_GUARD) == (0.02, 0.01, 4.0)


def test_norm_table_covers_its_axes():
    assert {(c["xk"], c["rk"], c["wk"]) for c in NORM} == set(oc.NORM_DTYPES)
    assert {(c["xk"], c["rk"], c["wk"], c["cols"]) for c in NORM} >= {(*t, cols) for t in oc.NORM_DTYPES for cols in oc.NORM_COLS}
    assert {c["rows"] for c in NORM} >= set(oc.NORM_ROWS) and {c["form"] for c in NORM} == set(oc.NORM_FORMS) and {c["opt"] for c in NORM} == set(oc.NORM_OPTIONS)
    for xk in ("f32", "bf16", "f16"):
        mine = [c for c in NORM if c["xk"] == xk]
        assert {c["form"] for c in mine} == set(oc.NORM_FORMS) and {c["opt"] for c in mine} == set(oc.NORM_OPTIONS), xk
        if xk != "f32":
            assert {(c["form"], c["opt"]) for c in mine} == {(f, o) for f in oc.NORM_FORMS for o in oc.NORM_OPTIONS}, xk
        assert {c["regime"] for c in mine} == set(oc.REGIMES) and {c["align"] for c in mine} == {0, 4, 1}
        assert {c["rpb"] for c in mine} >= {1, 3, 6} and any(c["rpb"] == c["rows"] for c in mine)
    for xk in ("bf16", "f16"):          # every instantiation in each 16-bit type; fp32 x has no 16-byte form
        mine = [c for c in NORM if c["xk"] == xk]
        assert {c["branch"] for c in mine} == set(oc.NORM_INSTANTIATIONS), xk
        four = [c for c in mine if c["branch"][2] == 16]
        assert {c["cols"] // 128 for c in four} == set(range(1, 9)) and {c["rows"] for c in four} == {4, 8, 12, 2052}
        assert any(c["rows"] == 12 and c["rpb"] == 6 for c in four), "two samples inside one wave"
        assert {c["opt"] for c in four} == set(oc.NORM_OPTIONS) and {c["form"] for c in four} == set(oc.NORM_FORMS)
        assert {c["cols"] // 128 for c in mine if c["flags"] == 1 and c["branch"] == (8, 2, 64)} == set(range(1, 9))
        assert any(c["form"] == "ln-wb" and c["opt"].startswith("full") and c["branch"][2] == 16 for c in mine), "LayerNorm with a bias on the fused form"
    assert {c["branch"] for c in NORM if c["xk"] == "f32"} == {(4, 4, 64), (4, 16, 64), (1, 16, 64), (1, 64, 64)}
    assert [(c["rows"], c["cols"], c["rpb"], c["xk"], c["rk"], c["opt"]) for c in NORM_P] == [(2048, cc, 1024, "bf16", "f32", "full") for cc in (640, 768)]
    hit = dict(mean100=0, zero=0, eps=0, pm4=0)
    for c in NORM:
        if c["regime"] != "edges":
            continue
        inp = oc.norm_inputs(c)
        if inp["residual"] is not None and c["form"] != "rms":
            hit["mean100"] += int((np.abs(inp["residual"].mean(-1) - 100.0) < 1.0).any())
        hit["zero"] += int((np.abs(inp["x"]).max(-1) == 0).any())
        hit["eps"] += int(c["form"] == "rms" and ((np.abs(inp["x"]).max(-1) < 1e-3) & (np.abs(inp["x"]).max(-1) > 0)).any())
        hit["pm4"] += int(inp["mod"] is not None and c["cols"] >= 4 and (np.nan_to_num(inp["mod"]) == 4.0).any() and (np.nan_to_num(inp["mod"]) == -4.0).any())
    assert all(v >= 5 for v in hit.values()), hit
    c = next(c for c in NORM if c["regime"] == "model" and c["rk"] == "f32" and c["xk"] != "f32" and oc.norm_uses(c)["res"])
    inp = oc.norm_inputs(c)
    assert 20.0 < inp["residual"].std() < 40.0 and 0.8 < inp["x"].std() < 1.3


def test_other_tables_cover_their_axes():
    pe = [c for c in PATCH if not c["known"]]
    assert {(c["C"], c["p"]) for c in pe} == set(oc.PE_CP) == {(c["C"], c["p"]) for c in PATCH if c["known"]}
    assert {c["K"] for c in pe} == {1, 3, 4, 12, 16, 20, 48, 64}
    assert {(c["K"], c["E"]) for c in pe} >= {(C * p * p, E) for C, p in oc.PE_CP for E in oc.PE_E if C * p * p * E * 4 <= 65536}
    assert any(c["K"] * c["E"] * 4 == 65536 for c in pe) and {c["E"] for c in pe} == set(oc.PE_E)
    assert {c["L"] for c in pe} >= {1, 9, 15, 16, 17, 33, 120, 289, 1089, 16641} and {c["B"] for c in pe} == set(oc.PE_BATCH)
    assert sum(c["gh"] != c["gw"] for c in pe) * 2 >= len(pe) and any((c["gh"], c["gw"]) == (3, 40) for c in pe)
    assert {(c["B"], c["L"]) for c in pe if c["L"] > 256} == {(64, 289), (8, 1089), (1, 16641)}
    assert all(c["E"] == 8 for c in pe if c["L"] == 16641)
    assert {(c["bias"], c["pos"]) for c in pe} == {(b, q) for b in (True, False) for q in oc.PE_POS}
    assert [(c["B"], c["C"], c["gh"], c["gw"], c["p"], c["E"]) for c in PATCH_P] == [(64, 3, 32, 32, 1, 640)]
    assert {(c["dim"], c["B"]) for c in TIMESTEP} == {(d, b) for d in oc.TS_DIM for b in oc.TS_BATCH}
    for d in oc.TS_DIM:
        assert {c["pitch"] > 0 for c in TIMESTEP if c["dim"] == d} == {True, False}, d
    seen = set()
    for c in TIMESTEP:
        seen |= set(oc.timestep_inputs(c)["t"].tolist())
    assert seen >= {0.0, 2.0 ** -20, 1.0, 1000.0, float(oc.round_to([999.0], "bf16")[0])}
    sk = [c for c in SKINNY if not c["known"]]
    assert {(c["k"], c["n"]) for c in sk} >= {(k, n) for k in oc.SK_K for n in oc.SK_N} | {(128, n) for n in oc.SK_WIDE}
    assert {c["k"] for c in SKINNY if c["known"]} == set(oc.SK_K) and all(not c["silu"] for c in SKINNY if c["known"])
    for side in (lambda k: k <= 640, lambda k: k > 640):          # two strips in registers | one
        assert {c["m"] for c in sk if side(c["k"])} == set(oc.SK_M)
        assert {(c["silu"], c["bias"]) for c in sk if side(c["k"])} == {(a, b) for a in (True, False) for b in (True, False)}
    assert {(c["n"] // 16 // 2048, c["n"] // 16 % 2048) for c in sk if c["n"] in oc.SK_WIDE} == {(j, r) for j in (1, 2, 3, 4) for r in (0, 1, 7)}
    assert {c["views"] for c in sk} == {True, False} and [(c["m"], c["k"], c["n"]) for c in SKINNY_P] == list(oc.SK_PRODUCTION)
    assert {(c["cols"], c["n_out"]) for c in FINAL} >= {(a, b) for a in oc.FL_COLS for b in oc.FL_NOUT} and {c["rows"] for c in FINAL} >= set(oc.FL_ROWS)
    assert {c["np"] for c in FINAL} == {5, 8, 16} and {c["cols"] for c in FINAL if c["np"] == 8} == {648, 768, 1024}
    assert {(c["bias"], c["regime"]) for c in FINAL} == {(b, r) for b in (True, False) for r in oc.FL_REGIMES}
    assert any(c["rows"] > 65536 and c["cols"] == 64 for c in FINAL) and [(c["rows"], c["cols"], c["n_out"]) for c in FINAL_P] == [(65536, 640, 3)]
    want = {("zigma_add_norm_fwd", w) for w in ("cols4097", "gate-without-branch", "shift-without-ymod", "mod-dtype")}
    want |= {(e, k) for e in ("zigma_patch_embed_fwd", "zigma_timestep_embed_fwd", "zigma_skinny_linear_fwd", "zigma_final_layer_fwd") for k in ("f16", "f32")}
    want |= {("zigma_skinny_linear_fwd", w) for w in ("m65", "k1152", "n24", "x-off-by-one")} | {("zigma_final_layer_fwd", w) for w in ("n_out17", "cols2056")}
    assert {(e, w) for e, w, _ in oc.REFUSALS} >= want | {("zigma_patch_embed_fwd", "above-64KB")}


# ---------------------------------------------------------------------------------------------------
# reference vs the torch restatement; the rounding model
# ---------------------------------------------------------------------------------------------------
MEASURED = {}           # (kernel, I/O kind, output) -> worst (excess / bound) of the fp32 model: printed by __main__


def _pin(ident, key, ref, again):
    e = oc.norm_err(ref, again.numpy()) if np.linalg.norm(ref) > 0 else float(again.norm())
    assert e < 1e-12, (ident, key, e)


def _model(c, key, model, ref, kind, terms=None):
    bound = oc.IO_BOUND[kind]
    assert np.isfinite(ref).all() and np.abs(ref).max() < 65504.0, (c["id"], key)
    assert oc.need(oc.round_to(ref, kind), ref, terms) < bound, (c["id"], key, "the rounded reference itself")
    if not np.linalg.norm(ref):
        assert not np.asarray(model).any(), (c["id"], key)
        return
    excess, d_model = oc.model_excess(model, ref, kind, terms)
    slot = (c["kernel"], kind, key)
    MEASURED[slot] = max(MEASURED.get(slot, 0.0), excess / bound)
    assert excess <= 0.5 * bound and d_model < bound, (c["id"], key, excess, d_model, bound, "change the case's inputs, not the limit")


@pytest.mark.parametrize("c", NORM + NORM_P, ids=_ids(NORM + NORM_P))
def test_norm_reference_and_rounding_model(c):
    inp, u = oc.norm_inputs(c), oc.norm_uses(c)
    ref, m32 = oc.norm_reference(c, inp), oc.norm_reference(c, inp, np.float32)
    win = lambda k, on: _t(oc.mod_window(c, inp, k)) if on else None
    xdt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[c["xk"]]
    again = ks.torch_add_norm(_t(inp["x"]), _t(inp["branch"]), win(2, u["branch"]), _t(inp["residual"]), _t(inp["weight"]), _t(inp["bias"]), win(0, u["mod"]),
                              win(1, u["mod"]), oc.EPS, c["form"] == "rms", xdt)
    keys = [k for k in ref if not k.startswith("_")]
    assert set(keys) == {k for k, on in (("x_out", u["x_out"]), ("residual_out", u["res_out"]), ("y_out", u["y_out"]), ("y_mod", u["mod"])) if on}
    for key in keys:
        _pin(c["id"], key, ref[key], again[key])
        _model(c, key, m32[key], ref[key], oc.norm_out_kind(c, key), ref["_terms"] if key == "y_mod" else None)
    exact, exact32 = oc.norm_exact(c, ref), oc.norm_exact(c, m32)
    assert set(exact) == ({k for k in ("x_out", "residual_out") if k in ref} if c["xk"] != "f32" or not u["branch"] else set())
    for key, want in exact.items():         # the fp32 evaluation has the same bits: one defined value
        assert np.array_equal(want, exact32[key]), (c["id"], key)


@pytest.mark.parametrize("c", PATCH + PATCH_P, ids=_ids(PATCH + PATCH_P))
def test_patch_reference_and_rounding_model(c):
    c = dict(c, B=min(c["B"], 2)) if c in PATCH_P else c          # (the production shape: its first two samples' worth here)
    inp = oc.patch_inputs(c)
    ref = oc.patch_reference(c, inp)["out"]
    _pin(c["id"], "out", ref, ks.torch_patch_embed(_t(inp["x"]), _t(inp["w"]), _t(inp["bias"]), _t(inp["pos"])))
    m32 = oc.patch_reference(c, inp, np.float32)["out"]
    _model(c, "out", m32, ref, "bf16")
    if c["known"]:
        assert np.array_equal(m32.astype(np.float64), ref) and np.array_equal(oc.round_to(ref, "bf16").astype(np.float64), ref) and np.abs(ref).max() > 8
        assert len(np.unique(inp["w"].reshape(c["E"], -1), axis=0)) > min(c["E"], 3 ** c["K"]) // 2


@pytest.mark.parametrize("c", TIMESTEP, ids=_ids(TIMESTEP))
def test_timestep_reference_and_rounding_model(c):
    inp = oc.timestep_inputs(c)
    ref = oc.timestep_reference(c, inp)["out"]
    assert ref.shape == (c["B"], c["dim"]) and inp["freqs"].shape == (c["dim"] // 2,) and np.array_equal(oc.round_to(inp["freqs"], "bf16"), inp["freqs"])
    _pin(c["id"], "out", ref, ks.torch_timestep_embed(_t(inp["t"]), _t(inp["freqs"]), c["dim"]))
    arg32 = inp["t"][:, None] * inp["freqs"][None]
    assert arg32.dtype == np.float32 and np.array_equal(arg32.astype(np.float64), inp["t"].astype(np.float64)[:, None] * inp["freqs"].astype(np.float64)[None])
    m32 = oc.timestep_reference(c, inp, np.float32)["out"]
    assert m32.dtype == np.float32
    _model(c, "out", m32, ref, "bf16")
    assert 4.0 * np.abs(m32.astype(np.float64) - ref).max() <= oc.TS_ABS_FLOOR, "the floor is 4 x the model's worst absolute error"
    rounded = oc.round_to(m32, "bf16")
    assert oc.timestep_worst(rounded, ref) <= 0.55 and oc.flipped_share(rounded, ref, "bf16") < oc.DELTA_FLIPS_MODEL, c["id"]


def test_timestep_floor_is_what_the_model_measured():
    worst = max(np.abs(oc.timestep_reference(c, i, np.float32)["out"].astype(np.float64) - oc.timestep_reference(c, i)["out"]).max()
                for c in TIMESTEP for i in [oc.timestep_inputs(c)])
    assert 4.0 * worst <= oc.TS_ABS_FLOOR <= 6.0 * worst, (worst, oc.TS_ABS_FLOOR)


@pytest.mark.parametrize("c", SKINNY + SKINNY_P, ids=_ids(SKINNY + SKINNY_P))
def test_skinny_reference_and_rounding_model(c):
    inp = oc.skinny_inputs(c)
    ref = oc.skinny_reference(c, inp)["out"]
    part = 4096 if c["n"] > 20000 else c["n"]       # (the restatement of the widest cases: their first 4096 features)
    again = ks.torch_skinny_linear(_t(inp["x"]), _t(inp["w"][:part]), None if inp["bias"] is None else _t(inp["bias"][:part]), c["silu"])
    _pin(c["id"], "out", ref[:, :part], again)
    m32 = oc.skinny_reference(c, inp, np.float32)["out"]
    _model(c, "out", m32, ref, "bf16")
    if c["known"]:
        assert np.array_equal(m32.astype(np.float64), ref) and np.array_equal(oc.round_to(ref, "bf16").astype(np.float64), ref) and np.abs(ref).max() > 8
        strips = inp["w"].reshape(c["n"] // 16, -1)
        assert len(np.unique(strips, axis=0)) == len(strips), "every strip has its own weight"
        assert (np.abs(inp["x"]).sum(-1) == 16).all()


@pytest.mark.parametrize("c", FINAL + FINAL_P, ids=_ids(FINAL + FINAL_P))
def test_final_reference_and_rounding_model(c):
    c = dict(c, rows=4096) if c in FINAL_P else c                 # (the production shape: 4096 rows' worth here)
    inp = oc.final_inputs(c)
    ref = oc.final_reference(c, inp)
    _pin(c["id"], "out", ref["out"], ks.torch_final_layer(_t(inp["x"]), _t(inp["w"]), _t(inp["bias"]), oc.FL_EPS))
    _model(c, "out", oc.final_reference(c, inp, np.float32)["out"], ref["out"], "bf16")
    if c["regime"] == "constant":
        const = np.ptp(inp["x"], axis=-1) == 0
        assert const.any() and (np.abs(ref["y"][const]).max() == 0) and (c["rows"] == 1 or not const.all())
    if c["regime"] == "mean50":
        assert 49.0 < inp["x"].mean() < 51.0 and 0.8 < inp["x"].std(-1).mean() < 1.3


# ---------------------------------------------------------------------------------------------------
# tests/test_gpu_outer_fwd.py on the CPU: float64 stand-ins at the C ABI
# ---------------------------------------------------------------------------------------------------
@pytest.fixture
def gpu_file(monkeypatch):
    import test_gpu_outer_fwd as gf
    ks.install_lib_call(monkeypatch)
    monkeypatch.setattr(gf, "DEV", "cpu")
    return gf


@pytest.mark.parametrize("c", NORM + NORM_P, ids=_ids(NORM + NORM_P))
def test_gpu_norm_checks_pass_on_the_stand_in(c, gpu_file, capsys):
    gpu_file.check_norm_case(c)
    assert ks.LAST_INSTANTIATION[0] == c["branch"], (c["id"], "the two restatements of launch_norm disagree")
    assert f"outer-sweep {c['id']}: " in capsys.readouterr().out


@pytest.mark.parametrize("c", PATCH + TIMESTEP + SKINNY + FINAL, ids=[f"{c['kernel']}-{c['id']}" for c in PATCH + TIMESTEP + SKINNY + FINAL])
def test_gpu_checks_pass_on_the_stand_in(c, gpu_file, capsys):
    gpu_file.CHECKS[c["kernel"]](c)
    assert f"outer-sweep {c['id']}: " in capsys.readouterr().out


@pytest.mark.parametrize("entry,what,status", oc.REFUSALS, ids=[f"{e[6:-4]}-{w}" for e, w, _ in oc.REFUSALS])
def test_gpu_refusals_pass_on_the_stand_in(entry, what, status, gpu_file):
    gpu_file.test_refusals(entry, what, status)


def test_gpu_checks_turn_red_on_a_wrong_row(gpu_file, monkeypatch):
    """one row of 65 559 taken with a stale statistic, one strip of 4103 without its bias, the sample index of a wave's first row, a write into the
    NaN surroundings: each is caught"""
    real_final, real_skinny, real_norm = ks.torch_final_layer, ks.torch_skinny_linear, ks.torch_add_norm

    def wrong_row(x, w, bias, eps):
        r = real_final(x, w, bias, eps)
        r[40000] = r[39999]
        return r

    def strip_without_bias(x, w, bias, silu):
        r = real_skinny(x, w, bias, silu)
        r[:, 16 * 4000:16 * 4001] -= bias[16 * 4000:16 * 4001]
        return r

    def first_rows_sample(x, branch, gate, *a):
        return real_norm(x, branch, None if gate is None else gate[(torch.arange(len(gate)) // 4) * 4], *a)
    big = next(c for c in FINAL if c["rows"] > 65536 and c["bias"])
    wide = next(c for c in SKINNY if c["n"] in oc.SK_WIDE and c["n"] >= 16 * 4096 and c["bias"] and not c["known"])
    two = next(c for c in NORM if c["branch"][2] == 16 and c["rows"] == 12 and c["rpb"] == 6 and oc.norm_uses(c)["x_out"])
    for name, bad, c in (("torch_final_layer", wrong_row, big), ("torch_skinny_linear", strip_without_bias, wide), ("torch_add_norm", first_rows_sample, two)):
        monkeypatch.setattr(ks, name, bad)
        with pytest.raises(AssertionError):
            gpu_file.CHECKS[c["kernel"]](c)
        monkeypatch.undo()
        ks.install_lib_call(monkeypatch)
        monkeypatch.setattr(gpu_file, "DEV", "cpu")
    real_run = gpu_file.final_run

    def spill(c, inp):
        w = real_run(c, inp)
        w["out"].buf[3, -1] = 1.0
        return w
    monkeypatch.setattr(gpu_file, "final_run", spill)
    with pytest.raises(AssertionError, match="surroundings"):
        gpu_file.check_final_case(FINAL[0] if FINAL[0]["rows"] > 3 else next(c for c in FINAL if c["rows"] > 3))


if __name__ == "__main__":
    for fn, cases in ((test_norm_reference_and_rounding_model, NORM + NORM_P), (test_patch_reference_and_rounding_model, PATCH + PATCH_P),
                      (test_skinny_reference_and_rounding_model, SKINNY + SKINNY_P), (test_final_reference_and_rounding_model, FINAL + FINAL_P)):
        for case in cases:
            try:
                fn(case)
            except AssertionError as err:
                print("FAILS", err)
    worst_abs = 0.0
    for case in TIMESTEP:
        i = oc.timestep_inputs(case)
        worst_abs = max(worst_abs, np.abs(oc.timestep_reference(case, i, np.float32)["out"].astype(np.float64) - oc.timestep_reference(case, i)["out"]).max())
    print(f"TS_ABS_FLOOR = {float(f'{4.4 * worst_abs:.2g}')!r}      # model's worst absolute error {worst_abs:.3e}")
    print("fp32 model, worst excess in units of the bound (limit 0.5):")
    for slot, v in sorted(MEASURED.items()):
        print(f"    {slot[0]:8s} {slot[1]:5s} {slot[2]:13s} {v:.3f}")
    print(f"RAISED = {RAISED!r}")

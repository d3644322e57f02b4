"""CPU checks of the case tables of tests/matmul_sweep_cases.py (linear_split_kernel behind zigma_linear_f32_split; wgrad_kernel and
wgrad_reduce_kernel behind zigma_linear_wgrad).
Coverage: the axis values the tables are meant to hold; every split cell passes x remap on / off x ragged / full x bias and every wgrad cell
BK x direct / split-K x output type x operand type is reached.  Restatements: the numpy split against zigma_amd.fp32_matmul.split bit for bit (and
float(hi) + float(lo) exact in fp32 and within 2^-16 |a| + 2^-134 of a over 10^6 random finite patterns); wgrad_bk / wgrad_slabs against zigma_linear_wgrad_workspace_bytes of
the built library, without a device.  References: pinned to < 1e-12 against independent float64 torch restatements (fp32_matmul.reference,
kernel_standins.torch_split_linear / torch_wgrad).  fp32 numpy model: needs less than HALF of every limit on every case (norm-wise before the
output rounding, row- and element-wise after it), and the rounded reference itself passes; no bound is raised, no seed was moved.  And every
function of tests/test_gpu_matmul_sweep.py runs here against the float64 stand-ins served at the C ABI, and turns red on one wrong row and on one
wrong element.

`python tests/test_matmul_sweep_cases_cpu.py` prints the worst need of the model per kernel and form."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]      # (run as a script)
import kernel_standins as ks  # noqa: E402
import matmul_sweep_cases as mc  # noqa: E402

SPLIT, WGRAD, PROD = mc.split_cases(), mc.wgrad_cases(), mc.production_cases()
DT = {"bf16": torch.bfloat16, "f16": torch.float16}
_ids = lambda cases: [c["id"] for c in cases]
_bf = lambda bits: torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16)


def small(c):
    """the wgrad production case at 1024 tokens (the float64 reference of 8192 costs 13 GFLOP on the host)"""
    return dict(c, m=1024) if c.get("production") and c["kernel"] == "wgrad" else c


# ---------------------------------------------------------------------------------------------------
# tables and coverage
# ---------------------------------------------------------------------------------------------------
def test_ids_are_unique_and_no_bound_is_raised():
    import test_gpu_multi_cast as tm
    import test_gpu_wgrad as tw
    every = SPLIT + WGRAD + PROD
    assert len({c["id"] for c in every}) == len(every)
    assert mc.SEED_MOVED == {}
    assert mc.TOL_TRUE == {3: 2.0 ** -14, 1: 2.0 ** -6} and mc.TOL_PLANES == 2.0 ** -16 and mc.IO_BOUND["f32"] == 2e-5 and mc.ROW_GUARD == 4.0
    assert mc.WG_BOUND16 == {"bf16": tw.BOUND16[torch.bfloat16], "f16": tw.BOUND16[torch.float16]} and mc.WG_BOUND32 == tw.BOUND32
    assert set(mc.SPECIALS) <= set(tm.SPECIALS) and {p for p in tm.SPECIALS if p & 0x7fffffff < 0x7f000000} == set(mc.SPECIALS)
    assert {p & 0x7fffffff for p in mc.BIG} >= {0x7f7f0000, 0x7f7f7fff, 0x7f7f8000, mc.FLT_MAX_BITS}


def test_split_table_covers_its_axes():
    f = {c["id"]: mc.split_fields(c) for c in SPLIT}
    plain = [c for c in SPLIT if not c["known"] and not c["nonfinite"]]
    assert {c["passes"] for c in SPLIT} == {1, 3}
    assert {c["m"] for c in SPLIT} >= set(mc.SPLIT_M) and {c["n"] for c in SPLIT} == set(mc.SPLIT_N) and {c["k"] for c in SPLIT} == set(mc.SPLIT_K)
    for passes in (1, 3):
        mine = [c for c in plain if c["passes"] == passes]
        assert {(f[c["id"]]["tiles"], f[c["id"]]["ragged"]) for c in mine} >= {(t, r) for t in mc.SPLIT_TILES for r in (False, True)}, passes
        assert {(f[c["id"]]["remap"], f[c["id"]]["ragged"], c["bias"]) for c in mine} == {(a, b, d) for a in (False, True) for b in (False, True) for d in (False, True)}
        assert {(c["k"], c["regime"]) for c in mine if c["n"] > 128} >= {(k, r) for k in mc.SPLIT_K for r in mc.SPLIT_REGIMES}, "every k on grids of several tile columns"
        assert {(c["m"], c["n"]) for c in mine} >= {(1016, 128), (392, 256)}, "8 tiles as 8 x 1 with 120 rows left, as 4 x 2 with 8 rows left"
        assert {c["x_pad"] for c in mine} == {0, 4, 64} and {c["out_pad"] for c in mine} == {0, 4}
        assert {(c["known"], c["regime"]) for c in SPLIT if c["passes"] == passes and c["known"] == "select"} == {("select", r) for r in mc.SPLIT_REGIMES}
        assert {c["known"] for c in SPLIT if c["passes"] == passes} == {None, "select", "exact-a", "exact-b", "exact-c", "periodic"}
        assert {c["nonfinite"] for c in SPLIT if c["passes"] == passes} == {None, "+inf", "-inf", "nan"}
    for c in SPLIT:
        sh = f[c["id"]]["shape"]
        assert sh["w_hi"][3] == c["k"] + 8 and sh["w_lo"][3] == c["k"] + 24 and sh["x"][4] == -c["m"] % 128 + 1
    assert [(c["m"], c["n"], c["k"], c["passes"]) for c in PROD if c["kernel"] == "split"] == [(2048, 640, 1280, 3)]


def test_wgrad_table_covers_its_axes():
    plain = [c for c in WGRAD if not c["known"]]
    assert {c["n"] for c in WGRAD} == set(mc.WG_N) and {c["k"] for c in WGRAD} == set(mc.WG_K) and {c["m"] for c in WGRAD} >= set(mc.WG_M)
    assert {(c["n"], c["k"]) for c in plain} >= {(n, k) for n in mc.WG_N for k in mc.WG_K}
    cells = {(bk, sk, o, kind) for bk in (64, 128) for sk in (False, True) for o in (False, True) for kind in mc.KINDS}
    assert {c["cell"] for c in plain} == cells and {c["cell"] for c in WGRAD if c["known"] == "ints"} >= {(bk, sk, o, kd) for bk, sk, o, kd in cells if o == (kd == "bf16")}
    for regime in mc.WG_REGIMES:
        assert {c["cell"] for c in plain if c["regime"] == regime} == cells, regime
    assert all(c["out32"] for c in plain if c["regime"] == "model" and c["kind"] == "f16" and c["m"] < 1000), "an fp16 subnormal RESULT is the output type's limit"
    for known in ("ints", None):
        assert {(c["m"], c["slabs"]) for c in WGRAD if c["known"] == known} >= {(m, s) for m in mc.WG_M for s in mc.WG_SLABS}, known
    assert {(c["kind"], c["out32"]) for c in WGRAD if c["known"] == "select"} == {(k, o) for k in mc.KINDS for o in (False, True)}
    auto = [c for c in WGRAD if c["m"] == 4104 and c["slabs"] == 0]
    assert auto and all(mc.wgrad_fields(c)["S"] > 1 for c in auto), "the library's own choice is more than one slab"
    empty = [c for c in WGRAD if c["slabs"] * 64 >= c["m"] + 64 and c["slabs"] > 1]
    assert {c["known"] for c in empty} >= {None, "ints"}, "slabs above the number of 64-token steps"
    for c in WGRAD:
        sh = mc.wgrad_fields(c)["shape"]
        assert sh["out"][3] > c["k"] and sh["dy"][3] > sh["dy"][2] + c["n"] and sh["x"][3] > sh["x"][2] + c["k"] and sh["dy"][4] == sh["x"][4] == 64
    assert [(c["m"], c["n"], c["k"], c["kind"]) for c in PROD if c["kernel"] == "wgrad"] == [(8192, 2560, 640, "bf16")]


@pytest.fixture(scope="module")
def library():
    from zigma_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.lib()


def test_wgrad_restatement_is_the_librarys_choice(library):
    """wgrad_slabs restated = zigma_linear_wgrad_workspace_bytes of the built library (host arithmetic, no device) on every case and around the
    thresholds of the library's own choice"""
    from zigma_amd import _lib
    extra = [dict(m=m, n=n, k=k, slabs=0, out32=False, out_pad=8) for m in (511, 512, 1023, 1024, 4104, 32768, 65536) for n, k in ((8, 8), (128, 64), (136, 72), (2560, 640), (72, 1280))]
    for c in WGRAD + PROD[1:] + extra:
        P = _lib.LinearWgradParams()
        P.m, P.n, P.k, P.dtype, P.out_dtype, P.slabs = c["m"], c["n"], c["k"], _lib.BF16, _lib.BF16, c["slabs"]
        assert library.zigma_linear_wgrad_workspace_bytes(ctypes.byref(P)) == mc.wgrad_fields(c)["workspace_bytes"], c
    assert mc.wgrad_fields(PROD[1])["S"] == 6 and mc.wgrad_bk(64) == 64 and mc.wgrad_bk(72) == 128


def test_numpy_split_is_the_definition():
    """bit for bit fp32_matmul.split on every case's x and on 10^6 random finite patterns; hi + lo is formed exactly in fp32 below the clamp;
    FLT_MAX gives hi = 0x7f7f and lo = 2^120, whose fp32 sum is +inf"""
    from zigma_amd.fp32_matmul import split
    rng = np.random.default_rng(7)
    pats = rng.integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(np.uint32)
    pats = pats[(pats & 0x7f800000) != 0x7f800000]
    arrays = [pats.view(np.float32), np.array(mc.BIG + mc.SPECIALS + tuple(p | 0x80000000 for p in mc.BIG), np.uint32).view(np.float32)]
    arrays += [mc.split_inputs(c)["x"].ravel() for c in SPLIT if c["regime"] == "edges" or c["nonfinite"]]
    for a in arrays:
        hi, lo = mc.split(a)
        th, tl = split(torch.from_numpy(np.ascontiguousarray(a)))
        ok = ~np.isnan(a)
        assert np.array_equal(hi[ok], th.view(torch.int16).numpy().view(np.uint16)[ok]) and np.array_equal(lo[ok], tl.view(torch.int16).numpy().view(np.uint16)[ok])
        assert np.isnan(mc.bf16_value(hi[~ok])).all() and not lo[~ok].any()
        below = ok & (np.abs(a) < mc.bf16_value(0x7f7f))
        h64, l64, a = mc.bf16_value(hi).astype(np.float64)[below], mc.bf16_value(lo).astype(np.float64)[below], a[below]
        below = slice(None)
        assert np.array_equal((h64 + l64).astype(np.float32).astype(np.float64)[below], (h64 + l64)[below]), "float(hi) + float(lo) is exact in fp32"
        assert (np.abs(h64 + l64 - a)[below] <= 2.0 ** -16 * np.abs(a[below]) + mc.PLANE_QUANTUM / 2).all(), "16 bits, or the bf16 subnormal grid"
    hi, lo = mc.split(np.array([mc.FLT_MAX], np.float32))
    assert hi[0] == 0x7f7f and mc.bf16_value(lo)[0] == 2.0 ** 120
    with np.errstate(over="ignore"):
        assert np.isposinf(mc.bf16_value(hi) + mc.bf16_value(lo))[0]


def test_edges_hold_what_they_are_meant_to():
    c = next(c for c in SPLIT if c["regime"] == "edges" and not c["known"] and c["seed"] % 2 == 0 and c["m"] >= 16)
    assert any(c["seed"] % 2 for c in SPLIT if c["regime"] == "edges" and not c["known"])
    inp, R = mc.split_inputs(c), mc.EDGE_ROWS
    ref = mc.split_reference(c, inp)
    bits = inp["x"].view(np.uint32)
    for r0 in mc.edge_blocks(c["m"]):
        big = bits[r0 + R["big"]] & 0x7fffffff
        top = {0x7f7f0000, 0x7f7f7fff, 0x7f7f8000, mc.FLT_MAX_BITS}
        assert top <= set(big.tolist()) and top <= set((bits[r0 + R["big_neg"]] & 0x7fffffff).tolist())
        pieces = (big >= mc.MAX_BF16_BITS).reshape(-1, 8).any(1)
        assert pieces.any() and not pieces.all() and (pieces.reshape(-1, 8).sum(1) <= 4).all(), "slow pieces next to ordinary ones of the same row"
        assert (bits[r0 + R["big_neg"]][big >= 0x7f7e0000] >> 31).all() and not bits[r0 + R["zero"]].any()
        sub = bits[r0 + R["subnormal"]] & 0x7fffffff
        assert (sub > 0).all() and (sub < 0x00800000).all()
        lo = mc.split(inp["x"][r0 + R["lo_subnormal"]])[1] & 0x7fff
        assert ((lo > 0) & (lo < 0x0080)).mean() > 0.3, "lo planes on the bf16 subnormal grid"
        assert not mc.split(inp["x"][r0 + R["pow2"]])[1].any() and set(mc.SPECIALS[:20]) <= set(bits[r0 + R["specials"]].tolist())
        assert np.abs(ref["true"][r0 + R["cancel"]] - (0 if inp["bias"] is None else inp["bias"])).max() < 1e-12 * ref["mag"][r0 + R["cancel"]].max(), "rows (a | a) against (b | -b)"
    assert not inp["w"][[2, c["n"] - 3]].any() and ref["mag"].max() < mc.FLT_MAX and np.abs(ref["true"]).max() < mc.FLT_MAX
    m = mc.split_inputs(next(c for c in SPLIT if c["regime"] == "model"))["x"]
    assert 20 < np.sqrt((m * m).mean()) < 50 and np.abs(m.mean(1)).max() > 10
    # wgrad
    c = next(c for c in WGRAD if c["regime"] == "model" and c["kind"] == "f16" and c["m"] >= 1000)
    dy = np.abs(mc.wgrad_inputs(c)["dy"])
    assert ((dy > 0) & (dy < 2.0 ** -14)).mean() > 0.2, "a share of the fp16 dy is subnormal"
    x = mc.wgrad_inputs(c)["x"]
    assert abs(np.sqrt((x * x).mean(1)) - 1).max() < 0.01 and x.mean() > 0.3
    for c in (c for c in WGRAD if c["regime"] == "edges" and not c["known"]):
        inp, e = mc.wgrad_inputs(c), mc.wgrad_edges(c["m"], c["n"])
        ref = mc.wgrad_reference(c, inp)
        assert not inp["dy"][:, e["zero_cols"]].any() and not ref["out"][e["zero_cols"]].any() and not inp["dy"][e["zero_dy"]].any() and not inp["x"][e["zero_x"]].any()
        assert ref["mag"].max() < mc.FLT_MAX and (c["out32"] or np.abs(ref["out"]).max() < 6e4), c["id"]
        if len(e["top"]):
            assert np.abs(inp["dy"][e["top"]]).max() > 5.9e4
        if len(e["pairs"]):
            assert np.array_equal(inp["dy"][e["pairs"]], inp["dy"][e["pairs"] + 1]) and np.array_equal(inp["x"][e["pairs"]], -inp["x"][e["pairs"] + 1])
    c = next(c for c in WGRAD if c["regime"] == "cancel" and c["m"] > 8)
    assert not mc.wgrad_reference(c, mc.wgrad_inputs(c))["out"].any()
    for c in (c for c in WGRAD if c["known"] == "ints"):
        inp = mc.wgrad_inputs(c)
        assert set(mc.ints_tokens(c["m"])) <= set(inp["tok"].tolist()) and (np.abs(inp["dy"][inp["tok"]]).sum(1) == 1).all() and (inp["x"] != 0).all()
        assert (np.abs(inp["dy"]).T @ np.abs(inp["x"])).max() <= 256, (c["id"], "every sum is an integer that bf16 holds")


# ---------------------------------------------------------------------------------------------------
# references vs the torch restatements; the fp32 model
# ---------------------------------------------------------------------------------------------------
MEASURED = {}           # form -> {limit: worst need of the fp32 model in units of the limit}


def _pin(c, key, ref, again):
    again = again.numpy()
    e = mc.norm_err(again, ref) if np.linalg.norm(ref) > 0 else float(np.linalg.norm(again))
    assert e < 1e-12, (c["id"], key, e)


def _record(form, need):
    slot = MEASURED.setdefault(form, {})
    for key, v in need.items():
        slot[key] = max(slot.get(key, 0.0), v)


@pytest.mark.parametrize("c", SPLIT + PROD[:1], ids=_ids(SPLIT + PROD[:1]))
def test_split_reference_and_model(c):
    from zigma_amd.fp32_matmul import reference
    inp = mc.split_inputs(c)
    if c["nonfinite"]:
        r0, c0 = mc.nonfinite_at(c)
        row = mc.split_row_reference(c, inp, r0)
        assert not np.isfinite(row).any() and (np.isnan(row).all() if c["nonfinite"] == "nan" else not np.isnan(row).all() or c["passes"] == 3)
        inp["x"][r0, c0] = 0.0
    ref = mc.split_reference(c, inp)
    x, bias = torch.from_numpy(inp["x"]), None if inp["bias"] is None else torch.from_numpy(inp["bias"])
    _pin(c, "planes", ref["planes"], ks.torch_split_linear(x, _bf(inp["w_hi"]), _bf(inp["w_lo"]), bias, c["passes"]))
    _pin(c, "true", ref["true"], reference(x, torch.from_numpy(inp["w"]), bias, "highest"))
    if c["known"] != "select":      # the planes are the split of w (a selection case's w_lo is the zero plane it is)
        wh, wl = mc.split(inp["w"])
        assert np.array_equal(wh, inp["w_hi"]) and np.array_equal(wl, inp["w_lo"])
        _pin(c, "planes (fp32_matmul.reference)", ref["planes"], reference(x, torch.from_numpy(inp["w"]), bias, {3: "high", 1: "medium"}[c["passes"]]))
    assert not inp["w_lo"].any() or c["known"] != "select"
    r = c["m"] - 3                  # the row-by-row form the non-finite table uses is the same reference
    assert np.abs(mc.split_row_reference(c, inp, r) - ref["planes"][r]).max() <= 1e-12 * ref["mag"][r].max()
    known = mc.split_known(c, inp)
    mask = None if known is None else np.isfinite(known)
    model = mc.split_model(c, inp)
    assert model.dtype == np.float32
    need = mc.split_need(c, model, ref, mask)
    _record(f"split{c['passes']} {c['known'] or c['regime']}", need)
    assert all(v < 0.5 for v in need.values()), (c["id"], need, "the fp32 model: another seed (SEED_MOVED), not another bound")
    if known is not None:           # exact in fp32 in the kernel's order
        assert np.array_equal(model.view(np.uint32)[mask] if mask is not None else model, known.view(np.uint32)[mask]), c["id"]
        if c["known"].startswith("exact"):
            assert ref["mag"].max() < 2 ** 24 and np.array_equal(ref["planes"], np.rint(ref["planes"]))
            assert (ref["planes"] != ref["true"]).mean() > (0.4 if c["passes"] == 1 or c["known"] == "exact-c" else -1)
        else:
            sel = inp["x"].view(np.uint32) == mc.FLT_MAX_BITS
            assert c["regime"] != "edges" or (sel.any() and (np.isposinf(known).any() == (c["passes"] == 3)))
    if c["known"] == "periodic":
        assert np.array_equal(model, np.tile(model[:8, :16], (c["m"] // 8, c["n"] // 16)))


@pytest.mark.parametrize("c", WGRAD + PROD[1:], ids=_ids(WGRAD + PROD[1:]))
def test_wgrad_reference_and_model(c):
    c = small(c)
    inp = mc.wgrad_inputs(c)
    ref = mc.wgrad_reference(c, inp)
    _pin(c, "out", ref["out"], ks.torch_wgrad(torch.from_numpy(inp["dy"]), torch.from_numpy(inp["x"])))
    kind = "f32" if c["out32"] else c["kind"]
    assert c["out32"] or np.abs(ref["out"]).max() < 6e4, (c["id"], "overflows fp16")
    own = mc.wgrad_need(c, mc.round_to(ref["out"], kind), ref)
    assert all(v < 1 for v in own.values()), (c["id"], own, "the rounded reference itself")
    model = mc.wgrad_model(c, inp)
    assert model.dtype == np.float32
    need = mc.wgrad_need(c, mc.round_to(model, kind), ref, norm_of=model)
    _record(f"{c['kernel_name']} {c['kind']}->{kind} {c['known'] or c['regime']}", need)
    assert all(v < 0.5 for v in need.values()), (c["id"], need, "the fp32 model: another seed (SEED_MOVED), not another bound")
    known = mc.wgrad_known(c, inp)
    if known is not None:
        assert np.array_equal(mc.round_to(model, kind).astype(np.float64), known) and np.array_equal(mc.round_to(known, kind).astype(np.float64), known)
        if c["known"] == "select":
            assert (np.count_nonzero(known, axis=1) == 0).sum() == c["n"] - c["m"] and len(set(inp["nu"].tolist())) == c["m"]


def test_worst_need_of_the_model():
    """(after the parametrised tests above) prints what the model measured, in units of each limit"""
    for form, need in sorted(MEASURED.items()):
        print(f"fp32 model, worst need in units of the limit: {form:44s} " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(need.items())))
    assert all(v < 0.5 for need in MEASURED.values() for v in need.values())


# ---------------------------------------------------------------------------------------------------
# tests/test_gpu_matmul_sweep.py on the CPU: float64 stand-ins at the C ABI
# ---------------------------------------------------------------------------------------------------
@pytest.fixture
def gpu_file(monkeypatch):
    import test_gpu_matmul_sweep as gf
    ks.install_lib_call(monkeypatch)
    monkeypatch.setattr(gf, "DEV", "cpu")
    return gf


@pytest.mark.parametrize("c", SPLIT + PROD[:1], ids=_ids(SPLIT + PROD[:1]))
def test_gpu_split_checks_pass_on_the_stand_in(c, gpu_file, capsys):
    gpu_file.check_split_case(c)
    assert f"matmul-sweep {c['id']}: " in capsys.readouterr().out


@pytest.mark.parametrize("c", WGRAD + PROD[1:], ids=_ids(WGRAD + PROD[1:]))
def test_gpu_wgrad_checks_pass_on_the_stand_in(c, gpu_file, capsys):
    gpu_file.check_wgrad_case(small(c))
    assert f"matmul-sweep {c['id']}: out " in capsys.readouterr().out


def test_gpu_checks_turn_red_on_a_wrong_row_and_on_a_wrong_element(gpu_file, monkeypatch):
    """one row from its neighbour, ONE element an fp32 / 16-bit ulp-scale step off, a dropped cross term, a read of the NaN row below x or beside
    dy, a dropped 64-token step, a write beside the output or behind the workspace: each is caught"""
    real_split, real_wgrad = ks.torch_split_linear, ks.torch_wgrad

    def wrong_row(*a):
        y = real_split(*a)
        y[100] = y[99]
        return y

    def wrong_element(*a):
        y = real_split(*a)
        y[77, -2] += 2.0 ** -12 * y[77].abs().max()               # (a few fp32 ulps of the row's largest element)
        return y

    def no_cross(x, w_hi, w_lo, bias, passes):
        return real_split(x, w_hi, torch.zeros_like(w_hi), bias, passes)

    def reads_below(x, *a):
        return real_split(torch.cat([x[:-1], x[-1:] + float("nan")]), *a)

    def wg_wrong_row(dy, x):
        out = real_wgrad(dy, x)
        if out.shape[0] > 9:
            out[9] = out[8]
        return out

    def wg_wrong_element(dy, x):
        out = real_wgrad(dy, x)
        out[-1, -1] += 2.0 ** -4 * (out.abs().max() + 1)          # (25 norm-wise bf16 bounds of the largest element)
        return out

    def wg_dropped_step(dy, x):
        return real_wgrad(dy[:-1], x[:-1])

    def wg_reads_beside(dy, x):
        return real_wgrad(torch.cat([dy[:, :-1], dy[:, -1:] + float("nan")], 1), x)
    plain = lambda regime, passes=3: next(c for c in SPLIT if c["regime"] == regime and not c["known"] and not c["nonfinite"] and c["passes"] == passes and c["m"] >= 136 and c["n"] >= 256)
    sel = next(c for c in SPLIT if c["known"] == "select" and c["passes"] == 3)
    for bad, c in ((wrong_row, plain("benign")), (wrong_row, plain("edges")), (wrong_element, plain("model")), (wrong_element, plain("benign", 1)), (no_cross, plain("benign")),
                   (no_cross, next(c for c in SPLIT if c["known"] == "exact-b" and c["passes"] == 3)), (reads_below, plain("benign")), (wrong_element, sel),
                   (wrong_row, next(c for c in SPLIT if c["known"] == "periodic"))):
        with monkeypatch.context() as mp:
            mp.setattr(ks, "torch_split_linear", bad)
            with pytest.raises(AssertionError):
                gpu_file.check_split_case(c)
    wg = lambda regime, **kw: next(c for c in WGRAD if c["regime"] == regime and not c["known"] and c["m"] >= 127 and c["n"] >= 24 and all(c[k] == v for k, v in kw.items()))
    ints = next(c for c in WGRAD if c["known"] == "ints" and c["m"] == 4104 and c["slabs"] == 3)
    for bad, c in ((wg_wrong_row, wg("benign", out32=True)), (wg_wrong_row, wg("model")), (wg_wrong_element, wg("benign", out32=False, kind="bf16")),
                   (wg_wrong_element, wg("edges", out32=True)), (wg_wrong_element, wg("cancel", out32=True)), (wg_dropped_step, ints), (wg_dropped_step, wg("benign", out32=True)),
                   (wg_reads_beside, wg("benign")), (wg_wrong_element, next(c for c in WGRAD if c["known"] == "select"))):
        with monkeypatch.context() as mp:
            mp.setattr(ks, "torch_wgrad", bad)
            with pytest.raises(AssertionError):
                gpu_file.check_wgrad_case(c)
    real_call = gpu_file._call

    def spill(c, name, P):
        real_call(c, name, P)
        if name == "zigma_linear_wgrad":
            ks._view(P.workspace + P.workspace_bytes, (1,), (1,), torch.float32)[0] = 1.0
        else:
            ks._view(P.out - 4, (1,), (1,), torch.float32)[0] = 1.0
    monkeypatch.setattr(gpu_file, "_call", spill)
    with pytest.raises(AssertionError, match="outside the output window"):
        gpu_file.check_split_case(SPLIT[0])
    with pytest.raises(AssertionError, match="outside the output window"):
        gpu_file.check_wgrad_case(wg("benign", slabs=3))


if __name__ == "__main__":
    for fn, cases in ((test_split_reference_and_model, SPLIT + PROD[:1]), (test_wgrad_reference_and_model, WGRAD + PROD[1:])):
        for case in cases:
            try:
                fn(case)
            except AssertionError as err:
                print("FAILS", err)
    for form, need in sorted(MEASURED.items()):
        print(f"fp32 model, worst need in units of the limit: {form:44s} " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(need.items())))
    print(f"SEED_MOVED = {mc.SEED_MOVED!r}")

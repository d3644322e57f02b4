"""CPU checks of the attention / glue sweep's case tables (tests/attn_cases.py): the tables cover every cell they are meant to cover; on exactly
these inputs the float64 references agree with float64 torch autograd through a plain softmax / matmul composition (< 1e-12 norm-wise, zero
gradients compare as zero); the rounding model (the repository's plain compositions in the case's I/O type, evaluated here on the CPU) stays
within 2 x the base bound of float64 — a condition on the INPUTS: a case that breaks it gets a lower gain, never a higher cap —; and the
reference ROUNDED to the output type stays below the base bound norm-wise and below 1 x the bound row by row.  So a failure of
tests/test_gpu_attn_sweep.py is the kernel's."""
import numpy as np
import pytest
import torch

import attn_cases as ac
from conftest import rel_err

FWD, BWD, GLUE = ac.xattn_fwd_cases(), ac.xattn_bwd_cases(), ac.glue_cases()
DT = {"bf16": torch.bfloat16, "f16": torch.float16}


def _ids(cases):
    return [c["id"] for c in cases]


# ---------------------------------------------------------------------------------------------------
# coverage
# ---------------------------------------------------------------------------------------------------
def _attn_coverage(cases, kinds, nctx, insts, inst_of, slices):
    assert len({c["id"] for c in cases}) == len(cases)
    assert {c["L"] for c in cases} == set(ac.ATTN_L) and {c["H"] for c in cases} == set(ac.HEADS) and {c["B"] for c in cases} == {1, 2, 3}
    assert {c["scale"] for c in cases} == set(ac.SCALES) and sum(c["scale"] != ac.SCALE0 for c in cases) >= 3
    assert all(c["B"] == 1 for c in cases if c["L"] >= 511 and c["H"] == 8) and any(c["L"] >= 511 and c["H"] == 8 for c in cases)
    assert all(c["n_ctx"] <= ac.D for c in cases if c["known"])
    for kind in kinds:
        mine = [c for c in cases if c["kind"] == kind]
        assert {c["n_ctx"] for c in mine} >= set(nctx), kind
        assert {17, 33} <= {c["L"] for c in mine}, kind                        # whole waves of a workgroup without a tile
        for key in ("q_slice", "pad") + slices:
            assert {c[key] for c in mine} == {True, False}, (kind, key)
        assert {c["kv"] for c in mine} == {"pair", "halves"}, kind
        assert any(c["known"] for c in mine), kind
        for inst in insts:
            cell = [c for c in mine if inst_of(c["n_ctx"]) == inst and not c["known"]]
            assert {ac.tiles(c["L"]) for c in cell} == {4, 8}, (kind, inst)
            for t, span in ((4, range(257, 512)), (8, range(513, 2000))):     # ragged last tile AND several workgroups of tokens, per tile count
                assert any(c["L"] in span and ac.ragged(c["L"]) and ac.chunks(c["L"]) > 1 and ac.tiles(c["L"]) == t for c in cell), (kind, inst, t)
            assert any(not ac.ragged(c["L"]) for c in cell) and any(ac.chunks(c["L"]) == 1 for c in cell), (kind, inst)
            assert 3 * sum(c["gain"] == 6 for c in cell) >= len(cell), (kind, inst)
            assert sum(c["twice"] for c in cell) >= 1, (kind, inst)


def test_xattn_fwd_table_covers_its_cells():
    assert 50 <= len(FWD) <= 70
    _attn_coverage(FWD, ("bf16", "f16"), ac.FWD_NCTX, ac.FWD_INSTS, ac.fwd_inst, ())
    assert {1, 15, 16, 17, 63, 64, 65, 79, 80, 111, 112, 113, 127, 5, 77, 128} <= set(ac.FWD_NCTX)
    assert [ac.fwd_inst(n) for n in (1, 64, 65, 80, 81, 112, 113, 128)] == [(5, True), (5, True), (5, False), (5, False), (8, True), (8, True),
                                                                            (8, False), (8, False)]
    assert all(c["known"] == "onehot+zero" for c in FWD if c["known"])
    assert [ac.tiles(L) for L in (511, 512, 513)] == [4, 8, 8] and [ac.chunks(L) for L in (256, 257, 512, 513, 1000, 1025)] == [1, 2, 1, 2, 2, 3]


def test_xattn_bwd_table_covers_its_cells():
    assert 20 <= len(BWD) <= 40 and {c["kind"] for c in BWD} == {"bf16"}
    _attn_coverage(BWD, ("bf16",), ac.BWD_NCTX, (5, 8), ac.bwd_inst, ("do_slice",))
    assert {79, 81, 96, 112, 5, 77, 128, 1} <= set(ac.BWD_NCTX)
    assert [ac.bwd_inst(n) for n in (80, 81)] == [5, 8]
    assert {c["known"] for c in BWD if c["known"]} == {"onehot", "onehot+zero"}
    assert any(c["n_ctx"] == 1 for c in BWD)


def test_glue_table_covers_its_cells():
    assert len({c["id"] for c in GLUE}) == len(GLUE) and {c["B"] for c in GLUE} == {1, 2, 3}
    assert {c["L"] for c in GLUE} == set(ac.GLUE_L) and {c["cols"] for c in GLUE} == set(ac.GLUE_COLS)
    assert all((c["B"], c["L"]) == (1, 64) for c in GLUE if c["cols"] == 8192)
    for key in ("s_add", "want_out", "want_sum", "a_slice", "dy_slice"):
        assert {bool(c[key]) for c in GLUE} == {True, False}, key
    assert {(c["want_out"], c["want_sum"]) for c in GLUE} == {(a, b) for a in (True, False) for b in (True, False)}
    assert sum(c["twice"] for c in GLUE) == 1 and any(c["L"] == 1088 and c["want_out"] and c["want_sum"] for c in GLUE)
    # one refusal per limit, each breaking exactly one (glue_bwd_eligible itself needs device tensors: test_gpu_attn_sweep.py)
    broken = [(r["L"] % 64 != 0, r["cols"] % 128 != 0, r["cols"] > 8192, r["kind"] == "f16") for r in ac.GLUE_REFUSALS]
    assert sorted(broken) == sorted([(True, False, False, False), (False, True, False, False), (False, False, True, False), (False, False, False, True)])


# ---------------------------------------------------------------------------------------------------
# the references against float64 autograd on these inputs; the rounding model's cap; the rounding floor
# ---------------------------------------------------------------------------------------------------
def _t64(a, grad=True):
    return torch.from_numpy(np.asarray(a, np.float64)).requires_grad_(grad)


def _torch_attention(q, k, v, H, scale):
    """softmax(scale q k^T) v per head: the plain composition autograd differentiates"""
    hd = lambda t: t.reshape(t.shape[0], t.shape[1], H, ac.D).transpose(1, 2)
    p = torch.softmax(hd(q) @ hd(k).transpose(-1, -2) * scale, -1)
    return (p @ hd(v)).transpose(1, 2).reshape(q.shape)


def _agree(got, want, ident):
    if np.linalg.norm(want) == 0.0:
        assert np.linalg.norm(got) == 0.0, ident             # (n_ctx = 1: dq and dk are identically zero in both)
    else:
        assert rel_err(got, want) < 1e-12, (ident, rel_err(got, want))


def _cap_and_floor(c, base, ref, model, skip=()):
    for key, want in ref.items():
        if key in skip:
            continue
        e_model = rel_err(model[key].double().numpy(), want)
        assert e_model <= ac.MODEL_CAP * base, (c["id"], key, e_model, "lower this case's gain")
        rounded = ac.round_to(want, c["kind"])
        assert rel_err(rounded, want) < base, (c["id"], key)
        assert ac.rowwise_worst(ac.head_rows(rounded, c["H"]), ac.head_rows(want, c["H"]), base) < 1.0, (c["id"], key)


@pytest.mark.parametrize("c", FWD, ids=_ids(FWD))
def test_xattn_fwd_reference_model_cap_and_rounding_floor(c):
    inp = ac.xattn_fwd_inputs(c)
    ref = ac.xattn_fwd_reference(c, inp)
    q, k, v = (_t64(inp[n], False) for n in "qkv")
    _agree(ref["out"], _torch_attention(q, k, v, c["H"], c["scale"]).numpy(), c["id"])
    lo = [torch.from_numpy(inp[n]).to(DT[c["kind"]]) for n in "qkv"]
    assert all(torch.equal(t.float(), torch.from_numpy(inp[n])) for t, n in zip(lo, "qkv"))          # the inputs ARE values of the I/O type
    _cap_and_floor(c, ac.FWD_BASE[c["kind"]], ref, ac.xattn_model(c, *lo))
    if c["known"]:
        ans = ac.xattn_known_answers(c, inp)
        hot = ~np.isnan(ans["out"])
        assert hot.any() and (~hot).any() and np.array_equal(ref["out"][hot], ans["out"][hot].astype(np.float64))        # float64 agrees: exp(-128) ~ 0
        zero_rows = ac.head_rows(~hot, c["H"]).all(-1)
        mean_v = ac.to_heads(inp["v"], c["H"]).mean(2)                                                # (B, H, 64)
        got = ac.head_rows(ref["out"], c["H"])
        for b, t, h in zip(*np.nonzero(zero_rows)):
            assert np.allclose(got[b, t, h], mean_v[b, h], rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("c", BWD, ids=_ids(BWD))
def test_xattn_bwd_reference_model_cap_and_rounding_floor(c):
    inp = ac.xattn_bwd_inputs(c)
    ref = ac.xattn_bwd_reference(c, inp)
    q, k, v = (_t64(inp[n]) for n in "qkv")
    _torch_attention(q, k, v, c["H"], c["scale"]).backward(_t64(inp["dout"], False))
    zero = ac.exact_zero(c)
    for key, leaf in (("dq", q), ("dk", k), ("dv", v)):
        if key in zero:         # analytically ds = p (dP - delta) with p = 1 or exp(-128): what float64 leaves is of that size, in both
            assert np.abs(ref[key]).max() < 1e-40 and leaf.grad.abs().max().item() < 1e-40, (c["id"], key)
        else:
            _agree(ref[key], leaf.grad.numpy(), (c["id"], key))
    if c["n_ctx"] == 1:
        assert not ref["dq"].any() and not ref["dk"].any()
    lo = [torch.from_numpy(inp[n]).to(DT[c["kind"]]) for n in ("q", "k", "v", "dout")]
    assert all(torch.equal(t.float(), torch.from_numpy(inp[n])) for t, n in zip(lo, ("q", "k", "v", "dout")))
    _cap_and_floor(c, ac.BWD_BASE, ref, ac.xattn_model(c, *lo), skip=zero)
    if c["known"] == "onehot":
        ans = ac.xattn_known_answers(c, inp)
        assert np.allclose(ref["dv"], ans["dv"], rtol=0, atol=1e-40), c["id"]       # multiples of 1/8 times probabilities of 1 or exp(-128)
    if c["n_ctx"] == 1:         # the absolute limit's helper: zero gradients rate 0, and a dq of the cancelling terms' size rates 1 / bound
        assert ac.nctx1_worst(c, inp, ref["dq"], ref["dk"], ac.BWD_BASE) == (0.0, 0.0)
        fake = c["scale"] * inp["dout"].astype(np.float64) * np.linalg.norm(ac.head_rows(inp["v"], c["H"]), axis=-1).repeat(ac.D, -1) \
            * np.linalg.norm(ac.head_rows(inp["k"], c["H"]), axis=-1).repeat(ac.D, -1)
        assert abs(ac.nctx1_worst(c, inp, fake, ref["dk"], ac.BWD_BASE)[0] * ac.BWD_BASE - 1.0) < 1e-6


@pytest.mark.parametrize("c", GLUE, ids=_ids(GLUE))
def test_glue_reference_vs_float64_autograd_and_rounding_floor(c):
    """modulate backward (s_add = 1): y = a (1 + s) + shift; gated add backward (s_add = 0): y = x + s a, both against the upstream gradient dy"""
    inp = ac.glue_inputs(c)
    ref = ac.glue_reference(c, inp)
    a, s = _t64(inp["a"]), _t64(inp["s"])
    sh = torch.zeros(c["B"], c["cols"], dtype=torch.float64, requires_grad=True)
    y = a * (c["s_add"] + s.unsqueeze(1)) + sh.unsqueeze(1)
    y.backward(_t64(inp["dy"], False))
    for key, want in (("out", a.grad), ("r1", s.grad), ("r2", sh.grad)):
        if ref[key] is None:
            assert not c["want_" + {"out": "out", "r2": "sum"}[key]]
            continue
        _agree(ref[key], want.numpy(), (c["id"], key))
        rounded = ac.round_to(ref[key], "bf16")
        assert rel_err(rounded, ref[key]) < ac.GLUE_BASE, (c["id"], key)
        # a row of `out` stays below 1 x the bound; ONE bf16 element can be half an ulp = 2^-8 of its value off, 1.3 x the bound: the reduced
        # sums' element-wise limit of ROW_GUARD x the bound leaves the kernel the other 2.7
        assert ac.glue_worst(key, rounded, ref[key], ac.GLUE_BASE) < (1.0 if key == "out" else 2.0 ** -8 / ac.GLUE_BASE + 1e-6), (c["id"], key)


# ---------------------------------------------------------------------------------------------------
# the refusals that need no device: both attention entry points judge the scale before they touch a pointer
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn,struct", [("zigma_cross_attn_fwd", "XAttnParams"), ("zigma_cross_attn_bwd", "XAttnBwdParams")])
def test_xattn_entry_points_refuse_a_scale_outside_the_softmax_domain(fn, struct):
    import ctypes
    import os
    from zigma_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    L = _lib.lib()
    codes = {}
    for scale in (0.0, -0.125, float("inf"), float("nan"), ac.SCALE0):
        P = getattr(_lib, struct)()
        P.batch, P.seqlen, P.n_ctx, P.heads, P.head_dim, P.dtype, P.scale = 1, 16, 5, 1, ac.D, _lib.BF16, scale
        codes[repr(scale)] = L.zigma_strerror(getattr(L, fn)(ctypes.byref(P), None))
    good = codes.pop(repr(ac.SCALE0))
    assert set(codes.values()) == {b"feature out of scope"} and good == b"required pointer is NULL", (codes, good)

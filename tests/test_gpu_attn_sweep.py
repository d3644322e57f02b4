"""Sweep of the text-conditioning side's kernels — zigma_cross_attn_fwd (bf16, fp16), zigma_cross_attn_bwd (bf16), zigma_scale_reduce_bwd
(bf16) — against float64, over the case tables of tests/attn_cases.py (coverage, reference soundness, the rounding model's cap and the
rounding floor: tests/test_attn_cases_cpu.py).

Every case: the entry point really served the call (the call trace: kernel name and the parameter block's n_ctx, seqlen, dtype, scale, chunks and
strides); every output is finite although the block the wrapper allocates it in held NaN beforehand and everything around the operands — the
other columns of the buffers q / dout / a / dy are sliced from, rows past seqlen and past n_ctx, the other thirds of the adaLN rows — is NaN, so a
read past either end poisons the result; norm-wise distance to float64 below the case bound max(base, 2 x e_model), base the existing tests'
bound of the same kernel and e_model the distance of the repository's plain composition (library GEMMs, P and dS rounded where the kernels round
them) on the same operands; and, since a norm hides one wrong row — the last token of a ragged tile, the first token of the second chunk —,
EVERY row of one token (or key) and head within ROW_GUARD x that bound of max(its own norm, the rms row norm), every element of the glue's reduced
sums within ROW_GUARD x the bound of max(|ref|, rms).  Known-answer cases compare exactly; marked cases run twice: bit-identical.  Production shapes
at the end: float64 torch autograd on the device as the reference.

Each case prints `attn-sweep <kernel> <type> <output> norm-wise <e> (bound <b>, model <m>) row-wise <r> [id]` (r in units of the bound) for
DESIGN.md's parity table.
"""
import numpy as np
import pytest
import torch

import attn_cases as ac
from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = {"bf16": torch.bfloat16, "f16": torch.float16}
FWD, BWD, GLUE = ac.xattn_fwd_cases(), ac.xattn_bwd_cases(), ac.glue_cases()
NAN = float("nan")
KV_TAIL, Q_TAIL, Q_LEAD = 3, 2, 64          # NaN rows past n_ctx; NaN rows past seqlen (pad); NaN columns in front of a column slice


def _ids(cases):
    return [c["id"] for c in cases]


def _np(t):
    return None if t is None else t.detach().double().cpu().numpy()


def _poison(*specs):
    """allocate and free NaN-filled tensors of the shapes / dtypes the wrapper is about to allocate: a recycled block then holds NaN, not
    the previous case's correct answer"""
    keep = [torch.full(shape, NAN, dtype=dtype, device=DEV) for shape, dtype in specs]
    torch.cuda.synchronize()
    del keep


def _traced(fn):
    from zigma_amd import _lib
    _lib.TRACE = []
    try:
        res = fn()
    finally:
        trace, _lib.TRACE = _lib.TRACE, None
    return res, trace


def _sliced(a, dtype, lead=0, tail=0):
    """(B, n, C) values as a view of a NaN-filled (B, n + tail, lead + C) device buffer"""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)
    if not (lead or tail):
        return t
    buf = torch.full((t.shape[0], t.shape[1] + tail, lead + t.shape[2]), NAN, dtype=dtype, device=DEV)
    buf[:, :t.shape[1], lead:] = t
    return buf[:, :t.shape[1], lead:]


def _kv(c, inp, dtype):
    """K / V as the case lays them out, in a NaN-filled buffer with KV_TAIL rows past n_ctx"""
    k, v = (torch.from_numpy(inp[n]).to(DEV).to(dtype) for n in "kv")
    Bsz, n, C = k.shape
    if c["kv"] == "pair":
        buf = torch.full((Bsz, n + KV_TAIL, 2, C), NAN, dtype=dtype, device=DEV)
        buf[:, :n, 0], buf[:, :n, 1] = k, v
        return buf[:, :n, 0], buf[:, :n, 1]
    buf = torch.full((Bsz, n + KV_TAIL, 2 * C), NAN, dtype=dtype, device=DEV)
    buf[:, :n, :C], buf[:, :n, C:] = k, v
    return buf[:, :n, :C], buf[:, :n, C:]


def _strides(c, sliced):
    """(batch stride, row stride) the case's layout gives a (B, L, C) operand"""
    row = c["H"] * ac.D + (Q_LEAD if sliced else 0)
    return ((c["L"] + (Q_TAIL if c["pad"] else 0)) * row, row)


def _check_block(c, P, dtype):
    from zigma_amd import _lib
    C = c["H"] * ac.D
    assert (P.batch, P.seqlen, P.n_ctx, P.heads, P.head_dim, P.dtype, P.flags) == (c["B"], c["L"], c["n_ctx"], c["H"], ac.D, _lib._DT[dtype], 0), c["id"]
    assert P.scale == np.float32(c["scale"]), (c["id"], P.scale)
    assert (P.q_batch_stride, P.q_row_stride) == _strides(c, c["q_slice"]), c["id"]
    assert P.k_row_stride == P.v_row_stride == 2 * C and P.k_batch_stride == P.v_batch_stride == (c["n_ctx"] + KV_TAIL) * 2 * C, c["id"]


def _compare(kernel, c, key, got, want, base, e_model):
    """norm-wise below the case bound, every (token | key, head) row within ROW_GUARD x the bound"""
    bound = ac.case_bound(base, e_model)
    assert got.shape == want.shape and np.isfinite(got).all(), (c["id"], key, "not finite: an element was left unwritten, or a NaN / inf was read or computed")
    e, r = rel_err(got, want), ac.rowwise_worst(ac.head_rows(got, c["H"]), ac.head_rows(want, c["H"]), bound)
    print(f"attn-sweep {kernel} {c['kind']} {key} norm-wise {e:.3e} (bound {bound:.2e}, model {e_model:.2e}) row-wise {r:.3g} [{c['id']}]")
    assert e < bound, (c["id"], key, e, bound)
    assert r <= ac.ROW_GUARD, (c["id"], key, r)


# ---------------------------------------------------------------------------------------------------
# attention forward
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", FWD, ids=_ids(FWD))
def test_xattn_fwd_sweep(c):
    from zigma_amd.attention import cross_attn, cross_attn_eligible
    dt, C = DT[c["kind"]], c["H"] * ac.D
    inp = ac.xattn_fwd_inputs(c)
    q = _sliced(inp["q"], dt, Q_LEAD if c["q_slice"] else 0, Q_TAIL if c["pad"] else 0)
    k, v = _kv(c, inp, dt)
    assert cross_attn_eligible(q, k, v, c["H"])

    def call():
        _poison(((c["B"], c["L"], C), dt))
        return _traced(lambda: cross_attn(q, k, v, c["H"], c["scale"]))
    out, trace = call()
    assert [t[:2] for t in trace] == [("zigma_cross_attn_fwd", "cross_attn_mfma")], c["id"]
    P = trace[0][2]
    _check_block(c, P, dt)
    assert (P.o_batch_stride, P.o_row_stride) == (c["L"] * C, C) and out.dtype == dt
    ref = ac.xattn_fwd_reference(c, inp)["out"]
    e_model = rel_err(_np(ac.xattn_model(c, q, k, v)["out"]), ref)
    _compare("xattn_fwd", c, "out", _np(out), ref, ac.FWD_BASE[c["kind"]], e_model)
    if c["known"]:      # the winning logit leads by 128: every other exponential is exactly zero and the row is v[j], bit for bit
        ans = torch.from_numpy(ac.xattn_known_answers(c, inp)["out"]).to(DEV)
        hot = ~torch.isnan(ans)
        assert hot.any() and torch.equal(out[hot], ans[hot].to(dt)), c["id"]
    if c["twice"]:
        assert torch.equal(call()[0], out), c["id"]


# ---------------------------------------------------------------------------------------------------
# attention backward
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", BWD, ids=_ids(BWD))
def test_xattn_bwd_sweep(c):
    from zigma_amd.attention import cross_attn_bwd, cross_attn_bwd_eligible
    dt, C, Bsz, L, n = DT[c["kind"]], c["H"] * ac.D, c["B"], c["L"], c["n_ctx"]
    inp = ac.xattn_bwd_inputs(c)
    tail = Q_TAIL if c["pad"] else 0
    q = _sliced(inp["q"], dt, Q_LEAD if c["q_slice"] else 0, tail)
    dout = _sliced(inp["dout"], dt, Q_LEAD if c["do_slice"] else 0, tail)
    k, v = _kv(c, inp, dt)
    assert cross_attn_bwd_eligible(q, k, v, c["H"]) and cross_attn_bwd_eligible(dout, k, v, c["H"])

    def call():
        _poison(((Bsz, L, C), dt), ((2, ac.chunks(L), Bsz, n, C), torch.float32))
        return _traced(lambda: cross_attn_bwd(q, k, v, dout, c["H"], c["scale"]))
    res, trace = call()
    assert [t[:2] for t in trace] == [("zigma_cross_attn_bwd", "cross_attn_bwd_mfma")], c["id"]
    P = trace[0][2]
    _check_block(c, P, dt)
    assert P.chunks == ac.chunks(L) and (P.do_batch_stride, P.do_row_stride) == _strides(c, c["do_slice"]), c["id"]
    assert (P.dq_batch_stride, P.dq_row_stride) == (L * C, C) and all(t.dtype == dt for t in res)
    got = dict(zip(("dq", "dk", "dv"), map(_np, res)))
    assert all(np.isfinite(g).all() for g in got.values()), c["id"]
    ref = ac.xattn_bwd_reference(c, inp)
    model = ac.xattn_model(c, q, k, v, dout)
    zero = ac.exact_zero(c)
    for key in ("dq", "dk", "dv"):
        if key in zero:             # one-hot probabilities: dS = P o (dP - delta) is 0 in every lane, whatever the summation order
            assert not got[key].any(), (c["id"], key, float(np.abs(got[key]).max()))
        elif n == 1 and key != "dv":
            continue                # below: the absolute limit
        else:
            _compare("xattn_bwd", c, key, got[key], ref[key], ac.BWD_BASE, rel_err(_np(model[key]), ref[key]))
    if n == 1:
        rq, rk = ac.nctx1_worst(c, inp, got["dq"], got["dk"], ac.BWD_BASE)
        print(f"attn-sweep xattn_bwd {c['kind']} dq/dk n_ctx=1: |dq| {rq:.3g}, |dk| {rk:.3g} of bound x the cancelling terms [{c['id']}]")
        assert rq <= 1.0 and rk <= 1.0, (c["id"], rq, rk)
    if c["known"] == "onehot":      # dv[j] = the fp32 sum of the dout rows that chose j (multiples of 1/8: exact in any order), rounded once
        ans = torch.from_numpy(ac.xattn_known_answers(c, inp)["dv"]).to(DEV).to(dt)
        assert torch.equal(res[2], ans), c["id"]
    if c["known"] == "onehot+zero":         # the one-hot rows among the rows of zeros still have dq = 0
        hot = torch.from_numpy(ac.onehot_choice(c) >= 0).to(DEV)
        assert not res[0].view(Bsz, L, c["H"], ac.D)[hot].any(), c["id"]
    if c["twice"]:
        assert all(torch.equal(a, b) for a, b in zip(call()[0], res)), c["id"]


# ---------------------------------------------------------------------------------------------------
# attention: refusals (RuntimeError, nothing launched)
# ---------------------------------------------------------------------------------------------------
def _small(dt, L=33, n=77, H=2, Bsz=2):
    g = torch.Generator().manual_seed(5)
    mk = lambda *s: torch.randn(*s, generator=g).to(DEV, dt)
    return mk(Bsz, L, H * ac.D), mk(Bsz, n, H * ac.D), mk(Bsz, n, H * ac.D), mk(Bsz, L, H * ac.D), H


def _no_launch(fn, match):
    """fn raises RuntimeError and no launch is recorded (the trace gets its entry after a successful launch only)"""
    from zigma_amd import _lib
    _lib.TRACE = []
    try:
        with pytest.raises(RuntimeError, match=match):
            fn()
        assert _lib.TRACE == []
    finally:
        _lib.TRACE = None


@pytest.mark.parametrize("scale", [0.0, -0.125, float("inf"), float("nan")], ids=["zero", "negative", "inf", "nan"])
def test_xattn_refuses_a_scale_outside_the_softmax_domain(scale):
    """the softmax takes its maximum over the raw scores and folds the scale into the exponent: a positive finite scale only, in both directions"""
    from zigma_amd.attention import cross_attn, cross_attn_bwd
    q, k, v, do, H = _small(torch.bfloat16)
    _no_launch(lambda: cross_attn(q, k, v, H, scale), "zigma_cross_attn_fwd")
    _no_launch(lambda: cross_attn(q.half(), k.half(), v.half(), H, scale), "zigma_cross_attn_fwd")
    _no_launch(lambda: cross_attn_bwd(q, k, v, do, H, scale), "zigma_cross_attn_bwd")


def test_xattn_refuses_shapes_types_and_strides_outside_its_limits():
    from zigma_amd.attention import cross_attn, cross_attn_bwd, cross_attn_bwd_eligible, cross_attn_eligible
    bf = torch.bfloat16
    q, k, v, do, H = _small(bf, n=129)
    assert not cross_attn_eligible(q, k, v, H) and not cross_attn_bwd_eligible(q, k, v, H)
    _no_launch(lambda: cross_attn(q, k, v, H), "cross_attn")
    _no_launch(lambda: cross_attn_bwd(q, k, v, do, H), "cross_attn_bwd")
    q, k, v, do, H = _small(torch.float16)               # fp16 into the backward: there is no fp16 backward kernel
    assert cross_attn_eligible(q, k, v, H) and not cross_attn_bwd_eligible(q, k, v, H)
    _no_launch(lambda: cross_attn_bwd(q, k, v, do, H), "cross_attn_bwd")
    q, k, v, do, H = _small(bf)
    C = H * ac.D
    wide = torch.randn(2, 33, C + 4, device=DEV).to(bf)
    for bad in (wide[..., :C], wide[..., 4:]):            # a row pitch of 8 bytes modulo 16; rows that start 8 bytes off
        assert bad.stride(1) % 8 != 0 and not cross_attn_eligible(bad, k, v, H)
        _no_launch(lambda: cross_attn(bad, k, v, H), "cross_attn")
        _no_launch(lambda: cross_attn_bwd(bad, k, v, do, H), "cross_attn_bwd")
        _no_launch(lambda: cross_attn_bwd(q, k, v, bad, H), "cross_attn_bwd")
    kwide = torch.randn(2, 77, C + 4, device=DEV).to(bf)[..., :C]
    _no_launch(lambda: cross_attn(q, kwide, v, H), "cross_attn")
    _no_launch(lambda: cross_attn_bwd(q, k, kwide, do, H), "cross_attn_bwd")


# ---------------------------------------------------------------------------------------------------
# glue backward
# ---------------------------------------------------------------------------------------------------
def _glue_device(c, inp):
    bf = torch.bfloat16
    dy = _sliced(inp["dy"], bf, ac.GLUE_SLICE if c["dy_slice"] else 0)
    a = _sliced(inp["a"], bf, ac.GLUE_SLICE if c["a_slice"] else 0)
    cols = c["cols"]
    sbuf = torch.full((c["B"], 3 * cols), NAN, dtype=bf, device=DEV)
    sbuf[:, cols:2 * cols] = torch.from_numpy(inp["s"]).to(DEV).to(bf)
    return dy, a, sbuf[:, cols:2 * cols]


def _glue_compare(ident, got, ref):
    for key, want in ref.items():
        g = got[key]
        if want is None:
            assert g is None, (ident, key)
            continue
        g = _np(g)
        assert g.shape == want.shape and np.isfinite(g).all(), (ident, key, "not finite")
        e, r = rel_err(g, want), ac.glue_worst(key, g, want, ac.GLUE_BASE)
        print(f"attn-sweep glue bf16 {key} norm-wise {e:.3e} (bound {ac.GLUE_BASE:.2e}, model -) row-wise {r:.3g} [{ident}]")
        assert e < ac.GLUE_BASE, (ident, key, e)
        assert r <= ac.ROW_GUARD, (ident, key, r)


@pytest.mark.parametrize("c", GLUE, ids=_ids(GLUE))
def test_glue_bwd_sweep(c):
    from zigma_amd import _lib
    from zigma_amd.layernorm import glue_bwd_eligible, scale_reduce_bwd
    Bsz, L, cols, bf = c["B"], c["L"], c["cols"], torch.bfloat16
    inp = ac.glue_inputs(c)
    dy, a, s = _glue_device(c, inp)
    assert glue_bwd_eligible(dy, a, s)

    def call(want_out):
        _poison(*([((Bsz, L, cols), bf)] * want_out + [((Bsz, L // 64, cols), torch.float32)] * (1 + c["want_sum"])))
        return _traced(lambda: scale_reduce_bwd(dy, a, s, s_add=float(c["s_add"]), want_out=want_out, want_sum=c["want_sum"]))
    res, trace = call(c["want_out"])
    assert [t[:2] for t in trace] == [("zigma_scale_reduce_bwd", "scale_reduce_bwd")], c["id"]
    P = trace[0][2]
    assert (P.rows, P.cols, P.rows_per_batch, P.dtype, P.flags, P.s_add) == (Bsz * L, cols, L, _lib.BF16, 0, float(c["s_add"])), c["id"]
    assert (P.dy_row_stride, P.a_row_stride, P.s_batch_stride) == (cols + ac.GLUE_SLICE * c["dy_slice"], cols + ac.GLUE_SLICE * c["a_slice"], 3 * cols)
    assert bool(P.out) == c["want_out"] and bool(P.r2) == c["want_sum"] and bool(P.r1), c["id"]
    _glue_compare(c["id"], dict(zip(("out", "r1", "r2"), res)), ac.glue_reference(c, inp))
    # the reduced sums do not depend on whether out is written: the other form returns the same r1 (and r2) bits, and None for out
    other, _ = call(not c["want_out"])
    assert (other[0] is None) == c["want_out"] and torch.equal(other[1], res[1]), c["id"]
    assert (other[2] is None and res[2] is None) or torch.equal(other[2], res[2]), c["id"]
    if c["twice"]:
        again, _ = call(c["want_out"])
        assert all((x is None and y is None) or torch.equal(x, y) for x, y in zip(again, res)), c["id"]


@pytest.mark.parametrize("r", ac.GLUE_REFUSALS, ids=[r["id"] for r in ac.GLUE_REFUSALS])
def test_glue_bwd_refuses_what_it_cannot_take(r):
    from zigma_amd.layernorm import glue_bwd_eligible, scale_reduce_bwd
    dt = DT[r["kind"]]
    dy, a, s = (torch.randn(*shape, device=DEV).to(dt) for shape in ((r["B"], r["L"], r["cols"]),) * 2 + ((r["B"], r["cols"]),))
    assert not glue_bwd_eligible(dy, a, s)
    _no_launch(lambda: scale_reduce_bwd(dy, a, s, s_add=1.0, want_sum=True), "zigma_scale_reduce_bwd")


# ---------------------------------------------------------------------------------------------------
# production shapes: float64 torch autograd on the device
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bf16", "f16"])
@pytest.mark.parametrize("Bsz,n", [(2, 77), (1, 128)], ids=["b2-n77", "b1-n128"])
def test_xattn_production_shape(Bsz, n, kind):
    """L = 1024, 8 heads, K / V the column halves of one batched projection (the layout the block produces): the forward in both I/O types,
    the backward in bf16, against float64 autograd through softmax(scale q k^T) v on the same operands."""
    from zigma_amd.attention import cross_attn, cross_attn_bwd
    L, H = 1024, 8
    C, dt = H * ac.D, DT[kind]
    c = dict(kind=kind, B=Bsz, L=L, H=H, n_ctx=n, scale=ac.SCALE0, id=f"production-{kind}-b{Bsz}-n{n}")
    g = torch.Generator().manual_seed(100 + n)
    mk = lambda *s: torch.randn(*s, generator=g).to(DEV).to(dt)
    q, kv, do = mk(Bsz, L, C), mk(Bsz, n, 2 * C), mk(Bsz, L, C)
    k, v = kv[..., :C], kv[..., C:]
    q64, k64, v64 = (t.double().requires_grad_(True) for t in (q, k, v))
    hd = lambda t: t.reshape(t.shape[0], t.shape[1], H, ac.D).transpose(1, 2)
    ref = (torch.softmax(hd(q64) @ hd(k64).transpose(-1, -2) * c["scale"], -1) @ hd(v64)).transpose(1, 2).reshape(Bsz, L, C)
    _poison(((Bsz, L, C), dt))
    out, trace = _traced(lambda: cross_attn(q, k, v, H))
    assert [t[:2] for t in trace] == [("zigma_cross_attn_fwd", "cross_attn_mfma")] and trace[0][2].k_row_stride == 2 * C
    _compare("xattn_fwd", c, "out", _np(out), _np(ref), ac.FWD_BASE[kind], rel_err(_np(ac.xattn_model(c, q, k, v)["out"]), _np(ref)))
    if kind != "bf16":
        return
    want = torch.autograd.grad(ref, (q64, k64, v64), do.double())
    _poison(((Bsz, L, C), dt), ((2, ac.chunks(L), Bsz, n, C), torch.float32))
    res, trace = _traced(lambda: cross_attn_bwd(q, k, v, do, H))
    assert [t[:2] for t in trace] == [("zigma_cross_attn_bwd", "cross_attn_bwd_mfma")] and trace[0][2].chunks == 2
    model = ac.xattn_model(c, q, k, v, do)
    for key, got, w in zip(("dq", "dk", "dv"), res, want):
        _compare("xattn_bwd", c, key, _np(got), _np(w), ac.BWD_BASE, rel_err(_np(model[key]), _np(w)))


@pytest.mark.parametrize("cols", [640, 768])
def test_glue_bwd_production_shape(cols):
    """(2, 1024, cols) as the block's modulate backward calls it (s_add = 1, both sums; s a third of the adaLN rows) against float64 autograd
    through y = a (1 + s) + shift"""
    from zigma_amd.layernorm import scale_reduce_bwd
    Bsz, L, bf = 2, 1024, torch.bfloat16
    g = torch.Generator().manual_seed(cols)
    mk = lambda *s: torch.randn(*s, generator=g).to(DEV).to(bf)
    dy, a, s = mk(Bsz, L, cols), mk(Bsz, L, cols), mk(Bsz, 3 * cols)[:, cols:2 * cols]
    a64, s64 = a.double().requires_grad_(True), s.double().requires_grad_(True)
    sh64 = torch.zeros(Bsz, cols, dtype=torch.float64, device=DEV, requires_grad=True)
    (a64 * (1 + s64.unsqueeze(1)) + sh64.unsqueeze(1)).backward(dy.double())
    _poison(((Bsz, L, cols), bf), ((Bsz, L // 64, cols), torch.float32), ((Bsz, L // 64, cols), torch.float32))
    res, trace = _traced(lambda: scale_reduce_bwd(dy, a, s, s_add=1.0, want_sum=True))
    assert [t[:2] for t in trace] == [("zigma_scale_reduce_bwd", "scale_reduce_bwd")]
    _glue_compare(f"production-{cols}", dict(zip(("out", "r1", "r2"), res)), dict(out=_np(a64.grad), r1=_np(s64.grad), r2=_np(sh64.grad)))

"""Classifier-free guidance on the GPU: the guided final-layer kernel zigma_final_layer_cfg_fwd (csrc/embed.hip) over the case table of
tests/cfg_cases.py, its exact invariants and refusals, ZigMa.forward_guided against the float64 oracle, and zigma_amd.guidance.Guided through the
ODE sampler and a captured graph.

The sweep fills the parameter block itself: `out` is a window of a NaN-filled buffer with non-compact row, channel, frame and sample strides.  Per case:
the bf16 LayerNorm rows the kernel reports (y_out) element by element against float64, at most DELTA_FLIPS of them off the correctly rounded value;
`out` against float64 evaluated on the kernel's OWN rows, IO_BOUND[out dtype] norm-wise and ROW_GUARD for every pixel row with
terms = ((1 - s) v_u, s v_c); everything outside the window still NaN.  Each case prints one `cfg-sweep` line.
"""
import ctypes

import numpy as np
import pytest
import torch

import cfg_cases as cc
from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
NAN = float("nan")
DT = {"f32": torch.float32, "bf16": BF}
CASES = cc.cfg_cases()


def _np(t):
    return t.detach().double().cpu().numpy()


def _dev(a, dtype=BF):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dtype)


def _block(c, x_c, x_u, w, bias, scale, out, y_out=None):
    """the parameter block of one call; out: the (B, [T,] C, H, W) window"""
    from zigma_amd import _lib
    P = _lib.FinalLayerCfgParams()
    P.rows, P.cols, P.n_out, P.dtype, P.out_dtype, P.flags, P.eps = c["rows"], c["cols"], c["n_out"], _lib.BF16, _lib._DT[out.dtype], 0, cc.CFG_EPS
    P.rows_per_sample, P.tokens_per_frame, P.grid_w, P.patch, P.chans = c["rps"], c["side"] ** 2, c["side"], c["patch"], c["chans"]
    P.x_row_stride = x_c.stride(0)
    P.out_sample_stride, P.out_chan_stride, P.out_row_stride = out.stride(0), out.stride(-3), out.stride(-2)
    P.out_frame_stride = out.stride(1) if c["frames"] else 0
    P.x_cond, P.x_uncond, P.weight, P.scale, P.out = x_c.data_ptr(), x_u.data_ptr(), w.data_ptr(), scale.data_ptr(), out.data_ptr()
    P.bias = None if bias is None else bias.data_ptr()
    P.y_out = None if y_out is None else y_out.data_ptr()
    return P


def _call(P):
    from zigma_amd import _lib
    _lib.call("zigma_final_layer_cfg_fwd", P, torch.device(DEV))
    assert _lib.last_kernel() == "final_layer_cfg", _lib.last_kernel()


def _operands(c, inp):
    """x rows as windows of a NaN-filled buffer with a pitch (both halves in ONE buffer, cond rows first, as the model passes them)"""
    rows, cols = c["rows"], c["cols"]
    xbuf = torch.full((2 * rows + 1, 8 + cols + 8), NAN, dtype=BF, device=DEV)
    x = xbuf[:2 * rows, 8:8 + cols]
    x.copy_(_dev(np.concatenate([inp["x_c"], inp["x_u"]], 0)))
    bias = None if inp["bias"] is None else _dev(inp["bias"])
    return xbuf, x[:rows], x[rows:], _dev(inp["w"]), bias, _dev(inp["scale"], torch.float32)


# ---------------------------------------------------------------------------------------------------
# (a) the sweep
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_cfg_sweep(c):
    inp = cc.cfg_inputs(c)
    xbuf, x_c, x_u, w, bias, scale = _operands(c, inp)
    shape, index = cc.out_window(c)
    buf = torch.full(shape, NAN, dtype=DT[c["out"]], device=DEV)
    out = buf[index]
    y = torch.full((2 * c["rows"] + 1, c["cols"]), NAN, dtype=BF, device=DEV)
    _call(_block(c, x_c, x_u, w, bias, scale, out, y))
    torch.cuda.synchronize()
    outside = torch.isnan(buf)
    outside[index] = True
    assert bool(outside.all()), (c["id"], "written outside the output window")
    assert bool(torch.isnan(y[-1]).all()) and bool(torch.isnan(xbuf[-1]).all()), (c["id"], "written past the LayerNorm rows / into x")
    y_own, got, bound = _np(y[:-1]), _np(out), cc.IO_BOUND[c["out"]]
    assert np.isfinite(y_own).all() and np.isfinite(got).all(), (c["id"], "an element was left unwritten, or a NaN / inf was computed")
    ref = cc.cfg_reference(c, inp, y_own=y_own)
    yw, flips = cc.elementwise_worst(y_own, ref["y"], cc.IO_BOUND["bf16"]), cc.flipped_share(y_own, ref["y"], "bf16")
    e = cc.norm_err(got, ref["out"]) if np.linalg.norm(ref["out"]) > 0 else float(np.linalg.norm(got))
    r = cc.row_ratio(got, ref["out"], bound, ref["terms"])
    print(f"cfg-sweep {c['id']}: y_out element-wise ratio {yw:.3g}, off the correctly rounded value in {flips:.4f}; out norm-wise {e:.3e} "
          f"(bound {bound:.2e}), row-wise ratio {r:.3g}")
    assert yw <= cc.ROW_GUARD and flips <= cc.DELTA_FLIPS, (c["id"], yw, flips)
    assert got.shape == ref["out"].shape and e <= bound and r <= cc.ROW_GUARD, (c["id"], e, bound, r)


# ---------------------------------------------------------------------------------------------------
# (b) exact invariants
# ---------------------------------------------------------------------------------------------------
INVARIANT = [c for c in CASES if c["rows"] < 65536][::5]


def _plain_unpatchified(c, x, w, bias):
    """zigma_final_layer_fwd on the rows x, unpatchified by torch's reshape + permute"""
    from zigma_amd.embed import final_layer
    v = final_layer(x.contiguous(), w, bias, cc.CFG_EPS)
    B, T, g, p, ch = c["batch"], c["frames"], c["side"], c["patch"], c["chans"]
    if T:
        return v.reshape(B, T, g, g, p, p, ch).permute(0, 1, 6, 2, 4, 3, 5).reshape(B, T, ch, g * p, g * p)
    return v.reshape(B, g, g, p, p, ch).permute(0, 5, 1, 3, 2, 4).reshape(B, ch, g * p, g * p)


@pytest.mark.parametrize("c", INVARIANT, ids=[c["id"] for c in INVARIANT])
def test_cfg_exact_invariants(c):
    """scale 0, and the same pointer for both halves with any finite scale: bit for bit the plain final layer of the uncond rows in bf16"""
    inp = cc.cfg_inputs(c)
    _, x_c, x_u, w, bias, _ = _operands(c, inp)
    shape = cc.out_window(c)[0][:-3] + (c["chans"],) + (c["side"] * c["patch"],) * 2
    want = _plain_unpatchified(c, x_u, w, bias)
    out = torch.full(shape, NAN, dtype=BF, device=DEV)
    _call(_block(c, x_c, x_u, w, bias, torch.zeros(c["batch"], device=DEV), out))
    assert torch.equal(out, want), (c["id"], "scale 0 is not the unconditional final layer")
    for s in (1.5, -3.0, 7.5):
        out.fill_(NAN)
        _call(_block(c, x_u, x_u, w, bias, torch.full((c["batch"],), s, device=DEV), out))
        assert torch.equal(out, want), (c["id"], s, "equal halves are not the plain final layer")


# ---------------------------------------------------------------------------------------------------
# (c) refusals
# ---------------------------------------------------------------------------------------------------
def _break(what, P, t):
    from zigma_amd import _lib
    if what == "rows-negative":
        P.rows = -4
    elif what in ("cols4", "cols12", "cols2056"):
        P.cols = int(what[4:])
    elif what in ("n_out0", "n_out17"):
        P.n_out = int(what[5:])
    elif what == "flags1":
        P.flags = 1
    elif what in ("f16", "f32-in"):
        P.dtype = _lib.F16 if what == "f16" else _lib.F32
    elif what == "out-f16":
        P.out_dtype = _lib.F16
    elif what == "patch0":
        P.patch = 0
    elif what == "n_out-not-p2c":
        P.chans = 2
    elif what == "rows-not-samples":
        P.rows_per_sample = 3
    elif what == "sample-not-frames":
        P.tokens_per_frame = 3
    elif what == "frame-not-grid":
        P.grid_w = 3
    elif what.startswith("null-"):
        setattr(P, what[5:], None)
    elif what == "x-off-by-one":
        P.x_uncond = P.x_uncond + 2
    elif what == "x-pitch-odd":
        P.x_row_stride = 68
    elif what == "weight-off-by-one":
        P.weight = P.weight + 2
    elif what == "y_out-off-by-one":
        P.y_out = t["y"].data_ptr() + 2
    else:
        raise KeyError(what)


@pytest.mark.parametrize("what,status", cc.REFUSALS, ids=[w for w, _ in cc.REFUSALS])
def test_cfg_refusals(what, status):
    from zigma_amd import _lib
    c = dict(rows=8, cols=64, n_out=3, rps=4, side=2, patch=1, chans=3, frames=0)
    bf = lambda *s: torch.ones(*s, dtype=BF, device=DEV)
    t = dict(x=bf(16, 2056), w=bf(17, 2056), scale=torch.ones(2, device=DEV), out=torch.full((2, 3, 2, 2), NAN, device=DEV), y=bf(17, 2056))
    P = _block(c, t["x"][:8], t["x"][8:], t["w"], None, t["scale"], t["out"])
    _call(P)                                   # the block is valid before it is broken
    assert bool(torch.isfinite(t["out"]).all())
    t["out"].fill_(NAN)
    before = [v.clone() for v in t.values()]
    if what == "null-block":
        L = _lib.lib()
        assert L.zigma_final_layer_cfg_fwd(None, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == status
    else:
        _break(what, P, t)
        with pytest.raises(RuntimeError, match=rf"\(status {status}\)"):
            _lib.call("zigma_final_layer_cfg_fwd", P, torch.device(DEV))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b, ) or (torch.isnan(a).all() and torch.isnan(b).all()) for a, b in zip(before, t.values())), (what, "a refused call wrote")


def test_cfg_empty_call_touches_nothing():
    c = dict(rows=0, cols=64, n_out=3, rps=4, side=2, patch=1, chans=3, frames=0)
    x, w, out = torch.ones(8, 64, dtype=BF, device=DEV), torch.ones(3, 64, dtype=BF, device=DEV), torch.full((1, 3, 2, 2), NAN, device=DEV)
    from zigma_amd import _lib
    _lib.call("zigma_final_layer_cfg_fwd", _block(c, x, x, w, None, torch.ones(1, device=DEV), out), torch.device(DEV))       # ZIGMA_OK
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


# ---------------------------------------------------------------------------------------------------
# (d) the model
# ---------------------------------------------------------------------------------------------------
TOY = dict(in_channels=4, embed_dim=64, depth=2, img_dim=8, patch_size=1, num_classes=4, scan_type="zigzagN8", use_pe=2)


def _toy(dtype=BF, **kw):
    from zigma_amd.model_zigma import ZigMa
    cfg = dict(TOY)
    cfg.update(kw)
    torch.manual_seed(0)
    m = ZigMa(device=DEV, dtype=dtype, class_dropout_prob=0.1 if cfg.get("num_classes", -1) > 0 else 0.0, **cfg).eval()
    with torch.no_grad():
        for blk in m.blocks:
            blk.adaLN_modulation[-1].weight.normal_(std=0.3)
            blk.adaLN_modulation[-1].bias.normal_(std=0.3)
        if cfg.get("num_classes", -1) > 0:
            m.y_embedder.embedding_table.weight.normal_(std=1.0)         # the condition matters: v_c and v_u differ
    return m, cfg


def _terms_err(got, vc, vu, s):
    """norm of the error over the norm of the two summands (1 - s) v_u and s v_c"""
    s = np.asarray(s, np.float64).reshape(-1, *([1] * (vc.ndim - 1)))
    a, b = (1 - s) * vu, s * vc
    return float(np.linalg.norm(got - (a + b)) / (np.linalg.norm(a) + np.linalg.norm(b)))


def test_forward_guided_vs_oracle(monkeypatch):
    """the toy class-conditional bf16 model against the float64 oracle's guided velocity (label 4 is the null row of its embedding table);
    the kernel path and the torch composition (USE_EMBED_KERNELS=False) under the same limit"""
    from oracle import zigma_oracle as zo
    from zigma_amd import _lib, embed
    m, cfg = _toy()
    g = torch.Generator().manual_seed(5)
    x, t, y = torch.randn(2, 4, 8, 8, generator=g).to(DEV), torch.tensor([0.25, 0.5], device=DEV), torch.tensor([1, 3], device=DEV)       # (1000 t is a bf16 value)
    scales = torch.tensor([1.5, 4.0], device=DEV)
    om = zo.ZigMaOracle({k: v.detach().float().cpu().numpy() for k, v in m.state_dict().items()}, cfg, dt=np.float64)
    xn, tn = x.to(BF).double().cpu().numpy(), t.double().cpu().numpy()          # (the model casts x to its dtype at the boundary)
    fr = zo.bf16_round                      # the frequency table and the timestep features are bf16 tensors of the model
    vc, vu = om.forward(xn, tn, np.array([1, 3]), freq_round=fr), om.forward(xn, tn, np.array([4, 4]), freq_round=fr)
    assert rel_err(vc, vu) > 0.05, "the toy model ignores its condition"
    with torch.no_grad():
        _lib.TRACE = []
        out = m.forward_guided(x, t, y, scales)
        names = [k for _, k, _ in _lib.TRACE]
        _lib.TRACE = None
        assert _lib.last_kernel() == "final_layer_cfg" and names.count("final_layer_cfg") == 1 and "final_layer" not in names
        assert out.shape == x.shape and out.dtype == x.dtype
        e_kernel = _terms_err(_np(out), vc, vu, [1.5, 4.0])
        assert torch.equal(m.forward_guided(x, t, y, 1.0), m(x, t, y))              # a float of 1.0: the plain conditional forward
        assert torch.equal(m.forward_guided(x.to(BF), t, y, scales, y_null=torch.tensor([4, 4], device=DEV)).float(),
                           m.forward_guided(x.to(BF), t, y, scales).float())
        assert m.forward_guided(x.to(BF), t, y, scales).dtype == BF
        monkeypatch.setattr(embed, "USE_EMBED_KERNELS", False)
        _lib.TRACE = []
        comp = m.forward_guided(x, t, y, scales)
        names = [k for _, k, _ in _lib.TRACE]
        _lib.TRACE = None
        assert "final_layer_cfg" not in names
        e_comp = _terms_err(_np(comp), vc, vu, [1.5, 4.0])
    print(f"cfg-model toy class-conditional bf16: guided kernel {e_kernel:.3e}, torch composition {e_comp:.3e} (limit 1e-2, terms norm)")
    assert e_kernel < 1e-2 and e_comp < 1e-2, (e_kernel, e_comp)


def test_forward_guided_text_and_video():
    """a text-conditional toy model with y_null = zeros, and a video toy model with 2 frames: the kernel path equals its own plain forwards combined,
    up to the roundings the kernel leaves out"""
    from zigma_amd import _lib
    for kw, xs in ((dict(num_classes=-1, has_text=True, d_context=32, n_context_token=7), (2, 4, 8, 8)),
                   (dict(video_frames=2, scan_type="zzvideo_sst", use_pe=0, tpe=True), (2, 2, 4, 8, 8))):
        m, cfg = _toy(**kw)
        g = torch.Generator().manual_seed(6)
        x, t = torch.randn(*xs, generator=g).to(DEV), torch.rand(2, generator=g).to(DEV)
        if cfg.get("has_text"):
            y, y_null = torch.randn(2, 7, 32, generator=g).to(DEV), torch.zeros(2, 7, 32, device=DEV)
        else:
            y, y_null = torch.tensor([0, 2], device=DEV), None
        with torch.no_grad():
            out = m.forward_guided(x, t, y, 4.0, y_null=y_null)
            assert _lib.last_kernel() == "final_layer_cfg"
            vc = m(x, t, y)
            vu = m(x, t, y_null if y_null is not None else torch.full_like(y, 4))
        assert out.shape == x.shape and out.dtype == torch.float32 and bool(torch.isfinite(out).all())
        e = _terms_err(_np(out), _np(vc), _np(vu), [4.0, 4.0])
        print(f"cfg-model {'text' if cfg.get('has_text') else 'video'} toy: guided kernel against its own two forwards combined {e:.3e}")
        assert e < 1e-2, e


# ---------------------------------------------------------------------------------------------------
# (e) sampler and graph
# ---------------------------------------------------------------------------------------------------
def test_guided_through_the_sampler():
    from zigma_amd.guidance import Guided
    from zigma_amd.transport import Sampler, create_transport
    m, _ = _toy()
    g = torch.Generator().manual_seed(7)
    z, y = torch.randn(2, 4, 8, 8, generator=g).to(DEV), torch.tensor([0, 2], device=DEV)
    fn = Sampler(create_transport()).sample_ode(sampling_method="euler", num_steps=4)
    with torch.no_grad():
        traj = fn(z, Guided(m, 4.0), y=y)
        ts, ones, x = torch.linspace(0.0, 1.0, 4).to(DEV), torch.ones(2, device=DEV), z
        for k in range(3):
            x = x + (ts[k + 1] - ts[k]) * m.forward_guided(x, ones * ts[k], y, 4.0)
    assert traj.shape == (4, 2, 4, 8, 8) and torch.equal(traj[-1], x)


def test_guided_graph_follows_set_scale():
    from zigma_amd.graphs import GraphedForward
    from zigma_amd.guidance import Guided
    m, _ = _toy()
    g = torch.Generator().manual_seed(8)
    x, t, y = torch.randn(2, 4, 8, 8, generator=g).to(DEV), torch.rand(2, generator=g).to(DEV), torch.tensor([1, 3], device=DEV)
    guided = Guided(m, [1.5, 4.0])
    graphed = GraphedForward(guided, x, t, y)
    with torch.no_grad():
        assert torch.equal(graphed(x, t, y), m.forward_guided(x, t, y, torch.tensor([1.5, 4.0], device=DEV)))
        guided.set_scale([7.5, -1.0])
        want = m.forward_guided(x, t, y, torch.tensor([7.5, -1.0], device=DEV))
        assert torch.equal(graphed(x, t, y), want)
        assert not torch.equal(want, m.forward_guided(x, t, y, torch.tensor([1.5, 4.0], device=DEV)))


# ---------------------------------------------------------------------------------------------------
# (f) autograd
# ---------------------------------------------------------------------------------------------------
def test_forward_guided_is_differentiable():
    """under autograd forward_guided is the composed expression v_u + s (v_c - v_u) of two differentiable forwards: the same gradient for x"""
    m, _ = _toy(dtype=torch.float32)
    g = torch.Generator().manual_seed(9)
    x, t, y = torch.randn(2, 4, 8, 8, generator=g).to(DEV), torch.rand(2, generator=g).to(DEV), torch.tensor([1, 3], device=DEV)
    probe = torch.randn(2, 4, 8, 8, generator=g).to(DEV)
    xa = x.clone().requires_grad_(True)
    (m.forward_guided(xa, t, y, 4.0) * probe).sum().backward()
    xb = x.clone().requires_grad_(True)
    vc, vu = m(xb, t, y), m(xb, t, torch.full_like(y, 4))
    ((vu + 4.0 * (vc - vu)) * probe).sum().backward()
    assert xa.grad is not None and bool(torch.isfinite(xa.grad).all()) and float(xa.grad.abs().max()) > 0
    assert rel_err(_np(xa.grad), _np(xb.grad)) < 1e-5, rel_err(_np(xa.grad), _np(xb.grad))

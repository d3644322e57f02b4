"""GPU tests of mixed precision: fp32 parameters under torch.autocast on the own 16-bit kernels (zigma_amd/amp.py and the op layer's autocast rules).

What the reference does with custom_fwd / custom_bwd (selective_scan_interface.py:295-312,368): the two GEMM weights of the Mamba inner are cast to the
autocast type, conv taps / A / D / delta_bias stay fp32, the backward runs without autocast and hands every parameter its gradient in the parameter's
own type.  Bounds: `tests/test_gpu_wgrad.py`'s BOUND32 for fp32 weight gradients against float64, the bf16 model-level limits of test_gpu_backward.py
(input gradient 8e-2, per-tensor cosine 0.95) and test_gpu_parity.py (output 4e-2) for the whole model.

Measured on the MI355X: every test prints its figures; DESIGN.md §6.2 quotes them."""
import ast
import contextlib

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.bfloat16, torch.float16]
BOUND32 = 2e-5                    # tests/test_gpu_wgrad.py


def N(t):
    return t.detach().double().cpu().numpy()


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def autocast(dtype):
    return torch.autocast("cuda", dtype=dtype)


# ---- 1. the Mamba inner, exact ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", [64, 100])
@pytest.mark.parametrize("mode", ["zigzag", "reset16"])
def test_inner_under_autocast_equals_the_hand_rounded_call(mode, L, dtype, monkeypatch):
    """mamba_inner_tok under autocast with fp32 weights against the same call without autocast on hand-rounded x_proj / dt_proj weights (conv taps, A, D
    and delta_bias fp32 in both): y, d(xz), d(conv weight / bias), dA, dD, d(delta_bias) bit for bit; the two GEMM weight gradients arrive in fp32, their
    rounding to the 16-bit type equals the hand-rounded run's gradient bit for bit and they are within BOUND32 of the float64 product of the operands the
    backward formed."""
    import zigma_amd.selective_scan_interface as ssi
    from oracle import zigma_oracle as zo
    g = torch.Generator(device="cpu").manual_seed(17 * L + (dtype == torch.float16))
    Bsz, Di, R, Nst = 2, 128, 8, 16
    mk = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(DEV)
    xz0 = mk(Bsz, L, 2 * Di).to(dtype)
    cw0, cb0 = mk(Di, 1, 4, sc=0.5), mk(Di, sc=0.1)
    xw0, dw0 = mk(R + 2 * Nst, Di, sc=Di ** -0.5), mk(Di, R, sc=R ** -0.5)
    A0 = (-torch.exp(torch.randn(Di, Nst, generator=g) * 0.5)).to(DEV)
    D0, db0 = mk(Di), (torch.rand(Di, generator=g) * 0.5).to(DEV)
    wgt = mk(Bsz, L, Di).to(dtype)
    side = int(L ** 0.5)
    kw = dict(perm=torch.as_tensor(zo.zigzag_paths(side)[1].copy()).to(DEV, torch.int32)) if mode == "zigzag" else dict(reset_period=16)
    seen = []
    real = ssi.wgrad

    def spy(dy2, x2, **k):
        out = real(dy2, x2, **k)
        seen.append((dy2.clone(), x2.clone(), out))
        return out

    monkeypatch.setattr(ssi, "wgrad", spy)
    from zigma_amd import amp
    res, casts = {}, dict(amp.STATS)
    for amp_run in (True, False):
        leaves = [t.clone().requires_grad_(True) for t in (xz0, cw0, cb0, xw0 if amp_run else xw0.to(dtype), dw0 if amp_run else dw0.to(dtype), A0, D0, db0)]
        del seen[:]
        with (autocast(dtype) if amp_run else contextlib.nullcontext()):
            y = ssi.mamba_inner_tok(*leaves, **kw)
        (y.float() * wgt.float()).sum().backward()
        res[amp_run] = (y.detach(), [t.grad for t in leaves], list(seen))
    # (these parameters are registered nowhere: each shadow is a one-entry launch of the cast kernel, and no arena is touched)
    assert amp.STATS["single_casts"] - casts["single_casts"] == 2 and amp.STATS["refresh_launches"] == casts["refresh_launches"]
    (ya, ga, sa), (yh, gh, sh) = res[True], res[False]
    assert ya.dtype == dtype and torch.equal(ya, yh)
    for i, name in ((0, "dxz"), (1, "d conv weight"), (2, "d conv bias"), (5, "dA"), (6, "dD"), (7, "d delta_bias")):
        assert ga[i].dtype == gh[i].dtype and torch.equal(ga[i], gh[i]), name
    assert all(ga[i].dtype == torch.float32 for i in (1, 2, 5, 6, 7))
    for i, name in ((3, "d x_proj weight"), (4, "d dt_proj weight")):
        assert ga[i].dtype == torch.float32 and gh[i].dtype == dtype
        same = torch.equal(ga[i].to(dtype), gh[i])
        print(f"inner {mode} L={L} {dtype} {name}: fp32 gradient rounded == hand-rounded run's: {same}; "
              f"differing elements {int((ga[i].to(dtype) != gh[i]).sum())} of {gh[i].numel()}")
        assert same, name
    assert len(sa) == 2 and len(sh) == 2
    for (dy2, x2, out), (dy2h, x2h, _) in zip(sa, sh):
        assert torch.equal(dy2, dy2h) and torch.equal(x2, x2h)                      # the backward formed the same operands
        err = rel_err(N(out), N(dy2.double().T @ x2.double()))
        print(f"inner {mode} L={L} {dtype} dW {tuple(out.shape)} fp32 vs float64: {err:.3e}")
        assert out.dtype == torch.float32 and err < BOUND32, err


# ---- 2. projections -----------------------------------------------------------------------------------------------------------------------------------
ROLE_SHAPES = {"in_proj": (2560, 640, False), "out_proj": (640, 1280, False), "to_q": (512, 640, False), "to_out": (640, 512, True)}      # n, k, bias (E = 640)


def _smallest_own_tokens(role, n, k):
    from zigma_amd import routing
    for tokens in range(8, 1 << 17, 8):
        if routing.route(role, tokens, n, k).kernel != "library":
            return tokens
    raise AssertionError(role)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("role", list(ROLE_SHAPES))
def test_projection_under_autocast_takes_the_route_of_the_16bit_model(role, dtype):
    """an fp32 nn.Linear weight beside a 16-bit activation under autocast, at the smallest token count the routing table serves with an own kernel:
    the plan is the table's row and the kernel that ran is that row's; the forward equals the same route on the hand-made shadow bit for bit; under
    autograd the forward and dX equal LinearTrainFn on a 16-bit twin bit for bit (both on zigma_linear_fwd, from the call trace) and dW / dbias arrive
    in fp32 within BOUND32 of float64."""
    from zigma_amd import _lib, amp, routing
    from zigma_amd.linear import plan, project, run
    from zigma_amd.wgrad import LinearTrainFn
    n, k, bias = ROLE_SHAPES[role]
    tokens = _smallest_own_tokens(role, n, k)
    g = torch.Generator(device="cpu").manual_seed(tokens + n)
    lin = torch.nn.Linear(k, n, bias=bias).to(DEV)
    if bias:
        with torch.no_grad():
            lin.bias.normal_(std=0.1)
    x = torch.randn(1, tokens, k, generator=g).to(DEV, dtype)
    dy = torch.randn(1, tokens, n, generator=g).to(DEV, dtype)
    ws, bs = lin.weight.detach().to(dtype), (lin.bias.detach().to(dtype) if bias else None)
    want = routing.route(role, tokens, n, k)
    with torch.no_grad(), autocast(dtype):
        r = plan(role, x, lin.weight, lin.bias)
        assert r.kernel == want.kernel and r.row == want.row and r.kernel != "library", (r, want)
        y = project(role, x, lin.weight, lin.bias)
        kern = _lib.last_kernel()
    assert kern.startswith(routing.kernel_name(r, tokens, n, k, bias=bias)), (kern, r)
    with torch.no_grad():
        r2 = plan(role, x, ws, bs)
        assert r2 == r
        y_ref = run(r2, x, ws, bs)
    assert y.dtype == dtype and torch.equal(y, y_ref)
    assert torch.equal(amp.shadow(lin.weight, dtype), ws)
    # autograd
    x1, x2 = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    wt, bt = ws.clone().requires_grad_(True), (bs.clone().requires_grad_(True) if bias else None)
    trace = []
    _lib.TRACE = trace
    try:
        with autocast(dtype):
            r_t = plan(role, x1, lin.weight, lin.bias)
            y1 = project(role, x1, lin.weight, lin.bias)
        y1.backward(dy)
    finally:
        _lib.TRACE = None
    assert r_t.kernel == "library" and r_t.row == "autograd"            # the block roles hand autograd calls to LinearTrainFn, whose route is "train"
    n_own = sum(1 for fn, _, _ in trace if fn == "zigma_linear_fwd")
    train_route = routing.route("train", tokens, n, k)
    assert train_route.kernel != "library" and n_own == 2, (train_route, [t[:2] for t in trace])          # forward and dX
    y2 = LinearTrainFn.apply(x2, wt, bt)
    y2.backward(dy)
    assert torch.equal(y1.detach(), y2.detach()) and torch.equal(x1.grad, x2.grad)
    dy2, xx = dy.reshape(-1, n), x.reshape(-1, k)
    err = rel_err(N(lin.weight.grad), N(dy2.double().T @ xx.double()))
    print(f"projection {role} {dtype} tokens={tokens} route {r.row} / train {train_route.row}: dW fp32 vs float64 {err:.3e}")
    assert lin.weight.grad.dtype == torch.float32 and err < BOUND32, err
    if bias:
        errb = rel_err(N(lin.bias.grad), N(dy2.double().sum(0)))
        print(f"projection {role} {dtype}: dbias fp32 vs float64 {errb:.3e}")
        assert lin.bias.grad.dtype == torch.float32 and errb < BOUND32, errb


# ---- 3. the model -------------------------------------------------------------------------------------------------------------------------------------
def _load(name, dtype=torch.float32):
    from zigma_amd.model_zigma import ZigMa
    g, gg = load_golden(name + ".npz"), load_golden("bwd_model_" + name + ".npz")
    cfg = ast.literal_eval(str(g["cfg"]))
    m = ZigMa(device=DEV, dtype=dtype, **cfg).eval()
    m.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd.")}, strict=True)
    return m, g, gg


def _grad_figures(m, g, gg, ctx):
    """input-gradient error and worst per-tensor cosine of the parameter gradients against the reference's fp32 autograd (loss = sum(out * wgt))"""
    x = T(g["x"]).requires_grad_(True)
    y = T(g["y"]) if "y" in g else None
    with ctx:
        out = m(x, T(g["t"]), y)
    (out * T(gg["wgt"])).sum().backward()
    worst, where = 1.0, None
    for k, p in m.named_parameters():
        if "g." + k not in gg or p.grad is None:
            continue
        a, b = N(p.grad).ravel(), gg["g." + k].ravel().astype(np.float64)
        if np.linalg.norm(b) < 1e-6:
            continue
        c = float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b) + 1e-30))
        if c < worst:
            worst, where = c, k
    return rel_err(N(x.grad), gg["gx"]), worst, where, rel_err(N(out), g["out"])


@pytest.mark.parametrize("name", ["zigma_uncond_zigzag8", "zigma_text_zigzag2"])
def test_model_gradients_under_autocast_close_to_fp32_reference(name):
    """the fp32 model under autocast(bf16) against the reference's fp32 autograd, with the limits of test_model_gradients_bf16_close_to_fp32_reference
    (input gradient < 8e-2, worst per-tensor cosine > 0.95): the autocast run rounds fewer operands than the bf16 model that test accepts.  The text
    model, which that test does not cover, runs its bf16 twin here: the autocast run's worst cosine is no lower than the twin's minus 0.01.  Every
    parameter with a reference gradient has a finite fp32 .grad."""
    from zigma_amd import amp
    m, g, gg = _load(name)
    before = dict(amp.STATS)
    gx, worst, where, eo = _grad_figures(m, g, gg, autocast(torch.bfloat16))
    print(f"model {name} autocast(bf16): out {eo:.3e}, input gradient {gx:.3e}, worst cosine {worst:.4f} ({where}); "
          f"refreshes {amp.STATS['refresh_launches'] - before['refresh_launches']}, single casts {amp.STATS['single_casts'] - before['single_casts']}")
    for k, p in m.named_parameters():
        assert p.dtype == torch.float32
        if "g." + k in gg:
            assert p.grad is not None and p.grad.dtype == torch.float32 and bool(torch.isfinite(p.grad).all()), k
    assert amp.STATS["refresh_launches"] - before["refresh_launches"] == 1 and amp.STATS["single_casts"] == before["single_casts"]
    if name == "zigma_text_zigzag2":
        mt, _, _ = _load(name, torch.bfloat16)
        gxt, worst_t, where_t, eot = _grad_figures(mt, g, gg, contextlib.nullcontext())
        print(f"model {name} bf16 twin: out {eot:.3e}, input gradient {gxt:.3e}, worst cosine {worst_t:.4f} ({where_t})")
        assert worst >= worst_t - 0.01, (worst, worst_t)
    assert gx < 8e-2, gx
    assert worst > 0.95, (worst, where)


@pytest.mark.parametrize("name", ["zigma_uncond_zigzag8", "zigma_text_zigzag2"])
def test_model_no_grad_under_autocast(name):
    """torch.no_grad() under autocast (a training script's periodic sampling): the fused block path on the shadows, within the bf16 model-level limit of
    test_model_bf16_vs_reference_golden (4e-2); the blocks' projections, x_proj and the scan ran on own kernels (from the call trace)"""
    from zigma_amd import _lib
    m, g, gg = _load(name)
    y = T(g["y"]) if "y" in g else None
    trace = []
    _lib.TRACE = trace
    try:
        with torch.no_grad(), autocast(torch.bfloat16):
            out = m(T(g["x"]), T(g["t"]), y)
    finally:
        _lib.TRACE = None
    err = rel_err(N(out), g["out"])
    served = sorted({kern for _, kern, _ in trace})
    print(f"model {name} no_grad autocast(bf16): out {err:.3e}; kernels {served}")
    assert out.dtype == torch.float32 and err < 4e-2, err
    fns = {fn for fn, _, _ in trace}
    assert {"zigma_selective_scan_fwd", "zigma_causal_conv1d_fwd", "zigma_add_norm_fwd", "zigma_multi_cast_fwd"} <= fns, fns
    # (the fixtures are below every own projection kernel's token count: the fused path's projections under autocast are
    #  test_fused_blocks_no_grad_under_autocast_run_the_routes_of_the_bf16_model below)


def test_fused_blocks_no_grad_under_autocast_run_the_routes_of_the_bf16_model():
    """the fused no-grad block path at a size the routing table serves with own projection kernels (2048 tokens, E = 128: out_proj / to_q / to_out on the
    few-token kernel): the fp32 model under autocast(bf16) launches the same projection kernels as its bf16 twin, and its output is within the
    model-level bf16 limit (4e-2) of the fp32 model's"""
    from zigma_amd import _lib
    from zigma_amd.model_zigma import ZigMa
    cfg = dict(in_channels=4, embed_dim=128, depth=2, img_dim=16, patch_size=1, has_text=True, d_context=32, n_context_token=7, scan_type="zigzagN8", use_pe=2)
    torch.manual_seed(0)
    m32 = ZigMa(device=DEV, dtype=torch.float32, **cfg).eval()
    with torch.no_grad():
        for blk in m32.blocks:
            blk.adaLN_modulation[-1].weight.normal_(std=0.05)
            blk.adaLN_modulation[-1].bias.normal_(std=0.3)
    m16 = ZigMa(device=DEV, dtype=torch.bfloat16, **cfg).eval()
    m16.load_state_dict(m32.state_dict())
    x, t, y = torch.randn(8, 4, 16, 16, device=DEV), torch.rand(8, device=DEV), torch.rand(8, 7, 32, device=DEV)
    kernels = {}
    outs = {}
    for tag, model, cast in (("autocast", m32, True), ("bf16", m16, False)):
        _lib.TRACE = []
        try:
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=cast):
                outs[tag] = model(x, t, y)
        finally:
            trace, _lib.TRACE = _lib.TRACE, None
        kernels[tag] = sorted(k for fn, k, _ in trace if fn in ("zigma_linear_fwd", "zigma_norm_linear_fwd"))
    with torch.no_grad():
        ref = m32(x, t, y)
    err = rel_err(N(outs["autocast"]), N(ref))
    print(f"fused blocks under autocast: projection kernels {kernels['autocast']}; out vs fp32 model {err:.3e} (bf16 twin {rel_err(N(outs['bf16']), N(ref)):.3e})")
    assert kernels["autocast"] == kernels["bf16"] and sum(k.startswith("linear_sm") for k in kernels["autocast"]) >= 6, kernels
    assert err < 4e-2, err


# ---- 4. the training loop -----------------------------------------------------------------------------------------------------------------------------
def _small_model():
    from zigma_amd.model_zigma import ZigMa
    torch.manual_seed(0)
    return ZigMa(in_channels=4, embed_dim=128, depth=2, img_dim=8, patch_size=1, scan_type="zigzagN8", use_pe=2, device=DEV, dtype=torch.float32).train()


@pytest.mark.parametrize("fused", [False, True])
def test_training_loop_under_autocast_refreshes_the_shadows_once_per_step(fused):
    """(fused=True: torch's fused AdamW writes the parameters without moving their version counters; the optimizer-step hook of amp.attach sees it)
    the 12-step AdamW loop of test_training_step_bf16_runs_and_decreases_loss on an fp32 model under autocast(bf16): finite decreasing loss, fp32
    parameters, after every optimizer step the next forward reads shadows equal to p.to(bf16) (a stale arena fails here), exactly one refresh launch per
    step, none for a second forward without a step, no single casts"""
    from zigma_amd import amp
    from zigma_amd.transport import create_transport
    m = _small_model()
    opt = torch.optim.AdamW(m.parameters(), lr=2e-3, fused=fused)
    tr = create_transport()
    x1 = torch.randn(8, 4, 8, 8, device=DEV)
    d = torch.bfloat16
    before = dict(amp.STATS)
    losses = []
    for step in range(12):
        opt.zero_grad(set_to_none=True)
        with autocast(d):
            loss = tr.training_losses(m, x1)["loss"].mean()
        grp = m._amp_group
        assert len(grp.params) == 2 * 4                                            # in_proj, x_proj, dt_proj, out_proj of two blocks
        assert amp.STATS["refresh_launches"] - before["refresh_launches"] == step + 1
        for p, s in zip(grp.params, grp.arenas[d]["shadows"]):
            assert torch.equal(s, p.detach().to(d)) and s.data_ptr() % 256 == 0
        if step in (3, 7):                                                         # the no-grad sampling inside a training script: nothing to cast,
            m.eval()                                                               # and nothing stale: at step 7 every cache of the fused path
            t_s = torch.linspace(0.1, 0.9, 8, device=DEV)                          # (adaLN stack, A / D / dt bias) was filled four optimizer steps ago
            with torch.no_grad(), autocast(d):
                o1 = m(x1, t_s)
            assert amp.STATS["refresh_launches"] - before["refresh_launches"] == step + 1
            m._cond_cache = None
            for blk in m.blocks:
                blk.mixer._const_cache.clear()
            with torch.no_grad(), autocast(d):
                o2 = m(x1, t_s)
            assert torch.equal(o1, o2), (step, float((o1 - o2).abs().max()))
            m.train()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print(f"autocast(bf16) loop losses: {losses[0]:.4f} -> {losses[-1]:.4f}; STATS {amp.STATS}")
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    assert all(p.dtype == torch.float32 and p.grad.dtype == torch.float32 for p in m.parameters() if p.grad is not None)
    assert amp.STATS["single_casts"] == before["single_casts"]


def test_training_loop_fp16_with_grad_scaler():
    from zigma_amd.transport import create_transport
    m = _small_model()
    opt = torch.optim.AdamW(m.parameters(), lr=2e-3)
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 10)
    tr = create_transport()
    x1 = torch.randn(8, 4, 8, 8, device=DEV)
    probe = m.blocks[0].mixer.in_proj.weight
    losses, stepped = [], 0
    for _ in range(4):
        opt.zero_grad(set_to_none=True)
        with autocast(torch.float16):
            loss = tr.training_losses(m, x1)["loss"].mean()
        scaler.scale(loss).backward()
        v = probe._version
        scaler.step(opt)
        scaler.update()
        stepped += probe._version != v
        losses.append(float(loss.detach()))
    print(f"autocast(fp16) + GradScaler: losses {losses}, steps taken {stepped} of 4, scale {scaler.get_scale()}")
    assert all(np.isfinite(losses)) and stepped >= 1
    assert all(p.dtype == torch.float32 for p in m.parameters())


def test_deepcopy_of_an_attached_model_attaches_its_own_group():
    """copy.deepcopy (an EMA copy) carries a copy of the group; the copy's first forward under autocast registers its OWN parameters instead of paying a
    one-entry cast per use"""
    import copy
    from zigma_amd import amp
    m = _small_model().eval()
    x, t = torch.randn(2, 4, 8, 8, device=DEV), torch.rand(2, device=DEV)
    with torch.no_grad(), autocast(torch.bfloat16):
        o = m(x, t)
    m2 = copy.deepcopy(m)
    assert amp.attached(m) and not amp.attached(m2)
    before = dict(amp.STATS)
    with torch.no_grad(), autocast(torch.bfloat16):
        o2 = m2(x, t)
    assert amp.attached(m2) and m2._amp_group.params[0] is m2.blocks[0].mixer.in_proj.weight and m._amp_group.params[0] is m.blocks[0].mixer.in_proj.weight
    assert amp.STATS["single_casts"] == before["single_casts"] and amp.STATS["refresh_launches"] == before["refresh_launches"] + 1
    assert torch.equal(o, o2)


def test_use_shadows_knob_is_bit_identical(monkeypatch):
    """amp.USE_SHADOWS = False (a `.to()` per use) gives the same loss and the same gradients, bit for bit"""
    from zigma_amd import amp
    from zigma_amd.transport import create_transport
    m = _small_model()
    with torch.no_grad():
        for blk in m.blocks:
            blk.adaLN_modulation[-1].weight.normal_(std=0.05)
            blk.adaLN_modulation[-1].bias.normal_(std=0.3)
    tr = create_transport()
    x1 = torch.randn(8, 4, 8, 8, device=DEV)
    res = {}
    for knob in (True, False):
        monkeypatch.setattr(amp, "USE_SHADOWS", knob)
        m.zero_grad(set_to_none=True)
        torch.manual_seed(3)
        before = dict(amp.STATS)
        with autocast(torch.bfloat16):
            loss = tr.training_losses(m, x1)["loss"].mean()
        loss.backward()
        if not knob:
            assert amp.STATS == before                                             # no launch of the cast kernel at all
        res[knob] = (loss.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None})
    assert torch.equal(res[True][0], res[False][0])
    assert res[True][1].keys() == res[False][1].keys() and len(res[True][1]) > 10
    for k in res[True][1]:
        assert torch.equal(res[True][1][k], res[False][1][k]), k

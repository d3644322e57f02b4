"""GPU tests of the fused training-step tail: zigma_optim_grad_sumsq / zigma_optim_prepare / zigma_optim_adamw (csrc/optim_step.hip) and
zigma_amd.optim.FusedAdamW.

Reference of the kernels: the float64 oracle of tests/optim_cases.py (pinned to torch on the CPU by tests/test_optim_cpu.py).  Bound: per element,
K x 2^-24 x the stream's scale, K = twice what an op-by-op float32 evaluation of the same chain shows against the oracle on the same inputs
(optim_cases.error_constant; 8.3 ... 11.4, computed from numpy, never from the kernel).  The oracle takes the clip coefficient the device computed:
it comes from a float32 sum of squares that is good to 1e-5 (below), far coarser than 2^-24, and is checked on its own against float64.
Every fp32 stream of the sweep is a window of a NaN-filled buffer, every shadow a window of a sentinel-filled one.

Measured on the MI355X: every test prints its figures; DESIGN.md §6.3 quotes them."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import optim_cases as oc

pytestmark = pytest.mark.gpu
DEV = "cuda"
FORMS = {"bf16": torch.bfloat16, "f16": torch.float16, "none": None}
OK, NULL, SHAPE, DTYPE, UNSUPPORTED = 0, -1, -2, -3, -6
ENTRY_POINTS = ("zigma_optim_grad_sumsq", "zigma_optim_prepare", "zigma_optim_adamw")


def _params(table, cmap, n_entries, n_chunks, state, partials, shadow_dtype, *, wd=0.0, max_norm=0.0, grad_scale=None, found_inf=None, chunk=oc.CHUNK, **over):
    from zigma_amd import _lib
    h = dict(oc.HYPER, **over)
    P = _lib.OptimParams()
    P.table, P.chunk_map, P.n_entries, P.n_chunks = _lib.ptr(table), _lib.ptr(cmap), n_entries, n_chunks
    P.partials, P.state, P.grad_scale, P.found_inf = _lib.ptr(partials), _lib.ptr(state), _lib.ptr(grad_scale), _lib.ptr(found_inf)
    P.lr, P.beta1, P.beta2, P.eps, P.weight_decay, P.max_grad_norm, P.ema_decay = h["lr"], h["beta1"], h["beta2"], h["eps"], wd, max_norm, h["ema_decay"]
    P.shadow_dtype, P.chunk, P.flags = (-1 if shadow_dtype is None else _lib._DT[shadow_dtype]), chunk, 0
    return P


def _three(P):
    from zigma_amd import _lib
    trace = []
    _lib.TRACE = trace
    try:
        for name in ENTRY_POINTS:
            _lib.call(name, P, torch.device(DEV, torch.cuda.current_device()))
    finally:
        _lib.TRACE = None
    torch.cuda.synchronize()
    return [t[:2] for t in trace]


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


# ---- 1. the sweep against float64 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", list(oc.CONFIGS))
def test_sweep_against_float64(name, form):
    """168 rows in ONE launch of each kernel: the sizes around every path, one present stream misplaced by 1 ... 3 elements on 132 rows (element by
    element), all on 16-byte boundaries on 36 (8 per lane and the tail), rows without EMA, rows without shadow.  p, m, v, ema within K of the oracle on
    every element; grad_norm within 1e-5 of float64 (a sum of non-negative terms with at most 16 + 9 float32 roundings per workgroup at chunk 4096 is
    good to 25 x 2^-24 < 3e-6 relative, the final sum is in double); the shadow BIT-equal to the kernel's own fp32 parameter rounded by `.to()`; the
    gradients bit-unchanged; everything outside the windows untouched.  form "none": shadow_dtype -1 with the table's shadow column filled in anyway —
    it is ignored, the buffer keeps its sentinel."""
    from zigma_amd import amp
    cfg, dtype = oc.CONFIGS[name], FORMS[form]
    rows = oc.sweep_values(1 + cfg["step0"], cfg["step0"] == 0)
    bufs, shadow_len, wins = oc.sweep_layout(rows)
    dev = {k: torch.from_numpy(bufs[k]).to(DEV) for k in oc.STREAMS}
    sh = torch.full((shadow_len,), oc.SENTINEL, dtype=torch.int16, device=DEV)
    assert all(t.data_ptr() % 16 == 0 for t in dev.values()) and sh.data_ptr() % 16 == 0
    addr = lambda w, k: 0 if w[k] is None else (sh.data_ptr() + 2 * w[k] if k == "shadow" else dev[k].data_ptr() + 4 * w[k])
    table_rows = [[addr(w, k) for k in ("p", "g", "m", "v", "ema", "shadow")] + [w["n"], 0] for w in wins]
    n_wide = sum(1 for r in table_rows if r[6] >= 8 and all(a % 16 == 0 for a in r[:6]))
    n_slow = sum(1 for r in table_rows if r[6] and any(a % 16 for a in r[:6]))
    assert len(rows) >= 150 and n_wide >= 24 and n_slow >= 120
    assert sum(r[4] == 0 for r in table_rows) >= 20 and sum(r[5] == 0 for r in table_rows) >= 20
    cmap_rows = amp.build_chunk_map([w["n"] for w in wins], oc.CHUNK)
    table = torch.tensor(table_rows, dtype=torch.int64).to(DEV)
    cmap = torch.tensor(cmap_rows, dtype=torch.int64).to(DEV)
    state = torch.zeros(8, device=DEV)
    state[0] = float(cfg["step0"])
    partials = torch.full((len(cmap_rows),), float("nan"), device=DEV)
    g_before = dev["g"].clone()
    P = _params(table, cmap, len(table_rows), len(cmap_rows), state, partials, dtype, wd=cfg["wd"], max_norm=cfg["max_norm"])
    kernels = _three(P)
    assert kernels == [("zigma_optim_grad_sumsq", "multi_sumsq"), ("zigma_optim_prepare", "step_prepare"),
                       ("zigma_optim_adamw", {"bf16": "multi_adamw_bf16", "f16": "multi_adamw_f16", "none": "multi_adamw"}[form])]
    st = state.cpu()
    step, skipped, gnorm, mult = float(st[0]), int(st.view(torch.int32)[1]), float(st[2]), float(st[3])
    norm64 = oc.grad_norm64([r["g"] for r in rows])
    clip64 = oc.clip_coef(norm64, cfg["max_norm"])
    print(f"sweep {name} {form}: grad_norm {gnorm!r} vs float64 {norm64!r} (rel {abs(gnorm - norm64) / norm64:.2e}); grad_mult {mult!r} vs {clip64!r}")
    assert step == cfg["step0"] + 1 and skipped == 0
    assert abs(gnorm - norm64) <= 1e-5 * norm64
    assert mult == 1.0 if clip64 == 1.0 else abs(mult - clip64) <= (1e-5 + 2.0 ** -23) * clip64
    h = oc.HYPER
    assert abs(float(st[4]) - h["lr"] / (1 - h["beta1"] ** step)) <= 2.0 ** -23 * float(st[4])
    assert abs(float(st[5]) - np.sqrt(1 - h["beta2"] ** step)) <= 2.0 ** -23 * float(st[5])
    K, _ = oc.error_constant(name)
    out = {k: dev[k].cpu().numpy() for k in oc.STREAMS}
    worst = {}
    for r, w in zip(rows, wins):
        n = w["n"]
        if not n:
            continue
        has_ema = w["ema"] is not None
        cut = lambda k: out[k][w[k]:w[k] + n]
        ref = oc.oracle_step(r["p"], r["g"], r["m"], r["v"], r["ema"] if has_ema else None, step=step, wd=cfg["wd"], grad_mult=mult, **h)
        got = (cut("p"), cut("m"), cut("v"), cut("ema") if has_ema else None)
        for k, x in oc.error_multiples(got, ref, (r["p"], r["m"], r["v"], r["ema"]), r["g"].astype(np.float64) * mult).items():
            worst[k] = max(worst.get(k, 0.0), x)
    print(f"sweep {name} {form}: worst error in units of 2^-24 x scale {worst}; K = {K:.3f}")
    assert max(worst.values()) <= K, (worst, K)
    assert torch.equal(_bits(dev["g"]), _bits(g_before))                                                  # the gradients: read only
    shc = sh.cpu()
    inside = {k: np.zeros(bufs[k].size, dtype=bool) for k in oc.STREAMS}
    sh_inside = torch.zeros(shadow_len, dtype=torch.bool)
    p_new = dev["p"].cpu()
    for w in wins:
        for k in oc.STREAMS:
            if w[k] is not None:
                inside[k][w[k]:w[k] + w["n"]] = True
        if w["shadow"] is not None and dtype is not None:
            sh_inside[w["shadow"]:w["shadow"] + w["n"]] = True
            want = p_new[w["p"]:w["p"] + w["n"]].to(dtype).view(torch.int16)
            assert torch.equal(shc[w["shadow"]:w["shadow"] + w["n"]], want), w
    assert bool((shc[~sh_inside] == oc.SENTINEL).all())
    for k in oc.STREAMS:
        assert np.array_equal(out[k].view(np.int32)[~inside[k]], bufs[k].view(np.int32)[~inside[k]]), k
        assert not np.isnan(out[k][inside[k]]).any(), k


# ---- 2. exact invariants --------------------------------------------------------------------------------------------------------------------------------
class _Case:
    """a few rows of ordinary tensors (all streams present, bf16 shadows): sizes across the paths, the second row misplaced by one element"""

    def __init__(self, seed=3, g_zero=False, first=False):
        g = torch.Generator().manual_seed(seed)
        self.ns, offs = [257, oc.CHUNK + 9, 8, 3 * oc.CHUNK], [0, 1, 0, 0]
        mk = lambda n, o, f: f(n + o).to(DEV)[o:]
        self.p = [mk(n, o, lambda k: torch.randn(k, generator=g)) for n, o in zip(self.ns, offs)]
        self.g = [mk(n, o, lambda k: torch.zeros(k) if g_zero else torch.randn(k, generator=g) * 0.1) for n, o in zip(self.ns, offs)]
        self.m = [mk(n, o, lambda k: torch.zeros(k) if first else torch.randn(k, generator=g) * 0.05) for n, o in zip(self.ns, offs)]
        self.v = [mk(n, o, lambda k: torch.zeros(k) if first else torch.rand(k, generator=g) * 0.01 + 1e-4) for n, o in zip(self.ns, offs)]
        self.ema = [t.clone() * 1.01 for t in self.p]
        self.sh = [torch.full((n,), oc.SENTINEL, dtype=torch.int16, device=DEV) for n in self.ns]
        from zigma_amd import amp
        rows = [[a.data_ptr(), b.data_ptr(), c.data_ptr(), d.data_ptr(), e.data_ptr(), f.data_ptr(), n, 0]
                for a, b, c, d, e, f, n in zip(self.p, self.g, self.m, self.v, self.ema, self.sh, self.ns)]
        cm = amp.build_chunk_map(self.ns, oc.CHUNK)
        self.table, self.cmap = torch.tensor(rows, dtype=torch.int64).to(DEV), torch.tensor(cm, dtype=torch.int64).to(DEV)
        self.n_chunks = len(cm)
        self.state = torch.zeros(8, device=DEV)
        self.state[0] = 0.0 if first else 41.0
        self.partials = torch.zeros(self.n_chunks, device=DEV)

    def outputs(self):
        return self.p + self.m + self.v + self.ema + self.sh + [self.state, self.partials]

    def snapshot(self):
        return [_bits(t).clone() for t in self.outputs()]

    def params(self, **kw):
        return _params(self.table, self.cmap, len(self.ns), self.n_chunks, self.state, self.partials, torch.bfloat16, **kw)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_zero_lr_and_zero_decay_leave_the_parameters():
    c = _Case()
    before = [_bits(t).clone() for t in c.p]
    m_before = [t.clone() for t in c.m]
    _three(c.params(lr=0.0, wd=0.0, max_norm=1.0))
    assert _same(before, [_bits(t) for t in c.p]) and float(c.state[0]) == 42.0
    assert all(not torch.equal(a, b) for a, b in zip(m_before, c.m))                                        # (the step did run)
    assert all(torch.equal(s, p.to(torch.bfloat16).view(torch.int16)) for s, p in zip(c.sh, c.p))


@pytest.mark.parametrize("how", ["found_inf", "inf_gradient", "nan_gradient"])
def test_a_skipped_step_changes_nothing(how):
    """found_inf = 1, or one inf / NaN in one gradient seen through the norm alone: p, m, v, ema, shadow and the step counter keep their bits, and
    `skipped` reads 1"""
    c = _Case()
    found = torch.ones(1, device=DEV) if how == "found_inf" else None
    if how != "found_inf":
        c.g[1][oc.CHUNK + 3] = float("inf") if how == "inf_gradient" else float("nan")
    before = [_bits(t).clone() for t in c.p + c.m + c.v + c.ema + c.sh]
    _three(c.params(wd=0.05, max_norm=1.0, found_inf=found))
    assert _same(before, [_bits(t) for t in c.p + c.m + c.v + c.ema + c.sh])
    assert float(c.state[0]) == 41.0 and int(c.state.view(torch.int32)[1]) == 1
    if how == "inf_gradient":
        assert float(c.state[2]) == float("inf")
    if how == "found_inf":                                                                                  # ... and a step without it is taken
        found.zero_()
        _three(c.params(wd=0.05, max_norm=1.0, found_inf=found))
        assert float(c.state[0]) == 42.0 and int(c.state.view(torch.int32)[1]) == 0 and not torch.equal(before[0], _bits(c.p[0]))


def test_zero_gradients_on_the_first_step_leave_weight_decay_only():
    c = _Case(g_zero=True, first=True)
    p0 = [t.clone() for t in c.p]
    wd = 0.1
    _three(c.params(wd=wd, max_norm=1.0))
    lr_wd = torch.tensor(np.float32(oc.HYPER["lr"] * wd), device=DEV)
    for a, b in zip(c.p, p0):
        assert torch.equal(_bits(a), _bits(b - b * lr_wd)) and not torch.equal(a, b)
    assert all(bool((t == 0).all()) for t in c.m + c.v) and float(c.state[0]) == 1.0 and float(c.state[2]) == 0.0 and float(c.state[3]) == 1.0


def test_two_runs_from_the_same_state_give_the_same_bits():
    a, b = _Case(seed=9), _Case(seed=9)
    grad_scale = torch.full((1,), 4.0, device=DEV)
    assert _same(a.snapshot(), b.snapshot())
    for c in (a, b):
        _three(c.params(wd=0.05, max_norm=0.5, grad_scale=grad_scale))
    assert _same(a.snapshot(), b.snapshot()) and float(a.state[0]) == 42.0
    # grad_scale: the norm is of the UNSCALED gradients, and the update sees grad * clip / scale
    norm = oc.grad_norm64([t.cpu().numpy() for t in a.g]) / 4.0
    assert abs(float(a.state[2]) - norm) <= 1e-5 * norm and abs(float(a.state[3]) - oc.clip_coef(norm, 0.5) / 4.0) <= 2e-5 * float(a.state[3])


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_zero_counts_and_rows_outside_the_table():
    """every refusal of the header, in its order, from each of the three entry points, with all outputs untouched; zero counts launch nothing;
    chunk-map rows outside the table (or past a tensor's end) are skipped"""
    from zigma_amd import _lib
    L = _lib.lib()
    c = _Case()
    c.partials.fill_(-7.0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    before = c.snapshot()

    def call(fn, **kw):
        P = c.params(wd=0.05, max_norm=1.0)
        for k, v in kw.items():
            setattr(P, k, v)
        rc = getattr(L, fn)(ctypes.byref(P), stream)
        torch.cuda.synchronize()
        return rc

    nan, inf = float("nan"), float("inf")
    cases = [(dict(n_entries=-1), SHAPE), (dict(n_chunks=-1), SHAPE), (dict(n_chunks=1 << 31), SHAPE), (dict(n_entries=-1, shadow_dtype=7), SHAPE),
             (dict(shadow_dtype=_lib.F32), DTYPE), (dict(shadow_dtype=7), DTYPE), (dict(shadow_dtype=-2), DTYPE), (dict(shadow_dtype=7, flags=1), DTYPE),
             (dict(flags=1), UNSUPPORTED), (dict(flags=1, n_entries=0), UNSUPPORTED),
             (dict(n_entries=0), OK), (dict(n_chunks=0), OK), (dict(n_entries=0, table=None, chunk_map=None, state=None, partials=None, chunk=0, lr=nan), OK),
             (dict(chunk=0), SHAPE), (dict(chunk=12), SHAPE), (dict(chunk=-4096), SHAPE), (dict(chunk=65544), SHAPE), (dict(chunk=12, beta1=1.0), SHAPE),
             (dict(beta1=1.0), UNSUPPORTED), (dict(beta1=-0.1), UNSUPPORTED), (dict(beta2=1.0), UNSUPPORTED), (dict(beta2=nan), UNSUPPORTED),
             (dict(eps=0.0), UNSUPPORTED), (dict(eps=-1e-8), UNSUPPORTED), (dict(eps=nan), UNSUPPORTED),
             (dict(lr=nan), UNSUPPORTED), (dict(lr=inf), UNSUPPORTED), (dict(lr=-inf), UNSUPPORTED)]
    for fn in ENTRY_POINTS:
        for kw, want in cases:
            assert call(fn, **kw) == want, (fn, kw, want)
            assert _same(before, c.snapshot()), (fn, kw)
    null_cases = {"zigma_optim_grad_sumsq": ["table", "chunk_map", "partials"], "zigma_optim_prepare": ["state"], "zigma_optim_adamw": ["table", "chunk_map", "state"]}
    for fn, names in null_cases.items():
        for n in names:
            assert call(fn, **{n: None}) == NULL and call(fn, **{n: None, "chunk": 12}) == NULL, (fn, n)          # (NULL is checked before the chunk)
            assert _same(before, c.snapshot()), (fn, n)
    assert L.zigma_optim_adamw(None, stream) == NULL
    # map rows outside the table: the streaming kernels skip them (the norm pass stores 0 as that workgroup's sum) and follow no pointer
    good = c.cmap.clone()
    for row in ([len(c.ns), 0], [-1, 0], [0, 257], [0, -8], [0, 1 << 40]):
        c.cmap[0] = torch.tensor(row, dtype=torch.int64)
        c.partials.fill_(-7.0)
        assert call("zigma_optim_grad_sumsq") == OK and float(c.partials[0]) == 0.0 and float(c.partials[1]) > 0.0, row
        st = c.state.clone()
        st.view(torch.int32)[1] = 0
        st[3], st[4], st[5] = 1.0, 1e-3, 1.0                                       # (a state block as a taken step's prepare leaves it)
        c.state.copy_(st)
        p_all = [t.clone() for t in c.p]
        assert call("zigma_optim_adamw") == OK
        assert torch.equal(c.p[0], p_all[0]) and bool((c.sh[0] == oc.SENTINEL).all()) and not torch.equal(c.p[1], p_all[1]), row
    c.cmap.copy_(good)
    # a prepare call without the norm pass (partials NULL): no norm, no clip, found_inf alone decides
    assert call("zigma_optim_prepare", partials=None) == OK
    assert bool(torch.isnan(c.state[2])) and float(c.state[3]) == 1.0 and int(c.state.view(torch.int32)[1]) == 0
    with pytest.raises(RuntimeError, match="status -3"):
        P = c.params()
        P.shadow_dtype = 9
        _lib.call("zigma_optim_adamw", P, c.state.device)


# ---- 4. the optimizer -------------------------------------------------------------------------------------------------------------------------------------
def _small_model():
    from zigma_amd.model_zigma import ZigMa
    torch.manual_seed(0)
    return ZigMa(in_channels=4, embed_dim=128, depth=2, img_dim=8, patch_size=1, scan_type="zigzagN8", use_pe=2, device=DEV, dtype=torch.float32).train()


def _batch():
    return torch.randn(8, 4, 8, 8, generator=torch.Generator().manual_seed(77)).to(DEV)


def _loss(tr, m, x1, dtype):
    torch.manual_seed(1234)                                                        # the same (t, noise) every step: the loss is one function, and it falls
    with torch.autocast("cuda", dtype=dtype):
        return tr.training_losses(m, x1)["loss"].mean()


def test_five_step_loop_writes_the_shadows_itself():
    """FusedAdamW(max_grad_norm, EMA copy, shadows=model) on an fp32 model under autocast(bf16): a finite falling loss; after every step the next forward
    reads shadows bit-equal to p.to(bf16) with NO refresh launch (the only one is the first forward's) and no single casts; exactly three zigma_optim_*
    launches per step; the EMA copy follows"""
    from zigma_amd import _lib, amp, optim
    from zigma_amd.transport import create_transport
    m = _small_model()
    ema = copy.deepcopy(m)
    opt = optim.FusedAdamW(m.parameters(), lr=2e-3, max_grad_norm=2.0, ema_params=ema, ema_decay=0.9, shadows=m)
    tr, x1, d = create_transport(), _batch(), torch.bfloat16
    before, steps0 = dict(amp.STATS), amp.step_count()
    losses = []
    tracked = list(zip(m.parameters(), ema.parameters()))[:8]
    ema_ref = [e.detach().double().clone() for _, e in tracked]
    for step in range(6):
        opt.zero_grad()
        loss = _loss(tr, m, x1, d)
        grp = m._amp_group
        assert amp.STATS["refresh_launches"] - before["refresh_launches"] == 1, step
        for p, s in zip(grp.params, grp.arenas[d]["shadows"]):
            assert torch.equal(_bits(s), _bits(p.detach().to(d))), step
        losses.append(float(loss.detach()))
        if step == 5:
            break
        loss.backward()
        trace = []
        _lib.TRACE = trace
        try:
            opt.step()
        finally:
            _lib.TRACE = None
        assert [t[:2] for t in trace] == [("zigma_optim_grad_sumsq", "multi_sumsq"), ("zigma_optim_prepare", "step_prepare"), ("zigma_optim_adamw", "multi_adamw_bf16")]
        assert amp.step_count() == steps0 + step + 1 and int(opt.skipped) == 0 and float(opt.step_count) == step + 1
        for r, (p, _) in zip(ema_ref, tracked):
            r.add_((p.detach().double() - r) * (1 - 0.9))
    print(f"FusedAdamW loop losses {losses}; last grad norm {float(opt.grad_norm):.4f}; STATS {amp.STATS} {optim.STATS}")
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    assert amp.STATS["single_casts"] == before["single_casts"]
    assert opt._tables.builds == 1                                                  # zero_grad kept the gradients where they were
    for r, (p, e) in zip(ema_ref, tracked):                                         # the EMA copy, updated where it lives, follows its recurrence
        assert float((e.detach().double() - r).abs().max()) <= 2e-6 * float(p.detach().abs().max()) and not torch.equal(e, p)
    assert all(e.dtype == torch.float32 for e in ema.parameters())


def _run_loop(kind, steps=5):
    from zigma_amd import optim
    from zigma_amd.transport import create_transport
    m = _small_model()
    ema = copy.deepcopy(m)
    ps, es = list(m.parameters()), list(ema.parameters())
    kw = dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
    decay = 0.9
    if kind == "own":
        opt = optim.FusedAdamW(ps, max_grad_norm=2.0, ema_params=es, ema_decay=decay, shadows=m, **kw)
    else:
        opt = torch.optim.AdamW(ps, fused=kind == "fused", foreach=kind == "foreach", **kw)
    tr, x1 = create_transport(), _batch()
    for _ in range(steps):
        opt.zero_grad()
        _loss(tr, m, x1, torch.bfloat16).backward()
        if kind != "own":
            torch.nn.utils.clip_grad_norm_(ps, 2.0)
        opt.step()
        if kind != "own":
            with torch.no_grad():                                                  # update_ema: ema = decay * ema + (1 - decay) * p
                torch._foreach_mul_(es, decay)
                torch._foreach_add_(es, [p.detach() for p in ps], alpha=1 - decay)
    return [p.detach().double().cpu() for p in ps], [e.detach().double().cpu() for e in es]


def _distance(a, b):
    """worst per-tensor relative L2 over parameters and EMA"""
    return max(float((x - y).norm() / y.norm().clamp_min(1e-30)) for s, t in zip(a, b) for x, y in zip(s, t))


def test_agreement_with_the_torch_composition_after_five_steps():
    """clip -> torch.optim.AdamW(fused=True) -> EMA formula against FusedAdamW, 5 steps from the same seed.  Yardstick D: what AdamW(fused=True) and
    AdamW(foreach=True) show against EACH OTHER in the same loop (two torch implementations; the code under test is not involved).  Limit max(2 D, 1e-6)."""
    fused, foreach, own = _run_loop("fused"), _run_loop("foreach"), _run_loop("own")
    D, got = _distance(foreach, fused), _distance(own, fused)
    print(f"5-step loop: D (torch fused vs torch foreach) = {D:.3e}; FusedAdamW vs torch fused = {got:.3e}; limit {max(2 * D, 1e-6):.3e}")
    assert got <= max(2 * D, 1e-6), (got, D)


def test_fp16_loop_with_the_stock_grad_scaler():
    """torch.amp.GradScaler(init_scale=2**16) hands the optimizer grad_scale / found_inf as device tensors (_step_supports_amp_scaling): in 6 steps at
    least one is skipped and one taken; a skipped step leaves every parameter, moment and EMA tensor bit-unchanged and halves the scale.  The batch is
    10 x unit normal: at unit scale no gradient of the 2^16-fold loss leaves fp16's range and nothing is ever skipped; at 10 x the loss and its
    gradients are ~100 x larger and the first two steps of a stock torch.optim.AdamW loop on the same data overflow (scale 65536 -> 16384), the rest are taken."""
    from zigma_amd import optim
    from zigma_amd.transport import create_transport
    m = _small_model()
    ema = copy.deepcopy(m)
    opt = optim.FusedAdamW(m.parameters(), lr=2e-3, max_grad_norm=2.0, ema_params=ema, shadows=(m, torch.float16))
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 16)
    tr, x1 = create_transport(), 10.0 * _batch()
    everything = lambda: list(m.parameters()) + list(ema.parameters()) + opt._m + opt._v + [opt.step_count]
    log = []
    for _ in range(6):
        opt.zero_grad()
        loss = _loss(tr, m, x1, torch.float16)
        scaler.scale(loss).backward()
        before, scale = [_bits(t.detach()).clone() for t in everything()], scaler.get_scale()
        scaler.step(opt)
        assert not hasattr(opt, "grad_scale") and not hasattr(opt, "found_inf")           # (GradScaler removes what it set)
        skipped = int(opt.skipped)
        scaler.update()
        same = _same(before, [_bits(t.detach()) for t in everything()])
        log.append((skipped, scale, scaler.get_scale(), float(opt.grad_norm), float(loss.detach())))
        if skipped:
            assert same and scaler.get_scale() == scale / 2
        else:
            assert not same and scaler.get_scale() == scale and np.isfinite(float(opt.grad_norm))
    print(f"fp16 + GradScaler(2**16): (skipped, scale before, after, grad norm, loss) {log}")
    assert any(s for s, *_ in log) and any(not s for s, *_ in log), log
    assert all(p.dtype == torch.float32 and bool(torch.isfinite(p).all()) for p in m.parameters())


def test_state_dict_travels_to_torch_adamw_and_back():
    """2 steps here, state_dict() into torch.optim.AdamW(fused=True), one step with identical gradients in both: parameters agree within 2 K units
    (each side within K of the exact step; K = the sweep's largest), then torch's state_dict back into a new FusedAdamW and one more step.  The small
    model's tensors, filled from the domain K was derived on: |p| in [1e-2, 1] (its zero-initialised tensors would put p next to 0, where |p_old| + |dp|
    is no scale for an update of size lr), gradients 0.02 x normal, lr = 1e-3 — four steps move no parameter by more than 4e-3."""
    from zigma_amd import optim
    K = max(oc.error_constant(n)[0] for n in oc.CONFIGS)
    gen = torch.Generator().manual_seed(21)
    m1 = _small_model()
    with torch.no_grad():
        for p in m1.parameters():
            sign = torch.where(torch.rand(p.shape, generator=gen) < 0.5, -1.0, 1.0)
            p.copy_((sign * 10.0 ** (-2.0 * torch.rand(p.shape, generator=gen))).to(DEV))
    m2, m3 = copy.deepcopy(m1), None
    ps1, ps2 = list(m1.parameters()), list(m2.parameters())
    kw = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)

    def grads(*sets):
        for group in zip(*sets):
            g = (torch.randn(group[0].shape, generator=gen) * 0.02).to(DEV)
            for p in group:
                p.grad = g.clone()

    def agree(a, b, old, what):
        worst = 0.0
        for x, y, o in zip(a, b, old):
            x, y, o = x.detach().double(), y.detach().double(), o.double()
            scale = (o.abs() + (x - o).abs()) * oc.U
            worst = max(worst, float(((x - y).abs() / scale.clamp_min(1e-300)).max()))
        print(f"state_dict interchange, {what}: worst parameter difference {worst:.2f} units of 2^-24 x (|p_old| + |dp|); limit {2 * K:.2f}")
        assert worst <= 2 * K, what

    opt1 = optim.FusedAdamW(ps1, **kw)
    for _ in range(2):
        grads(ps1)
        opt1.step()
    for p, q in zip(ps1, ps2):
        q.data.copy_(p.data)
    opt2 = torch.optim.AdamW(ps2, fused=True, **kw)
    opt2.load_state_dict(opt1.state_dict())
    assert all(float(opt2.state[q]["step"]) == 2.0 for q in ps2) and len({opt2.state[q]["step"].data_ptr() for q in ps2}) == len(ps2)
    old = [p.detach().clone() for p in ps1]
    grads(ps1, ps2)
    opt1.step()
    opt2.step()
    agree(ps1, ps2, old, "FusedAdamW -> torch AdamW(fused)")
    m3 = copy.deepcopy(m2)
    ps3 = list(m3.parameters())
    opt3 = optim.FusedAdamW(ps3, lr=1.0)                                            # (the loaded group brings torch's lr, betas, eps and decay)
    opt3.load_state_dict(opt2.state_dict())
    assert float(opt3.step_count) == 3.0 and opt3.param_groups[0]["lr"] == 1e-3 and opt3.param_groups[0]["weight_decay"] == 0.05
    assert all(torch.equal(opt3.state[a]["exp_avg"], opt2.state[b]["exp_avg"]) for a, b in zip(ps3, ps2))
    old = [p.detach().clone() for p in ps2]
    grads(ps2, ps3)
    opt2.step()
    opt3.step()
    assert float(opt3.step_count) == 4.0
    agree(ps3, ps2, old, "torch AdamW(fused) -> FusedAdamW")


def test_a_captured_step_replays_bit_for_bit():
    """one eager step (it builds the tables), then one step captured under torch.cuda.graph on static gradients: three replays equal three eager steps
    bit for bit — parameters, moments, EMA, shadow-free, the device step counter"""
    from zigma_amd import optim
    gen = torch.Generator().manual_seed(4)
    shapes = [(300, 70), (oc.CHUNK + 1,), (5,), (64, 64)]
    base = [torch.randn(*s, generator=gen) for s in shapes]
    grads = [(torch.randn(*s, generator=gen) * 0.1).to(DEV) for s in shapes]

    def make():
        ps = [torch.nn.Parameter(t.clone().to(DEV)) for t in base]
        es = [t.clone().to(DEV) for t in base]
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        return ps, es, optim.FusedAdamW(ps, lr=1e-2, weight_decay=0.05, max_grad_norm=1.0, ema_params=es, ema_decay=0.9)

    pa, ea, oa = make()
    pb, eb, ob = make()
    for _ in range(4):
        oa.step()
    ob.step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ob.step()
    assert float(ob.step_count) == 1.0 and ob._tables.builds == 1                   # capturing ran nothing and uploaded nothing
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    out = lambda ps, es, o: [_bits(t.detach()) for t in ps + es + o._m + o._v + [o._block]]
    assert float(ob.step_count) == 4.0 and float(oa.step_count) == 4.0
    assert _same(out(pa, ea, oa), out(pb, eb, ob))
    assert not torch.equal(pa[0].detach().cpu(), base[0])

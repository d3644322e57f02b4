"""GPU tests of the 16-bit training-step tail: zigma_optim16_grad_sumsq / zigma_optim16_adamw (csrc/optim_step.hip) with the existing
zigma_optim_prepare between them, and zigma_amd.optim.FusedAdamW16.

Reference of the arithmetic: the float64 oracle of tests/optim_cases.py on the kernel's float32 value BEFORE its rounding (the dbg_x32 hook), within
K x 2^-24 x the stream's scale, K from numpy alone (optim16_cases.error_constant).  The rounding and its random bits are restated bit for bit in
tests/optim16_cases.py (pinned on the CPU by tests/test_optim16_cpu.py): the stored bf16 parameter must EQUAL sr_bf16(dbg_x32, dbg_bits), and dbg_bits
must EQUAL bits16(...).  Every stream of the sweep is a window of a NaN-filled buffer."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import optim16_cases as c16
import optim_cases as oc

pytestmark = pytest.mark.gpu
DEV = "cuda"
OK, NULL, SHAPE, DTYPE, UNSUPPORTED = 0, -1, -2, -3, -6
SEED, STREAM = 0x0123456789abcdef, 7
BF = torch.bfloat16


def _i16(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b):
    return all(torch.equal(_i16(x), _i16(y)) for x, y in zip(a, b))


def _blocks(table, cmap, n_entries, n_chunks, max_numel, state, partials, *, wd=0.0, max_norm=0.0, flags=0, seed=SEED, stream=STREAM, chunk=oc.CHUNK, **over):
    """-> (zigma_optim16_params_t, the zigma_optim_params_t of the prepare launch between the two)"""
    from zigma_amd import _lib
    h = dict(oc.HYPER, **over)
    P, Q = _lib.Optim16Params(), _lib.OptimParams()
    for B in (P, Q):
        B.table, B.chunk_map, B.n_entries, B.n_chunks = _lib.ptr(table), _lib.ptr(cmap), n_entries, n_chunks
        B.partials, B.state = _lib.ptr(partials), _lib.ptr(state)
        B.lr, B.beta1, B.beta2, B.eps, B.weight_decay, B.max_grad_norm, B.ema_decay = h["lr"], h["beta1"], h["beta2"], h["eps"], wd, max_norm, h["ema_decay"]
        B.chunk = chunk
    P.max_numel, P.seed_lo, P.seed_hi, P.stream, P.flags = max_numel, seed & 0xffffffff, seed >> 32, stream, flags
    Q.shadow_dtype, Q.flags = -1, 0
    return P, Q


def _three(P, Q):
    from zigma_amd import _lib
    trace = []
    _lib.TRACE = trace
    try:
        dev = torch.device(DEV, torch.cuda.current_device())
        _lib.call("zigma_optim16_grad_sumsq", P, dev)
        _lib.call("zigma_optim_prepare", Q, dev)
        _lib.call("zigma_optim16_adamw", P, dev)
    finally:
        _lib.TRACE = None
    torch.cuda.synchronize()
    return [t[:2] for t in trace]


# ---- 1. - 4. the kernels on the sweep -----------------------------------------------------------------------------------------------------------------------
class _Sweep:
    """the 168 rows of optim_cases.SIZES x 14 as windows of NaN-filled device buffers, one table, one chunk map; pid = 3 i + 1 (not the row's index)"""

    def __init__(self, name, with_ema=True, hooks=True):
        from zigma_amd import amp
        self.cfg = cfg = oc.CONFIGS[name]
        self.rows = c16.sweep_values(1 + cfg["step0"], cfg["step0"] == 0)
        self.bufs, self.wins = c16.sweep_layout(self.rows)
        self.with_ema = with_ema
        self.dev = {k: torch.from_numpy(self.bufs[k].view(np.int16) if self.bufs[k].dtype == np.uint16 else self.bufs[k]).to(DEV) for k in c16.STREAMS}
        n_p = self.bufs["p"].size
        self.dbg_x = torch.full((n_p,), float("nan"), device=DEV)
        self.dbg_b = torch.full((n_p,), c16.SENTINEL, dtype=torch.int16, device=DEV)
        assert all(t.data_ptr() % 16 == 0 for t in self.dev.values())
        addr = lambda w, k: 0 if w[k] is None or (k == "ema" and not with_ema) else self.dev[k].data_ptr() + c16.WIDTH[k] * w[k]
        self.pids = [3 * i + 1 for i in range(len(self.wins))]
        trows = [[addr(w, k) for k in c16.STREAMS] + [w["n"], pid, self.dbg_x.data_ptr() + 4 * w["p"] if hooks else 0, self.dbg_b.data_ptr() + 2 * w["p"] if hooks else 0, 0]
                 for w, pid in zip(self.wins, self.pids)]
        self.n_wide = sum(1 for r in trows if r[5] >= 8 and all(a % 16 == 0 for a in r[:5]))
        self.n_slow = sum(1 for r in trows if r[5] and any(a % 16 for a in r[:5]))
        cm = amp.build_chunk_map([w["n"] for w in self.wins], oc.CHUNK)
        self.table, self.cmap = torch.tensor(trows, dtype=torch.int64).to(DEV), torch.tensor(cm, dtype=torch.int64).to(DEV)
        self.n_entries, self.n_chunks = len(trows), len(cm)
        self.state = torch.zeros(8, device=DEV)
        self.state[0] = float(cfg["step0"])
        self.partials = torch.full((self.n_chunks,), float("nan"), device=DEV)

    def blocks(self, **kw):
        return _blocks(self.table, self.cmap, self.n_entries, self.n_chunks, max(w["n"] for w in self.wins), self.state, self.partials, wd=self.cfg["wd"],
                       max_norm=self.cfg["max_norm"], **kw)

    def everything(self):
        return [self.dev[k] for k in c16.STREAMS] + [self.dbg_x, self.dbg_b, self.state]

    def host(self):
        out = {k: self.dev[k].cpu().numpy() for k in c16.STREAMS}
        out["p"], out["g"] = out["p"].view(np.uint16), out["g"].view(np.uint16)
        return out, self.dbg_x.cpu().numpy(), self.dbg_b.cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("with_ema", [True, False], ids=["ema", "noema"])
@pytest.mark.parametrize("name", list(oc.CONFIGS))
def test_sweep_against_float64_and_the_restated_rounding(name, with_ema):
    """168 rows in ONE launch of each kernel, first and later step, with and without clipping, with and without EMA (some rows never have one):
    dbg_bits == bits16 bit for bit; dbg_x32, m, v, ema within K of the float64 oracle; the stored p == sr_bf16(dbg_x32, dbg_bits) bit for bit; the
    gradients and everything outside the windows untouched; a second run with the hooks NULL gives the same p, m, v, ema bit for bit"""
    s = _Sweep(name, with_ema)
    assert len(s.rows) == 168 and s.n_wide >= 24 and s.n_slow >= (100 if with_ema else 80)          # (without EMA the rows that misplace it are aligned)
    P, Q = s.blocks()
    assert _three(P, Q) == [("zigma_optim16_grad_sumsq", "multi_sumsq16"), ("zigma_optim_prepare", "step_prepare"), ("zigma_optim16_adamw", "multi_adamw16_sr")]
    st = s.state.cpu()
    step, skipped, gnorm, mult = float(st[0]), int(st.view(torch.int32)[1]), float(st[2]), float(st[3])
    norm64 = oc.grad_norm64([r["g"] for r in s.rows])
    clip64 = oc.clip_coef(norm64, s.cfg["max_norm"])
    print(f"sweep16 {name}: grad_norm {gnorm!r} vs float64 {norm64!r} (rel {abs(gnorm - norm64) / norm64:.2e}); grad_mult {mult!r} vs {clip64!r}")
    assert step == s.cfg["step0"] + 1 and skipped == 0
    assert abs(gnorm - norm64) <= 1e-5 * norm64
    assert mult == 1.0 if clip64 == 1.0 else abs(mult - clip64) <= (1e-5 + 2.0 ** -23) * clip64
    K, _ = c16.error_constant(name)
    out, dbg_x, dbg_b = s.host()
    worst, h = {}, oc.HYPER
    inside = {k: np.zeros(s.bufs[k].size, dtype=bool) for k in c16.STREAMS}
    for r, w, pid in zip(s.rows, s.wins, s.pids):
        n = w["n"]
        has_ema = with_ema and w["ema"] is not None
        for k in c16.STREAMS:
            if w[k] is not None and (k != "ema" or has_ema):
                inside[k][w[k]:w[k] + n] = True
        if not n:
            continue
        cut = lambda k: out[k][w[k]:w[k] + n]
        bits, x32 = dbg_b[w["p"]:w["p"] + n], dbg_x[w["p"]:w["p"] + n]
        assert np.array_equal(bits, c16.bits16(n, SEED, pid, int(step), STREAM)), (pid, n)
        assert np.array_equal(cut("p"), c16.sr_bf16(x32, bits)), (pid, n)
        ref = oc.oracle_step(r["p"], r["g"], r["m"], r["v"], r["ema"] if has_ema else None, step=step, wd=s.cfg["wd"], grad_mult=mult, **h)
        got = (x32, cut("m"), cut("v"), cut("ema") if has_ema else None)
        for k, x in oc.error_multiples(got, ref, (r["p"], r["m"], r["v"], r["ema"]), r["g"].astype(np.float64) * mult).items():
            worst[k] = max(worst.get(k, 0.0), x)
    print(f"sweep16 {name} {'ema' if with_ema else 'noema'}: worst error in units of 2^-24 x scale {worst}; K = {K:.3f}")
    assert max(worst.values()) <= K, (worst, K)
    assert np.array_equal(out["g"], s.bufs["g"])                                                          # the gradients: read only
    bits_of = lambda a: a.view(np.int32) if a.dtype == np.float32 else a
    for k in c16.STREAMS:
        assert np.array_equal(bits_of(out[k])[~inside[k]], bits_of(s.bufs[k])[~inside[k]]), k
    assert np.all(np.isnan(dbg_x[~inside["p"]])) and np.all(dbg_b[~inside["p"]] == c16.SENTINEL) and not np.isnan(dbg_x[inside["p"]]).any()
    assert not np.isnan(out["m"][inside["m"]]).any() and not (out["p"][inside["p"]] == c16.NAN16).any()
    # the hooks change nothing: the same step from the same state without them
    t = _Sweep(name, with_ema, hooks=False)
    _three(*t.blocks())
    assert _same([s.dev[k] for k in c16.STREAMS] + [s.state, s.partials], [t.dev[k] for k in c16.STREAMS] + [t.state, t.partials])
    assert bool(torch.isnan(t.dbg_x).all()) and bool((t.dbg_b == c16.SENTINEL).all())


def test_rounding_nearest_stores_the_nearest_value_and_draws_no_bits():
    s = _Sweep("later_wd_noclip")
    P, Q = s.blocks(flags=c16.NEAREST)
    assert _three(P, Q)[2] == ("zigma_optim16_adamw", "multi_adamw16_nearest")
    out, dbg_x, dbg_b = s.host()
    assert np.all(dbg_b == c16.SENTINEL)                                                                  # the bits hook is untouched
    moved = 0
    for w in s.wins:
        n, at = w["n"], w["p"]
        assert np.array_equal(out["p"][at:at + n], c16.rne_bf16(dbg_x[at:at + n])), w
        moved += int((out["p"][at:at + n] != s.bufs["p"][at:at + n]).sum())
    assert moved > 0 and float(s.state[0]) == 1001.0
    t = _Sweep("later_wd_noclip")                                                                         # the float32 values do not depend on the rounding
    _three(*t.blocks())
    assert torch.equal(_i16(s.dbg_x), _i16(t.dbg_x)) and _same([s.dev[k] for k in ("m", "v", "ema")], [t.dev[k] for k in ("m", "v", "ema")])
    assert not torch.equal(s.dev["p"], t.dev["p"])


def test_norm_pass_against_float64_and_bit_identical_partials():
    """zigma_optim16_grad_sumsq + zigma_optim_prepare against grad_norm64 within 1e-5 relative (the bound of the fp32 test: at most 16 + 9 float32 roundings
    per workgroup on a sum of non-negative terms, the final sum in double); two runs give bit-identical partials"""
    from zigma_amd import _lib
    s = _Sweep("later_nowd_clip")
    P, Q = s.blocks()
    dev = torch.device(DEV, torch.cuda.current_device())
    _lib.call("zigma_optim16_grad_sumsq", P, dev)
    first = s.partials.clone()
    s.partials.fill_(float("nan"))
    _lib.call("zigma_optim16_grad_sumsq", P, dev)
    assert _lib.last_kernel() == "multi_sumsq16"
    _lib.call("zigma_optim_prepare", Q, dev)
    torch.cuda.synchronize()
    assert torch.equal(_i16(first), _i16(s.partials)) and bool(torch.isfinite(first).all())
    norm64 = oc.grad_norm64([r["g"] for r in s.rows])
    got = float(s.state[2])
    print(f"norm16: {got!r} vs float64 {norm64!r}, rel {abs(got - norm64) / norm64:.2e}")
    assert abs(got - norm64) <= 1e-5 * norm64
    # per workgroup against float64 too
    from zigma_amd import amp
    cm = amp.build_chunk_map([w["n"] for w in s.wins], oc.CHUNK)
    want = np.array([float(np.sum(s.rows[e]["g"][o:o + oc.CHUNK].astype(np.float64) ** 2)) for e, o in cm])
    assert np.all(np.abs(first.cpu().numpy().astype(np.float64) - want) <= 25 * 2.0 ** -24 * want)


@pytest.mark.parametrize("how", ["inf", "nan"])
def test_a_skipped_step_leaves_every_byte(how):
    """one non-finite gradient with clipping on: p, m, v, ema, both hooks and the step counter keep their bits, `skipped` reads 1"""
    s = _Sweep("later_nowd_clip")
    w = s.wins[-1]
    s.dev["g"][w["g"] + w["n"] - 3] = torch.tensor(0x7f80 if how == "inf" else 0x7fc0, dtype=torch.int16)
    before = [t.clone() for t in s.everything()]
    _three(*s.blocks())
    after = s.everything()
    assert _same(before[:-1], after[:-1])
    assert float(s.state[0]) == 1000.0 and int(s.state.view(torch.int32)[1]) == 1
    if how == "inf":
        assert float(s.state[2]) == float("inf")


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------------------------
class _Case:
    """three rows of ordinary tensors, the second misplaced by one element"""

    def __init__(self, seed=3):
        from zigma_amd import amp
        g = torch.Generator().manual_seed(seed)
        self.ns, offs = [257, oc.CHUNK + 9, 16], [0, 1, 0]
        mk = lambda n, o, f, dt: f(n + 8).to(DEV, dt)[o:o + n]
        self.p = [mk(n, o, lambda k: torch.randn(k, generator=g), BF) for n, o in zip(self.ns, offs)]
        self.g = [mk(n, o, lambda k: torch.randn(k, generator=g) * 0.1, BF) for n, o in zip(self.ns, offs)]
        self.m = [mk(n, o, lambda k: torch.randn(k, generator=g) * 0.05, torch.float32) for n, o in zip(self.ns, offs)]
        self.v = [mk(n, o, lambda k: torch.rand(k, generator=g) * 0.01 + 1e-4, torch.float32) for n, o in zip(self.ns, offs)]
        self.ema = [t.float() * 1.01 for t in self.p]
        self.rows = [[a.data_ptr(), b.data_ptr(), c.data_ptr(), d.data_ptr(), e.data_ptr(), n, i, 0, 0, 0]
                     for i, (a, b, c, d, e, n) in enumerate(zip(self.p, self.g, self.m, self.v, self.ema, self.ns))]
        cm = amp.build_chunk_map(self.ns, oc.CHUNK)
        self.table, self.cmap = torch.tensor(self.rows, dtype=torch.int64).to(DEV), torch.tensor(cm, dtype=torch.int64).to(DEV)
        self.n_chunks = len(cm)
        self.state = torch.zeros(8, device=DEV)
        self.state[0] = 41.0
        self.partials = torch.full((self.n_chunks,), -7.0, device=DEV)

    def snapshot(self):
        return [_i16(t).clone() for t in self.p + self.m + self.v + self.ema + [self.state, self.partials]]

    def blocks(self, **kw):
        return _blocks(self.table, self.cmap, len(self.ns), self.n_chunks, max(self.ns), self.state, self.partials, **kw)


def test_refusals_in_the_documented_order_and_rows_the_kernels_skip():
    """every refusal of the header from both entry points, each also paired with a LATER one to show the order, with all outputs untouched; zero counts
    launch nothing; rows the host cannot see into (a NULL stream, numel above max_numel, an offset off the octet grid) are skipped by the kernels"""
    from zigma_amd import _lib
    L = _lib.lib()
    c = _Case()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    before = c.snapshot()

    def call(fn, **kw):
        P, _ = c.blocks(wd=0.05, max_norm=1.0)
        for k, v in kw.items():
            setattr(P, k, v)
        rc = getattr(L, fn)(ctypes.byref(P), stream)
        torch.cuda.synchronize()
        return rc

    nan, inf = float("nan"), float("inf")
    ordered = [(dict(table=None), NULL), (dict(chunk_map=None), NULL),
               (dict(n_entries=-1), SHAPE), (dict(n_chunks=-1), SHAPE), (dict(n_chunks=1 << 31), SHAPE),
               (dict(max_numel=-1), SHAPE), (dict(max_numel=1 << 35), SHAPE), (dict(max_numel=1 << 40), SHAPE),
               (dict(chunk=0), SHAPE), (dict(chunk=12), SHAPE), (dict(chunk=-4096), SHAPE), (dict(chunk=65544), SHAPE),
               (dict(flags=2), UNSUPPORTED), (dict(flags=3), UNSUPPORTED), (dict(flags=-1), UNSUPPORTED),
               (dict(beta1=1.0), UNSUPPORTED), (dict(beta1=-0.1), UNSUPPORTED), (dict(beta2=1.0), UNSUPPORTED), (dict(beta2=nan), UNSUPPORTED),
               (dict(eps=0.0), UNSUPPORTED), (dict(eps=-1e-8), UNSUPPORTED), (dict(eps=nan), UNSUPPORTED), (dict(eps=inf), UNSUPPORTED),
               (dict(lr=nan), UNSUPPORTED), (dict(lr=inf), UNSUPPORTED), (dict(weight_decay=nan), UNSUPPORTED), (dict(max_grad_norm=inf), UNSUPPORTED),
               (dict(ema_decay=nan), UNSUPPORTED)]
    own_null = {"zigma_optim16_grad_sumsq": "partials", "zigma_optim16_adamw": "state"}
    for fn in own_null:
        for kw, want in ordered + [({own_null[fn]: None}, NULL)]:
            assert call(fn, **kw) == want, (fn, kw, want)
            if "n_entries" not in kw:                                    # every refusal comes before "nothing to launch"
                assert call(fn, **kw, n_entries=0) == want, (fn, kw)
            assert _same(before, c.snapshot()), (fn, kw)
        # the order between the classes: NULL, then the shapes, then the flags and hyperparameters
        assert call(fn, table=None, n_entries=-1) == NULL and call(fn, **{own_null[fn]: None}, chunk=12, flags=2) == NULL
        assert call(fn, n_chunks=-1, flags=2) == SHAPE and call(fn, max_numel=1 << 35, lr=nan) == SHAPE and call(fn, chunk=12, flags=2, beta1=1.0) == SHAPE
        assert _same(before, c.snapshot())
        assert getattr(L, fn)(None, stream) == NULL
        for kw in (dict(n_entries=0), dict(n_chunks=0)):                 # nothing is launched
            assert call(fn, **kw) == OK and _same(before, c.snapshot()), (fn, kw)
        assert call(fn, flags=c16.NEAREST, n_chunks=0) == OK
    # the other call's pointer is not asked for
    assert call("zigma_optim16_grad_sumsq", state=None) == OK and call("zigma_optim16_adamw", partials=None, n_chunks=0) == OK
    with pytest.raises(RuntimeError, match="status -2"):
        P, _ = c.blocks()
        P.chunk = 12
        _lib.call("zigma_optim16_adamw", P, c.state.device)
    # rows the kernels skip: nothing of them is followed or written, the norm pass stores 0
    st = c.state.clone()
    st.view(torch.int32)[1] = 0
    st[3], st[4], st[5] = 1.0, 1e-3, 1.0                                 # (a state block as a taken step's prepare leaves it)
    good_table, good_cmap = c.table.clone(), c.cmap.clone()

    def run_both(**kw):
        c.partials.fill_(-7.0)
        c.state.copy_(st)
        keep = [t.clone() for t in c.p + c.m + c.v + c.ema]
        assert call("zigma_optim16_grad_sumsq", **kw) == OK and call("zigma_optim16_adamw", **kw) == OK
        return [not torch.equal(_i16(a), _i16(b)) for a, b in zip(keep[:3], c.p)], keep

    for col in range(4):                                                 # NULL p, g, m, v of row 0
        c.table[0, col] = 0
        changed, keep = run_both()
        assert changed == [False, True, True] and float(c.partials[0]) == 0.0 and float(c.partials[1]) > 0.0, col
        assert _same(keep[3:4] + keep[6:7] + keep[9:10], [c.m[0], c.v[0], c.ema[0]])
        c.table.copy_(good_table)
    changed, _ = run_both(max_numel=oc.CHUNK)                            # row 1 has CHUNK + 9 elements
    assert changed == [True, False, True] and float(c.partials[1]) == 0.0 and float(c.partials[2]) == 0.0 and float(c.partials[0]) > 0.0
    for row in ([len(c.ns), 0], [-1, 0], [0, 257], [0, -8], [0, 4], [0, 1 << 40]):
        c.cmap[0] = torch.tensor(row, dtype=torch.int64)
        changed, _ = run_both()
        assert changed == [False, True, True] and float(c.partials[0]) == 0.0, row
    c.cmap.copy_(good_cmap)
    changed, _ = run_both()
    assert changed == [True, True, True]


# ---- 6. - 10. the optimizer -------------------------------------------------------------------------------------------------------------------------------
def _stall_run(kind):
    """256 steps on 4096 parameters equal to 1.0 under a constant positive gradient -> (p as float64, the EMA as float64, did any bit of p ever change)"""
    from zigma_amd import optim
    c = c16.STALL
    kw = dict(lr=c["lr"], betas=(c["beta1"], c["beta2"]), eps=c["eps"], weight_decay=c["wd"], ema_decay=c["ema_decay"])
    dt = torch.float32 if kind == "fp32" else BF
    p = torch.nn.Parameter(torch.full((c["n"],), c["p0"], device=DEV, dtype=dt))
    p.grad = torch.full((c["n"],), c["g"], device=DEV, dtype=dt)
    if kind == "fp32":
        ema = [p.detach().clone()]
        opt = optim.FusedAdamW([p], ema_params=ema, **kw)
    else:
        opt = optim.FusedAdamW16([p], ema=True, rounding=kind, seed=c["seed"], **kw)
        ema = opt.ema_tensors()
    start = p.detach().clone()
    changed = torch.zeros((), dtype=torch.bool, device=DEV)
    for _ in range(c["steps"]):
        opt.step()
        changed |= (_i16(p.detach()) != _i16(start)).any()
    assert float(opt.step_count) == c["steps"] and int(opt.skipped) == 0
    return p.detach().double().cpu(), ema[0].double().cpu(), bool(changed)


def test_the_stalled_update_moves():
    """lr = 1e-4 on weights of 1.0: with rounding="nearest" no bit of p ever changes; with stochastic rounding the mean of p over the 4096 elements lies
    within 5 sigma of the fp32 FusedAdamW run's mean on the same inputs (sigma from the per-step fractions, optim16_cases.stall_sigma), and the fp32 EMA
    of the 16-bit run moves, within the same band of the fp32 run's EMA"""
    sigma, moved64 = c16.stall_sigma()
    p32, e32, _ = _stall_run("fp32")
    pn, en, changed_n = _stall_run("nearest")
    ps, es, changed_s = _stall_run("stochastic")
    print(f"stall: fp32 mean moved {1 - float(p32.mean()):.6f} (float64 {moved64:.6f}); stochastic mean {float(ps.mean()):.6f} vs fp32 {float(p32.mean()):.6f}: "
          f"{abs(float(ps.mean() - p32.mean())) / sigma:.2f} sigma (sigma {sigma:.3e}); EMA {float(es.mean()):.7f} vs {float(e32.mean()):.7f}: "
          f"{abs(float(es.mean() - e32.mean())) / sigma:.3f} sigma; nearest moved: {changed_n}")
    assert abs((1 - float(p32.mean())) - moved64) < 1e-5 and abs(moved64 - 0.0256) < 1e-4
    assert not changed_n and bool((pn == 1.0).all())
    assert changed_s and abs(float(ps.mean() - p32.mean())) <= 5 * sigma
    assert len(set(ps.tolist())) > 4                                                                      # a random walk of ulp-size jumps, not one common value
    assert float(es.mean()) < 1.0 - 1e-4 and abs(float(es.mean() - e32.mean())) <= 5 * sigma and float(e32.mean()) < 1.0 - 1e-4
    assert float(en.mean()) > float(e32.mean())                                                          # (under nearest the EMA follows a p that never moves)


def _dist_run(kind):
    from zigma_amd import optim
    c = c16.DIST
    w, g = c16.dist_inputs()
    kw = dict(lr=c["lr"], betas=(c["beta1"], c["beta2"]), eps=c["eps"], weight_decay=c["wd"])
    dt = torch.float32 if kind == "fp32" else BF
    p = torch.nn.Parameter(torch.from_numpy(w).to(DEV, dt))
    p.grad = torch.from_numpy(g).to(DEV, dt)
    assert torch.equal(p.detach().float().cpu(), torch.from_numpy(w))
    opt = optim.FusedAdamW([p], **kw) if kind == "fp32" else optim.FusedAdamW16([p], rounding=kind, seed=c["seed"], **kw)
    for _ in range(c["steps"]):
        opt.step()
    return p.detach().double().cpu()


def test_distance_to_the_fp32_trajectory():
    """65 536 weights N(0, 0.02^2), persistent-sign gradients, lr = 1e-4, 256 steps: the RMS distance of the stochastic run to the fp32-master FusedAdamW
    run is at most HALF that of the nearest run (the numpy simulation of the same inputs gives 0.17 at 64 steps, tests/test_optim16_cpu.py)"""
    ref, rne, sr = _dist_run("fp32"), _dist_run("nearest"), _dist_run("stochastic")
    d_rne, d_sr = float((rne - ref).pow(2).mean().sqrt()), float((sr - ref).pow(2).mean().sqrt())
    print(f"distance to the fp32 trajectory after 256 steps: nearest {d_rne:.3e}, stochastic {d_sr:.3e}, ratio {d_sr / d_rne:.3f}")
    assert d_rne > 0 and d_sr <= 0.5 * d_rne


def _pair(seed, stream, base, grads):
    from zigma_amd import optim
    ps = [torch.nn.Parameter(t.clone()) for t in base]
    for p, g in zip(ps, grads):
        p.grad = g.clone()
    return ps, optim.FusedAdamW16(ps, lr=1e-3, weight_decay=0.05, max_grad_norm=1.0, ema=True, ema_decay=0.9, seed=seed, stream=stream)


def test_determinism_and_what_the_bits_depend_on():
    """two optimizers with the same seed on cloned tensors stay bit-identical over 5 steps; another seed or stream does not; two parameters of equal size
    and equal content with different pid are rounded differently"""
    gen = torch.Generator().manual_seed(8)
    t0, g0 = torch.randn(5003, generator=gen).to(DEV, BF), (torch.randn(5003, generator=gen) * 0.1).to(DEV, BF)
    base, grads = [t0, t0.clone(), torch.randn(70, 9, generator=gen).to(DEV, BF)], [g0, g0.clone(), torch.randn(70, 9, generator=gen).to(DEV, BF)]
    runs = {"a": _pair(5, 0, base, grads), "twin": _pair(5, 0, base, grads), "seed": _pair(6, 0, base, grads), "stream": _pair(5, 1, base, grads)}
    for _ in range(5):
        for ps, opt in runs.values():
            opt.step()
    out = {k: [p.detach() for p in ps] + opt._m + opt._v + opt.ema_tensors() + [opt._block] for k, (ps, opt) in runs.items()}
    assert _same(out["a"], out["twin"]) and float(runs["a"][1].step_count) == 5.0
    for other in ("seed", "stream"):
        assert not torch.equal(_i16(out["a"][0]), _i16(out[other][0])), other
        assert (out["a"][0].float() - out[other][0].float()).abs().max() <= 0.05              # ... by roundings, not by the arithmetic
    a, b = out["a"][0], out["a"][1]
    assert not torch.equal(_i16(a), _i16(b)) and float((_i16(a) != _i16(b)).float().mean()) > 0.1


def _small_model():
    from zigma_amd.model_zigma import ZigMa
    torch.manual_seed(0)
    return ZigMa(in_channels=4, embed_dim=128, depth=2, img_dim=8, patch_size=1, scan_type="zigzagN8", use_pe=2, device=DEV, dtype=BF).train()


def test_a_captured_step_replays_bit_for_bit_on_a_bf16_model():
    """tiny bf16 ZigMa, gradients of one backward kept static: one eager step, one captured, three replays == four eager steps of a twin, bit for bit
    (parameters, moments, EMA, the device step counter: every replay reads the counter on the device and draws fresh bits).  After the steps the caches
    keyed on the optimizer-step count (Mamba._scan_consts, ZigMa._batched_conditioning) see the new parameters.  (They are compared tensor by tensor.)"""
    from zigma_amd import amp, optim
    from zigma_amd.mamba_simple import Mamba
    from zigma_amd.transport import create_transport
    ma = _small_model()
    x1 = torch.randn(8, 4, 8, 8, generator=torch.Generator().manual_seed(77)).to(DEV)
    x, t = x1.to(BF), torch.full((8,), 0.5, device=DEV)
    with torch.no_grad():
        ma.eval()(x, t)                                                                # the fused forward of the sampling path: fills the caches
        ma.train()
        mx = next(m for m in ma.modules() if isinstance(m, Mamba))
        A0, Wm0 = mx._scan_consts("")[0].clone(), ma._cond_cache[1].clone()
        assert mx._scan_consts("")[0] is mx._scan_consts("")[0]                            # (cached)
    torch.manual_seed(1234)
    create_transport().training_losses(ma, x1)["loss"].mean().backward()
    mb = copy.deepcopy(ma)
    for pa, pb in zip(ma.parameters(), mb.parameters()):
        pb.grad = None if pa.grad is None else pa.grad.clone()
    kw = dict(lr=2e-3, weight_decay=0.05, max_grad_norm=2.0, ema=True, ema_decay=0.9, seed=99, stream=1)
    oa, ob = optim.FusedAdamW16(ma.parameters(), **kw), optim.FusedAdamW16(mb.parameters(), **kw)
    assert all(p.grad is None or p.grad.dtype == BF for p in ma.parameters()) and sum(p.grad is not None for p in ma.parameters()) > 10
    steps0 = amp.step_count()
    for _ in range(4):
        oa.step()
    assert amp.step_count() == steps0 + 4                                              # the optimizer-step hook sees this class
    ob.step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ob.step()
    assert float(ob.step_count) == 1.0 and ob._tables.builds == 1                      # capturing ran nothing and uploaded nothing
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    out = lambda m, o: [p.detach() for p in m.parameters()] + o._m + o._v + o.ema_tensors() + [o._block]
    assert float(oa.step_count) == 4.0 and float(ob.step_count) == 4.0 and int(oa.skipped) == 0
    assert _same(out(ma, oa), out(mb, ob))
    # the caches (filled by the forward before the steps): what they hand out after the steps is derived from the parameters as they are now
    with torch.no_grad():
        ma.eval()(x, t)
        A1, Wm1 = mx._scan_consts("")[0], ma._cond_cache[1]
        assert torch.equal(A1, -torch.exp(mx.A_log.float())) and not torch.equal(A1, A0)
        assert torch.equal(Wm1, torch.cat([b.adaLN_modulation[-1].weight for b in ma.blocks], 0)) and not torch.equal(Wm1, Wm0)
    assert ma._cond_cache[0][-1] == amp.step_count()


def test_state_dict_round_trip_torch_dict_and_the_ema_copy():
    """continuing from a state_dict() round trip is bit-identical to not interrupting; a torch.optim.AdamW(fused=True) dict of the same bf16 model
    loads (bf16 moments widened, one step counter); copy_ema_to gives rne_bf16 of the EMA"""
    from zigma_amd import optim
    gen = torch.Generator().manual_seed(4)
    shapes = [(300, 70), (oc.CHUNK + 1,), (5,), (64, 64)]
    base = [torch.randn(*s, generator=gen).to(DEV, BF) for s in shapes]
    grads = [[(torch.randn(*s, generator=gen) * 0.1).to(DEV, BF) for s in shapes] for _ in range(5)]
    kw = dict(lr=1e-2, weight_decay=0.05, max_grad_norm=1.0, ema=True, ema_decay=0.9, seed=31, stream=2)

    def make(**over):
        ps = [torch.nn.Parameter(t.clone()) for t in base]
        return ps, optim.FusedAdamW16(ps, **dict(kw, **over))

    def run(ps, opt, which):
        for i in which:
            for p, g in zip(ps, grads[i]):
                p.grad = g.clone() if p.grad is None else p.grad.copy_(g)
            opt.step()

    pa, oa = make()
    run(pa, oa, range(5))
    pb, ob = make()
    run(pb, ob, range(3))
    sd = ob.state_dict()
    pc, oc_ = make(seed=1, stream=0, lr=1.0)                                            # (the loaded group brings seed, stream and the hyperparameters)
    with torch.no_grad():
        for q, p in zip(pc, pb):
            q.copy_(p)
    oc_.load_state_dict(sd)
    assert float(oc_.step_count) == 3.0 and oc_.param_groups[0]["seed"] == 31 and oc_.param_groups[0]["lr"] == 1e-2
    run(pc, oc_, range(3, 5))
    out = lambda ps, o: [p.detach() for p in ps] + o._m + o._v + o.ema_tensors() + [o._block[:1]]
    assert _same(out(pa, oa), out(pc, oc_)) and float(oa.step_count) == 5.0
    # torch's dict of the same bf16 model
    pt = [torch.nn.Parameter(t.clone()) for t in base]
    ot = torch.optim.AdamW(pt, lr=1e-3, weight_decay=0.02, fused=True)
    for _ in range(2):
        for p, g in zip(pt, grads[0]):
            p.grad = g.clone()
        ot.step()
    pd, od = make()
    od.load_state_dict(ot.state_dict())
    assert float(od.step_count) == 2.0 and od.param_groups[0]["weight_decay"] == 0.02 and od.param_groups[0]["seed"] == 31
    assert all(torch.equal(od.state[a]["exp_avg"], ot.state[b]["exp_avg"].float()) and od.state[a]["exp_avg"].dtype == torch.float32 for a, b in zip(pd, pt))
    run(pd, od, [1])
    assert float(od.step_count) == 3.0 and int(od.skipped) == 0 and all(bool(torch.isfinite(p).all()) for p in pd)
    # the sampling copy
    lin = torch.nn.Sequential(torch.nn.Linear(40, 30), torch.nn.Linear(30, 7)).to(DEV, BF)
    ol = optim.FusedAdamW16(lin.parameters(), lr=1e-2, ema=True, ema_decay=0.5, seed=3)
    for _ in range(3):
        for p in lin.parameters():
            p.grad = torch.randn(p.shape, generator=gen).to(DEV, BF)
        ol.step()
    twin = copy.deepcopy(lin)
    ol.copy_ema_to(twin)
    torch.cuda.synchronize()
    for q, e, p in zip(twin.parameters(), ol.ema_tensors(), lin.parameters()):
        want = c16.rne_bf16(e.cpu().numpy().reshape(-1))
        assert np.array_equal(q.detach().cpu().view(torch.int16).numpy().view(np.uint16).reshape(-1), want)
        assert not torch.equal(q.detach(), p.detach())
    with pytest.raises(ValueError, match="parameters"):
        ol.copy_ema_to(torch.nn.Linear(40, 30).to(DEV, BF))
    with pytest.raises(ValueError, match="bfloat16"):
        ol.copy_ema_to(copy.deepcopy(lin).float())

"""GPU tests of the on-device SDE sampler: the step kernel zigma_sde_step_fwd against the numpy restatement of tests/sde_cases.py (Philox
words bit for bit, the output against float64 on those integers), its refusals, the distribution of its normals, zigma_sde_advance, and
Sampler.sample_sde(noise="device") eager and as a captured graph.

`pytest -s` prints one line per sweep case: how much of its limit the output used and the worst ratio of the kernel's normals.
"""
import ctypes

import numpy as np
import pytest
import torch

import sde_cases as sc
from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
CASES = sc.sde_cases()
PAD = 8                     # elements in front of and behind every window: 16-byte aligned in every type
SENTINEL = 0x5a5a5a5a


def _state(seed, stream, step):
    words = np.array([seed & 0xffffffff, seed >> 32, stream, step], dtype=np.uint32)
    return torch.from_numpy(words.view(np.int32).copy()).to(DEV)


def _window(values, dtype, n):
    """(buffer, window): n elements inside a NaN-filled buffer"""
    buf = torch.full((n + 2 * PAD,), NAN, dtype=dtype, device=DEV)
    win = buf[PAD:PAD + n]
    if values is not None:
        win.copy_(torch.from_numpy(np.ascontiguousarray(values)).to(DEV).to(dtype))
    return buf, win


def _bits_window(n):
    words = 4 * (-(-n // 4))
    buf = torch.full((words + 8,), SENTINEL, dtype=torch.int32, device=DEV)
    return buf, buf[4:4 + words]


def _raw(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _launch(c, inp):
    """one launch of the case from fresh buffers -> dict of every buffer and window"""
    from zigma_amd import _lib
    from zigma_amd.transport import sde_device as sd
    dt, n = DT[c["kind"]], c["n"]
    r = dict(coef=torch.from_numpy(inp["coef"]).to(DEV), state=_state(c["seed"], c["stream"], c["step"]) if c["state"] else None)
    for k in "abc":
        r[k + "_buf"], r[k] = _window(inp[k], dt, n) if inp[k] is not None else (None, None)
    r["out_buf"], r["out"] = (r["a_buf"], r["a"]) if c["alias"] else _window(None, dt, n)
    r["bits_buf"], r["bits"] = _bits_window(n) if c["state"] else (None, None)
    sd.sde_step(r["out"], r["a"], r["b"], r["c"], coef=r["coef"], row=c["row"], rows_per_step=c["rps"], state=r["state"], absolute=c["absolute"],
                elem_offset=c["offset"], bits_out=r["bits"])
    assert _lib.last_kernel() == "sde_step", _lib.last_kernel()
    torch.cuda.synchronize()
    return r


def _kernel_normals(seed, stream, step, offset, n):
    """the kernel's own normals: every operand absent, cn = 1, fp32 out = fma(1, xi, +0) = xi"""
    from zigma_amd.transport import sde_device as sd
    coef = torch.tensor([[NAN, NAN, NAN, 1.0]], device=DEV)
    out = torch.empty(n, device=DEV)
    sd.sde_step(out, coef=coef, row=0, state=_state(seed, stream, step), absolute=True, elem_offset=offset)
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------------------------------------------
# (a) the sweep
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_sde_sweep(c):
    inp = sc.sde_inputs(c)
    ref = sc.sde_reference(c, inp)
    r = _launch(c, inp)
    n = c["n"]
    # the raw words, bit for bit; no Philox work (and no store) where cn is 0
    if c["state"]:
        words = r["bits"].cpu().numpy().view(np.uint32).reshape(-1, 4)
        if c["cn0"]:
            assert (words == SENTINEL).all(), "bits_out written although cn == 0"
        else:
            assert np.array_equal(words, ref["words"]), "the Philox words differ from the restatement"
        edge = r["bits_buf"].cpu().numpy()
        assert (edge[:4] == SENTINEL).all() and (edge[-4:] == SENTINEL).all(), "bits_out written outside its window"
    # the output against float64 on those integers, element by element and norm-wise
    got = r["out"].float().cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all(), "an element of the window was left unwritten"
    err = np.abs(got - ref["out"])
    allow = np.maximum(ref["allow"], 1e-300)              # (no operand and no noise: out is exactly 0)
    used = float(np.max(err / allow))
    used_norm = float(np.linalg.norm(err) / np.linalg.norm(allow))
    # the normal itself, from a launch that stores it unchanged
    ratio = 0.0
    if not c["cn0"]:
        z = _kernel_normals(c["seed"], c["stream"], c["step"], c["offset"], n).cpu().numpy()
        ratio = sc.normal_ratio(z, ref["xi"])
    print(f"sde-sweep {c['id']}: out uses {used:.3f} of its element-wise limit, {used_norm:.3f} norm-wise; normal ratio {ratio:.2f} (K = {sc.NORMAL_K:g})")
    assert used <= 1.0 and used_norm <= 1.0, (c["id"], used, used_norm)
    assert ratio <= sc.NORMAL_K, (c["id"], ratio)
    # NaN stays everywhere outside the windows, the operands are unchanged
    for k in ("a", "b", "c", "out"):
        buf = r[k + "_buf"]
        if buf is not None:
            assert bool(torch.isnan(buf[:PAD]).all()) and bool(torch.isnan(buf[PAD + n:]).all()), (c["id"], k, "written outside the window")
    for k in ("a", "b", "c"):
        if r[k] is not None and not (k == "a" and c["alias"]):
            assert np.array_equal(r[k].float().cpu().numpy(), inp[k]), (c["id"], k, "an operand changed")
    assert np.array_equal(r["coef"].cpu().numpy(), inp["coef"], equal_nan=True)
    if c["state"]:
        assert torch.equal(r["state"], _state(c["seed"], c["stream"], c["step"])), "the step kernel wrote the state"
    # a relaunch from the same buffers' contents is bit-identical
    again = _launch(c, inp)
    assert torch.equal(_raw(again["out_buf"]), _raw(r["out_buf"])), (c["id"], "a relaunch differs")
    if c["state"]:
        assert torch.equal(again["bits_buf"], r["bits_buf"])


# ---------------------------------------------------------------------------------------------------
# (b) refusals, in the header's order
# ---------------------------------------------------------------------------------------------------
def _valid_block(t):
    from zigma_amd import _lib
    return _lib.SdeStepParams(n=16, elem_offset=8, coef_rows=4, dtype=_lib.F32, flags=0, rows_per_step=1, row=1, a=t["a"].data_ptr(), b=None, c=t["c"].data_ptr(),
                              out=t["out"].data_ptr(), coef=t["coef"].data_ptr(), state=t["state"].data_ptr(), bits_out=t["bits"].data_ptr())


def _break(what, P, t):
    if what == "n-negative":
        P.n = -1
    elif what == "offset-negative":
        P.elem_offset = -4
    elif what == "offset-not-quad":
        P.elem_offset = 6
    elif what == "rows_per_step0":
        P.rows_per_step = 0
    elif what == "row-negative":
        P.row = -1
    elif what == "coef_rows0":
        P.coef_rows = 0
    elif what == "absolute-row-past-table":
        P.flags, P.row = sc.ROW_ABSOLUTE, 4
    elif what == "flags2":
        P.flags = 2
    elif what == "dtype3":
        P.dtype = 3
    elif what == "null-out":
        P.out = None
    elif what == "null-coef":
        P.coef = None
    elif what == "null-state-relative":
        P.state, P.bits_out = None, None
    elif what == "null-state-bits":
        P.state, P.flags = None, sc.ROW_ABSOLUTE
    elif what.endswith("-off-by-one"):
        field = {"a": "a", "c": "c", "out": "out", "coef": "coef", "state": "state", "bits": "bits_out"}[what.split("-")[0]]
        setattr(P, field, getattr(P, field) + 4)
    else:
        raise KeyError(what)


@pytest.mark.parametrize("what,status", sc.REFUSALS, ids=[w for w, _ in sc.REFUSALS])
def test_sde_refusals(what, status):
    from zigma_amd import _lib
    t = dict(a=torch.ones(32, device=DEV), c=torch.ones(32, device=DEV), out=torch.full((32,), NAN, device=DEV), coef=torch.ones(8, 4, device=DEV),
             state=torch.zeros(8, dtype=torch.int32, device=DEV), bits=torch.full((32,), SENTINEL, dtype=torch.int32, device=DEV))
    P = _valid_block(t)
    _lib.call("zigma_sde_step_fwd", P, torch.device(DEV))             # the block is valid before it is broken
    torch.cuda.synchronize()
    assert bool(torch.isfinite(t["out"][:16]).all()) and bool(torch.isnan(t["out"][16:]).all())
    t["out"].fill_(NAN)
    t["bits"].fill_(SENTINEL)
    before = [v.clone() for v in t.values()]
    if what == "null-block":
        L = _lib.lib()
        assert L.zigma_sde_step_fwd(None, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == status
        assert L.zigma_sde_advance(None, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == status
    else:
        _break(what, P, t)
        with pytest.raises(RuntimeError, match=rf"\(status {status}\)"):
            _lib.call("zigma_sde_step_fwd", P, torch.device(DEV))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) or (torch.isnan(a).all() and torch.isnan(b).all()) for a, b in zip(before, t.values())), (what, "a refused call wrote")


def test_sde_refusal_order_and_empty_call():
    """a block with several faults reports the one the header lists first; n == 0 is ZIGMA_OK before any pointer is looked at"""
    from zigma_amd import _lib
    t = dict(a=torch.ones(32, device=DEV), c=torch.ones(32, device=DEV), out=torch.full((32,), NAN, device=DEV), coef=torch.ones(8, 4, device=DEV),
             state=torch.zeros(8, dtype=torch.int32, device=DEV), bits=torch.full((32,), SENTINEL, dtype=torch.int32, device=DEV))
    order = [w for w, _ in sc.REFUSALS if w != "null-block"]
    status = dict(sc.REFUSALS)
    for first, second in zip(order, order[1:]):
        if {first, second} <= {"null-state-relative", "null-state-bits"} or (first.endswith("off-by-one") and second.endswith("off-by-one")):
            continue                                   # (two forms of one check)
        P = _valid_block(t)
        _break(second, P, t)
        _break(first, P, t)
        with pytest.raises(RuntimeError, match=rf"\(status {status[first]}\)"):
            _lib.call("zigma_sde_step_fwd", P, torch.device(DEV))
    P = _valid_block(t)
    P.n, P.out, P.coef, P.state = 0, None, None, None
    _lib.call("zigma_sde_step_fwd", P, torch.device(DEV))             # ZIGMA_OK
    torch.cuda.synchronize()
    assert bool(torch.isnan(t["out"]).all()) and bool((t["bits"] == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------
# (c) the distribution of the kernel's normals
# ---------------------------------------------------------------------------------------------------
def dist_draws(draw):
    """draw(seed, stream, step) -> N normals; -> (z, the neighbouring draws)"""
    s, w, k = sc.DIST_SEED, sc.DIST_STREAM, sc.DIST_STEP
    return draw(s, w, k), {"step + 1": draw(s, w, k + 1), "stream 1": draw(s, 1, k), "seed + 1": draw(s + 1, w, k)}


def test_sde_normals_distribution():
    draws = {}

    def draw(seed, stream, step):
        z = _kernel_normals(seed, stream, step, 0, sc.DIST_N).cpu().numpy()
        draws[(seed, stream, step)] = z
        return z
    z, others = dist_draws(draw)
    for name, value, bound in sc.distribution_checks(z, others):
        print(f"sde-dist {name}: {value:.3e} (limit {bound:.3e})")
        assert value <= bound, (name, value, bound)
    worst = max(sc.normal_ratio(z, sc.field(*key, 0, sc.DIST_N)[1]) for key, z in draws.items())
    print(f"sde-dist worst normal ratio over {len(draws)} x 2^20 normals: {worst:.2f} (K = {sc.NORMAL_K:g})")
    assert worst <= sc.NORMAL_K, worst
    assert float(np.max(np.abs(z))) <= np.sqrt(48 * np.log(2)) * (1 + 1e-6)          # the tail reach the header states


# ---------------------------------------------------------------------------------------------------
# (d) zigma_sde_advance
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", (1, 5))
@pytest.mark.parametrize("n_t", (1, 2))
def test_sde_advance(n_t, batch):
    from zigma_amd import _lib
    from zigma_amd.transport import sde_device as sd
    num_steps = 4
    times = torch.arange(num_steps * n_t, dtype=torch.float32, device=DEV).view(num_steps, n_t) * 0.125 + 0.0625
    buf = torch.full((n_t * batch + 8,), NAN, device=DEV)
    t_out = buf[4:4 + n_t * batch].view(n_t, batch)
    state = _state(7, 3, 0)
    for calls in range(1, num_steps + 3):
        sd.sde_advance(state, times, t_out)
        assert _lib.last_kernel() == "sde_advance"
        torch.cuda.synchronize()
        assert state.cpu().tolist() == [7, 0, 3, calls], "the counter, and only the counter, moves"
        want = times[min(calls, num_steps - 1)].view(n_t, 1).expand(n_t, batch)       # past the table: the last row (the clamp)
        assert torch.equal(t_out, want), (calls, t_out)
        assert bool(torch.isnan(buf[:4]).all()) and bool(torch.isnan(buf[4 + n_t * batch:]).all()), "written past t_out"
    P = _lib.SdeAdvanceParams(state=state.data_ptr(), times=times.data_ptr(), t_out=t_out.data_ptr(), n_rows=num_steps, n_t=n_t, batch=batch, flags=0)
    for field, value, status in (("n_t", 3, -2), ("batch", 0, -2), ("n_rows", 0, -2), ("flags", 1, -6), ("state", None, -1), ("times", None, -1), ("t_out", None, -1),
                                 ("state", state.data_ptr() + 4, -4)):
        Q = _lib.SdeAdvanceParams.from_buffer_copy(P)
        setattr(Q, field, value)
        with pytest.raises(RuntimeError, match=rf"\(status {status}\)"):
            _lib.call("zigma_sde_advance", Q, torch.device(DEV))
    torch.cuda.synchronize()
    assert state.cpu().tolist() == [7, 0, 3, num_steps + 2]


# ---------------------------------------------------------------------------------------------------
# (e) the sampler, eager
# ---------------------------------------------------------------------------------------------------
def _model():
    from test_gpu_cfg import _toy
    return _toy(torch.float32, num_classes=-1)[0]


def _transport():
    from zigma_amd.transport import ModelType, PathType, Transport, WeightType
    return Transport(model_type=ModelType.VELOCITY, path_type=PathType.LINEAR, loss_type=WeightType.NONE, train_eps=1e-3, sample_eps=1e-3)


def _reference_loop(fn, z, model, xis, monkeypatch):
    """the existing composed loop, its th.randn handing out the given increments in order"""
    it = iter(xis)
    with monkeypatch.context() as mp:
        mp.setattr(torch, "randn", lambda *a, **k: next(it).cpu())
        with torch.no_grad():
            return fn(z, model)


SAMPLER_CASES = (("Euler", "Mean"), ("Euler", "Tweedie"), ("Heun", "Mean"), ("Heun", "Tweedie"))


@pytest.mark.parametrize("method,last", SAMPLER_CASES, ids=["-".join(c) for c in SAMPLER_CASES])
def test_sampler_device_noise_matches_the_composed_loop(method, last, monkeypatch):
    """noise="device" against the EXISTING loop on the same fp32 toy ZigMa, fed the kernel's own increments through th.randn: final state to
    final state.  The two differ by fp32 re-association of the step arithmetic only, so the limit is twice the distance of the existing loop
    from itself run with float64 step arithmetic (model evaluated in fp32 either way), measured in the test.  On an MI355X (B = 2, 5 steps,
    sigma diffusion 0.5; device path vs loop / the loop's own distance): Euler-Mean 1.02e-7 / 8.57e-8, Euler-Tweedie 1.13e-7 / 9.17e-8,
    Heun-Mean 1.06e-7 / 8.08e-8, Heun-Tweedie 1.03e-7 / 8.46e-8 (profiles/sde_gpu_tests.txt)."""
    from zigma_amd.transport import Sampler
    m = _model()
    calls = [0]

    def model(x, t, **kw):
        calls[0] += 1
        return m(x, t, **kw)
    kw = dict(sampling_method=method, diffusion_form="sigma", diffusion_norm=0.5, last_step=last, num_steps=5)
    seed, stream = 0xfeedface12345678, 3
    z = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(11)).to(DEV)
    xis = [_kernel_normals(seed, stream, k, 0, z.numel()).view(z.shape) for k in range(4)]
    smp = Sampler(_transport())
    ref = _reference_loop(smp.sample_sde(**kw), z, model, xis, monkeypatch)
    ref_calls, calls[0] = calls[0], 0
    ref64 = _reference_loop(smp.sample_sde(**kw), z.double(), lambda x, t, **k: m(x.float(), t.float(), **k).double(), xis, monkeypatch)
    fn = smp.sample_sde(noise="device", seed=seed, stream=stream, **kw)
    with torch.no_grad():
        xs = fn(z, model)
    assert calls[0] == ref_calls == (1 if method == "Euler" else 2) * 4 + 1, "the number of model evaluations"
    assert len(xs) == len(ref) == 5 and all(x.shape == z.shape and x.dtype == z.dtype for x in xs)
    own = rel_err(ref[-1].double().cpu().numpy(), ref64[-1].cpu().numpy())
    dist = rel_err(xs[-1].double().cpu().numpy(), ref[-1].double().cpu().numpy())
    print(f"sde-sampler {method}-{last}: device path vs composed loop {dist:.3e}; composed loop fp32 vs float64 step arithmetic {own:.3e} (limit: twice that)")
    assert 0 < own < 1e-5 and dist <= 2 * own, (dist, own)
    with torch.no_grad():
        again = fn(z, model)
        assert all(torch.equal(a, b) for a, b in zip(xs, again)), "the same seed gives another trajectory"
        other_seed = smp.sample_sde(noise="device", seed=seed + 1, stream=stream, **kw)(z, model)
        other_stream = smp.sample_sde(noise="device", seed=seed, stream=stream + 1, **kw)(z, model)
    assert not torch.equal(other_seed[-1], xs[-1]) and not torch.equal(other_stream[-1], xs[-1]) and not torch.equal(other_seed[-1], other_stream[-1])


def test_sampler_device_noise_refuses_what_it_cannot_run():
    from zigma_amd.transport import Sampler
    smp = Sampler(_transport())
    fn = smp.sample_sde(noise="device", num_steps=3)
    with pytest.raises(ValueError, match="CUDA tensor"):
        fn(torch.zeros(2, 4), lambda x, t: x)
    with pytest.raises(ValueError, match="CUDA tensor"):
        fn(torch.zeros(2, 4, device=DEV, dtype=torch.float64), lambda x, t: x)
    for dt in DT.values():             # all three state types run; a model that answers in another type is cast at the boundary
        xs = fn(torch.ones(2, 6, device=DEV, dtype=dt), lambda x, t: -x.float())
        assert len(xs) == 3 and xs[-1].dtype == dt and bool(torch.isfinite(xs[-1].float()).all())


# ---------------------------------------------------------------------------------------------------
# (f) the sampler, one captured graph per step
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ("Euler", "Heun"))
def test_sampler_graph_equals_eager(method):
    from zigma_amd.transport import Sampler
    m = _model()
    smp = Sampler(_transport())
    kw = dict(sampling_method=method, diffusion_form="sigma", diffusion_norm=0.5, num_steps=5, noise="device", stream=2)
    z = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(12)).to(DEV)
    eager, graphed = smp.sample_sde(seed=21, **kw), smp.sample_sde(seed=21, graph=True, **kw)
    with torch.no_grad():
        want, got = eager(z, m), graphed(z, m)
        assert graphed.captures == 1 and len(got) == 5
        assert all(torch.equal(a, b) for a, b in zip(want, got)), "the captured step differs from the eager one"
        # a second trajectory after reset() with a new seed reuses the capture and equals its eager twin
        graphed.noise.reset(seed=22)
        eager.noise.reset(seed=22)
        z2 = z.flip(0).contiguous()
        want2, got2 = eager(z2, m), graphed(z2, m)
        assert graphed.captures == 1
        assert all(torch.equal(a, b) for a, b in zip(want2, got2)) and not torch.equal(got2[-1], got[-1])


def test_sampler_graph_follows_guided_set_scale():
    from test_gpu_cfg import _toy
    from zigma_amd.guidance import Guided
    from zigma_amd.transport import Sampler
    m, _ = _toy()
    smp = Sampler(_transport())
    kw = dict(sampling_method="Euler", diffusion_form="sigma", diffusion_norm=0.5, num_steps=4, noise="device", seed=5)
    z, y = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(13)).to(DEV), torch.tensor([1, 3], device=DEV)
    guided = Guided(m, [1.5, 4.0])
    graphed, eager = smp.sample_sde(graph=True, **kw), smp.sample_sde(**kw)
    with torch.no_grad():
        first = graphed(z, guided, y=y)
        assert all(torch.equal(a, b) for a, b in zip(first, eager(z, guided, y=y)))
        guided.set_scale([7.5, -1.0])
        second = graphed(z, guided, y=y)
        assert graphed.captures == 1, "set_scale() must not need a new capture"
        assert all(torch.equal(a, b) for a, b in zip(second, eager(z, guided, y=y)))
        assert not torch.equal(first[-1], second[-1])


# ---------------------------------------------------------------------------------------------------
# (g) end to end against the reference noise, no network: Gaussian data on the linear path
# ---------------------------------------------------------------------------------------------------
def test_device_and_reference_noise_sample_the_same_process():
    """x1 ~ N(0, s^2) has the closed-form velocity v(x, t) = (t s^2 - (1 - t)) / (t^2 s^2 + (1 - t)^2) x.  2^18 elements, 50 Euler-Maruyama steps,
    sigma diffusion: the final sample variance under device noise and under the reference's CPU noise estimate the same discretised process
    (the discretisation bias cancels), so they differ by sampling error only: six standard errors of the difference of two variance estimates."""
    from zigma_amd.transport import Sampler, create_transport
    s, N = 2.0, 2 ** 18

    def velocity(x, t):
        tt = t.view(-1, 1).to(x)
        return (tt * s * s - (1 - tt)) / (tt * tt * s * s + (1 - tt) ** 2) * x
    smp = Sampler(create_transport())
    kw = dict(sampling_method="Euler", diffusion_form="sigma", num_steps=50)
    z = torch.randn(64, N // 64, generator=torch.Generator().manual_seed(14)).to(DEV)
    torch.manual_seed(15)
    with torch.no_grad():
        ref = smp.sample_sde(**kw)(z, velocity)[-1]
        dev = smp.sample_sde(noise="device", seed=16, **kw)(z, velocity)[-1]
    v_ref, v_dev = float(ref.double().var()), float(dev.double().var())
    bound = 6 * s * s * np.sqrt(2 / N) * np.sqrt(2)
    print(f"sde-gaussian: final variance {v_dev:.4f} (device noise) vs {v_ref:.4f} (reference noise), target {s * s:g}; |difference| {abs(v_dev - v_ref):.2e} (limit {bound:.2e})")
    assert abs(v_dev - v_ref) <= bound and abs(v_ref - s * s) < 0.5

"""CPU checks of the on-device SDE sampler: the numpy restatement of tests/sde_cases.py against the generator's known answers, the case table,
the plan of zigma_amd/transport/sde_device.py against the existing composed loop in float64, the new parameter blocks, and the GPU file's
sweep and refusal checks on a numpy stand-in at the C ABI.  The kernels themselves run in tests/test_gpu_sde.py.
"""
import ast
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import sde_cases as sc  # noqa: E402

CASES = sc.sde_cases()
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "sde_sampler.npz"))
GOLDEN_CASES = ast.literal_eval(str(GOLDEN["cases"]))


def _ids(cases):
    return [c["id"] for c in cases]


# ---------------------------------------------------------------------------------------------------
# the restatement and the table
# ---------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    for ctr, key, want in sc.KNOWN_ANSWERS:
        got = sc.philox4x32_10(np.array(ctr, dtype=np.uint64), np.array(key, dtype=np.uint64))
        assert [int(v) for v in got] == list(want), (ctr, key, [hex(int(v)) for v in got])
    # ... and the vectorised field: quad 2^32 - 1 and the carry into the counter's high word
    edge = sc.field_words(5, 6, 7, 2 ** 34 - 4, 8)
    assert np.array_equal(edge[0], sc.philox4x32_10(np.array([0xffffffff, 0, 7, 6], np.uint64), np.array([5, 0], np.uint64)))
    assert np.array_equal(edge[1], sc.philox4x32_10(np.array([0, 1, 7, 6], np.uint64), np.array([5, 0], np.uint64)))


def test_normal_map_edges():
    """u in (0, 1], never 0; the tail reach; exact zeros; normal j of a quad"""
    w = np.array([[0, 0, 0xffffffff, 0x40000000], [0xffffff00, 0x80000000, 0x000000ff, 0xc0000000]], np.uint32)
    z = sc.normals_f64(w).reshape(2, 4)
    reach = np.sqrt(48 * np.log(2))
    assert z[0, 0] == pytest.approx(reach) and abs(z[0, 1]) < 1e-15              # u = 2^-24, angle 0
    assert z[0, 2] == 0 and z[0, 3] == 0                                          # u = 1: rho = 0
    assert z[1, 0] == 0 and z[1, 1] == 0 and abs(z[1, 3] + reach) < 1e-12         # angle 3 pi / 2 at u = 2^-24
    assert np.isfinite(z).all()


def test_table_coverage():
    ids = _ids(CASES)
    assert len(set(ids)) == len(ids)
    got = lambda k, cases=CASES: {c[k] for c in cases}
    assert got("n") == set(sc.SDE_N) and got("kind") == set(sc.SDE_KINDS)
    assert sc.SDE_N[-1] == 4 * 256 * 2 + 3 and any(n % 8 == 0 for n in sc.SDE_N) and any(n % 4 == 0 and n % 8 for n in sc.SDE_N)
    for kind in sc.SDE_KINDS:          # every axis in every I/O type
        sub = [c for c in CASES if c["kind"] == kind]
        assert got("present", sub) == set(sc.SDE_SUBSETS), kind
        assert got("offset", sub) == set(sc.SDE_OFFSETS) and got("step", sub) == set(sc.SDE_STEPS) and got("stream", sub) == set(sc.SDE_STREAMS), kind
        assert got("absolute", sub) == {True, False} and got("cn0", sub) == {True, False} and got("alias", sub) == {True, False}, kind
        assert got("rps", sub) == set(sc.SDE_ROWS_PER_STEP), kind
    assert any(not c["state"] for c in CASES) and all(c["cn0"] and c["absolute"] for c in CASES if not c["state"])
    assert any(not c["absolute"] and c["step"] * c["rps"] + c["row"] >= sc.SDE_COEF_ROWS for c in CASES), "no case reads the clamped row"
    assert any(not c["absolute"] and c["step"] == 1 and c["table_row"] == c["rps"] + c["row"] for c in CASES), "no case reads a row of a later step"
    assert all(c["alias"] <= c["present"][0] for c in CASES)
    assert sc.SDE_OFFSETS[1] == 2 ** 34 - 4 and (sc.SDE_OFFSETS[2] // 4) % 2 == 1 and all(o % 4 == 0 for o in sc.SDE_OFFSETS)
    assert len(sc.REFUSALS) == len({w for w, _ in sc.REFUSALS})


@pytest.mark.parametrize("c", CASES, ids=_ids(CASES))
def test_rounded_reference_passes(c):
    """the float64 reference rounded to the case's type stays inside the limit the kernel is held to, with the float32 model of the normals"""
    inp = sc.sde_inputs(c)
    ref = sc.sde_reference(c, inp)
    assert np.isfinite(ref["out"]).all() and ref["out"].shape == (c["n"],)
    xi32 = None if c["cn0"] else sc.normals_f32(ref["words"])[:c["n"]]
    model, _ = sc.launch_f64(inp["coef"][c["table_row"]], inp["a"], inp["b"], inp["c"], xi32)
    got = sc.round_to(np.broadcast_to(model, (c["n"],)), c["kind"]).astype(np.float64)
    assert np.all(np.abs(got - ref["out"]) <= np.maximum(ref["allow"], 1e-300)), c["id"]


# ---------------------------------------------------------------------------------------------------
# the distribution of the exact map, at the coordinates the GPU file draws at
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exact_draws():
    import test_gpu_sde as gf
    words = {}

    def draw(seed, stream, step):
        words[(seed, stream, step)] = sc.field_words(seed, stream, step, 0, sc.DIST_N)
        return sc.normals_f64(words[(seed, stream, step)])
    z, others = gf.dist_draws(draw)
    return z, others, words


def test_exact_map_passes_the_distribution_checks(exact_draws):
    z, others, _ = exact_draws
    assert z.size == sc.DIST_N and set(others) == {"step + 1", "stream 1", "seed + 1"}
    for name, value, bound in sc.distribution_checks(z, others):
        assert value <= bound, (name, value, bound)
    assert float(np.max(np.abs(z))) <= np.sqrt(48 * np.log(2))


def test_float32_model_of_the_map_keeps_half_the_bound(exact_draws):
    """logf, sqrtf, sincospif and the product each rounded once: within NORMAL_K / 2 units of 2^-24 max(|xi|, 2^-10) of the float64 map"""
    worst = max(sc.normal_ratio(sc.normals_f32(w), sc.normals_f64(w)) for w in exact_draws[2].values())
    assert worst <= sc.NORMAL_K / 2, worst


# ---------------------------------------------------------------------------------------------------
# the plan against the existing loop
# ---------------------------------------------------------------------------------------------------
def _toy_model(x, t, **kw):
    tt = t.view(-1, *([1] * (x.dim() - 1)))
    return torch.tanh(x) * (0.3 + tt) - 0.5 * x


def _golden_sampler(i):
    from zigma_amd.transport import ModelType, PathType, Sampler, Transport, WeightType
    path, pred, smp, form, norm, last, lss, n = GOLDEN_CASES[i]
    mt = {"velocity": ModelType.VELOCITY, "noise": ModelType.NOISE, "score": ModelType.SCORE}[pred]
    pt = {"Linear": PathType.LINEAR, "GVP": PathType.GVP, "VP": PathType.VP}[path]
    tr = Transport(model_type=mt, path_type=pt, loss_type=WeightType.NONE, train_eps=1e-3, sample_eps=1e-3)
    return Sampler(tr), dict(sampling_method=smp, diffusion_form=form, diffusion_norm=norm, last_step=last, last_step_size=lss, num_steps=n)


def _evaluate_plan(plan, x0, xis, model):
    """the planned rows in float64 numpy, the model at the plan's times -> list of num_steps states"""
    x, xs, B = np.asarray(x0, np.float64), [], x0.shape[0]
    m = lambda x, t, dt=torch.float64: model(torch.from_numpy(x), torch.full((B,), float(t), dtype=dt)).numpy()
    rows = plan.coef.reshape(-1, 4)
    for k in range(plan.num_steps - 1):
        r, t = rows[k * plan.rows_per_step:], plan.times[k]
        if plan.method == "Euler":
            x = sc.launch_f64(r[0], x, m(x, t[0]), None, xis[k])[0]
        else:
            xhat = sc.launch_f64(r[0], x, None, None, xis[k])[0]
            xp = sc.launch_f64(r[1], xhat, m(xhat, t[0]), None, None)[0]
            x = sc.launch_f64(r[2], xhat, xp, m(xp, t[1]), None)[0]
        xs.append(x)
    # (Sampler.sample_sde hands the last step a float32 time tensor whatever the state's type)
    xs.append(x if plan.last_step is None else sc.launch_f64(rows[plan.last_row], x, m(x, plan.times[-1][0], torch.float32), None, None)[0])
    return xs


@pytest.mark.parametrize("i", range(len(GOLDEN_CASES)), ids=["-".join(str(v) for v in c[:6]) for c in GOLDEN_CASES])
def test_plan_reproduces_the_existing_loop_in_float64(i, monkeypatch):
    """with th.randn handing out the restated increments, the existing `sde` loop in float64 and the float64 evaluation of the planned rows are two
    evaluations of the same affine maps: only re-association separates them (1e-12 relative)"""
    from zigma_amd.transport import sde_device as sd
    smp, kw = _golden_sampler(i)
    x0 = torch.from_numpy(GOLDEN[f"x0_{i}"]).double()
    n = kw["num_steps"]
    xis = [sc.field(77 + i, 2, k, 0, x0.numel())[1].reshape(x0.shape) for k in range(n - 1)]
    it = iter(xis)
    with monkeypatch.context() as mp:
        mp.setattr(torch, "randn", lambda *a, **k: torch.from_numpy(next(it)))
        want = smp.sample_sde(**kw)(x0, _toy_model)
    assert next(it, None) is None, "the existing loop drew fewer increments than the plan has steps"
    plan = sd.make_plan(smp, time_dtype=torch.float64, **kw)
    assert plan.coef.shape == ((n - 1) * plan.rows_per_step + 1, 4) and plan.coef.dtype == np.float64 and np.isfinite(plan.coef).all()
    got = _evaluate_plan(plan, x0.numpy(), xis, _toy_model)
    assert len(got) == len(want) == n
    for k in (n // 2, n - 1):
        w = want[k].numpy()
        assert np.linalg.norm(got[k] - w) <= 1e-12 * np.linalg.norm(w), (i, k, np.linalg.norm(got[k] - w) / np.linalg.norm(w))
    # (the same trajectory in float32 is the committed golden of the reference: the restated noise is not its noise, so only the shapes compare)
    assert want[-1].shape == GOLDEN[f"last_{i}"].shape


@pytest.mark.parametrize("i", range(len(GOLDEN_CASES)), ids=["-".join(str(v) for v in c[:6]) for c in GOLDEN_CASES])
def test_plan_times_are_the_existing_loops_bit_for_bit(i):
    """the float32 times the existing loop hands the model, in order, are the plan's table"""
    from zigma_amd.transport import sde_device as sd
    smp, kw = _golden_sampler(i)
    seen = []

    def model(x, t, **k):
        assert t.dtype == torch.float32 and bool((t == t[0]).all())
        seen.append(t[0].clone())
        return _toy_model(x, t)
    torch.manual_seed(0)
    smp.sample_sde(**kw)(torch.from_numpy(GOLDEN[f"x0_{i}"]), model)
    plan = sd.make_plan(smp, **kw)
    assert plan.times.dtype == np.float32 and plan.times.shape == (kw["num_steps"], plan.n_t)
    want = plan.times[:-1].reshape(-1).tolist() + ([] if kw["last_step"] is None else [plan.times[-1, 0]])
    got = torch.stack(seen).numpy()
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), np.asarray(want, np.float32).view(np.uint32))
    assert (plan.times[-1] == plan.times[-1, 0]).all()


def test_non_finite_coefficients_raise_when_the_plan_is_made():
    from zigma_amd.transport import ModelType, PathType, Sampler, Transport, WeightType
    tr = Transport(model_type=ModelType.SCORE, path_type=PathType.LINEAR, loss_type=WeightType.NONE, train_eps=0, sample_eps=0)
    with pytest.raises(ValueError, match=r"non-finite coefficient .* step 0 .*SBDM"):
        Sampler(tr).sample_sde(noise="device", num_steps=5)                     # a score model asked to start at t = 0


def test_sample_sde_arguments():
    from zigma_amd.transport import Sampler, create_transport
    smp = Sampler(create_transport())
    with pytest.raises(ValueError, match="graph=True needs noise='device'"):
        smp.sample_sde(graph=True)
    with pytest.raises(ValueError, match="'reference' or 'device'"):
        smp.sample_sde(noise="cpu")
    with pytest.raises(ValueError, match="seed"):
        smp.sample_sde(noise="device", diffusion_form="sigma", seed=2 ** 64, num_steps=3)
    with pytest.raises(ValueError, match="stream"):
        smp.sample_sde(noise="device", diffusion_form="sigma", stream=2 ** 32, num_steps=3)
    with pytest.raises(NotImplementedError):
        smp.sample_sde(noise="device", sampling_method="nope", num_steps=3)
    fn = smp.sample_sde(noise="device", diffusion_form="sigma", seed=2 ** 64 - 1, stream=2 ** 32 - 1, num_steps=3)
    with pytest.raises(ValueError, match="CUDA tensor in float32, bfloat16 or float16"):
        fn(torch.zeros(2, 4), lambda x, t: x)


@pytest.mark.parametrize("cname,st", [("zigma_sde_step_params_t", "SdeStepParams"), ("zigma_sde_advance_params_t", "SdeAdvanceParams"), ("zigma_sde_state_t", "SdeState")])
def test_sde_structs_match_the_header(cname, st):
    """sizeof / offsetof as gcc sees include/zigma_hip.h equal the ctypes mirrors"""
    from zigma_amd import _lib
    st = getattr(_lib, st)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "zigma_hip.h"', "int main(void){", f'printf("{cname} %zu\\n", sizeof({cname}));']
    lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in st._fields_] + ["return 0;}"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "a.c"), os.path.join(d, "a.out")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    got = dict(ln.split() for ln in out.strip().splitlines())
    assert int(got[cname]) == ctypes.sizeof(st)
    for f, _ in st._fields_:
        assert int(got[f"{cname}.{f}"]) == getattr(st, f).offset, f
    assert ctypes.sizeof(_lib.SdeState) == 16 and {"zigma_sde_step_fwd", "zigma_sde_advance"} <= set(_lib.EXPORTS) and _lib.SDE_ROW_ABSOLUTE == sc.ROW_ABSOLUTE
    hdr = open(os.path.join(ROOT, "include", "zigma_hip.h")).read()
    assert "#define ZIGMA_ABI_VERSION 11 " in hdr and "#define ZIGMA_SDE_ROW_ABSOLUTE 1 " in hdr


# ---------------------------------------------------------------------------------------------------
# the GPU file's sweep and refusal checks on the CPU, served at the C ABI by the numpy restatement
# ---------------------------------------------------------------------------------------------------
MUTATION = {"kind": None}          # None | "counter-swapped" | "noise-reused" | "tail-unwritten"


def _standin_sde_step(P):
    import kernel_standins as ks
    refuse = ks._refuse
    if P.n < 0 or P.n > 0x7fffffff * 2048:
        refuse(-2)
    if P.elem_offset < 0 or P.elem_offset % 4 or P.elem_offset > 2 ** 63 - 1 - P.n:
        refuse(-2)
    if P.rows_per_step < 1 or P.row < 0:
        refuse(-2)
    absolute = bool(P.flags & 1)
    if P.coef_rows < 1 or (absolute and P.row >= P.coef_rows):
        refuse(-2)
    if P.flags & ~1:
        refuse(-6)
    if P.dtype not in (0, 1, 2):
        refuse(-3)
    if P.n == 0:
        return ks.LAST_KERNEL[0]
    if not (P.out and P.coef):
        refuse(-1)
    if not P.state and (not absolute or P.bits_out):
        refuse(-1)
    if any((q or 0) % 16 for q in (P.a, P.b, P.c, P.out, P.coef, P.state, P.bits_out)):
        refuse(-4)
    n, dt = P.n, ks._io_dtype(P.dtype)
    state = None if not P.state else ks._view(P.state, (4,), (1,), torch.int32).numpy().view(np.uint32)
    r = P.row if absolute else min(int(state[3]) * P.rows_per_step + P.row, P.coef_rows - 1)
    row = ks._view(P.coef, (P.coef_rows, 4), (4, 1), torch.float32)[r].double().numpy()
    ops = [None if not q else ks._view(q, (n,), (1,), dt).double().numpy() for q in (P.a, P.b, P.c)]
    xi = None
    if state is not None and row[3] != 0:
        seed, stream, step = int(state[0]) | (int(state[1]) << 32), int(state[2]), int(state[3])
        if MUTATION["kind"] == "counter-swapped":
            stream, step = step, stream
        if MUTATION["kind"] == "noise-reused":
            step = 0
        words, xi = sc.field(seed, stream, step, P.elem_offset, n)
        if P.bits_out:
            ks._view(P.bits_out, (words.size,), (1,), torch.int32).copy_(torch.from_numpy(words.reshape(-1).view(np.int32).copy()))
    out = np.broadcast_to(sc.launch_f64(row, ops[0], ops[1], ops[2], xi)[0], (n,))
    keep = n - 1 if MUTATION["kind"] == "tail-unwritten" and n % 8 else n
    ks._view(P.out, (n,), (1,), dt)[:keep].copy_(torch.from_numpy(np.array(out[:keep])).float().to(dt))
    return "sde_step"


@pytest.fixture
def gpu_file(monkeypatch):
    import kernel_standins as ks
    import test_gpu_sde as gf
    ks.install_lib_call(monkeypatch)
    from zigma_amd import _lib

    def call(fn_name, params, device):
        assert fn_name == "zigma_sde_step_fwd", fn_name
        ks.LAST_KERNEL[0] = _standin_sde_step(params)
    monkeypatch.setattr(_lib, "call", call)
    monkeypatch.setattr(gf, "DEV", "cpu")
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    monkeypatch.setitem(MUTATION, "kind", None)
    return gf


@pytest.mark.parametrize("c", CASES, ids=_ids(CASES))
def test_gpu_sweep_checks_pass_on_the_stand_in(c, gpu_file, capsys):
    gpu_file.test_sde_sweep(c)
    assert f"sde-sweep {c['id']}: " in capsys.readouterr().out


@pytest.mark.parametrize("what,status", [r for r in sc.REFUSALS if r[0] != "null-block"], ids=[w for w, _ in sc.REFUSALS if w != "null-block"])
def test_gpu_refusal_checks_pass_on_the_stand_in(what, status, gpu_file):
    gpu_file.test_sde_refusals(what, status)


def test_gpu_refusal_order_check_passes_on_the_stand_in(gpu_file):
    gpu_file.test_sde_refusal_order_and_empty_call()


@pytest.mark.parametrize("mutation,message", [("counter-swapped", "Philox words"), ("noise-reused", "Philox words"), ("tail-unwritten", "left unwritten")])
def test_gpu_sweep_checks_notice_a_wrong_kernel(mutation, message, gpu_file, monkeypatch):
    """a kernel that swaps two counter words, reuses one step's noise for every step, or leaves a tail element unwritten turns cases red"""
    monkeypatch.setitem(MUTATION, "kind", mutation)
    red = 0
    for c in CASES:
        try:
            gpu_file.test_sde_sweep(c)
        except AssertionError as e:       # (in place, an unwritten element keeps the operand's value: the limit catches it, not the NaN check)
            assert message in str(e) or (mutation == "tail-unwritten" and c["alias"]), (c["id"], str(e))
            red += 1
    assert red >= 3, (mutation, red)

"""Host side of the 16-bit training-step tail (zigma_amd.optim.FusedAdamW16, zigma_optim16_* of include/zigma_hip.h): the ctypes mirrors, the
registration in the build, the exact invariants and the unbiasedness of the rounding restated in tests/optim16_cases.py, the octet rule of its bits, the
two simulations whose inputs the GPU tests reuse, and the optimizer's host logic.  No GPU."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import optim16_cases as c16
import optim_cases as oc
import sde_cases as sc
from test_optim_cpu import checked_instantiations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_optim16_structs_match_the_header():
    """sizeof / offsetof as gcc sees include/zigma_hip.h (the recipe of test_optim_cpu.py); the ABI is still 11"""
    from zigma_amd import _lib
    structs = {"zigma_optim16_params_t": _lib.Optim16Params, "zigma_optim16_row_t": _lib.Optim16Row}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "zigma_hip.h"', "int main(void){"]
    for cname, st in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in st._fields_:
            lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines.append('printf("abi %d\\n", ZIGMA_ABI_VERSION);')
    lines.append('printf("nearest %d\\n", ZIGMA_OPTIM16_NEAREST);')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "a.c"), os.path.join(d, "a.out")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    got = {l.split()[0]: int(l.split()[1]) for l in out.strip().splitlines()}
    for cname, st in structs.items():
        assert got[cname] == ctypes.sizeof(st), cname
        for f, _ in st._fields_:
            assert got[f"{cname}.{f}"] == getattr(st, f).offset, (cname, f)
    assert got["zigma_optim16_row_t"] == 8 * c16.ROW_WORDS                           # what optim.py writes: ten int64 per row
    assert [getattr(_lib.Optim16Row, f).offset // 8 for f in ("p", "g", "m", "v", "ema", "numel", "pid", "dbg_x32", "dbg_bits")] == list(range(9))
    assert got["abi"] == 11 and got["nearest"] == _lib.OPTIM16_NEAREST == c16.NEAREST


def test_symbols_sources_and_kernels_are_registered():
    from zigma_amd import _lib, build, optim
    for name in ("zigma_optim16_grad_sumsq", "zigma_optim16_adamw", "zigma_optim_prepare"):
        assert name in _lib.EXPORTS
    assert "optim_step.hip" in build.SOURCES and build.SOURCE_FLAGS["optim_step.hip"] == build._RES
    assert "multi_sumsq_kernel" in build.NO_SCRATCH_KERNELS and "multi_adamw_kernel" in build.NO_SCRATCH_KERNELS
    assert checked_instantiations() == (7, 2, 5)          # the bf16 norm kernel and the two bf16 update kernels are among the checked ones
    hdr = open(os.path.join(ROOT, "include", "zigma_hip.h")).read()
    assert "#define ZIGMA_ABI_VERSION 11 " in hdr and "(11, no block changed): zigma_optim16_* added" in hdr
    src = open(os.path.join(ROOT, "zigma_amd", "csrc", "optim_step.hip")).read()
    assert "multi_sumsq_kernel<zigma_optim16_row_t>" in src and "StoreBf16<true>" in src and "StoreBf16<false>" in src
    # one copy of the generator, in the shared header
    csrc = os.path.join(ROOT, "zigma_amd", "csrc")
    holders = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h", ".inc")) and "u32x4 philox4x32_10(" in open(os.path.join(csrc, f)).read()]
    assert holders == ["zigma_common.h"]
    assert issubclass(optim.FusedAdamW16, torch.optim.Optimizer)


# ---- the rounding ---------------------------------------------------------------------------------------------------------------------------------------
def _varied(n, seed):
    rng = np.random.RandomState(seed)
    x = (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-30, 30, n)).astype(np.float32)
    x[:6] = np.array([0.0, -0.0, 1e-40, -1e-40, 3.3e38, -3.3e38], np.float32)          # zeros, subnormals, near the largest finite value
    return x


def test_rne_restatement_is_torchs_rounding():
    x = _varied(1 << 16, 1)
    x[6:9] = [np.inf, -np.inf, np.nan]
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    ok = ~np.isnan(x)                                                                      # (torch's bits of a NaN differ between its CPU paths; NaN stays NaN)
    assert np.array_equal(c16.rne_bf16(x)[ok], want[ok]) and np.all(np.isnan(c16.widen(c16.rne_bf16(x)[~ok]))) and (~ok).sum() == 1
    assert np.array_equal(c16.widen(c16.rne_bf16(x))[:6], torch.from_numpy(x[:6]).to(torch.bfloat16).float().numpy())


def test_exact_invariants_of_the_stochastic_rounding():
    x = _varied(1 << 14, 2)
    u = x.view(np.uint32)
    rep = c16.widen((u >> 16).astype(np.uint16))                                           # bf16-representable values
    for r in (0, 1, 0x7fff, 0x8000, 0xfffe, 0xffff):
        assert np.array_equal(c16.sr_bf16(rep, np.full(rep.size, r, np.uint16)), (u >> 16).astype(np.uint16)), r          # unchanged for every r
    assert np.array_equal(c16.sr_bf16(x, np.zeros(x.size, np.uint16)), (u >> 16).astype(np.uint16))                      # r = 0 truncates
    inexact = (u & 0xffff) != 0
    away = c16.sr_bf16(x, np.full(x.size, 0xffff, np.uint16))
    assert inexact.sum() > 16000 and np.array_equal(away[inexact], ((u >> 16) + 1).astype(np.uint16)[inexact])          # r = 65535: away from zero
    assert np.all(np.abs(c16.widen(away[inexact]).astype(np.float64)) > np.abs(x[inexact].astype(np.float64)))
    r = np.random.RandomState(3).randint(0, 1 << 16, x.size).astype(np.uint16)
    assert np.array_equal(c16.sr_bf16(-x, r), c16.sr_bf16(x, r) ^ np.uint16(0x8000))                                     # negatives mirror positives
    got = c16.widen(c16.sr_bf16(x, r)).astype(np.float64)
    lo, hi = c16.widen((u >> 16).astype(np.uint16)).astype(np.float64), c16.widen(away).astype(np.float64)
    assert np.all((got == lo) | (got == hi))                                                                               # one of the two neighbours
    # the carry out of the largest finite value gives inf, as round-to-nearest does
    big = np.array([3.4e38, -3.4e38], np.float32)
    assert list(c16.sr_bf16(big, np.full(2, 0xffff, np.uint16))) == [0x7f80, 0xff80] == list(c16.rne_bf16(big))
    # inf and NaN take the nearest path whatever the bits
    sp = np.array([np.inf, -np.inf, np.nan, -np.nan], np.float32)
    sp = np.concatenate([sp, np.array([0x7f800001, 0xffc12345, 0x7fbfffff], np.uint32).view(np.float32)])
    for rr in (0, 0x8000, 0xffff):
        assert np.array_equal(c16.sr_bf16(sp, np.full(sp.size, rr, np.uint16)), c16.rne_bf16(sp)), rr
    assert list(c16.rne_bf16(sp[:2])) == [0x7f80, 0xff80] and np.all(np.isnan(c16.widen(c16.rne_bf16(sp[2:]))))


@pytest.mark.parametrize("low16", [4096, 32768, 61440])
def test_the_restatement_is_unbiased(low16):
    """x = 1.0 + k 2^-23 with the low 16 bits = low16: over 2^14 elements the share rounded up lies within 5 sigma of f = low16 / 65536,
    sigma = sqrt(f (1 - f) / n).  Bits at seed 1234, pid 3, step 7, stream 0."""
    n = 1 << 14
    x = np.full(n, np.uint32(0x3f800000 + low16), np.uint32).view(np.float32)
    up = c16.sr_bf16(x, c16.bits16(n, 1234, 3, 7, 0)) == 0x3f81
    f = low16 / 65536.0
    sigma = np.sqrt(f * (1 - f) / n)
    dev = abs(up.mean() - f) / sigma
    print(f"low16 {low16}: share rounded up {up.mean():.5f}, expected {f:.5f}, {dev:.2f} sigma")
    assert dev <= 5.0
    assert abs(float(c16.widen(c16.sr_bf16(x, c16.bits16(n, 1234, 3, 7, 0))).astype(np.float64).mean()) - float(x[0])) <= 5 * sigma * 2.0 ** -7


def test_bits_follow_the_octet_rule():
    """element i takes half j & 1 of word j >> 1 (j = i & 7) of the Philox output at counter (i >> 3, pid, step, stream): the same bits whichever piece or
    path processes it — a prefix, the piece that starts at a chunk offset, the element alone"""
    seed, pid, step, stream = 0x0123456789abcdef, 5, 9, 2
    n = 3 * oc.CHUNK + 5
    bits = c16.bits16(n, seed, pid, step, stream)
    assert bits.dtype == np.uint16 and bits.size == n
    for i in (0, 1, 7, 8, 9, 4095, 4096, 4097, n - 1):
        w = sc.philox4x32_10(np.array([i >> 3, pid, step, stream], np.uint64), (seed & 0xffffffff, seed >> 32))
        j = i & 7
        assert int(bits[i]) == (int(w[j >> 1]) >> (16 * (j & 1))) & 0xffff, i
    for m in (1, 7, 8, 9, 257, oc.CHUNK + 1):
        assert np.array_equal(c16.bits16(m, seed, pid, step, stream), bits[:m])
    # a piece at a chunk offset (a multiple of 8) is whole octets of the tensor
    off = 2 * oc.CHUNK
    o = np.arange(off >> 3, (off >> 3) + 4, dtype=np.uint64)
    w = sc.philox4x32_10(np.stack([o, np.full_like(o, pid), np.full_like(o, step), np.full_like(o, stream)], -1), (seed & 0xffffffff, seed >> 32))
    assert np.array_equal(np.stack([w & 0xffff, w >> 16], -1).reshape(-1).astype(np.uint16), bits[off:off + 32])
    # every coordinate matters
    for other in ((seed + 1, pid, step, stream), (seed, pid + 1, step, stream), (seed, pid, step + 1, stream), (seed, pid, step, stream + 1), (seed ^ (1 << 40), pid, step, stream)):
        assert (c16.bits16(4096, *other) == bits[:4096]).mean() < 0.01
    assert abs(bits.astype(np.float64).mean() / 65535.0 - 0.5) < 5 / np.sqrt(12 * n)


# ---- the sweep's inputs and the two simulations --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(oc.CONFIGS))
def test_error_constant_of_the_16_bit_sweep(name):
    """K from numpy alone on the bf16-rounded sweep: about ten roundings, K <= 16"""
    K, worst = c16.error_constant(name)
    print(f"K16[{name}] = {K:.3f}; worst multiples per stream {worst}")
    assert 0 < K <= 16
    rows = c16.sweep_values(1 + oc.CONFIGS[name]["step0"], oc.CONFIGS[name]["step0"] == 0)
    for r in rows:
        assert np.array_equal(c16.round_bf16(r["p"]), r["p"]) and np.array_equal(c16.round_bf16(r["g"]), r["g"])
    assert len(rows) == 14 * len(oc.SIZES) == 168 and max(len(r["p"]) for r in rows) == 3 * 4096 + 5


def test_sweep_layout_windows_are_disjoint_and_cover_both_paths():
    rows = c16.sweep_values(1, True)
    bufs, wins = c16.sweep_layout(rows)
    for k in c16.STREAMS:
        spans = sorted((w[k], w[k] + w["n"]) for w in wins if w[k] is not None)
        assert all(a[1] < b[0] for a, b in zip(spans, spans[1:]) if a[1] > a[0])
        assert spans[-1][1] < bufs[k].size and spans[0][0] > 0
    q = lambda w, k: w[k] is None or (w[k] * c16.WIDTH[k]) % 16 == 0
    wide = [w for w in wins if w["n"] >= 8 and all(q(w, k) for k in c16.STREAMS)]
    assert len(wide) >= 24 and len(wins) - len(wide) >= 120
    assert any(w["ema"] is None for w in wide) and any(w["ema"] is not None for w in wide) and sum(w["ema"] is None for w in wins) >= 20
    # one present stream at a time, a bf16 stream by 1 ... 7 elements
    offs = set()
    for i, w in enumerate(wins):
        off = [k for k in c16.STREAMS if not q(w, k)]
        assert len(off) == (0 if i >= len(oc.SIZES) * 11 else 1), i
        offs.update((k, w[k] % (16 // c16.WIDTH[k])) for k in off)
    assert {o for k, o in offs if k == "p"} == set(range(1, 8)) and {k for k, _ in offs} == set(c16.STREAMS)
    assert bufs["p"].dtype == np.uint16 and int((bufs["p"] == c16.NAN16).sum()) == bufs["p"].size - sum(w["n"] for w in wins)
    assert int(np.isnan(bufs["m"]).sum()) == bufs["m"].size - sum(w["n"] for w in wins)


def test_stall_sigma_and_displacement():
    """the headline test's band from the per-step fractions: the fp32 mean moves by about 0.0256, sigma of the 4096-element mean is about 1.5e-4; and
    the same steps with round-to-nearest never move a 1.0 (the update is 1e-4, half an ulp below 1.0 is 2^-9 = 1.95e-3)"""
    sigma, moved = c16.stall_sigma()
    print(f"stall: sigma of the mean {sigma:.3e}, float64 displacement {moved:.6f}")
    assert 0.0250 < moved < 0.0257 and 1.0e-4 < sigma < 2.0e-4 and moved > 100 * sigma
    c = c16.STALL
    p, m, v = np.ones(4, np.float32), np.zeros(4, np.float32), np.zeros(4, np.float32)
    for t in range(1, 33):
        x, m, v, _ = oc.step_f32(p, np.full(4, c["g"], np.float32), m, v, None, step=t, lr=c["lr"], beta1=c["beta1"], beta2=c["beta2"], eps=c["eps"], wd=0.0, ema_decay=0.0)
        assert np.all(x < 1.0) and np.array_equal(c16.round_bf16(x), p)


def test_distance_simulation_shows_the_inputs_satisfy_the_condition():
    """the GPU distance test's inputs, without the kernel: float32 AdamW arithmetic with the three write-backs.  The stochastic run's RMS distance to the
    float32 trajectory is at most half the nearest run's at 64 steps already (the GPU test runs 256, where the ratio is smaller still)."""
    rne, sr = c16.dist_simulation(steps=64)
    print(f"distance simulation, 64 steps: nearest {rne:.3e}, stochastic {sr:.3e}, ratio {sr / rne:.3f}")
    assert sr <= 0.5 * rne and rne > 0
    w, g = c16.dist_inputs()
    assert np.array_equal(c16.round_bf16(w), w) and np.array_equal(c16.round_bf16(g), g) and abs(float(w.std()) - 0.02) < 1e-3 and np.all(g != 0)


# ---- host logic of the optimizer ------------------------------------------------------------------------------------------------------------------------
def _bf(*shape):
    return torch.nn.Parameter(torch.randn(*shape).to(torch.bfloat16))


def test_constructor_refusals():
    """no fallback: whatever the kernel does not take raises at construction, and says where it belongs"""
    from zigma_amd import optim
    F = optim.FusedAdamW16
    cpu = [_bf(4, 4)]
    with pytest.raises(ValueError, match="needs a GPU"):
        F(cpu)
    real = optim._device_ok
    optim._device_ok = lambda t: True                                              # from here on the CPU tensors stand in for device tensors
    try:
        F(cpu)
        with pytest.raises(ValueError, match="GradScaler will not unscale 16-bit gradients"):
            F([torch.nn.Parameter(torch.randn(4, 4).half())])
        with pytest.raises(ValueError, match="zigma_amd.optim.FusedAdamW"):
            F([torch.nn.Parameter(torch.randn(4, 4))])
        with pytest.raises(ValueError, match="bfloat16 only"):
            F([torch.nn.Parameter(torch.randn(4, 4).double())])
        with pytest.raises(ValueError, match="bfloat16 only"):
            F([_bf(3), torch.nn.Parameter(torch.randn(4))])
        with pytest.raises(ValueError, match="not contiguous"):
            F([torch.nn.Parameter(torch.randn(4, 6).to(torch.bfloat16).t())])
        with pytest.raises(ValueError, match="sparse"):
            F([torch.randn(4, 4).to_sparse().requires_grad_(True)])
        with pytest.raises(TypeError):
            F([3.0])
        with pytest.raises(ValueError, match="one parameter group"):
            F([dict(params=[_bf(3)]), dict(params=[_bf(3)], lr=1e-2)])
        with pytest.raises(ValueError, match="one parameter group"):
            F(cpu).add_param_group(dict(params=[_bf(3)]))
        for kw in (dict(amsgrad=True), dict(maximize=True)):
            with pytest.raises(ValueError, match="amsgrad and maximize"):
                F(cpu, **kw)
        for kw in (dict(lr=-1.0), dict(lr=float("nan")), dict(lr=float("inf")), dict(lr=torch.tensor(1e-3)), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)),
                   dict(eps=0.0), dict(eps=-1e-8), dict(weight_decay=-0.1), dict(max_grad_norm=0.0), dict(max_grad_norm=float("inf")), dict(ema_decay=1.5),
                   dict(rounding="up"), dict(rounding=None), dict(seed=-1), dict(seed=1 << 64), dict(seed=1.5), dict(stream=-1), dict(stream=1 << 32)):
            with pytest.raises(ValueError):
                F(cpu, **kw)
        o = F(cpu, seed=(1 << 64) - 1, stream=(1 << 32) - 1, rounding="nearest")
        assert isinstance(o, torch.optim.Optimizer) and o.param_groups[0]["rounding"] == "nearest"
        with pytest.raises(RuntimeError, match="ema=False"):
            o.ema_tensors()
        # the fp32 class keeps refusing 16-bit tensors
        with pytest.raises(ValueError, match="float32 only"):
            optim.FusedAdamW(cpu)
    finally:
        optim._device_ok = real


def test_rows_carry_the_index_in_the_group_as_pid():
    from zigma_amd import optim

    class S:
        def __init__(self, ptr, n):
            self.ptr, self.n = ptr, n

        def data_ptr(self):
            return self.ptr

        def numel(self):
            return self.n

    ns = [10, 5000, 0, 8192]
    mk = lambda base: [S(base + 0x10000 * i, n) for i, n in enumerate(ns)]
    ps, gs, ms, vs, es = mk(0x1000000), mk(0x2000000), mk(0x3000000), mk(0x4000000), mk(0x5000000)
    rows = optim.step_rows16(ps, gs, ms, vs, es)
    assert rows[1] == (0x1010000, 0x2010000, 0x3010000, 0x4010000, 0x5010000, 5000, 1, 0, 0, 0) and all(len(r) == c16.ROW_WORDS for r in rows)
    gs[1] = None                                                                   # parameter 1 got no gradient: the others keep their pid
    rows = optim.step_rows16(ps, gs, ms, vs, None)
    assert [r[6] for r in rows] == [0, 2, 3] and [r[4] for r in rows] == [0, 0, 0]
    T = optim.StepTables(width=10, numel_col=5)
    assert T.update(rows, "cpu") and T.table.shape == (3, 10) and T.cmap.tolist() == [[0, 0], [2, 0], [2, 4096]] and not T.update(list(rows), "cpu")
    assert T.update([], "cpu") and T.table.shape == (1, 10) and T.n_chunks == 0


def test_state_dict_keeps_float32_state_and_the_rounding_coordinates():
    """state[p] has torch's keys over fp32 arenas plus "ema" (initialised from the parameters); state_dict() copies, with rounding / seed / stream in the
    group; it loads back WITHOUT rounding the fp32 state to the parameters' bf16 (torch's own load_state_dict would), torch.optim.AdamW's dict on the same
    bf16 model loads with its bf16 moments widened, and per-parameter steps that disagree are refused"""
    from zigma_amd import optim
    real = optim._device_ok
    optim._device_ok = lambda t: True
    try:
        torch.manual_seed(0)
        base = [torch.randn(4, 4).to(torch.bfloat16), torch.randn(3).to(torch.bfloat16), torch.randn(2, 3, 5).to(torch.bfloat16)]
        mk = lambda: [torch.nn.Parameter(t.clone()) for t in base]
        ps = mk()
        opt = optim.FusedAdamW16(ps, lr=2e-3, weight_decay=0.1, ema=True, seed=77, stream=3)
        assert all(set(opt.state[p]) == {"step", "exp_avg", "exp_avg_sq", "ema"} for p in ps)
        assert all(opt.state[p][k].dtype == torch.float32 and opt.state[p][k].shape == p.shape and opt.state[p][k].data_ptr() % 256 == 0 for p in ps for k in ("exp_avg", "exp_avg_sq", "ema"))
        assert all(torch.equal(e, p.detach().float()) for e, p in zip(opt.ema_tensors(), ps))
        opt._block[0] = 7.0
        fine = 1.0 + 2.0 ** -20                                                    # not a bf16 value
        for i, p in enumerate(ps):
            opt.state[p]["exp_avg"].fill_(fine * (i + 1))
            opt.state[p]["exp_avg_sq"].fill_(fine * 0.5)
            opt.state[p]["ema"].fill_(fine * 3)
        sd = opt.state_dict()
        g = sd["param_groups"][0]
        assert (g["rounding"], g["seed"], g["stream"], g["lr"]) == ("stochastic", 77, 3, 2e-3)
        assert len({sd["state"][k]["step"].data_ptr() for k in sd["state"]}) == 3 and sd["state"][1]["ema"].data_ptr() != opt.state[ps[1]]["ema"].data_ptr()
        opt2 = optim.FusedAdamW16(mk(), ema=True, seed=1)
        opt2.load_state_dict(sd)
        q = opt2.param_groups[0]["params"]
        assert float(opt2.step_count) == 7.0 and opt2.param_groups[0]["seed"] == 77 and opt2.param_groups[0]["stream"] == 3 and opt2.param_groups[0]["weight_decay"] == 0.1
        for a, b in zip(q, ps):
            for k in ("exp_avg", "exp_avg_sq", "ema"):
                assert torch.equal(opt2.state[a][k], opt.state[b][k]) and opt2.state[a][k].dtype == torch.float32
            assert opt2.state[a]["step"].data_ptr() == opt2.step_count.data_ptr()
        # torch.optim.AdamW on the same bf16 model: bf16 moments, no rounding coordinates in its group
        ref = torch.optim.AdamW(mk(), lr=1e-3, weight_decay=0.02)
        for p in ref.param_groups[0]["params"]:
            p.grad = torch.ones_like(p)
        ref.step()
        ref.step()
        assert ref.state[ref.param_groups[0]["params"][0]]["exp_avg"].dtype == torch.bfloat16
        opt3 = optim.FusedAdamW16(mk(), ema=True, seed=5, rounding="nearest")
        ema_before = [e.clone() for e in opt3.ema_tensors()]
        opt3.load_state_dict(ref.state_dict())
        q3 = opt3.param_groups[0]["params"]
        assert float(opt3.step_count) == 2.0 and opt3.param_groups[0]["seed"] == 5 and opt3.param_groups[0]["rounding"] == "nearest" and opt3.param_groups[0]["weight_decay"] == 0.02
        assert all(torch.equal(opt3.state[a]["exp_avg"], ref.state[b]["exp_avg"].float()) and torch.equal(opt3.state[a]["exp_avg_sq"], ref.state[b]["exp_avg_sq"].float())
                   for a, b in zip(q3, ref.param_groups[0]["params"]))
        assert all(torch.equal(a, b) for a, b in zip(ema_before, opt3.ema_tensors()))          # a dict without "ema" leaves it
        ref2 = torch.optim.AdamW(mk())
        ref2.load_state_dict(sd)                                                   # ours -> torch (its cast to bf16 is torch's own)
        assert float(ref2.state[ref2.param_groups[0]["params"][2]]["step"]) == 7.0
        bad = ref.state_dict()
        bad["state"][1]["step"] = torch.tensor(3.0)
        with pytest.raises(ValueError, match="steps disagree"):
            optim.FusedAdamW16(mk()).load_state_dict(bad)
        bad2 = opt.state_dict()
        bad2["param_groups"][0]["rounding"] = "sideways"
        o4 = optim.FusedAdamW16(mk())
        with pytest.raises(ValueError, match="rounding"):
            o4.load_state_dict(bad2)
        assert o4.param_groups[0]["rounding"] == "stochastic"
        bad3 = opt.state_dict()
        bad3["param_groups"][0]["params"] = [0, 1]
        with pytest.raises(ValueError, match="has 2 parameters"):
            optim.FusedAdamW16(mk()).load_state_dict(bad3)
    finally:
        optim._device_ok = real


def test_the_bf16_findings_on_the_cpu():
    """the two findings that motivate the class, as they are: an EMA kept in bf16 with decay 0.9999 does not move (the increment is below half an ulp),
    and torch's AdamW on bf16 weights equal to 1.0 at lr = 1e-4 does not move them"""
    ema, p = torch.ones(16, dtype=torch.bfloat16), torch.full((16,), 1.5, dtype=torch.bfloat16)
    e32 = ema.float()
    for _ in range(1000):
        ema.mul_(0.9999).add_(p, alpha=1 - 0.9999)
        e32.mul_(0.9999).add_(p.float(), alpha=1 - 0.9999)
    assert bool((ema == 1.0).all()) and abs(float(e32[0]) - 1.0475) < 2e-3
    w = torch.nn.Parameter(torch.ones(16, dtype=torch.bfloat16))
    opt = torch.optim.AdamW([w], lr=1e-4, weight_decay=0.0)
    for _ in range(50):
        w.grad = torch.full_like(w, 0.5)
        opt.step()
    assert bool((w == 1.0).all())

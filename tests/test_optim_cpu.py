"""Host side of the fused training-step tail (zigma_amd/optim.py, zigma_optim_* of include/zigma_hip.h): the ctypes mirrors, the registration in the
build, the float64 oracle of tests/optim_cases.py pinned to torch, the error constant K of the GPU sweep, and the optimizer's host logic.  No GPU."""
import copy
import ctypes
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import optim_cases as oc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_optim_structs_match_the_header():
    """sizeof / offsetof of the parameter block, the table row and the state block as gcc sees include/zigma_hip.h (the recipe of test_amp_cpu.py)"""
    from zigma_amd import _lib
    structs = {"zigma_optim_params_t": _lib.OptimParams, "zigma_optim_row_t": _lib.OptimRow, "zigma_optim_state_t": _lib.OptimState}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "zigma_hip.h"', "int main(void){"]
    for cname, st in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in st._fields_:
            lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines.append('printf("abi %d\\n", ZIGMA_ABI_VERSION);')
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
    assert got["zigma_optim_row_t"] == 64 and got["zigma_optim_state_t"] == 32          # what optim.py writes: eight int64 per row, eight words of state
    assert [getattr(_lib.OptimState, f).offset for f in ("step", "skipped", "grad_norm", "grad_mult", "step_size", "bc2_sqrt")] == [0, 4, 8, 12, 16, 20]
    assert got["abi"] == 11


@functools.lru_cache(maxsize=None)
def checked_instantiations():
    """-> (what build.check_no_scratch counts in a compile of csrc/optim_step.hip alone, the norm kernels among them, the update kernels among them)"""
    from zigma_amd import build
    with tempfile.TemporaryDirectory() as d:
        cmd = [build.HIPCC, *build.FLAGS, *build._RES, "-c", os.path.join(build.CSRC, "optim_step.hip"), "-o", os.path.join(d, "optim_step.o")]
        remarks = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    names = [ln.split("Function Name: ")[1].split()[0] for ln in remarks.splitlines() if "remark: Function Name: " in ln]
    return build.check_no_scratch(remarks, "optim_step.hip"), sum("multi_sumsq_kernel" in n for n in names), sum("multi_adamw_kernel" in n for n in names)


def test_symbols_sources_and_kernels_are_registered():
    from zigma_amd import _lib, build
    for name in ("zigma_optim_grad_sumsq", "zigma_optim_prepare", "zigma_optim_adamw"):
        assert name in _lib.EXPORTS
    assert "optim_step.hip" in build.SOURCES and build.SOURCE_FLAGS["optim_step.hip"] == build._RES
    assert "multi_sumsq_kernel" in build.NO_SCRATCH_KERNELS and "multi_adamw_kernel" in build.NO_SCRATCH_KERNELS
    assert checked_instantiations() == (7, 2, 5)          # both tails' kernels are instantiations of those two: 2 norm (fp32, bf16), 5 update (3 fp32, 2 bf16)
    hdr = open(os.path.join(ROOT, "include", "zigma_hip.h")).read()
    assert "#define ZIGMA_ABI_VERSION 11 " in hdr and "(11, no block changed): zigma_optim_* added" in hdr
    assert os.path.exists(os.path.join(ROOT, "zigma_amd", "csrc", "optim_step.hip"))


@pytest.mark.parametrize("wd,max_norm,with_ema", [(0.0, None, False), (0.05, None, True), (0.0, 0.5, True), (0.05, 0.5, False), (0.05, 1e9, True)])
def test_oracle_agrees_with_torch_in_float64(wd, max_norm, with_ema):
    """3 steps of the oracle against float64 torch.optim.AdamW + clip_grad_norm_ (BEFORE the step, in both) + the update_ema formula on CPU tensors:
    <= 1e-12 relative on every parameter, moment and EMA tensor"""
    g = torch.Generator().manual_seed(5)
    shapes = [(7, 5), (33,), (1,), (4, 3, 2)]
    ps = [torch.nn.Parameter(torch.randn(*s, generator=g, dtype=torch.float64)) for s in shapes]
    ema = [p.detach().clone() for p in ps]
    opt = torch.optim.AdamW(ps, lr=oc.HYPER["lr"], betas=(oc.HYPER["beta1"], oc.HYPER["beta2"]), eps=oc.HYPER["eps"], weight_decay=wd)
    mine = [dict(p=p.detach().numpy().copy(), m=np.zeros(s), v=np.zeros(s), ema=e.numpy().copy() if with_ema else None) for p, e, s in zip(ps, ema, shapes)]
    worst = 0.0
    for step in (1, 2, 3):
        grads = [torch.randn(*s, generator=g, dtype=torch.float64) * 10.0 ** (step - 2) for s in shapes]
        for p, gr in zip(ps, grads):
            p.grad = gr.clone()
        mult = 1.0
        if max_norm is not None:
            norm = float(torch.nn.utils.clip_grad_norm_(ps, max_norm))
            assert abs(norm - oc.grad_norm64([x.numpy() for x in grads])) <= 1e-12 * norm
            mult = oc.clip_coef(norm, max_norm)
            assert (mult < 1.0) == (norm > max_norm)
        opt.step()
        if with_ema:
            for e, p in zip(ema, ps):                                          # utils/train_utils.py update_ema: ema = decay * ema + (1 - decay) * p
                e.mul_(oc.HYPER["ema_decay"]).add_(p.detach(), alpha=1 - oc.HYPER["ema_decay"])
        for st, gr, p, e in zip(mine, grads, ps, ema):
            st["p"], st["m"], st["v"], st["ema"] = oc.oracle_step(st["p"], gr.numpy(), st["m"], st["v"], st["ema"], step=step, wd=wd, grad_mult=mult, **oc.HYPER)
            pairs = [(st["p"], p.detach().numpy()), (st["m"], opt.state[p]["exp_avg"].numpy()), (st["v"], opt.state[p]["exp_avg_sq"].numpy())]
            if with_ema:
                pairs.append((st["ema"], e.numpy()))
            for a, b in pairs:
                worst = max(worst, float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))))
    print(f"oracle vs float64 torch (wd {wd}, max_norm {max_norm}, ema {with_ema}): worst relative difference {worst:.3e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("name", list(oc.CONFIGS))
def test_error_constant_of_the_sweep(name):
    """K: the float32 op-by-op evaluation against the oracle on the sweep's own inputs, in units of 2^-24 of each stream's scale, doubled.  The chain
    has about ten roundings, so K <= 16, or the inputs are badly chosen.  Measured here: 10.05 / 9.47 / 11.36 / 8.31."""
    K, worst = oc.error_constant(name)
    print(f"K[{name}] = {K:.3f}; worst multiples per stream {worst}")
    assert 0 < K <= 16
    rows = oc.sweep_values(1 + oc.CONFIGS[name]["step0"], oc.CONFIGS[name]["step0"] == 0)
    allv = {k: np.abs(np.concatenate([r[k] for r in rows])) for k in oc.STREAMS}
    assert all(np.all(np.isfinite(a)) and a.max() < 1e19 for a in allv.values())                       # squares stay finite in fp32
    assert allv["p"].min() >= 0.99e-4 and allv["p"].max() <= 10.01
    norm = oc.grad_norm64([r["g"] for r in rows])
    assert (oc.clip_coef(norm, oc.CONFIGS[name]["max_norm"]) < 1.0) == (oc.CONFIGS[name]["max_norm"] == 1.0)        # clip active where the name says so


def test_sweep_layout_windows_are_disjoint_and_cover_both_paths():
    rows = oc.sweep_values(1, True)
    bufs, shadow_len, wins = oc.sweep_layout(rows)
    assert len(rows) >= 150 and sorted(set(len(r["p"]) for r in rows)) == sorted(oc.SIZES)
    for k in oc.STREAMS + ("shadow",):
        spans = sorted((w[k], w[k] + w["n"]) for w in wins if w[k] is not None)
        assert all(a[1] < b[0] for a, b in zip(spans, spans[1:]) if a[1] > a[0])                           # at least one untouched element between windows
        assert spans[-1][1] < (shadow_len if k == "shadow" else bufs[k].size)
    q = lambda w, k: w[k] is None or w[k] % (8 if k == "shadow" else 4) == 0
    wide = [w for w in wins if w["n"] >= 8 and all(q(w, k) for k in oc.STREAMS + ("shadow",))]
    assert len(wide) >= 24 and len(wins) - len(wide) >= 120
    assert any(w["ema"] is None for w in wide) and any(w["shadow"] is None for w in wide) and any(w["ema"] is not None and w["shadow"] is not None for w in wide)
    assert sum(w["ema"] is None for w in wins) >= 20 and sum(w["shadow"] is None for w in wins) >= 20
    assert int(np.isnan(bufs["p"]).sum()) == bufs["p"].size - sum(w["n"] for w in wins)


# ---- host logic of the optimizer ------------------------------------------------------------------------------------------------------------------
def test_arena_layout_for_four_byte_slots():
    from zigma_amd import amp, optim
    numels = [72 * 128, 3, 0, 1, 257, 64, 65]
    offsets, total = amp.arena_layout(numels, itemsize=4)
    assert all(o % 256 == 0 for o in offsets) and total % 256 == 0
    spans = sorted((o, o + 4 * n) for o, n in zip(offsets, numels) if n)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= total
    like = [torch.empty(72, 128), torch.empty(3), torch.empty(0), torch.empty(1), torch.empty(257), torch.empty(8, 8), torch.empty(5, 13)]
    arena, views = optim.arena_views(like, "cpu")
    assert all(v.dtype == torch.float32 and v.shape == t.shape and v.is_contiguous() and v.data_ptr() % 256 == 0 for v, t in zip(views, like))
    assert all(bool((v == 0).all()) for v in views)
    lo, hi = arena.data_ptr(), arena.data_ptr() + arena.numel()
    assert all(lo <= v.data_ptr() and v.data_ptr() + 4 * v.numel() <= hi for v in views if v.numel())
    views[4].fill_(1.0)
    assert float(views[3].sum()) == 0.0 and float(views[5].sum()) == 0.0


class _Standin:
    def __init__(self, ptr, n):
        self.ptr, self.n = ptr, n

    def data_ptr(self):
        return self.ptr

    def numel(self):
        return self.n


def test_tables_are_rebuilt_only_when_pointers_move():
    from zigma_amd import optim
    ns = [10, 5000, 0, 8192]
    mk = lambda base: [_Standin(base + 0x10000 * i, n) for i, n in enumerate(ns)]
    ps, gs, ms, vs, es = mk(0x1000000), mk(0x2000000), mk(0x3000000), mk(0x4000000), mk(0x5000000)
    sh = [_Standin(0x6000000, 10), None, None, _Standin(0x6010000, 8192)]
    rows = optim.step_rows(ps, gs, ms, vs, es, sh)
    assert rows[1] == (0x1010000, 0x2010000, 0x3010000, 0x4010000, 0x5010000, 0, 5000, 0) and rows[0][5] == 0x6000000 and len(rows) == 4
    T = optim.StepTables(chunk=4096)
    assert T.update(rows, "cpu") and T.builds == 1
    assert T.table.dtype == torch.int64 and T.table.shape == (4, 8) and T.table.tolist() == [list(r) for r in rows]
    assert T.cmap.tolist() == [[0, 0], [1, 0], [1, 4096], [3, 0], [3, 4096]] and T.n_chunks == 5 and T.partials.numel() == 5
    table, cmap = T.table, T.cmap
    for _ in range(3):                                                             # the same pointers: nothing is rebuilt
        assert not T.update(optim.step_rows(ps, gs, ms, vs, es, sh), "cpu")
    assert T.table is table and T.cmap is cmap and T.builds == 1
    gs[1] = _Standin(0x7000000, 5000)                                              # a gradient moved (zero_grad(set_to_none=True)): new table, same map
    assert T.update(optim.step_rows(ps, gs, ms, vs, es, sh), "cpu") and T.builds == 2
    assert T.table is not table and T.cmap is cmap and T.table[1, 1].item() == 0x7000000
    gs[3] = None                                                                   # a parameter without a gradient leaves the table, as torch skips it
    rows = optim.step_rows(ps, gs, ms, vs, es, sh)
    assert len(rows) == 3 and T.update(rows, "cpu") and T.n_chunks == 3 and T.cmap.tolist() == [[0, 0], [1, 0], [1, 4096]]
    assert optim.step_rows(ps, gs, ms, vs, None, None)[0][4:6] == (0, 0)
    assert T.update([], "cpu") and T.n_chunks == 0


def test_constructor_refusals():
    """no fallback: whatever the kernel does not take raises at construction"""
    from zigma_amd import optim
    F = optim.FusedAdamW
    cpu = [torch.nn.Parameter(torch.randn(4, 4))]
    with pytest.raises(ValueError, match="needs a GPU"):
        F(cpu)
    ok = lambda t: True
    real = optim._device_ok
    optim._device_ok = ok                                                          # from here on the CPU tensors stand in for device tensors
    try:
        F(cpu)
        for bad, what in ((torch.bfloat16, "float32 only"), (torch.float16, "float32 only"), (torch.float64, "float32 only")):
            with pytest.raises(ValueError, match=what):
                F([torch.nn.Parameter(torch.randn(4, 4).to(bad))])
        with pytest.raises(ValueError, match="not contiguous"):
            F([torch.nn.Parameter(torch.randn(4, 6).t())])
        with pytest.raises(ValueError, match="sparse"):
            F([torch.randn(4, 4).to_sparse().requires_grad_(True)])
        with pytest.raises(ValueError, match="one parameter group"):
            F([dict(params=[torch.nn.Parameter(torch.randn(3))]), dict(params=[torch.nn.Parameter(torch.randn(3))], lr=1e-2)])
        opt = F(cpu)
        with pytest.raises(ValueError, match="one parameter group"):
            opt.add_param_group(dict(params=[torch.nn.Parameter(torch.randn(3))]))
        for kw in (dict(amsgrad=True), dict(maximize=True)):
            with pytest.raises(ValueError, match="amsgrad and maximize"):
                F(cpu, **kw)
        for kw in (dict(lr=-1.0), dict(lr=float("nan")), dict(lr=float("inf")), dict(lr=torch.tensor(1e-3)), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)),
                   dict(eps=0.0), dict(eps=-1e-8), dict(weight_decay=-0.1), dict(max_grad_norm=0.0), dict(max_grad_norm=float("inf")), dict(ema_decay=1.5)):
            with pytest.raises(ValueError):
                F(cpu, **kw)
        p2 = [torch.nn.Parameter(torch.randn(4, 4)), torch.nn.Parameter(torch.randn(3))]
        with pytest.raises(ValueError, match="1 ema tensors for 2"):
            F(p2, ema_params=[torch.randn(4, 4)])
        with pytest.raises(ValueError, match="has shape"):
            F(p2, ema_params=[torch.randn(4, 4), torch.randn(4)])
        with pytest.raises(ValueError, match="float32 only"):
            F(p2, ema_params=[torch.randn(4, 4), torch.randn(3).double()])
        with pytest.raises(ValueError, match="IS parameter"):
            F(p2, ema_params=[p.detach() for p in p2])
        with pytest.raises(ValueError, match="shadows is a module"):
            F(p2, shadows=torch.randn(3))
        with pytest.raises(ValueError, match="shadows is a module"):
            F(p2, shadows=(torch.nn.Linear(2, 2), torch.float32))
        lin = torch.nn.Linear(4, 3)
        o = F(lin.parameters(), ema_params=copy.deepcopy(lin))                     # a module's parameters() as the EMA set
        assert [e.shape for e in o._ema] == [p.shape for p in lin.parameters()]
        assert isinstance(o, torch.optim.Optimizer) and F._step_supports_amp_scaling is True and not hasattr(o, "grad_scale")
    finally:
        optim._device_ok = real


def test_state_dict_round_trip_of_names_and_shapes():
    """state[p] carries torch's key names over views of two arenas and ONE step; state_dict() has torch.optim.AdamW's layout (copies, a step per
    parameter) and loads into it and back; per-parameter steps that disagree are refused"""
    from zigma_amd import optim
    real = optim._device_ok
    optim._device_ok = lambda t: True
    try:
        mk = lambda: [torch.nn.Parameter(torch.randn(4, 4)), torch.nn.Parameter(torch.randn(3)), torch.nn.Parameter(torch.randn(2, 3, 5))]
        ps = mk()
        opt = optim.FusedAdamW(ps, lr=2e-3, weight_decay=0.1)
        assert all(set(opt.state[p]) == {"step", "exp_avg", "exp_avg_sq"} and opt.state[p]["exp_avg"].shape == p.shape for p in ps)
        assert all(opt.state[p]["step"].data_ptr() == opt.step_count.data_ptr() and opt.state[p]["exp_avg"].data_ptr() % 256 == 0 for p in ps)
        opt._block[0] = 7.0
        for i, p in enumerate(ps):
            opt.state[p]["exp_avg"].fill_(i + 1.0)
            opt.state[p]["exp_avg_sq"].fill_(0.5 * (i + 1))
        sd = opt.state_dict()
        ref = torch.optim.AdamW(mk(), lr=1e-3)
        for p in ref.param_groups[0]["params"]:
            p.grad = torch.zeros_like(p)
        ref.step()
        sd_ref = ref.state_dict()
        assert set(sd) == set(sd_ref) and set(sd["state"]) == set(sd_ref["state"]) == {0, 1, 2}
        assert set(sd_ref["param_groups"][0]) <= set(sd["param_groups"][0])
        for k in sd["state"]:
            assert set(sd["state"][k]) == set(sd_ref["state"][k])
            assert all(sd["state"][k][n].shape == sd_ref["state"][k][n].shape and sd["state"][k][n].dtype == torch.float32 for n in sd["state"][k])
        assert len({sd["state"][k]["step"].data_ptr() for k in sd["state"]}) == 3 and sd["state"][1]["exp_avg"].data_ptr() != opt.state[ps[1]]["exp_avg"].data_ptr()
        ref.load_state_dict(sd)                                                    # ours -> torch
        q = ref.param_groups[0]["params"]
        assert all(float(ref.state[p]["step"]) == 7.0 for p in q) and float(ref.state[q[2]]["exp_avg"][0, 0, 0]) == 3.0 and ref.param_groups[0]["lr"] == 2e-3
        ref.param_groups[0].update(fused=None, foreach=False)                      # (a CPU step in this test)
        for p in q:
            p.grad = torch.ones_like(p)
        ref.step()
        opt2 = optim.FusedAdamW(mk())
        arena_ptr = opt2.state[opt2.param_groups[0]["params"][0]]["exp_avg"].data_ptr()
        opt2.load_state_dict(ref.state_dict())                                     # torch -> ours: into the arenas, one step
        q2 = opt2.param_groups[0]["params"]
        assert float(opt2.step_count) == 8.0 and opt2.state[q2[0]]["exp_avg"].data_ptr() == arena_ptr
        assert all(torch.equal(opt2.state[a]["exp_avg"], ref.state[b]["exp_avg"]) and torch.equal(opt2.state[a]["exp_avg_sq"], ref.state[b]["exp_avg_sq"])
                   for a, b in zip(q2, q))
        assert all(opt2.state[a]["step"].data_ptr() == opt2.step_count.data_ptr() for a in q2) and opt2.param_groups[0]["weight_decay"] == 0.1
        bad = ref.state_dict()
        bad["state"][1]["step"] = torch.tensor(3.0)
        with pytest.raises(ValueError, match="steps disagree"):
            optim.FusedAdamW(mk()).load_state_dict(bad)
        bad2 = ref.state_dict()
        bad2["param_groups"][0]["amsgrad"] = True
        with pytest.raises(ValueError, match="amsgrad"):
            optim.FusedAdamW(mk()).load_state_dict(bad2)
    finally:
        optim._device_ok = real


def test_freshness_record_of_the_shadow_arena():
    """amp._Group.fresh / written_by_step on CPU stand-in parameters: a fresh arena marked inside a step is fresh again once the optimizer-step hook has
    counted that step, and stale after any other optimizer's step or a write that moves `_version`"""
    from zigma_amd import amp
    ps = [torch.nn.Parameter(torch.randn(8, 8)), torch.nn.Parameter(torch.randn(5))]
    grp = amp._Group(ps)
    d = torch.bfloat16
    assert not grp.fresh(d)
    a = grp._arena(d)
    assert not grp.fresh(d)
    a["keys"] = [(amp.step_count(), p._version, p.data_ptr()) for p in ps]          # (what refresh() records after its launch)
    assert grp.fresh(d)
    grp.written_by_step(d)
    assert not grp.fresh(d)                                                        # the step has not been counted yet
    other = torch.nn.Parameter(torch.randn(2))
    other.grad = torch.zeros(2)
    torch.optim.SGD([other], lr=0.1).step()                                        # the hook counts it
    assert grp.fresh(d)
    torch.optim.SGD([other], lr=0.1).step()
    assert not grp.fresh(d)
    a["keys"] = [(amp.step_count(), p._version, p.data_ptr()) for p in ps]
    with torch.no_grad():
        ps[1].add_(1.0)
    assert not grp.fresh(d)

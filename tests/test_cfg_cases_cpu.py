"""CPU checks of the guided final layer's case table (tests/cfg_cases.py), of the new parameter block and of the constructor surface that
goes with it.  The kernel itself runs in tests/test_gpu_cfg.py.

`python tests/test_cfg_cases_cpu.py` prints, per case, what the rounded reference, the fp32 model and the composed path need.
"""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:          # (run as a script: the oracle package lives at the repository root)
    sys.path.insert(0, ROOT)

import cfg_cases as cc  # noqa: E402

CASES = cc.cfg_cases()
SHORT = [c for c in CASES if c["rows"] < 65536]
HIGH = [c for c in CASES if min(c["scales"]) >= 4.0 and c["out"] == "bf16"]


def _ids(cases):
    return [c["id"] for c in cases]


def test_table_coverage():
    ids = _ids(CASES)
    assert len(set(ids)) == len(ids)
    got = lambda k: {c[k] for c in SHORT}
    assert got("cols") == set(cc.CFG_COLS) and {c["np"] for c in CASES} == {5, 8, 16}
    assert {(c["patch"], c["chans"]) for c in SHORT} == set(cc.CFG_PC) and max(c["n_out"] for c in CASES) == 16
    assert got("side") == set(cc.CFG_SIDE) and got("frames") == set(cc.CFG_FRAMES) and got("batch") == set(cc.CFG_BATCH)
    for key, values in (("cols", cc.CFG_COLS), ("patch", (1, 2, 4)), ("frames", cc.CFG_FRAMES), ("batch", cc.CFG_BATCH)):
        for v in values:              # both output types and both bias forms at every column count, patch, frame form and batch
            sub = [c for c in SHORT if c[key] == v]
            assert {c["out"] for c in sub} == {"f32", "bf16"}, (key, v)
            assert {c["bias"] for c in sub} == {True, False}, (key, v)
    assert {s for c in CASES for s in c["scales"]} == set(cc.CFG_SCALES)
    assert all(len(set(c["scales"])) > 1 for c in CASES if c["batch"] > 1), "the samples of one call share a scale"
    assert all(len(c["scales"]) == c["batch"] for c in CASES)
    assert len(HIGH) >= 15 and {c["np"] for c in HIGH} == {5, 8, 16}
    long = [c for c in CASES if c["rows"] > 65536]          # the second trip of the row loop, in both output types
    assert {c["out"] for c in long} == {"f32", "bf16"} and all(c["cols"] == 64 and c["side"] == 257 and c["batch"] == 1 for c in long)
    assert len(cc.REFUSALS) == len({w for w, _ in cc.REFUSALS})


def test_window_is_non_compact():
    for c in SHORT:
        shape, index = cc.out_window(c)
        buf = torch.empty(shape)
        win = buf[index]
        ref = torch.empty(win.shape)
        assert win.stride(-1) == 1 and all(win.stride(d) > ref.stride(d) for d in range(win.dim() - 1) if win.shape[d] > 1 or d >= win.dim() - 3), c["id"]


def test_unpatchify_is_the_models():
    """cfg_cases.unpatchify against ZigMa.unpatchify / unpatchify_video themselves"""
    from zigma_amd.model_zigma import ZigMa
    for c in (c for c in SHORT if c["side"] > 1):
        class M:
            out_channels = c["chans"]
            x_embedder = type("E", (), dict(patch_size=(c["patch"],) * 2))
        rows = np.arange(c["rows"] * c["n_out"], dtype=np.float64).reshape(c["rows"], c["n_out"])
        t = torch.from_numpy(rows).view(c["batch"], c["rps"], c["n_out"])
        want = ZigMa.unpatchify_video(M, t, c["frames"]) if c["frames"] else ZigMa.unpatchify(M, t)
        assert np.array_equal(cc.unpatchify(c, rows), want.numpy()), c["id"]


@pytest.mark.parametrize("c", CASES, ids=_ids(CASES))
def test_fp32_model_passes(c):
    """the rounded float64 reference and the fp32 step-by-step model (LayerNorm rows first, then the output against float64 on the model's own
    rows) stay inside the limits the kernel is held to"""
    inp = cc.cfg_inputs(c)
    ref, bound = cc.cfg_reference(c, inp), cc.IO_BOUND[c["out"]]
    assert np.isfinite(ref["out"]).all() and ref["out"].shape == cc.out_window(c)[0][:-3] + (c["chans"],) + (c["side"] * c["patch"],) * 2
    rounded = cc.need(cc.round_to(ref["out"], c["out"]), ref["out"], ref["terms"])
    assert rounded <= bound, (c["id"], "the rounded reference misses the bound: move the seed (SEED_MOVED)", rounded)
    y, out = cc.cfg_model(c, inp)
    assert cc.flipped_share(y, ref["y"], "bf16") <= cc.DELTA_FLIPS_MODEL, c["id"]
    assert cc.elementwise_worst(y, ref["y"], cc.IO_BOUND["bf16"]) <= cc.ROW_GUARD, c["id"]
    own = cc.cfg_reference(c, inp, y_own=y)
    d = cc.need(out, own["out"], own["terms"])
    assert d <= bound, (c["id"], d, bound)


@pytest.mark.parametrize("c", HIGH, ids=_ids(HIGH))
def test_composed_path_leaves_the_bound(c):
    """the sweep discriminates: with every scale >= 4 the composition of two bf16-rounded velocities misses the bound the kernel is held to"""
    inp = cc.cfg_inputs(c)
    ref = cc.cfg_reference(c, inp)
    d = cc.need(cc.cfg_composed(c, inp), ref["out"], ref["terms"])
    assert d > cc.IO_BOUND["bf16"], (c["id"], d)


def test_cfg_struct_matches_the_header():
    """sizeof / offsetof of zigma_final_layer_cfg_params_t as gcc sees include/zigma_hip.h equal the ctypes mirror"""
    from zigma_amd import _lib
    cname, st = "zigma_final_layer_cfg_params_t", _lib.FinalLayerCfgParams
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
    assert "zigma_final_layer_cfg_fwd" in _lib.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "zigma_hip.h")).read()
    assert "(11, no block changed): zigma_optim_* added" in hdr and "#define ZIGMA_ABI_VERSION 11 " in hdr


def test_constructor_surface():
    """class_dropout_prob: the default leaves state_dict as it was, 0.1 adds the null row; forward_guided refuses what it cannot guide"""
    from zigma_amd.model_zigma import ZigMa
    kw = dict(in_channels=4, embed_dim=32, depth=2, img_dim=8, device="cpu", num_classes=4)
    torch.manual_seed(0)
    plain = ZigMa(**kw)
    torch.manual_seed(0)
    same = ZigMa(class_dropout_prob=0.0, **kw)
    torch.manual_seed(0)
    null = ZigMa(class_dropout_prob=0.1, **kw)
    sd, sd0, sd1 = plain.state_dict(), same.state_dict(), null.state_dict()
    assert list(sd) == list(sd0) == list(sd1)
    assert all(torch.equal(sd[k], sd0[k]) for k in sd)
    assert sd["y_embedder.embedding_table.weight"].shape == (4, 32) and sd1["y_embedder.embedding_table.weight"].shape == (5, 32)
    assert all(sd[k].shape == sd1[k].shape for k in sd if k != "y_embedder.embedding_table.weight")
    assert null.y_embedder.dropout_prob == 0.1
    dropped = null.y_embedder.token_drop(torch.tensor([0, 1, 2, 3]), force_drop_ids=torch.tensor([1, 0, 1, 0]))
    assert dropped.tolist() == [4, 1, 4, 3]                  # training drops labels to the null row
    x, t, y = torch.zeros(2, 4, 8, 8), torch.zeros(2), torch.tensor([1, 2])
    with pytest.raises(ValueError, match="no null class"):
        plain.forward_guided(x, t, y, 4.0)
    with pytest.raises(ValueError, match="nothing to guide"):
        ZigMa(in_channels=4, embed_dim=32, depth=2, img_dim=8, device="cpu").forward_guided(x, t, None, 4.0)
    text = ZigMa(in_channels=4, embed_dim=32, depth=2, img_dim=8, device="cpu", has_text=True, d_context=16, n_context_token=3)
    with pytest.raises(ValueError, match="y_null"):
        text.forward_guided(x, t, torch.zeros(2, 3, 16), 4.0)
    with pytest.raises(NotImplementedError):                # the reference's stub stays a stub
        null.forward_with_cfg(x, t, y, 4.0)


def test_guided_wrapper_refuses_cpu_tensors():
    from zigma_amd import embed
    x, w = torch.zeros(2, 4, 64, dtype=torch.bfloat16), torch.zeros(3, 64, dtype=torch.bfloat16)
    geom = dict(patch=1, chans=3, grid=2, frames=0, out_dtype=torch.float32)
    assert not embed.final_layer_guided_eligible(x, w, None, torch.ones(1), **geom)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        embed.final_layer_guided(x, w, None, 1e-6, torch.ones(1), **geom)


# ---------------------------------------------------------------------------------------------------
# the GPU file's sweep and refusal checks on the CPU, served at the C ABI by a float64 torch restatement of the entry point
# ---------------------------------------------------------------------------------------------------
def _standin_cfg_fwd(P):
    import kernel_standins as ks
    refuse = ks._refuse
    if P.rows < 0 or P.cols < 8 or P.n_out < 1:
        refuse(-2)
    if P.flags != 0:
        refuse(-6)
    if P.dtype != 2 or P.out_dtype not in (0, 2):
        refuse(-3)
    if P.cols % 8 or P.cols > 2048 or P.n_out > 16 or min(P.rows_per_sample, P.tokens_per_frame, P.grid_w, P.patch, P.chans) < 1:
        refuse(-2)
    if P.patch * P.patch * P.chans != P.n_out or P.rows % P.rows_per_sample or P.rows_per_sample % P.tokens_per_frame or P.tokens_per_frame % P.grid_w:
        refuse(-2)
    if P.rows == 0:
        return ks.LAST_KERNEL[0]
    if not (P.x_cond and P.x_uncond and P.weight and P.scale and P.out):
        refuse(-1)
    if P.x_cond % 16 or P.x_uncond % 16 or P.x_row_stride % 8 or P.weight % 16 or (P.y_out or 0) % 16:
        refuse(-4)
    bf, F = torch.bfloat16, torch.nn.functional
    rows, cols, B = P.rows, P.cols, P.rows // P.rows_per_sample
    x = torch.cat([ks._view(q, (rows, cols), (P.x_row_stride, 1), bf) for q in (P.x_cond, P.x_uncond)]).double()
    w, bias = ks._view(P.weight, (P.n_out, cols), (cols, 1), bf).double(), ks._view(P.bias, (P.n_out,), (1,), bf)
    y = ks._r(F.layer_norm(x, (cols,), eps=float(P.eps)), bf)
    if P.y_out:
        ks._view(P.y_out, (2 * rows, cols), (cols, 1), bf).copy_(y.float().to(bf))
    v = F.linear(y, w, None if bias is None else bias.double())
    s = ks._view(P.scale, (B,), (1,), torch.float32).double().repeat_interleave(P.rows_per_sample)[:, None]
    r = v[rows:] + s * (v[:rows] - v[rows:])
    T, g, p, ch = P.rows_per_sample // P.tokens_per_frame, P.grid_w, P.patch, P.chans
    gh = P.tokens_per_frame // g
    odt = torch.float32 if P.out_dtype == 0 else bf
    out = ks._view(P.out, (B, T, ch, gh * p, g * p), (P.out_sample_stride, P.out_frame_stride, P.out_chan_stride, P.out_row_stride, 1), odt)
    out.copy_(r.view(B, T, gh, g, p, p, ch).permute(0, 1, 6, 2, 4, 3, 5).reshape(B, T, ch, gh * p, g * p).float().to(odt))
    return "final_layer_cfg"


@pytest.fixture
def gpu_file(monkeypatch):
    import kernel_standins as ks
    import test_gpu_cfg as gf
    ks.install_lib_call(monkeypatch)
    from zigma_amd import _lib
    served = _lib.call

    def call(fn_name, params, device):
        if fn_name != "zigma_final_layer_cfg_fwd":
            return served(fn_name, params, device)
        ks.LAST_KERNEL[0] = _standin_cfg_fwd(params)
    monkeypatch.setattr(_lib, "call", call)
    monkeypatch.setattr(gf, "DEV", "cpu")
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    return gf


@pytest.mark.parametrize("c", SHORT + CASES[-1:], ids=_ids(SHORT + CASES[-1:]))
def test_gpu_sweep_checks_pass_on_the_stand_in(c, gpu_file, capsys):
    gpu_file.test_cfg_sweep(c)
    assert f"cfg-sweep {c['id']}: " in capsys.readouterr().out


@pytest.mark.parametrize("what,status", [r for r in cc.REFUSALS if r[0] != "null-block"], ids=[w for w, _ in cc.REFUSALS if w != "null-block"])
def test_gpu_refusal_checks_pass_on_the_stand_in(what, status, gpu_file):
    gpu_file.test_cfg_refusals(what, status)
    gpu_file.test_cfg_empty_call_touches_nothing()


def test_gpu_sweep_checks_notice_a_wrong_kernel(gpu_file, monkeypatch):
    """a kernel that forgets a sample's own scale, or writes one element outside the window, fails the sweep"""
    import kernel_standins as ks
    c = next(c for c in SHORT if c["batch"] > 1 and c["out"] == "bf16")
    real = ks._view

    def first_scale_only(ptr, shape, strides, dtype):
        v = real(ptr, shape, strides, dtype)
        return v[:1].expand(shape) if dtype == torch.float32 and len(shape) == 1 else v
    monkeypatch.setattr(ks, "_view", first_scale_only)
    with pytest.raises(AssertionError):
        gpu_file.test_cfg_sweep(c)
    monkeypatch.setattr(ks, "_view", real)

    def spill(ptr, shape, strides, dtype):
        v = real(ptr, shape, strides, dtype)
        if len(shape) == 5:
            real(ptr, (shape[-1] + 1,), (1,), dtype)[-1] = 1.0
        return v
    monkeypatch.setattr(ks, "_view", spill)
    with pytest.raises(AssertionError, match="outside"):
        gpu_file.test_cfg_sweep(c)


if __name__ == "__main__":
    for c in CASES:
        inp = cc.cfg_inputs(c)
        ref = cc.cfg_reference(c, inp)
        y, out = cc.cfg_model(c, inp)
        own = cc.cfg_reference(c, inp, y_own=y)
        print(f"{c['id']}: rounded reference {cc.need(cc.round_to(ref['out'], c['out']), ref['out'], ref['terms']):.2e}, fp32 model "
              f"{cc.need(out, own['out'], own['terms']):.2e}, composed {cc.need(cc.cfg_composed(c, inp), ref['out'], ref['terms']):.2e} "
              f"(bound {cc.IO_BOUND[c['out']]:.1e})")
    sys.exit(0)

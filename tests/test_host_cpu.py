"""CPU tests of the host side: C-ABI surface, struct layout, scan-order tables, module/state_dict
compatibility, transport logic, and the no-fallback rule.  No GPU, no compute calls into the library."""
import ast
import ctypes
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden, rel_err
from oracle import zigma_oracle as zo


@pytest.fixture(scope="module")
def libpath():
    from zigma_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.LIB_PATH


def test_cabi_exports_every_declared_symbol(libpath):
    hdr = open(os.path.join(ROOT, "include", "zigma_hip.h")).read()
    declared = set(re.findall(r"\b(zigma_[a-z0-9_]+)\s*\(", hdr))
    assert {"zigma_selective_scan_fwd", "zigma_causal_conv1d_fwd", "zigma_add_norm_fwd"} <= declared
    L = ctypes.CDLL(libpath)
    for name in declared:
        assert hasattr(L, name), name
    L.zigma_abi_version.restype = ctypes.c_int
    L.zigma_strerror.restype = ctypes.c_char_p
    assert L.zigma_abi_version() == 11
    assert L.zigma_strerror(-2) == b"size out of the supported range"
    from zigma_amd import _lib
    assert set(_lib.EXPORTS) <= declared


def test_ctypes_structs_match_the_header():
    """sizeof/offsetof of every field, as gcc sees include/zigma_hip.h, equal the ctypes mirror."""
    from zigma_amd import _lib
    structs = {"zigma_scan_params_t": _lib.ScanParams, "zigma_conv_params_t": _lib.ConvParams,
               "zigma_norm_params_t": _lib.NormParams, "zigma_dtproj_params_t": _lib.DtProjParams,
               "zigma_scan_bwd_params_t": _lib.ScanBwdParams, "zigma_conv_bwd_params_t": _lib.ConvBwdParams,
               "zigma_norm_bwd_params_t": _lib.NormBwdParams, "zigma_xattn_params_t": _lib.XAttnParams, "zigma_xproj_params_t": _lib.XProjParams,
               "zigma_linear_params_t": _lib.LinearParams, "zigma_conv_xproj_params_t": _lib.ConvXProjParams,
               "zigma_glue_bwd_params_t": _lib.GlueBwdParams, "zigma_xattn_bwd_params_t": _lib.XAttnBwdParams, "zigma_patch_embed_params_t": _lib.PatchEmbedParams,
               "zigma_timestep_embed_params_t": _lib.TimestepEmbedParams, "zigma_final_layer_params_t": _lib.FinalLayerParams,
               "zigma_skinny_params_t": _lib.SkinnyParams, "zigma_calib_params_t": _lib.CalibParams}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "zigma_hip.h"', "int main(void){"]
    for cname, st in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f, _ in st._fields_:
            lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "a.c"), os.path.join(d, "a.out")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    got = dict(l.split() for l in out.strip().splitlines())
    for cname, st in structs.items():
        assert int(got[cname]) == ctypes.sizeof(st), cname
        for f, _ in st._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(st, f).offset, (cname, f)


def test_flag_constants_match_the_header():
    """the Python mirrors of the header's flag / kernel-id constants (a drifted copy would select another kernel silently)"""
    import re
    from zigma_amd import _lib
    import zigma_amd.linear as zl
    hdr = open(os.path.join(ROOT, "include", "zigma_hip.h")).read()
    defs = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"#define\s+(ZIGMA_\w+)\s+(0x[0-9a-fA-F]+|\d+)\b", hdr)}
    assert defs["ZIGMA_LINEAR_WS"] == zl.LINEAR_WS_FLAG and defs["ZIGMA_LINEAR_SM"] == zl.LINEAR_SM_FLAG
    assert defs["ZIGMA_SCAN_KERNEL_TOK2"] == _lib.SCAN_KERNEL_TOK2
    assert defs["ZIGMA_SCAN_Z_PREACTIVATED"] == _lib.SCAN_Z_PREACTIVATED and defs["ZIGMA_SCAN_PROBE_V1"] == _lib.SCAN_PROBE_V1
    assert defs["ZIGMA_SCAN_PROBE_PRIO_SHIFT"] == _lib.SCAN_PROBE_PRIO_SHIFT and defs["ZIGMA_SCAN_PROBE_R5_SHIFT"] == _lib.SCAN_PROBE_R5_SHIFT
    assert defs["ZIGMA_ABI_VERSION"] == 11


def test_knobs_env_override():
    """ZIGMA_KNOBS: the one environment override of the module-level knobs (A/B tools); unknown names raise"""
    import subprocess
    import sys
    code = ("import zigma_amd.mamba_simple as m, zigma_amd.model_zigma as z, zigma_amd.routing as r; "
            "print(m.GATE_IN_IN_PROJ, z.FUSE_OUT_PROJ_ADD, r.POLICY, r.route('in_proj', 65536, 2560, 640).row)")
    env = dict(os.environ, ZIGMA_KNOBS="mamba_simple.GATE_IN_IN_PROJ=True, model_zigma.FUSE_OUT_PROJ_ADD=False,routing.DISABLED=in_proj.ws+to_q.sm")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.split() == ["True", "False", "auto", "in_proj.halves"], (out.stdout, out.stderr[-400:])
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, ZIGMA_KNOBS=""), capture_output=True, text=True)
    assert out.stdout.split() == ["False", "True", "auto", "in_proj.ws"], out.stdout
    bad = subprocess.run([sys.executable, "-c", "import zigma_amd.mamba_simple"], cwd=ROOT, env=dict(os.environ, ZIGMA_KNOBS="mamba_simple.NO_SUCH=1"),
                         capture_output=True, text=True)
    assert bad.returncode != 0 and "no knob" in bad.stderr
    bad = subprocess.run([sys.executable, "-c", "import zigma_amd.model_zigma"], cwd=ROOT, env=dict(os.environ, ZIGMA_KNOBS="linear.X=1"),
                         capture_output=True, text=True)
    assert bad.returncode != 0 and "names no module with knobs" in bad.stderr


def test_no_routing_environment_switches():
    """the product path reads no per-feature environment variable for its routing: ZIGMA_KNOBS (tools), ZIGMA_AMD_LIB (A/B
    builds) and HIPCC (the build) are the only ones besides torch.distributed's rendezvous variables"""
    allowed = {"ZIGMA_KNOBS", "ZIGMA_AMD_LIB", "HIPCC", "RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "L4W_STORE_NT", "L4W_RES_AHEAD"}
    seen = set()
    for dirpath, _, files in os.walk(os.path.join(ROOT, "zigma_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                seen |= set(re.findall(r"environ(?:\.get|\.setdefault)?\(?\[?\s*[\"']([A-Z0-9_]+)[\"']", src))
    assert seen <= allowed, seen - allowed


# The cells of the sweep below that run on the LIBRARY (F.linear = hipBLASLt), reviewed one by one.  Everything else of
# E x tokens x role runs on an own kernel.  Why each group is here:
#   in_proj, every E, 4096 tokens           below 8192 tokens the library ties or beats every own form (tools/linear_ws_probe.py: a tie at 4096)
#   out_proj, E = 512, 16 384 tokens        k = 1024 is not a 128-feature-panel width and 64 x 2 = 128 tiles is below the 4-wave kernel's floor (E = 1024: 256 tiles, own)
#   in_proj, E = 768, >= 65 536 tokens      measured: the library is the faster kernel there (routing.py row in_proj.library_k768)
ROUTING_LIBRARY_CELLS = {
    ("in_proj", 512, 4096), ("in_proj", 640, 4096), ("in_proj", 768, 4096), ("in_proj", 1024, 4096),
    ("out_proj", 512, 16384),
    ("in_proj", 768, 65536), ("in_proj", 768, 131072),      # E = 768 from 65 536 tokens on: hipBLASLt is 3 % faster inside config 3y's forward than the 4-wave kernel (round 6 A/B)
}


def test_routing_table(libpath):
    """zigma_amd/routing.py: ONE table decides which kernel serves which projection.  Sweep E x tokens x role: (i) a row is chosen, deterministically,
    and its kernel's shape limits hold; (ii) the cells that fall to the library are exactly the reviewed list above; (iii) the shipped shapes land on the
    rows the profiles were taken with; (iv) the knobs (POLICY, DISABLED) do what they say.  (The limits are the built library's plan: routing.serves.)"""
    import zigma_amd.routing as zr
    lib_cells = set()
    for E in (512, 640, 768, 1024):
        shapes = {"in_proj": (4 * E, E), "out_proj": (E, 2 * E), "to_q": (512, E), "to_out": (E, 512)}
        for tokens in (4096, 8192, 16384, 32768, 65536, 131072):
            for role, (n, k) in shapes.items():
                r = zr.route(role, tokens, n, k)
                assert r == zr.route(role, tokens, n, k) and r.kernel in zr.KERNELS and r.row.startswith(role + ".")
                assert zr.serves(r.kernel, tokens, n, k), (role, E, tokens, r)
                if r.kernel == "library":
                    lib_cells.add((role, E, tokens))
    assert lib_cells == ROUTING_LIBRARY_CELLS, (lib_cells - ROUTING_LIBRARY_CELLS, ROUTING_LIBRARY_CELLS - lib_cells)
    # (iii) the README model at B = 64 and the shipped yamls' E = 768 at B = 64 / 8
    assert zr.route("in_proj", 65536, 2560, 640).row == "in_proj.ws" and zr.route("in_proj", 65536, 3072, 768).row == "in_proj.library_k768" and zr.route("in_proj", 32768, 3072, 768).row == "in_proj.tiled_wide_k"
    assert zr.route("out_proj", 65536, 640, 1280) == zr.Route("tiled", True, "out_proj.tiled") and zr.route("out_proj", 16384, 640, 1280).row == "out_proj.ws128"
    assert zr.route("out_proj", 8192, 768, 1536).row == "out_proj.sm" and zr.route("to_q", 8192, 512, 640).row == "to_q.sm"
    assert zr.route("to_out", 65536, 640, 512) == zr.Route("tiled", True, "to_out.tiled") and zr.route("to_q", 65536, 512, 640).row == "to_q.tiled"
    assert zr.kernel_name(zr.route("in_proj", 32768, 3072, 768), 32768, 3072, 768) == "linear4w_256x256"
    assert zr.kernel_name(zr.route("to_q", 16384, 512, 640), 16384, 512, 640) == "linear_tn_"
    # the 128-feature-panel form holds at most 32 panels — in_proj of an E = 1280 / 1536 model must not be claimed for it
    assert not zr.serves_ws(16384, 5120, 1280) and not zr.serves_ws(16384, 6144, 1536) and zr.serves_ws(16384, 4096, 1280)
    assert zr.route("in_proj", 16384, 5120, 1280).kernel == "tiled" and zr.route("in_proj", 16384, 6144, 1536).kernel == "tiled"
    # the training path (forward product and dX of every block projection): weight-stationary where it serves, then tiled, then the library
    for E in (512, 640, 768, 1024):
        for tokens in (4096, 8192, 16384, 65536, 4096 + 8, 100):
            for n, k in ((4 * E, E), (E, 4 * E), (E, 2 * E), (2 * E, E), (512, E), (E, 512)):
                want = ("ws" if zr.serves_ws(tokens, n, k) and k in (512, 640) else "ws128" if zr.serves_ws(tokens, n, k)
                        else "tiled" if zr.serves_tiled(tokens, n, k) else "library")
                assert zr.route("train", tokens, n, k) == zr.Route(want, False, "train." + want), (E, tokens, n, k)
    assert zr.route("train", 65536, 2560, 640).row == "train.ws" and zr.route("train", 65536, 640, 1280).row == "train.ws128"
    assert zr.route("train", 65536, 640, 2560).row == "train.tiled" and zr.route("train", 65536, 100, 640).row == "train.library"
    # the text projections (B x 77 rows padded to 256): tiled wherever it serves
    assert zr.route("text", 5120, 18 * 2 * 512, 640) == zr.Route("tiled", False, "text.tiled") and zr.route("text", 256, 640, 768).row == "text.tiled"
    assert zr.route("text", 256, 100, 768).row == "text.library"
    assert [r.row for r in zr.candidates("in_proj", 65536, 2560, 640)] == ["in_proj.ws", "in_proj.halves", "in_proj.library"]
    # (iv) knobs
    try:
        zr.DISABLED = {"in_proj.ws"}
        assert zr.route("in_proj", 32768, 2560, 640).row == "in_proj.halves" and zr.route("in_proj", 16384, 2560, 640).row == "in_proj.library"
        zr.DISABLED = "out_proj.tiled+out_proj.ws128"
        assert zr.route("out_proj", 65536, 640, 1280).row == "out_proj.library"
        zr.DISABLED, zr.POLICY = "", "off"
        assert all(zr.route(role, 65536, n, k).kernel == "library" for role, n, k in (("in_proj", 2560, 640), ("to_out", 640, 512)))
        assert all(zr.route(role, 65536, 2560, 640) == zr.Route("library", False, "policy.off") for role in ("text", "train"))
        zr.POLICY = "all"
        assert zr.route("in_proj", 65536, 2560, 640) == zr.Route("tiled", False, "policy.all") and zr.route("out_proj", 16384, 640, 1280).fuse_add
        assert zr.route("train", 65536, 2560, 640).row == "train.ws" and zr.route("text", 5120, 640, 768).row == "text.tiled"      # as under "auto"
        zr.POLICY, zr.DISABLED = "auto", "train.ws+train.ws128+text.tiled"
        assert zr.route("train", 65536, 2560, 640).row == "train.tiled" and zr.route("train", 65536, 640, 1280).row == "train.tiled"
        assert zr.route("text", 5120, 640, 768).row == "text.library"
    finally:
        zr.DISABLED, zr.POLICY = "", "auto"
    with pytest.raises(ValueError):
        zr.route("x_proj", 1, 1, 1)


def test_project_on_cpu_falls_to_the_reference_composition():
    """linear.project on tensors the own kernels cannot take (CPU, fp32) is F.linear (+ the gated add), never an own kernel and never an error"""
    from zigma_amd.linear import project
    g = torch.Generator().manual_seed(3)
    x, w, b = torch.randn(2, 256, 64, generator=g), torch.randn(128, 64, generator=g), torch.randn(128, generator=g)
    res, gate = torch.randn(2, 256, 128, generator=g), torch.randn(2, 128, generator=g)
    assert torch.equal(project("in_proj", x, w), torch.nn.functional.linear(x, w))
    assert torch.allclose(project("to_out", x, w, b, residual=res, gate=gate), res + gate[:, None] * torch.nn.functional.linear(x, w, b), atol=1e-5)


def test_build_refuses_a_spilling_scan_kernel():
    """zigma_amd/build.py parses the resource-usage remarks of the scan TUs: an instantiation of scan_tok2_kernel with scratch memory or a spilled
    register fails the build (its inline-asm d16_hi row loads are invisible to the register allocator — ADVICE r5)"""
    from zigma_amd import build
    ok = ("x.inc:69:1: remark: Function Name: _ZN5zigma16scan_tok2_kernelINS_4BF16ELb1EEEv [-Rpass-analysis=kernel-resource-usage]\n"
          "x.inc:69:1: remark:     VGPRs: 89 [-Rpass-analysis=kernel-resource-usage]\n"
          "x.inc:69:1: remark:     ScratchSize [bytes/lane]: 0 [-Rpass-analysis=kernel-resource-usage]\n"
          "x.inc:69:1: remark:     VGPRs Spill: 0 [-Rpass-analysis=kernel-resource-usage]\n"
          "x.inc:9:1: remark: Function Name: _ZN5zigma5otherEv [-Rpass-analysis=kernel-resource-usage]\n"
          "x.inc:9:1: remark:     ScratchSize [bytes/lane]: 64 [-Rpass-analysis=kernel-resource-usage]\n")
    assert build.check_no_scratch(ok, "x.hip") == 1
    with pytest.raises(RuntimeError, match="must not spill"):
        build.check_no_scratch(ok.replace("ScratchSize [bytes/lane]: 0", "ScratchSize [bytes/lane]: 16"), "x.hip")
    with pytest.raises(RuntimeError, match="must not spill"):
        build.check_no_scratch(ok.replace("VGPRs Spill: 0", "VGPRs Spill: 3"), "x.hip")
    with pytest.raises(RuntimeError, match="no instantiation"):
        build.check_no_scratch("", "x.hip")


def test_linear_ws_policy_limits_on_cpu_tensors():
    """linear_ws_eligible never claims a CPU tensor or a shape outside the kernel's limits (the C side re-checks and refuses)"""
    from zigma_amd.linear import linear_ws_eligible
    x = torch.zeros(4096, 640, dtype=torch.bfloat16)
    assert not linear_ws_eligible(x, torch.zeros(2560, 640, dtype=torch.bfloat16))          # not on the device


def test_scan_paths_bit_exact_vs_reference_tables():
    from zigma_amd import scan_paths as sp
    g = load_golden("paths.npz")
    for n in (4, 8, 16, 32):
        zz, hh = sp.zigzag_path(n), sp.hilbert_path(n)
        assert len(zz) == 8 and len(hh) == 8
        for i in range(8):
            assert zz[i].dtype == np.int64 and np.array_equal(zz[i], g[f"zigzag_{n}_{i}"])
            assert np.array_equal(sp.reverse_permut_np(zz[i]), g[f"zigzag_rev_{n}_{i}"])
            assert np.array_equal(hh[i], g[f"hilbert_{n}_{i}"])
    for a, b in zip(sp.hilbert_path(128), zo.hilbert_paths(128)):
        assert np.array_equal(a, b)
    t = sp.to_device_tables(sp.zigzag_path(4), "cpu")
    assert t[0].dtype == torch.int32 and t[7].tolist() == [15, 11, 7, 3, 2, 6, 10, 14, 13, 9, 5, 1, 0, 4, 8, 12]


@pytest.mark.parametrize("name", ["zigma_text_zigzag2", "zigma_uncond_zigzag8", "zigma_class_v2", "zigma_hilbert2",
                                  "zigma_video_sst"])
def test_state_dict_is_reference_compatible(name):
    """same keys and shapes as the reference module built with the same constructor arguments"""
    from zigma_amd.model_zigma import ZigMa
    g = load_golden(name + ".npz")
    cfg = ast.literal_eval(str(g["cfg"]))
    m = ZigMa(device="cpu", **cfg)
    ref = {k[3:]: v.shape for k, v in g.items() if k.startswith("sd.")}
    mine = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert set(mine) == set(ref)
    for k in ref:
        assert mine[k] == tuple(ref[k]), k
    m.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd.")}, strict=True)
    # per-layer row tables follow the reference's layer -> table assignment
    om = zo.ZigMaOracle({k[3:]: v for k, v in g.items() if k.startswith("sd.")}, cfg)
    if om.paths is not None:
        for i, blk in enumerate(m.blocks):
            assert np.array_equal(blk.mixer._perm.numpy().astype(np.int64), om.paths[i]), i


def test_constructor_surface_and_defaults():
    from zigma_amd.model_zigma import ZigMa
    m = ZigMa(in_channels=4, embed_dim=32, depth=2, img_dim=8, device="cpu")           # default scan_type v2
    assert "blocks.0.mixer.A_b_log" in m.state_dict() and m.final_layer.linear.weight.shape == (4, 32)
    assert all(float(b.adaLN_modulation[-1].weight.detach().abs().sum()) == 0 for b in m.blocks)   # adaLN-zero init
    with pytest.raises(ValueError):
        ZigMa(in_channels=4, embed_dim=32, depth=2, img_dim=8, device="cpu", scan_type="v1")
    m = ZigMa(in_channels=4, embed_dim=32, depth=2, img_dim=8, device="cpu", scan_type="parallelN2")
    with pytest.raises(NotImplementedError):
        m.forward_with_cfg(None, None, None, 1.0)


def test_no_cpu_fallback():
    """the product path refuses CPU tensors instead of silently computing somewhere else"""
    from zigma_amd.causal_conv1d_interface import causal_conv1d_fn
    from zigma_amd.layernorm import rms_norm_fn
    from zigma_amd.selective_scan_interface import selective_scan_fn
    u = torch.randn(1, 4, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        selective_scan_fn(u, u, -torch.rand(4, 2), torch.randn(1, 2, 8), torch.randn(1, 2, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        causal_conv1d_fn(u, torch.randn(4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rms_norm_fn(u, torch.ones(8), None)
    src = "".join(open(os.path.join(ROOT, "zigma_amd", f)).read() for f in os.listdir(os.path.join(ROOT, "zigma_amd"))
                  if f.endswith(".py"))
    assert "oracle" not in src.replace("the CPU oracle", "")      # product never imports the oracle


def test_transport_rules_and_fixed_grid_solvers():
    from zigma_amd.transport import ModelType, Sampler, create_transport
    tr = create_transport()                                   # Linear / velocity
    assert tr.model_type == ModelType.VELOCITY and tr.train_eps == 0 and tr.sample_eps == 0
    assert tr.check_interval(0, 0, sde=False, eval=True) == (0, 1)
    assert create_transport("Linear", "noise").train_eps == 1e-3
    vp = create_transport("VP", "velocity")
    assert vp.train_eps == 1e-5 and vp.check_interval(vp.train_eps, vp.sample_eps, eval=True)[1] == 1 - vp.sample_eps
    with pytest.raises(ValueError):
        create_transport(prediction="nope")
    x0 = torch.tensor([[1.0, 2.0], [3.0, -4.0]], dtype=torch.float64)
    model = lambda x, t: -x * (1 + t.view(-1, 1))
    for method in ("euler", "midpoint", "heun2", "rk4"):
        fn = Sampler(tr).sample_ode(sampling_method=method, num_steps=9)
        got = fn(x0, model)
        ref = zo.sample_ode_fixed(lambda x, t: -x * (1 + t[:, None]), x0.numpy(), num_steps=9,
                                  method=method, dt=np.float64)
        assert got.shape == (9, 2, 2) and rel_err(got.numpy(), ref) < 1e-6, method
    exact = x0 * np.exp(-1.5)
    for method, tol in (("dopri5", 1e-4), ("bosh3", 2e-3), ("adaptive_heun", 2e-2)):
        got = Sampler(tr).sample_ode(sampling_method=method, num_steps=4, rtol=1e-5, atol=1e-8)(x0, model)
        assert got.shape == (4, 2, 2) and rel_err(got[-1].numpy(), exact.numpy()) < tol, method
    # the adaptive controller (torchdiffeq's rules, restated) against the independent float64 host restatement in the
    # oracle: same accepted / rejected sequence, same NFE, same trajectory; one host read per step, none elsewhere
    from zigma_amd.transport import integrators as integ
    stiff = lambda x, t: -x * (1 + t.view(-1, 1)) + torch.sin(3 * x)
    got = Sampler(tr).sample_ode(sampling_method="dopri5", num_steps=7, rtol=1e-3, atol=1e-6)(x0, stiff)
    st = integ.AdaptiveStats
    ref, nfe, acc, rej = zo.sample_ode_dopri5(lambda x, t: -x * (1 + t[:, None]) + np.sin(3 * x), x0.numpy(), num_steps=7)
    assert (st.nfe, st.accepted, st.steps - st.accepted) == (nfe, acc, rej) and rej > 0
    assert st.host_reads == st.steps
    assert got.shape == (7, 2, 2) and np.abs(got.numpy() - ref).max() < 1e-6
    rev = Sampler(tr).sample_ode(sampling_method="euler", num_steps=3, reverse=True)(x0, lambda x, t: torch.ones_like(x))
    assert torch.allclose(rev[-1], x0 - 1)                    # reverse integrates from t=1 down to 0
    # ... and with the default adaptive solver (data -> noise; decreasing time grid like torchdiffeq accepts): y' = -y(1 + t)
    # from t = 1 down to 0 is y0 * exp(1.5); bosh3 through the same sign flip; a non-monotonic grid raises
    for method, tol in (("dopri5", 1e-4), ("bosh3", 2e-3)):
        rev = Sampler(tr).sample_ode(sampling_method=method, num_steps=5, rtol=1e-5, atol=1e-8, reverse=True)(x0, model)
        assert rev.shape == (5, 2, 2) and rel_err(rev[-1].numpy(), (x0 * np.exp(1.5)).numpy()) < tol, method
    fwd = integ.odeint(lambda t, y: -y, x0, torch.tensor([0.0, 0.25, 1.0]), method="dopri5", rtol=1e-6, atol=1e-9)
    bwd = integ.odeint(lambda t, y: -y, fwd[-1], torch.tensor([1.0, 0.25, 0.0]), method="dopri5", rtol=1e-6, atol=1e-9)
    assert torch.allclose(bwd[-1], x0, rtol=1e-5) and torch.allclose(bwd[1], fwd[1], rtol=1e-5)
    with pytest.raises(ValueError):
        integ.odeint(lambda t, y: -y, x0, torch.tensor([0.0, 0.5, 0.25]), method="dopri5")
    with pytest.raises(RuntimeError):                         # a NaN from the model stops the solve instead of spinning to max_steps
        integ.odeint(lambda t, y: y * float("nan"), x0, torch.tensor([0.0, 1.0]), method="dopri5")
    # likelihood ODE on a field with a known divergence: v(x, t) = a x  ->  div = a * dim exactly (Rademacher probes give
    # the exact trace of a diagonal Jacobian), z = x e^{-a}, logp(x) = prior_logp(z) - a * dim
    a = 0.7
    xs = torch.randn(3, 2, 2, 2)
    logp, z = Sampler(tr).sample_ode_likelihood(sampling_method="dopri5", num_steps=5, rtol=1e-6, atol=1e-8)(
        xs, lambda x, t: a * x)
    assert torch.allclose(z, xs * math.exp(-a), rtol=1e-4, atol=1e-5)
    assert torch.allclose(logp, tr.prior_logp(xs * math.exp(-a)) - a * 8, rtol=1e-4, atol=1e-4)
    logp_e, _ = Sampler(tr).sample_ode_likelihood(sampling_method="rk4", num_steps=21)(xs, lambda x, t: a * x)
    assert torch.allclose(logp_e, logp, rtol=1e-4, atol=1e-3)


def test_sde_sampler_matches_reference_golden():
    """Sampler.sample_sde (Euler-Maruyama / Heun, every last-step rule, SBDM / sigma / linear / ... diffusions, all three
    paths and predictions) against trajectories of the unmodified reference on the same CPU RNG stream
    (oracle/make_golden_sde.py).  The reference evaluates the model twice per drift; one evaluation must give the same."""
    import ast
    from zigma_amd.transport import ModelType, PathType, Sampler, Transport, WeightType
    g = np.load(os.path.join(ROOT, "tests", "golden", "sde_sampler.npz"))
    cases = ast.literal_eval(str(g["cases"]))

    calls = [0]

    def toy_model(x, t, **kw):
        calls[0] += 1
        tt = t.view(-1, *([1] * (x.dim() - 1)))
        return torch.tanh(x) * (0.3 + tt) - 0.5 * x

    for i, (path, pred, smp, form, norm, last, lss, n) in enumerate(cases):
        mt = {"velocity": ModelType.VELOCITY, "noise": ModelType.NOISE, "score": ModelType.SCORE}[pred]
        pt = {"Linear": PathType.LINEAR, "GVP": PathType.GVP, "VP": PathType.VP}[path]
        tr = Transport(model_type=mt, path_type=pt, loss_type=WeightType.NONE, train_eps=1e-3, sample_eps=1e-3)
        fn = Sampler(tr).sample_sde(sampling_method=smp, diffusion_form=form, diffusion_norm=norm, last_step=last,
                                    last_step_size=lss, num_steps=n)
        torch.manual_seed(100 + i)
        x0 = torch.randn(3, 2, 4, 4)
        assert np.array_equal(x0.numpy(), g[f"x0_{i}"])
        calls[0] = 0
        xs = fn(x0, toy_model)
        assert len(xs) == n
        for key, got in (("last", xs[-1]), ("mid", xs[len(xs) // 2])):
            ref = g[f"{key}_{i}"]
            err = np.linalg.norm(got.numpy() - ref) / np.linalg.norm(ref)
            assert err < 1e-5, (i, key, err)
        per_step = 1 if smp == "Euler" else 2
        assert calls[0] == per_step * (n - 1) + (0 if last is None else 1)   # the reference needs twice as many
    const = Sampler(Transport(model_type=ModelType.VELOCITY, path_type=PathType.LINEAR, loss_type=WeightType.NONE,
                              train_eps=1e-3, sample_eps=1e-3)).sample_sde(diffusion_form="constant", diffusion_norm=0.1,
                                                                           num_steps=5)
    assert torch.isfinite(const(torch.randn(2, 3), toy_model)[-1]).all()    # the reference raises TypeError here
    with pytest.raises(NotImplementedError):
        Sampler(tr).sample_sde(sampling_method="nope")(x0, toy_model)


def test_plans_match_closed_forms():
    from zigma_amd.transport import path
    t = torch.tensor([0.25, 0.5])
    x0, x1 = torch.randn(2, 3), torch.randn(2, 3)
    _, xt, ut = path.ICPlan().plan(t, x0, x1)
    assert torch.allclose(xt, t[:, None] * x1 + (1 - t[:, None]) * x0) and torch.allclose(ut, x1 - x0)
    g = path.GVPCPlan()
    a, da = g.compute_alpha_t(t)
    s, ds = g.compute_sigma_t(t)
    assert torch.allclose(a ** 2 + s ** 2, torch.ones(2)) and torch.allclose(a * da + s * ds, torch.zeros(2), atol=1e-6)
    # velocity -> score -> velocity round trip on the linear path
    v = torch.randn(2, 3)
    p = path.ICPlan()
    sc = p.get_score_from_velocity(v, xt, t)
    assert torch.allclose(p.get_velocity_from_score(sc, xt, t), v, atol=1e-4)


@pytest.mark.parametrize("name", ["zigma_text_zigzag2", "zigma_uncond_zigzag8", "zigma_class_v2", "zigma_hilbert2",
                                  "zigma_video_sst"])
def test_module_plumbing_with_oracle_standins(name, monkeypatch):
    """ZigMa / Block / Mamba host logic (token-major layouts, row tables, pending gated residuals, video
    reshapes) with the three HIP entry points replaced by oracle-backed stand-ins: must reproduce the
    reference's golden output.  (The real kernels are checked against the same vectors in the gpu tests.)"""
    import kernel_standins
    from zigma_amd.model_zigma import ZigMa
    kernel_standins.install(monkeypatch)
    g = load_golden(name + ".npz")
    cfg = ast.literal_eval(str(g["cfg"]))
    m = ZigMa(device="cpu", **cfg).eval()
    m.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd.")}, strict=True)
    y = g.get("y")
    if y is not None:
        y = torch.from_numpy(y)
        y = y.long() if cfg.get("num_classes", -1) > 0 else y
    with torch.no_grad():
        out = m(torch.from_numpy(g["x"]), torch.from_numpy(g["t"]), y)
    assert rel_err(out.numpy(), g["out"]) < 2e-5, rel_err(out.numpy(), g["out"])


def test_video16_no_copy_temporal_path_host_logic(monkeypatch):
    """16-frame model: the temporal layers take the no-copy arrangement (batch = k, sequence = (b, t) on strided views,
    tiled time tables, reset_period = T).  Host logic with oracle-backed stand-ins against the REFERENCE's output
    (tests/golden/r2_small_video16.npz, oracle/make_golden_r2.py; weights regenerated by oracle/param_fill.py)."""
    import kernel_standins
    import zigma_amd.mamba_simple as ms
    from oracle.param_fill import fill_state
    from zigma_amd.model_zigma import ZigMa
    kernel_standins.install(monkeypatch)
    resets = []
    real = ms.mamba_inner_tok
    monkeypatch.setattr(ms, "mamba_inner_tok", lambda *a, **k: (resets.append(k.get("reset_period", 0)), real(*a, **k))[1])
    g = load_golden("r2_small_video16.npz")
    cfg = ast.literal_eval(str(g["cfg"]))
    m = fill_state(ZigMa(device="cpu", **cfg), int(g["seed"])).eval()
    with torch.no_grad():
        out = m(torch.from_numpy(g["x"]), torch.from_numpy(g["t"]), torch.from_numpy(g["y"]))
    assert resets.count(16) == 2 and resets.count(0) == 4            # s s t s s t
    assert rel_err(out.numpy(), g["out"]) < 2e-5, rel_err(out.numpy(), g["out"])


@pytest.mark.parametrize("name", ["r2_small_video16", "r6_zigzag8_e768", "r6_sweep2_e768"])
def test_oracle_model_vs_r2_reference_goldens(name):
    """the numpy oracle against the round-2 / round-6 reference outputs (16-frame video model; the shipped yamls' E = 768 layer shapes with
    zigzagN8 and with the bidirectional `v2`; param_fill weights)."""
    from oracle.param_fill import fill_state
    from zigma_amd.model_zigma import ZigMa
    g = load_golden(name + ".npz")
    cfg = ast.literal_eval(str(g["cfg"]))
    m = fill_state(ZigMa(device="cpu", **cfg), int(g["seed"]))
    om = zo.ZigMaOracle({k: v.numpy() for k, v in m.state_dict().items()}, cfg)
    out = om.forward(g["x"], g["t"], g.get("y"))
    assert rel_err(out, g["out"]) < 2e-5, rel_err(out, g["out"])


@pytest.mark.parametrize("name", ["r6_zigzag8_e768", "r6_sweep2_e768"])
def test_e768_host_logic_vs_reference(name, monkeypatch):
    """Host logic of the E = 768 models (every shipped yaml: config/model/zigzag8_b1_pe2.yaml, sweep2_b1_pe2.yaml) with oracle-backed kernel
    stand-ins against the REFERENCE's fp32 output: row tables of zigzagN8, the reversed table + second parameter set of `v2`
    (mamba_simple.py:304-339)."""
    import kernel_standins
    from oracle.param_fill import fill_state
    from zigma_amd.model_zigma import ZigMa
    kernel_standins.install(monkeypatch)
    g = load_golden(name + ".npz")
    cfg = ast.literal_eval(str(g["cfg"]))
    m = fill_state(ZigMa(device="cpu", **cfg), int(g["seed"])).eval()
    with torch.no_grad():
        out = m(torch.from_numpy(g["x"]), torch.from_numpy(g["t"]), None)
    assert rel_err(out.numpy(), g["out"]) < 2e-5, rel_err(out.numpy(), g["out"])


def test_postprocess_matches_reference_formulas():
    """sample_acc.py:319-321,362-377: latent / 0.18215 -> decode -> clamp(127.5 x + 128, 0, 255) -> uint8 (truncation);
    video latents decoded per sample and stacked along dim 1."""
    from zigma_amd import postprocess as pp
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 4, 8, 8, generator=g)
    dec = lambda z: torch.tanh(z[:, :3].repeat_interleave(2, -1).repeat_interleave(2, -2))      # toy "VAE": 4x8x8 -> 3x16x16
    got = pp.finish_samples(x, dec, world=1)
    ref = torch.clamp(127.5 * dec(x / 0.18215) + 128.0, 0, 255).to(dtype=torch.uint8)
    assert got.dtype == torch.uint8 and got.shape == (3, 3, 16, 16) and torch.equal(got, ref)
    assert torch.equal(pp.to_uint8(torch.tensor([-1.5, -1.0, 0.0, 0.999, 1.0, 2.0])),
                       torch.tensor([0, 0, 128, 255, 255, 255], dtype=torch.uint8))
    assert torch.equal(pp.finish_samples(x, None, world=1), pp.to_uint8(x))                       # pixel-space model: no decode
    v = torch.randn(2, 5, 4, 8, 8, generator=g)
    gv = pp.decode_latents(v, dec, is_video=True)
    rv = torch.stack([dec(v[i] / 0.18215) for i in range(2)], dim=1)
    assert gv.shape == (5, 2, 3, 16, 16) and torch.equal(gv, rv)


def test_drop_path_is_applied_once_per_block_in_train_mode(monkeypatch):
    """Stochastic depth (reference model_zigma.py:406-437,963-975): once per block on the incoming branch when a residual
    stream exists, once before the final norm.  DropPath is mocked to the deterministic x -> 2x so a double application
    shows up as a factor; the fused_add_norm=True path must equal the literal non-fused composition."""
    import kernel_standins
    from zigma_amd import model_zigma as mz
    kernel_standins.install(monkeypatch)
    calls = []
    monkeypatch.setattr(mz.DropPath, "forward", lambda self, x: (calls.append(1), x * 2.0)[1])
    g = load_golden("zigma_uncond_zigzag8.npz")
    cfg = dict(ast.literal_eval(str(g["cfg"])), drop_path_rate=0.5)
    sd = {k[3:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("sd.")}
    outs = []
    for fused in (True, False):
        m = mz.ZigMa(device="cpu", **dict(cfg, fused_add_norm=fused)).train()
        m.load_state_dict(sd, strict=True)
        calls.clear()
        with torch.no_grad():
            outs.append(m(torch.from_numpy(g["x"]), torch.from_numpy(g["t"]), None))
        live = sum(isinstance(b.drop_path, mz.DropPath) for b in m.blocks[1:])     # rate 0 -> nn.Identity (blocks 0, 1)
        assert live == cfg["depth"] - 2 and len(calls) == live + 1, (fused, len(calls))
    assert rel_err(outs[0].numpy(), outs[1].numpy()) < 2e-5
    m.eval()
    calls.clear()
    with torch.no_grad():
        m(torch.from_numpy(g["x"]), torch.from_numpy(g["t"]), None)
    assert rel_err(outs[0].numpy(), g["out"]) > 1e-2       # the mock really changes the result in train mode


def test_extension_shims_under_the_reference_python(monkeypatch):
    """the reference's OWN `mamba_inner_fn` (MambaInnerFn.forward) runs on the shim modules.
    Its two extension calls are replayed from tests/golden/shim_calls_mamba_inner.npz (recorded from the reference's Python by
    oracle/make_golden_shim_calls.py): entry-point names, argument order, the views / strides / aliasing the reference passes
    (x and z are the two halves of one xz buffer, delta is a transposed view), the result arity it unpacks.  Kernels are replaced
    by the oracle stand-ins here (CPU); each result is compared with the reference's own pure-torch function on the same operands,
    the inputs must come back untouched (callee allocates), and out_proj of the gated scan output must give mamba_inner_fn's output."""
    import importlib
    import sys
    import kernel_standins
    import torch.nn.functional as F
    kernel_standins.install(monkeypatch)
    from zigma_amd import _lib, extension_shims
    monkeypatch.setattr(_lib, "require_device", lambda *a: torch.device("cpu"))
    for name in ("selective_scan_cuda", "causal_conv1d_cuda"):
        monkeypatch.delitem(sys.modules, name, raising=False)
    ss, cc = extension_shims.install()
    assert importlib.import_module("selective_scan_cuda") is ss and importlib.import_module("causal_conv1d_cuda") is cc
    rec = load_golden("shim_calls_mamba_inner.npz")
    assert list(rec["calls"]) == ["causal_conv1d_cuda.causal_conv1d_fwd", "selective_scan_cuda.fwd"]
    storages = [torch.from_numpy(rec[f"s{k}"].copy()) for k in range(sum(k.startswith("s") and k[1:].isdigit() for k in rec))]

    def replay(i):
        mod, fn = str(rec["calls"][i]).split(".")
        args = []
        for j, kind in enumerate(rec[f"c{i}_kinds"]):
            if kind == "none":
                args.append(None)
            elif kind == "bool":
                args.append(bool(rec[f"c{i}_a{j}_value"]))
            else:
                off, nd, *rest = rec[f"c{i}_a{j}_view"].tolist()
                args.append(torch.as_strided(storages[int(rec[f"c{i}_a{j}_storage"])], rest[:nd], rest[nd:], off))
        with torch.no_grad():
            res = getattr(importlib.import_module(mod), fn)(*args)
        assert (len(res) if isinstance(res, (list, tuple)) else -1) == int(rec[f"c{i}_nret"]), (mod, fn)
        return args, res

    (x, w, b, silu), conv_out = replay(0)
    assert x.stride() == (9216, 96, 1) and silu is True                  # the x half of xz, not copied by the caller
    assert conv_out.shape == x.shape and rel_err(conv_out.numpy(), rec["c0_expect"]) < 5e-6
    (u, delta, A, B, C, D, z, db, softplus), (out, last, out_z) = replay(1)
    assert z.storage_offset() == 4608 and z.untyped_storage().data_ptr() == storages[0].untyped_storage().data_ptr()
    assert delta.stride() == (96, 192, 1) and B.shape == (2, 1, 16, 96) and softplus is True
    assert out.shape == delta.shape and out_z.shape == z.shape and last.shape[:2] == u.shape[:2]
    assert rel_err(out.numpy(), rec["c1_expect_out"]) < 5e-6 and rel_err(out_z.numpy(), rec["c1_expect_out_z"]) < 5e-6
    for k, s in enumerate(storages):
        assert np.array_equal(s.numpy(), rec[f"s{k}"]), f"storage {k} written by the callee"
    g = load_golden("mamba_inner.npz")
    y = F.linear(out_z.transpose(1, 2), torch.from_numpy(g["out_proj_w"]), torch.from_numpy(g["out_proj_b"]))
    assert rel_err(y.numpy(), g["out"]) < 5e-6


def test_sequence_split_policy():
    """host-side choice of the scan's sequence split (no GPU): only when the plain grid cannot fill the chip."""
    from zigma_amd.selective_scan_interface import split_chunk_len
    assert split_chunk_len(64, 1280, 1024) == 0                      # headline batch: 1280 workgroups, single pass
    assert split_chunk_len(1, 1280, 1024) == 32                      # one sample: 20 workgroups -> 32 chunks of 32 steps
    assert split_chunk_len(4, 1280, 1024) == 112 and split_chunk_len(16, 1280, 1024) == 0
    assert split_chunk_len(4, 1280, 16384) == 1024 and split_chunk_len(64, 1280, 16384) == 0   # 80 wgs x 16 chunks = 5 per CU
    assert split_chunk_len(1, 1280, 16384) == 256 and split_chunk_len(30, 1280, 4096) == 1376
    assert split_chunk_len(1, 1280, 128) == 0 and split_chunk_len(2, 1536, 4096, reset_period=16) == 0
    for b in range(1, 11):
        c = split_chunk_len(b, 1280, 1024)
        assert c % 16 == 0 and c >= 32 and -(-1024 // c) >= 2


_PLAN_DRIVER = r"""
#include "scan_plan.h"
using namespace zigma;
// what the library reports for a call: the plan, or for a sliced batch the plan of the slice its walk ends on
extern "C" int plan(const zigma_scan_params_t *p, int *fields, const char **kernel) {
    ScanPlan s;
    for_each_scan_call(*p, [&s](const zigma_scan_params_t &, const ScanPlan &each) { s = each; return each.family ? int(ZIGMA_OK) : each.status; });
    fields[0] = s.status; fields[1] = s.family; fields[2] = s.info1;
    *kernel = s.kernel;
    return s.status;
}
extern "C" int split_ok(const zigma_scan_params_t *p) { return tok2_split_ok(*p); }
"""


def _compile_plan(driver):
    """a driver around one of the HIP-free plan headers of zigma_amd/csrc, compiled on its own with g++ and loaded"""
    with tempfile.TemporaryDirectory() as d:
        src, so = os.path.join(d, "plan.cpp"), os.path.join(d, "libplan.so")
        open(src, "w").write(driver)
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                        "-I", os.path.join(ROOT, "zigma_amd", "csrc"), src, "-o", so], check=True)
        return ctypes.CDLL(so)


def _plan_caller(L, params_type, names, fn="plan", field_type=ctypes.c_int):
    """plan(P) -> dict of the driver's integer fields and the kernel string"""
    entry = getattr(L, fn)
    entry.argtypes = [ctypes.POINTER(params_type), ctypes.POINTER(field_type), ctypes.POINTER(ctypes.c_char_p)]

    def plan(P):
        f, k = (field_type * len(names))(), ctypes.c_char_p()
        entry(ctypes.byref(P), f, ctypes.byref(k))
        return dict(zip(names, f), kernel=k.value.decode() if k.value else None)
    return plan


@pytest.fixture(scope="module")
def scan_plan():
    """plan_scan() of zigma_amd/csrc/scan_plan.h compiled on its own with g++ (no HIP): plan(params) -> status, family, info1, kernel;
    split_ok(params)"""
    from zigma_amd import _lib
    L = _compile_plan(_PLAN_DRIVER)
    L.split_ok.argtypes = [ctypes.POINTER(_lib.ScanParams)]
    plan = _plan_caller(L, _lib.ScanParams, ("status", "family", "info1"))
    plan.split_ok = lambda P: bool(L.split_ok(ctypes.byref(P)))
    return plan


def _split_dtp_block(batch, d_inner, seqlen, chunk_len):
    """the scan block of the sequence split with dt_proj in its first pass (x, the delta workspace, dt_x / dt_w), on operands the in-kernel dt_proj
    accepts at every size: bf16, dt_rank 40, 16 states, 72-wide x_dbl rows, every activation one broadcast row (pitch 0: no in-sample offset grows
    with seqlen)"""
    from zigma_amd import _lib
    P = _lib.ScanParams()
    P.batch, P.dim, P.seqlen, P.dstate, P.n_groups, P.chunk_len = batch, d_inner, seqlen, 16, 1, chunk_len
    P.io_dtype = P.bc_dtype = _lib.BF16
    P.delta_softplus, P.is_variable_B, P.is_variable_C = 1, 1, 1
    for k, name in enumerate(("u", "delta", "z", "out_z")):
        setattr(P, name, (k + 1) << 40), setattr(P, f"{name}_d_stride", 1)
    for name, col in (("B", 40), ("C", 56)):
        setattr(P, name, (5 << 40) + col * 2), setattr(P, f"{name}_l_stride", 72), setattr(P, f"{name}_dstate_stride", 1)
    P.A, P.A_d_stride, P.A_dstate_stride, P.x = 6 << 40, 16, 1, 7 << 40
    P.dt_x, P.dt_w, P.dt_rank, P.dt_x_l_stride, P.dt_w_row_stride = 5 << 40, 8 << 40, 40, 72, 40
    return P


def test_split_chunks_pass_the_c_side_split_limits(monkeypatch, scan_plan, libpath):
    """split_chunk_len under the default knobs only returns chunks the C side's sequence split accepts, and the library serves the split with dt_proj
    inside (what plan_inner asks before it takes "in_split") exactly where tok2_split_ok (scan_plan.h, compiled) says yes — including the chunks a
    raised SPLIT_MAX_WGS produces and more than 65535 chunks."""
    import zigma_amd.selective_scan_interface as ssi
    from zigma_amd import _lib
    Ls = (16, 32, 48, 128, 240, 256, 272, 1008, 1024, 1040, 2048, 4080, 4096, 4112, 8192, 16384, 65552, 1 << 20)
    Dis = (64, 128, 640, 1280, 1536, 3072, 4096)
    served = lambda b, di, L, c: _lib.plan("zigma_selective_scan_fwd", _split_dtp_block(b, di, L, c)) == (0, "scan_tok2_n16_split_dtproj")
    split_ok = lambda b, di, L, c: scan_plan.split_ok(_split_dtp_block(b, di, L, c))

    def sweep():
        hits = []
        for b in range(1, 1025):
            for di in Dis:
                for L in Ls:
                    c = ssi.split_chunk_len(b, di, L)
                    if c:
                        hits.append((b, di, L, c, served(b, di, L, c)))
        return hits
    hits = sweep()
    assert len(hits) > 1000 and all(ok for *_, ok in hits)
    assert all(split_ok(b, di, L, c) for b, di, L, c, _ in hits)
    monkeypatch.setattr(ssi, "SPLIT_MAX_WGS", 1024)
    hits = sweep()
    refused = [h for h in hits if not h[4]]
    assert refused and all(b * (di // 64) >= 768 for b, di, *_ in refused)
    assert all(ok == split_ok(b, di, L, c) for b, di, L, c, ok in hits)
    assert served(1, 64, 16 * 65535, 16) and not served(1, 64, 16 * 65536, 16)
    assert not served(1, 64, 1024, 24) and not served(1, 64, 1024, 1024) and not served(1, 64, 1024, 0)
    # ... and the same answers through the predicate plan_inner calls, on descriptors as it passes them
    bf = torch.bfloat16
    asks = lambda c, L=1024: ssi.dt_in_scan_eligible(_Dev(bf, 1, L, 64), _Dev(bf, 1, L, 72), _Dev(bf, 64, 40), dstate=16, chunk_len=c)
    assert asks(32) and not asks(24) and not asks(1024) and asks(16, 16 * 65535) and not asks(16, 16 * 65536)


@pytest.mark.parametrize("name", sorted(__import__("scan_plan_cases").CASES))
def test_scan_plan_case_table(name, scan_plan, libpath):
    """plan_scan() (compiled) on the parameter block scan_raw builds for every case of the table: status, family, info, last kernel; and the built
    library's host-only query (zigma_selective_scan_fwd_plan, no device here) answers the same status and kernel"""
    import scan_plan_cases
    from zigma_amd import _lib
    case, want = scan_plan_cases.CASES[name]
    got, asked = scan_plan_cases.call(case, "cpu", lambda P: (scan_plan(P), _lib.plan("zigma_selective_scan_fwd", P)))
    family = got["family"] or None
    assert (got["status"], family, (family, got["info1"]) if family else None, got["kernel"]) == tuple(want)
    assert asked == (want.status, want.kernel)


def _Dev(dtype, *shape, ptr=1 << 20, pitched=None, cuda=True):
    """a GPU tensor as the eligibility predicates read it — the package's own descriptor (_lib.Desc: shape, strides, dtype, address): contiguous, or with
    these strides (a view of a wider allocation); nothing is allocated"""
    from zigma_amd._lib import Desc
    return Desc(dtype, shape, tuple(pitched) if pitched else tuple(math.prod(shape[i + 1:]) for i in range(len(shape))), ptr, cuda)


def test_dt_in_scan_eligible_agrees_with_the_plan(scan_plan):
    """dt_in_scan_eligible() (Python) says yes exactly where plan_scan() takes the in-kernel dt_proj form, for the parameter block
    mamba_inner_tok passes: u and x_dbl fresh contiguous rows, z the second half of xz, B / C columns of x_dbl, no delta"""
    from zigma_amd import _lib
    from zigma_amd.selective_scan_interface import dt_in_scan_eligible
    seen = set()
    for dt in (torch.bfloat16, torch.float16, torch.float32):
        for B in (1, 65536):
            for L in (16, 24, 1024, 1 << 19):
                for Di in (64, 96, 1280):
                    for R in (16, 32, 40, 64, 72):
                        for N in (8, 16):
                            for rp in (0, 16, 24):
                                for off in (0, 2):
                                    W, es = R + 2 * N, 2 if dt != torch.float32 else 4
                                    u, x_dbl = _Dev(dt, B, L, Di), _Dev(dt, B, L, W, ptr=(1 << 24) + off * es)
                                    z = _Dev(dt, B, L, Di, pitched=(L * 2 * Di, 2 * Di, 1))
                                    w = _Dev(dt, Di, R, ptr=1 << 28)
                                    P = _lib.ScanParams()
                                    P.batch, P.dim, P.seqlen, P.dstate, P.n_groups, P.reset_period = B, Di, L, N, 1, rp
                                    P.io_dtype = P.bc_dtype = {torch.bfloat16: 2, torch.float16: 1, torch.float32: 0}[dt]
                                    P.delta_softplus, P.is_variable_B, P.is_variable_C, P.chunk_len = 1, 1, 1, 2048
                                    for name, t, d0 in (("u", u, 0), ("z", z, 1 << 26), ("out_z", u, 1 << 27)):
                                        setattr(P, name, t.data_ptr() + d0)
                                        setattr(P, f"{name}_batch_stride", t.stride(0)), setattr(P, f"{name}_l_stride", t.stride(1))
                                        setattr(P, f"{name}_d_stride", 1)
                                    for name, col in (("B", R), ("C", R + N)):
                                        setattr(P, name, x_dbl.data_ptr() + col * es)
                                        setattr(P, f"{name}_batch_stride", x_dbl.stride(0)), setattr(P, f"{name}_l_stride", x_dbl.stride(1))
                                        setattr(P, f"{name}_dstate_stride", 1)
                                    P.A, P.A_d_stride, P.A_dstate_stride = 1 << 29, N, 1
                                    P.dt_x, P.dt_w, P.dt_rank = x_dbl.data_ptr(), w.data_ptr(), R
                                    P.dt_x_batch_stride, P.dt_x_l_stride, P.dt_w_row_stride = x_dbl.stride(0), x_dbl.stride(1), w.stride(0)
                                    pl = scan_plan(P)
                                    planned = pl["status"] == 0 and pl["kernel"] is not None and "dtproj" in pl["kernel"]
                                    assert dt_in_scan_eligible(u, x_dbl, w, rp, None, dstate=N, z=z) == planned, (dt, B, L, Di, R, N, rp, off, pl)
                                    seen.add(planned)
    assert seen == {True, False}


_FRONT_PLAN_DRIVER = r"""
#include "front_plan.h"
using namespace zigma;
static int report(const FrontPlan &s, int *f, const char **kernel) {
    f[0] = s.status; f[1] = s.gx; f[2] = s.gy; f[3] = s.gz; f[4] = s.block; f[5] = s.tok; f[6] = s.silu; f[7] = s.contig_l; f[8] = s.width;
    f[9] = s.stages; f[10] = s.waves; f[11] = s.splitk;
    *kernel = s.kernel;
    return s.status;
}
// what the library reports for a call: the plan, or for a sliced batch the plan of the slice its walk ends on
extern "C" int plan_conv(const zigma_conv_params_t *p, int *f, const char **kernel) {
    FrontPlan s;
    for_each_conv_call(*p, [&s](const zigma_conv_params_t &, const FrontPlan &each) { s = each; return each.status; });
    return report(s, f, kernel);
}
extern "C" int plan_cx(const zigma_conv_xproj_params_t *p, int *f, const char **kernel) { return report(plan_conv_x_proj(*p), f, kernel); }
extern "C" int plan_xp(const zigma_xproj_params_t *p, int *f, const char **kernel) { return report(plan_x_proj(*p), f, kernel); }
extern "C" int plan_dt(const zigma_dtproj_params_t *p, int *f, const char **kernel) { return report(plan_dt_proj(*p), f, kernel); }
"""
_FRONT_FIELDS = ("status", "gx", "gy", "gz", "block", "tok", "silu", "contig_l", "width", "stages", "waves", "splitk")


@pytest.fixture(scope="module")
def front_plan():
    """plan_conv1d() / plan_conv_x_proj() / plan_x_proj() / plan_dt_proj() of zigma_amd/csrc/front_plan.h compiled on their own with g++ (no HIP):
    plan(params) -> status, grid, block, switches, kernel, by the type of the parameter block"""
    from zigma_amd import _lib
    L = _compile_plan(_FRONT_PLAN_DRIVER)
    by_type = {t: _plan_caller(L, t, _FRONT_FIELDS, fn) for t, fn in ((_lib.ConvParams, "plan_conv"), (_lib.ConvXProjParams, "plan_cx"),
                                                                      (_lib.XProjParams, "plan_xp"), (_lib.DtProjParams, "plan_dt"))}
    return lambda P: by_type[type(P)](P)


@pytest.mark.parametrize("name", sorted(__import__("front_plan_cases").CASES))
def test_front_plan_case_table(name, front_plan, libpath):
    """the four plans (compiled) on the parameter block the product's bindings build for every case of the table: status, last kernel; and the built
    library's host-only queries (zigma_*_fwd_plan, no device here) answer the same"""
    import front_plan_cases
    from zigma_amd import _lib
    (got, asked), _ = front_plan_cases.call(name, "cpu", lambda fn, P: (front_plan(P), _lib.plan(fn, P)))
    assert (got["status"], got["kernel"]) == tuple(front_plan_cases.CASES[name][2]) == asked


def test_front_plan_geometry(front_plan):
    """grid, block and template switches of the serving leaves against the closed forms of the kernels' headers"""
    import front_plan_cases

    def geometry(name, *fields):
        got, _ = front_plan_cases.call(name, "cpu", lambda fn, P: front_plan(P))
        return tuple(got[f] for f in fields)
    conv = ("gx", "gy", "gz", "block", "tok", "width", "silu", "contig_l")
    assert geometry("conv_tok_L17_w3_silu", *conv) == (1, 2, 2, 64, 1, 3, 1, 0)
    assert geometry("conv_tok_L1_w2_silu", *conv) == (1, 1, 2, 64, 1, 2, 1, 0) and geometry("conv_tok_L17_w4", *conv) == (1, 2, 2, 64, 1, 4, 0, 0)
    assert geometry("conv_tok_sliced_65536_samples", *conv) == (1, 1, 1, 64, 1, 4, 1, 0)               # the last slice: one sample
    assert geometry("conv_generic_channel_first", *conv) == (1, 1, 1, 256, 0, 0, 0, 1)                 # ceil(2 * 4 * 17 / 256) blocks
    assert geometry("conv_generic_dim_6", *conv) == (1, 1, 1, 256, 0, 0, 0, 0)
    cx = ("gx", "gy", "gz", "block", "stages", "waves")
    assert [geometry(f"cx_served_flags_{f}", *cx) for f in ("0", "1", "2", "3_f16")] == [(2, 1, 1, 256, 2, 4), (2, 1, 1, 256, 3, 4), (1, 1, 1, 512, 2, 8),
                                                                                       (1, 1, 1, 512, 3, 8)]
    xp = ("gx", "gy", "gz", "block", "splitk")
    assert geometry("xp_splitk", *xp) == (1, 1, 1, 512, 1) and geometry("xp_splitk_k_1536_f16_m_33", *xp) == (2, 1, 1, 512, 1)
    assert geometry("xp_streaming_k_1792", *xp) == (1, 1, 1, 512, 0) and geometry("xp_streaming_16384_rows", *xp) == (64, 1, 1, 512, 0)
    assert geometry("xp_splitk_16383_rows", *xp) == (512, 1, 1, 512, 1)
    dt = ("gx", "gy", "gz", "block")
    assert geometry("dt_served_1_row", *dt) == (1, 1, 1, 256) and geometry("dt_served_513_rows_f16", *dt) == (1, 2, 1, 256)


_TORCH_ID = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


def _sweep_verdict(eligible, pl, kernels, policy, point, seen):
    """one point of a predicate sweep: predicate true => the plan serves with one of `kernels`; predicate false where the plan serves => one of the
    named `policy` clauses ({name: holds at this point}) explains it"""
    served = pl["status"] == 0 and pl["kernel"] is not None
    if eligible:
        assert served and pl["kernel"] in kernels, (point, pl)
    elif served:
        why = [name for name, holds in policy.items() if holds]
        assert why, ("the predicate refuses what the plan serves and no policy clause says why", point, pl)
        seen.update(why)
    seen.add(bool(eligible))


def test_x_proj_eligible_agrees_with_the_plan(front_plan):
    """x_proj_eligible() (Python) against plan_x_proj() (compiled) on the parameter block x_proj() builds: yes only where the plan serves, with the kernel
    the token count implies; no where the plan serves only by one of its three policy clauses"""
    from zigma_amd import _lib
    from zigma_amd.selective_scan_interface import x_proj_eligible
    seen = set()
    for dt in (torch.bfloat16, torch.float16, torch.float32):
        for tokens in (1, 255, 256, 16383, 16384):
            for k in (64, 128, 256, 1280, 1536, 1792):
                for n in (0, 8, 96, 97):
                    for x_pitch in (k, k + 4, k + 8):
                        for w_pitch in (k, k + 4, k + 8):
                            for x_off, w_off in ((0, 0), (2, 0), (8, 0), (0, 2), (0, 8)):
                                u = _Dev(dt, tokens, k, ptr=(1 << 30) + x_off * 2, pitched=(x_pitch, 1))
                                w = _Dev(dt, n, k, ptr=(1 << 36) + w_off * 2, pitched=(w_pitch, 1))
                                P = _lib.XProjParams()
                                P.m, P.n, P.k, P.dtype = tokens, n, k, _TORCH_ID[dt]
                                P.x_row_stride, P.w_row_stride, P.out_row_stride = u.stride(0), w.stride(0), n
                                P.x, P.w, P.out = u.data_ptr(), w.data_ptr(), 1 << 40
                                policy = {"tokens >= 256": tokens < 256, "tokens >= 16384 or k <= 1536": tokens < 16384 and k > 1536,
                                          "u.is_contiguous()": x_pitch != k}
                                kernels = ("x_proj_splitk",) if tokens < 16384 else ("x_proj_mfma",)
                                _sweep_verdict(x_proj_eligible(u, w), front_plan(P), kernels, policy, (dt, tokens, k, n, x_pitch, w_pitch, x_off, w_off), seen)
    assert seen == {True, False, "tokens >= 256", "tokens >= 16384 or k <= 1536", "u.is_contiguous()"}, seen


def test_dt_proj_eligible_agrees_with_the_plan(front_plan):
    """dt_proj_eligible() (Python) against plan_dt_proj() (compiled) on the parameter block dt_proj_softplus() builds: the predicate has no policy
    clause, so it says yes exactly where the plan serves"""
    from zigma_amd import _lib
    from zigma_amd.selective_scan_interface import dt_proj_eligible
    seen = set()
    for dt in (torch.bfloat16, torch.float16, torch.float32):
        for tokens in (1, 512, 513):
            for R in (0, 4, 8, 40, 48, 56):
                for Di in (64, 96, 1280):
                    for width in (R + 32, R + 36, R + 40):
                        for w_pitch in (R, R + 4, R + 8):
                            for x_off, w_off in ((0, 0), (2, 0), (8, 0), (0, 2), (0, 8)):
                                x_dbl = _Dev(dt, tokens, width, ptr=(1 << 30) + x_off * 2)
                                w = _Dev(dt, Di, R, ptr=(1 << 36) + w_off * 2, pitched=(w_pitch, 1))
                                P = _lib.DtProjParams()
                                P.m, P.n, P.k, P.dtype, P.softplus = tokens, Di, R, _TORCH_ID[dt], 1
                                P.x_row_stride, P.w_row_stride, P.out_row_stride = x_dbl.stride(0), w.stride(0), Di
                                P.x, P.w, P.out, P.bias = x_dbl.data_ptr(), w.data_ptr(), 1 << 40, 1 << 42
                                _sweep_verdict(dt_proj_eligible(x_dbl, R, w), front_plan(P), ("dt_proj_softplus_mfma",), {},
                                               (dt, tokens, R, Di, width, w_pitch, x_off, w_off), seen)
    assert seen == {True, False}, seen


def test_conv_x_proj_eligible_agrees_with_the_plan(front_plan):
    """conv_x_proj_eligible() (Python) against plan_conv_x_proj() (compiled) on the parameter block conv_x_proj() builds (x_half the first half of an
    in_proj output, fresh u and x_dbl, no reset_period: the entry point has none): yes only where the plan serves; no where the plan serves only by
    CONV_X_PROJ_MIN_POSITIONS or because conv_w / conv_b / perm are not contiguous, which the parameter block cannot say"""
    from zigma_amd import _lib
    from zigma_amd.selective_scan_interface import CONV_X_PROJ_MIN_POSITIONS, conv_x_proj_eligible
    seen = set()
    offs = ((0, 0, 0, 0), (2, 0, 0, 0), (8, 0, 0, 0), (0, 2, 0, 0), (0, 8, 0, 0), (0, 0, 2, 0), (0, 0, 8, 0), (0, 0, 0, 2), (0, 0, 0, 8))
    for dt in (torch.bfloat16, torch.float16, torch.float32):
        for Bsz, L in ((1, 256), (1, 16384), (1, 16384 - 32), (64, 1024), (512, 32), (513, 32), (16, 1040), (16, 1048), (2, 8192 - 128)):
            for Di in (64, 96, 1280):
                for n in (0, 8, 12, 72, 96, 104):
                    for x_pitch in (2 * Di, 2 * Di + 4, 2 * Di + 8):
                        for w_pitch in (Di, Di + 4, Di + 8):
                            for x_off, cw_off, cb_off, w_off in offs:
                                for loose in ("", "conv_w", "conv_b", "perm") if (x_off, cw_off, cb_off, w_off) == (0, 0, 0, 0) else ("",):
                                    x = _Dev(dt, Bsz, L, Di, ptr=(1 << 30) + x_off * 2, pitched=(L * x_pitch, x_pitch, 1))
                                    cw, cb = _Dev(dt, Di, 4, ptr=(1 << 34) + cw_off * 2), _Dev(dt, Di, ptr=(1 << 35) + cb_off * 2)
                                    w = _Dev(dt, n, Di, ptr=(1 << 36) + w_off * 2, pitched=(w_pitch, 1))
                                    perm = _Dev(torch.int32, L, ptr=1 << 38)
                                    if loose:
                                        {"conv_w": cw, "conv_b": cb, "perm": perm}[loose].strides = (8, 1) if loose == "conv_w" else (2,)
                                    P = _lib.ConvXProjParams()
                                    P.batch, P.seqlen, P.dim, P.n, P.dtype = Bsz, L, Di, n, _TORCH_ID[dt]
                                    P.x_batch_stride, P.x_l_stride, P.u_batch_stride, P.u_l_stride = x.stride(0), x.stride(1), L * Di, Di
                                    P.w_row_stride, P.out_row_stride = w.stride(0), n
                                    P.x, P.conv_weight, P.conv_bias, P.w = x.data_ptr(), cw.data_ptr(), cb.data_ptr(), w.data_ptr()
                                    P.u, P.out, P.x_row_index = 1 << 40, 1 << 41, perm.data_ptr()
                                    policy = {"CONV_X_PROJ_MIN_POSITIONS": Bsz * L < CONV_X_PROJ_MIN_POSITIONS, "is_contiguous()": bool(loose)}
                                    _sweep_verdict(conv_x_proj_eligible(x, cw, cb, w, perm), front_plan(P), ("conv_x_proj_mfma",), policy,
                                                   (dt, Bsz, L, Di, n, x_pitch, w_pitch, x_off, cw_off, cb_off, w_off, loose), seen)
    assert seen == {True, False, "CONV_X_PROJ_MIN_POSITIONS", "is_contiguous()"}, seen


def test_inner_plan_rules(monkeypatch):
    """plan_inner: the front, dt and accumulate rules in their order, with the kernels' eligibility predicates patched (CPU tensors)"""
    import zigma_amd.selective_scan_interface as ssi
    bf = torch.bfloat16
    B, L, Di, R, N = 64, 1024, 1280, 40, 16
    xz, w, cb = torch.zeros(B, L, 2 * Di, dtype=bf), torch.zeros(Di, 4, dtype=bf), torch.zeros(Di, dtype=bf)
    xw, dw, A, db = torch.zeros(R + 2 * N, Di, dtype=bf), torch.zeros(Di, R, dtype=bf), torch.zeros(Di, N), torch.zeros(Di)
    seen = []
    for name in ("conv_x_proj_eligible", "x_proj_eligible", "dt_in_scan_eligible", "dt_proj_eligible"):
        monkeypatch.setattr(ssi, name, lambda *a, _n=name, **k: (seen.append(_n), True)[1])
    P = lambda xz=xz, **k: ssi.plan_inner(xz[:, :, :Di], xz[:, :, Di:], w, cb, xw, dw, A, db, **k)
    assert P() == ssi.InnerPlan("conv_x_proj", "in_scan", 0, False)
    assert P(add_to=xz[:, :, :Di]) == ssi.InnerPlan("conv_x_proj", "in_scan", 0, True)
    assert P(train=True) == ssi.InnerPlan("conv_x_proj", "linear", 0, False)
    assert P(B_proj_bias=db) == ssi.InnerPlan("conv_x_proj", "kernel", 0, False)
    assert P(delta_softplus=False) == ssi.InnerPlan("conv_x_proj", "linear", 0, False)
    seen.clear()
    assert P() == ssi.InnerPlan("conv_x_proj", "in_scan", 0, False) and seen == ["conv_x_proj_eligible", "dt_in_scan_eligible"]
    monkeypatch.setattr(ssi, "ACCUMULATE_IN_SCAN", False)
    assert P(add_to=xz[:, :, :Di]).accumulate is False
    monkeypatch.setattr(ssi, "USE_CONV_X_PROJ", False)
    assert P().front == "conv+x_proj" and P(train=True).front == "conv+linear"
    monkeypatch.setattr(ssi, "USE_X_PROJ_KERNEL", False)
    assert P().front == "conv+linear"
    small = xz[:4, :, :]                                             # 80 workgroups: the sequence split, chunks of 112 steps
    assert P(small) == ssi.InnerPlan("conv+linear", "in_split", 112, False)
    assert P(small, add_to=small[:, :, :Di]) == ssi.InnerPlan("conv+linear", "in_split", 112, False)
    assert P(small, z_preactivated=True).dt == "kernel" and P(small, train=True) == ssi.InnerPlan("conv+linear", "linear", 0, False)
    assert ssi.plan_inner(small[:, :, :Di], small[:, :, Di:], w, cb, xw, dw, A, None).dt == "kernel"
    monkeypatch.setattr(ssi, "DT_PROJ_IN_SPLIT", False)
    assert P(small) == ssi.InnerPlan("conv+linear", "kernel", 112, False)
    monkeypatch.setattr(ssi, "DT_PROJ_IN_SCAN", False)
    assert P().dt == "kernel"
    monkeypatch.setattr(ssi, "dt_proj_eligible", lambda *a: False)
    assert P().dt == "linear"


def test_differentiable_predicate():
    from zigma_amd.selective_scan_interface import differentiable
    a, b = torch.zeros(2), torch.zeros(2, requires_grad=True)
    assert not differentiable(a, None) and differentiable(a, None, b)
    with torch.no_grad():
        assert not differentiable(a, b)


def test_linear_train_fn_matches_autograd_and_slab_rule():
    """zigma_amd.wgrad: LinearTrainFn (F.linear with the slab-wise weight gradient) gives autograd's gradients; the slab rule returns a
    power of two that divides the rows into slabs of at least 256 rows (multiples of 8)."""
    from zigma_amd.wgrad import LinearTrainFn, _slabs, wgrad
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 40, 24, generator=g, requires_grad=True)
    w = torch.randn(16, 24, generator=g, requires_grad=True)
    b = torch.randn(16, generator=g, requires_grad=True)
    dy = torch.randn(3, 40, 16, generator=g)
    ref = torch.autograd.grad(torch.nn.functional.linear(x, w, b), (x, w, b), dy)
    got = torch.autograd.grad(LinearTrainFn.apply(x, w, b), (x, w, b), dy)
    for a, r in zip(got, ref):
        assert torch.allclose(a, r, rtol=1e-5, atol=1e-5)
    assert torch.allclose(wgrad(dy.reshape(-1, 16), x.detach().reshape(-1, 24)), ref[1], rtol=1e-5, atol=1e-5)
    for m, n, k in ((65536, 2560, 640), (65536, 72, 1280), (65536, 1280, 40), (4096, 512, 640), (1000, 64, 64), (256, 640, 640)):
        s = _slabs(m, n, k)
        assert s >= 1 and (s & (s - 1)) == 0 and (s == 1 or (m % s == 0 and m // s >= 256 and (m // s) % 8 == 0)), (m, n, k, s)


_LINEAR_PLAN_DRIVER = r"""
#include "linear_plan.h"
using namespace zigma;
extern "C" int plan(const zigma_linear_params_t *p, int *fields, const char **kernel) {
    const LinearPlan s = plan_linear(*p);
    fields[0] = s.status; fields[1] = s.family; fields[2] = s.pw; fields[3] = s.panels; fields[4] = s.ranges; fields[5] = s.tiles_per_xcd;
    *kernel = s.kernel;
    return s.status;
}
"""
LIN_TN, LIN_4W, LIN_WS, LIN_SM = 1, 2, 3, 4         # enum LinearFamily


@pytest.fixture(scope="module")
def linear_plan():
    """plan_linear() of zigma_amd/csrc/linear_plan.h compiled on its own with g++ (no HIP): plan(params) -> status, family, the weight-stationary
    kernel's pw / panels / ranges / tiles_per_xcd, kernel"""
    from zigma_amd import _lib
    return _plan_caller(_compile_plan(_LINEAR_PLAN_DRIVER), _lib.LinearParams, ("status", "family", "pw", "panels", "ranges", "tiles_per_xcd"))


def _linear_params(tokens, n, k, flags=0, x_pitch=None, bias=0):
    """the parameter block zigma_amd.linear.linear builds for a plain bf16 projection of aligned operands into a fresh output"""
    from zigma_amd import _lib
    P = _lib.LinearParams()
    P.m, P.n, P.k, P.dtype, P.flags, P.silu_from_col = tokens, n, k, _lib.BF16, flags, n
    P.x_row_stride, P.w_row_stride, P.out_row_stride = x_pitch or k, k, n
    P.x, P.w, P.out, P.bias = 1 << 30, 1 << 36, 1 << 40, bias or None
    return P


@pytest.mark.parametrize("name", sorted(__import__("linear_plan_cases").CASES))
def test_linear_plan_case_table(name, linear_plan):
    """plan_linear() (compiled) on the parameter block zigma_amd.linear.linear builds for every case of the table: status, last kernel"""
    import linear_plan_cases
    case, want = linear_plan_cases.CASES[name]
    got, _ = linear_plan_cases.call(case, "cpu", linear_plan)
    assert (got["status"], got["kernel"]) == tuple(want) and (got["family"] != 0) == (want.kernel is not None)


def test_linear_mirrors_agree_with_the_plan(linear_plan, libpath):
    """The Python side's answers about zigma_linear_fwd's kernel families against plan_linear() compiled with g++ from the header (independent of the built
    library the predicates ask), on the edges of every rule: for each of ws / ws128 / sm / tiled, the family's public predicate (linear_ws_eligible,
    linear_sm_eligible, linear_eligible) and routing.serves(kern) hold exactly where the plan serves the call flagged for that family (and panel width); the
    block linear_block builds for the call is, byte for byte, the block the plan was asked about; routing.kernel_name is a prefix of the plan's kernel on every
    served cell (contiguous out, tokens * n * 2 < 2^32; a bias alone is passed on).  Then the rules that stay in Python, one by one."""
    from zigma_amd import linear as zl, routing as zr
    bf = torch.bfloat16
    flags = {"ws": zl.LINEAR_WS_FLAG, "ws128": zl.LINEAR_WS_FLAG, "sm": zl.LINEAR_SM_FLAG, "tiled": 0}
    eligible = {"ws": zl.linear_ws_eligible, "ws128": zl.linear_ws_eligible, "sm": zl.linear_sm_eligible, "tiled": zl.linear_eligible}
    served_by = {"ws": lambda pl: pl["family"] == LIN_WS and pl["pw"] == 256, "ws128": lambda pl: pl["family"] == LIN_WS and pl["pw"] == 128,
                 "sm": lambda pl: pl["family"] == LIN_SM, "tiled": lambda pl: pl["family"] in (LIN_TN, LIN_4W)}
    seen = {kern: set() for kern in flags}
    with torch.no_grad():
        for tokens in (8, 104, 128, 256, 512, 8192, 65536 + 8):
            for n in (128, 384, 640, 4096, 8192, 8320):
                for k in (64, 128, 192, 640, 768, 1280, 1536):
                    w = _Dev(bf, n, k, ptr=1 << 36)
                    for pitch in (k, k + 4, k + 8, k + 128):
                        x = _Dev(bf, tokens, k, ptr=1 << 30, pitched=(pitch, 1))
                        for bias_ptr in (0, 1 << 42, (1 << 42) + 4, (1 << 42) + 2):      # absent, or on a 16- / 4- / 2-byte boundary
                            bias = _Dev(bf, n, ptr=bias_ptr) if bias_ptr else None
                            assert tokens * n * 2 < 1 << 32
                            for kern, flag in flags.items():
                                P = _linear_params(tokens, n, k, flag, pitch, bias_ptr)
                                assert bytes(zl.linear_block(x, w, bias, flags=flag)) == bytes(P)
                                pl = linear_plan(P)
                                served = pl["status"] == 0 and served_by[kern](pl)
                                mirror = eligible[kern](x, w, bias) and zr.serves(kern, tokens, n, k)
                                assert mirror == served, (kern, tokens, n, k, pitch, bias_ptr, pl)
                                seen[kern].add(served)
                                if served:
                                    name = zr.kernel_name(kern, tokens, n, k, bias=bias is not None, residual=False)
                                    assert pl["kernel"].startswith(name), (kern, tokens, n, k, pitch, bias_ptr, pl, name)
                                if pitch == k and not bias_ptr:        # the canonical call of the shape: routing.serves is the plan's answer alone
                                    assert zr.serves(kern, tokens, n, k) == served, (kern, tokens, n, k, pl)
        assert all(v == {True, False} for v in seen.values()), seen
        # what a block cannot say: each rule on a call that every predicate accepts without it
        x, w, b = _Dev(bf, 8, 1024, 640), _Dev(bf, 2560, 640, ptr=1 << 36), _Dev(bf, 2560, ptr=1 << 42)
        ok = lambda x=x, w=w, b=b: zl.linear_eligible(x, w, b) and zl.linear_ws_eligible(x, w, None) and zl.linear_sm_eligible(x, w, b)
        assert ok()
        assert not ok(x=_Dev(bf, 8, 1024, 640, cuda=False))                                                      # the device
        assert not ok(w=_Dev(torch.float16, 2560, 640, ptr=1 << 36)) and not ok(b=_Dev(torch.float16, 2560, ptr=1 << 42))          # one dtype
        assert not ok(x=_Dev(bf, 8, 1024, 640, pitched=(1024 * 1280, 1280, 2))) and not ok(w=_Dev(bf, 2560, 640, ptr=1 << 36, pitched=(1280, 2)))   # unit channel stride
        assert not ok(b=_Dev(bf, 2560, ptr=1 << 42, pitched=(2,)))                                              # bias stride
        assert not ok(x=_Dev(bf, 8, 1024, 640, pitched=(1024 * 768, 768, 1))) and ok(x=_Dev(bf, 8192, 640, pitched=(768, 1)))       # a > 2-D x must be contiguous
        assert not ok(w=_Dev(bf, 2560, 768, ptr=1 << 36))                                                       # x and weight share k
        # ... and of the gated residual: one dtype, residual rows of all samples in one pitch, unit channel strides, (B, rows, k) input
        res, gate = _Dev(bf, 8, 1024, 2560, ptr=1 << 44), _Dev(bf, 8, 2560, ptr=1 << 45)
        gated = lambda x=x, res=res, gate=gate: zl.gated_residual_eligible(x, res, gate)
        assert gated() and not gated(x=_Dev(bf, 8192, 640)) and not gated(res=_Dev(torch.float16, 8, 1024, 2560, ptr=1 << 44))
        assert not gated(gate=_Dev(torch.float16, 8, 2560, ptr=1 << 45)) and not gated(res=_Dev(bf, 8, 1024, 2560, ptr=1 << 44, pitched=(1025 * 2560, 2560, 1)))
        assert not gated(res=_Dev(bf, 8, 1024, 2560, ptr=1 << 44, pitched=(1024 * 5120, 5120, 2))) and not gated(gate=_Dev(bf, 8, 2560, ptr=1 << 45, pitched=(5120, 2)))
        assert gated(res=_Dev(bf, 8, 1024, 2560, ptr=1 << 44, pitched=(1024 * 2568, 2568, 1))) and not gated(res=_Dev(bf, 8, 1024, 2560, ptr=(1 << 44) + 8))
    grad = _Dev(bf, 8, 1024, 640)
    grad.requires_grad = True
    with torch.enable_grad():
        assert ok() and not ok(x=grad)                                                                           # the autograd rule
    with torch.no_grad():
        assert ok(x=grad)


@pytest.mark.parametrize("m,n", [(65536, 2560), (65536, 512), (32768, 2560), (4096, 8192), (5632, 1024), (512 * 43, 256), (16384, 1280)])
def test_linear_ws_work_partition_covers_every_tile_once(m, n, linear_plan):
    """The workgroup -> (panel, token range) assignment of csrc/linear_ws.hip on the panels / ranges / tiles_per_xcd plan_linear() (compiled) launches
    it with: XCD x = blockIdx % 8 owns the x-th eighth of the 64-token
    tiles, slot = blockIdx / 8 -> panel = slot % panels, range = slot / panels, the range's tiles split as evenly as integers allow.  Every
    (panel, tile) pair must be computed by exactly one workgroup, ranges must be non-empty, and the per-workgroup tile counts of one launch
    may differ by at most one (the kernel's load balance)."""
    from zigma_amd.linear import LINEAR_WS_FLAG
    pl = linear_plan(_linear_params(m, n, 640, LINEAR_WS_FLAG))
    assert pl["status"] == 0 and pl["kernel"] == "linear_ws"
    panels, ranges, tiles_per_xcd = pl["panels"], pl["ranges"], pl["tiles_per_xcd"]
    assert tiles_per_xcd >= ranges
    seen, counts = {}, []
    for block in range(256):
        xcd, slot = block & 7, block >> 3
        if slot >= panels * ranges:
            continue
        panel, rng = slot % panels, slot // panels
        t_lo = xcd * tiles_per_xcd + (rng * tiles_per_xcd) // ranges
        t_hi = xcd * tiles_per_xcd + ((rng + 1) * tiles_per_xcd) // ranges
        assert t_hi > t_lo
        counts.append(t_hi - t_lo)
        for t in range(t_lo, t_hi):
            assert (panel, t) not in seen
            seen[(panel, t)] = block
    assert len(seen) == panels * (m // 64)
    assert max(counts) - min(counts) <= 1


_OUTER_PLAN_DRIVER = r"""
#include "outer_plan.h"
#include "attn_plan.h"
#include "wgrad_plan.h"
using namespace zigma;
static int outer(const OuterPlan &s, int *f, const char **kernel) {
    f[0] = s.status; f[1] = s.gx; f[2] = s.gy; f[3] = 1; f[4] = s.block; f[5] = int(s.lds); f[6] = s.inst; f[7] = s.silu;
    *kernel = s.kernel;
    return s.status;
}
static int attn(const AttnPlan &s, int *f, const char **kernel) {
    f[0] = s.status; f[1] = s.gx; f[2] = s.gy; f[3] = s.gz; f[4] = s.block; f[5] = 0; f[6] = s.nkb; f[7] = s.masked; f[8] = s.tiles; f[9] = s.chunks; f[10] = s.has_r2;
    *kernel = s.kernel;
    return s.status;
}
extern "C" int plan_pe(const zigma_patch_embed_params_t *p, int *f, const char **k) { return outer(plan_patch_embed(*p), f, k); }
extern "C" int plan_te(const zigma_timestep_embed_params_t *p, int *f, const char **k) { return outer(plan_timestep_embed(*p), f, k); }
extern "C" int plan_sk(const zigma_skinny_params_t *p, int *f, const char **k) { return outer(plan_skinny_linear(*p), f, k); }
extern "C" int plan_fl(const zigma_final_layer_params_t *p, int *f, const char **k) { return outer(plan_final_layer(*p), f, k); }
extern "C" int plan_cfg(const zigma_final_layer_cfg_params_t *p, int *f, const char **k) { return outer(plan_final_layer_cfg(*p), f, k); }
extern "C" int plan_xa(const zigma_xattn_params_t *p, int *f, const char **k) { return attn(plan_cross_attn(*p), f, k); }
extern "C" int plan_xb(const zigma_xattn_bwd_params_t *p, int *f, const char **k) { return attn(plan_cross_attn_bwd(*p), f, k); }
extern "C" int plan_gb(const zigma_glue_bwd_params_t *p, int *f, const char **k) { return attn(plan_scale_reduce_bwd(*p), f, k); }
extern "C" int plan_wg(const zigma_linear_wgrad_params_t *p, int *f, const char **kernel) {
    const WgradPlan s = plan_wgrad(*p);
    f[0] = s.status; f[1] = s.gx; f[2] = s.gy; f[3] = 1; f[4] = s.block; f[5] = int(s.need); f[6] = s.bk; f[7] = s.slabs; f[8] = int(s.slab_rows); f[9] = s.n_tiles;
    *kernel = s.kernel;
    return s.status;
}
extern "C" int chunks(int seqlen) { return attn_bwd_chunks(seqlen); }
"""
_OUTER_FIELDS = ("status", "gx", "gy", "gz", "block", "bytes", "inst", "switch", "tiles", "chunks", "has_r2")       # (inst / switch: K | NP | k / 32, SiLU; NKB, masked; bk, slabs)


@pytest.fixture(scope="module")
def outer_plan():
    """the nine plans of zigma_amd/csrc/outer_plan.h, attn_plan.h and wgrad_plan.h compiled on their own with g++ (no HIP): plan(params) -> status, grid,
    block, LDS / workspace bytes, switches, kernel, by the type of the parameter block"""
    from zigma_amd import _lib
    L = _compile_plan(_OUTER_PLAN_DRIVER)
    by_type = {t: _plan_caller(L, t, _OUTER_FIELDS, fn) for t, fn in (
        (_lib.PatchEmbedParams, "plan_pe"), (_lib.TimestepEmbedParams, "plan_te"), (_lib.SkinnyParams, "plan_sk"), (_lib.FinalLayerParams, "plan_fl"),
        (_lib.FinalLayerCfgParams, "plan_cfg"), (_lib.XAttnParams, "plan_xa"), (_lib.XAttnBwdParams, "plan_xb"), (_lib.GlueBwdParams, "plan_gb"),
        (_lib.LinearWgradParams, "plan_wg"))}
    plan = lambda P: by_type[type(P)](P)
    plan.chunks = L.chunks
    return plan


def test_outer_plan_case_table(outer_plan, libpath):
    """the nine plans (compiled) on the parameter block the product's builders fill for every case of the table: status, last kernel; and the built
    library's host-only queries (no device here) answer the same.  Every case in ONE test (the table has 212 of them): all that differ are reported
    together; tests/test_gpu_outer_plan_query.py runs them one by one."""
    import outer_plan_cases as oc
    from zigma_amd import _lib
    wrong = {}
    for name, (_, _, want) in oc.CASES.items():
        fn, P, _ = oc.block(name, "cpu")
        got = outer_plan(P)
        if not (got["status"], got["kernel"]) == tuple(want) == _lib.plan(fn, P):
            wrong[name] = (got["status"], got["kernel"], _lib.plan(fn, P), tuple(want))
    assert not wrong, wrong
    assert {c[0] for c in oc.CASES.values()} == set(oc.ENTRY) and len(oc.ENTRY) == 9


def test_outer_plan_geometry(outer_plan):
    """grid, block, dynamic LDS / workspace bytes and template switches of the serving leaves against the closed forms of the kernels' headers"""
    import outer_plan_cases as oc

    def geometry(name, *fields):
        got = outer_plan(oc.block(name, "cpu")[1])
        return tuple(got[f] for f in fields)
    pe = ("gx", "gy", "block", "bytes", "inst")
    assert [geometry(f"pe_served_{k}", *pe) for k in ("K16", "K3", "K4_no_bias_no_pos", "K12", "K8_any", "weight_64KB")] == [
        (1, 2, 256, 16 * 64 * 4, 16), (4, 2, 256, 3 * 64 * 4, 3), (4, 2, 256, 4 * 64 * 4, 4), (1, 2, 256, 12 * 64 * 4, 12), (1, 2, 256, 8 * 64 * 4, 0),
        (1, 2, 256, 65536, 0)]
    # 4096 tokens = 256 workgroups of 16 tokens at most: 1024 / 64 / 16 per sample below 8 / below 64 / from 64 samples
    assert [geometry(f"pe_served_batch_{b}", "gx", "gy") for b in (7, 8, 63, 64)] == [(256, 7), (64, 8), (64, 63), (16, 64)]
    assert geometry("te_served", "gx", "block") == (1, 256) and geometry("te_served_257_pairs", "gx", "block") == (2, 256)
    sk = ("gx", "block", "bytes", "inst", "switch")
    assert geometry("sk_served_k128_m1", *sk) == (1, 512, 64 * 136 * 2, 4, 0) and geometry("sk_served_k128_m64_silu", *sk) == (1, 512, 64 * 136 * 2, 4, 1)
    assert geometry("sk_served_k1024_m1_silu_no_bias", *sk) == (1, 512, 64 * 1032 * 2, 32, 1) and geometry("sk_served_k1024_m64", *sk) == (1, 512, 64 * 1032 * 2, 32, 0)
    assert geometry("sk_served_out_plus_8_bytes_n_4112", "gx") == (33,)
    for entry, rows in (("fl", 5), ("cfg", 8)):
        got = [geometry(f"{entry}_served_cols_{c}_n_out_{n}", "gx", "block", "bytes", "inst") for c, n in ((8, 1), (640, 16), (648, 3), (1024, 1), (1032, 16), (2048, 16))]
        assert got == [(1, 256, 8 * 1 * 2, 5), (1, 256, 640 * 16 * 2, 5), (1, 256, 648 * 3 * 2, 8), (1, 256, 1024 * 2, 8), (1, 256, 1032 * 16 * 2, 16),
                       (1, 256, 2048 * 16 * 2, 16)], (entry, rows)
    assert geometry("fl_served_no_bias_17_rows", "gx") == (2,)
    xa = ("gx", "gy", "gz", "block", "inst", "switch", "tiles")
    assert [geometry(f"xa_served_n_ctx_{n}", *xa) for n in (1, 64, 65, 80, 81, 112, 113, 128)] == [
        (1, 2, 2, 256, nkb, masked, 4) for nkb, masked in ((5, 1), (5, 1), (5, 0), (5, 0), (8, 1), (8, 1), (8, 0), (8, 0))]
    assert geometry("xa_served_f16_511_tokens", *xa) == (2, 2, 1, 256, 5, 0, 4) and geometry("xa_served_512_tokens_kv_halves", *xa) == (1, 2, 1, 256, 5, 0, 8)
    xb = ("gx", "gy", "gz", "block", "inst", "tiles", "chunks")
    assert [geometry(f"xb_served_n_ctx_{n}", *xb) for n in (1, 80, 81, 128)] == [(1, 2, 2, 256, nkb, 4, 1) for nkb in (5, 5, 8, 8)]
    assert geometry("xb_served_511_tokens", *xb) == (2, 2, 1, 256, 5, 4, 2) and geometry("xb_served_513_tokens_kv_halves", *xb) == (2, 2, 1, 256, 5, 8, 2)
    gb = ("gx", "block", "has_r2")
    assert geometry("gb_served_cols_128_both_sums", *gb) == (2, 256, 1) and geometry("gb_served_cols_128_one_sum_no_out", *gb) == (2, 256, 0)
    assert geometry("gb_served_cols_8192_both_sums", *gb) == (1, 256, 1) and geometry("gb_served_cols_8192_one_sum_s_a_third_of_its_rows", *gb) == (1, 256, 0)
    wg = ("gx", "gy", "block", "bytes", "inst", "switch", "tiles", "chunks")      # tiles, slabs, threads, workspace bytes, bk, S, slab_rows, n_tiles
    assert geometry("wg_served_k64_m511", *wg) == (1, 1, 256, 0, 64, 1, 512, 1) and geometry("wg_served_k72_m512", *wg) == (1, 1, 256, 0, 128, 1, 512, 1)
    assert geometry("wg_served_k64_m1024_two_slabs", *wg) == (1, 2, 256, 2 * 16 * 64 * 4, 64, 2, 512, 1)
    assert geometry("wg_served_k72_m1024_f16", *wg) == (1, 2, 256, 2 * 16 * 72 * 4, 128, 2, 512, 1)
    assert geometry("wg_served_forced_3_slabs_fp32_out", *wg) == (1, 3, 256, 3 * 16 * 64 * 4, 64, 3, 64, 1)
    assert geometry("wg_served_fp32_out_pitch_68_x_a_column_view", *wg) == (1, 1, 256, 0, 128, 1, 64, 1)


def test_outer_predicates_agree_with_the_plans_and_the_parent_commit(outer_plan, libpath):
    """each of the nine predicates over its sweep (tests/outer_predicate_cases.py): a yes is served by the compiled plan with the expected kernel, on the
    block the product's builder fills; a no that the plan would serve is explained by a clause Python keeps for itself; every clause and both verdicts are
    seen.  The answers are the ones recorded on the parent commit, but for the listed exceptions (a yes of the parent to a block the library does not
    launch).  That allow-list is small: at most 2 % of the recorded points, and it is exactly the points where the parent's hand-written predicates said
    yes to a block the compiled plans do not launch.  All nine in ONE test, like the 551 routes of test_linear_route_cases.py."""
    import importlib
    import outer_predicate_cases as pc
    total = unserved = 0
    for which, (module, _, builder, _, sweep) in pc.SWEEPS.items():
        builder = getattr(importlib.import_module("zigma_amd." + module), builder)
        got, recorded = pc.answers(which), "".join(pc.RECORDED[which])
        points, seen, clauses = list(sweep()), set(), set()
        assert len(points) == len(got) == len(recorded), which
        total += len(points)
        for (point, args, kwargs, policy, kernels), eligible, was in zip(points, got, recorded):
            a, k = pc.block_args(which, args, kwargs)
            pl = outer_plan(builder(*a, **k))
            _sweep_verdict(eligible, pl, kernels, policy, (which, point), seen)
            clauses |= set(policy)
            unserved += was == "1" and pl["kernel"] is None
            if eligible != (was == "1"):
                assert was == "1" and (which, point) in pc.EXCEPTIONS and pl["kernel"] is None, (which, point, "the recorded answer", was, "now", eligible, pl)
            else:
                assert (which, point) not in pc.EXCEPTIONS, (which, point, "a listed exception that is none")
        assert seen == {True, False} | clauses, (which, seen, clauses)
    assert {w for w, _ in pc.EXCEPTIONS} <= set(pc.SWEEPS)
    assert unserved == len(pc.EXCEPTIONS) <= pc.MAX_EXCEPTIONS * total, (unserved, len(pc.EXCEPTIONS), total)


def test_chunks_and_workspace_bytes_answer_as_the_plans_do(outer_plan, libpath):
    """zigma_cross_attn_bwd_chunks and zigma_linear_wgrad_workspace_bytes are the fields of plan_cross_attn_bwd() / plan_wgrad()"""
    import outer_plan_cases as oc
    from zigma_amd import _lib
    L = _lib.lib()
    for seqlen in (-1, 0, 1, 255, 256, 257, 511, 512, 513, 1024, 1025, 65536):
        assert L.zigma_cross_attn_bwd_chunks(seqlen) == outer_plan.chunks(seqlen) == (0 if seqlen <= 0 else -(-seqlen // (256 if seqlen < 512 else 512)))
    for name in (n for n, c in oc.CASES.items() if c[0] == "cross_attn_bwd" and c[2].kernel):
        P = oc.block(name, "cpu")[1]
        assert outer_plan(P)["chunks"] == P.chunks == L.zigma_cross_attn_bwd_chunks(P.seqlen)
    for name in (n for n, c in oc.CASES.items() if c[0] == "linear_wgrad"):
        P = oc.block(name, "cpu")[1]
        pl = outer_plan(P)
        assert L.zigma_linear_wgrad_workspace_bytes(ctypes.byref(P)) == pl["bytes"] == (pl["switch"] * P.n * P.k * 4 if pl["switch"] > 1 else 0), name
    for m, n, k, slabs in ((65536, 2560, 640, 0), (65536, 72, 1280, 0), (4096, 640, 1280, 0), (512, 8, 8, 0), (100, 8192, 8192, 7), (1, 8, 8, 4096)):
        P = _lib.LinearWgradParams()
        P.m, P.n, P.k, P.slabs, P.dtype, P.out_dtype = m, n, k, slabs, _lib.BF16, _lib.BF16          # (no operands: the size is asked before they exist)
        pl = outer_plan(P)
        assert pl["status"] == -1 and L.zigma_linear_wgrad_workspace_bytes(ctypes.byref(P)) == pl["bytes"] == (pl["switch"] * n * k * 4 if pl["switch"] > 1 else 0)
        assert pl["switch"] == (slabs or max(1, min(64, m // 512, -(-512 // (-(-n // 128) * -(-k // (64 if k <= 64 else 128)))))))


_BWD_PLAN_DRIVER = r"""
#include "norm_plan.h"
#include "bwd_plan.h"
using namespace zigma;
static int norm(const NormPlan &s, int64_t *f, const char **kernel) {
    f[0] = s.status; f[1] = s.gx; f[2] = 1; f[3] = 1; f[4] = s.block; f[5] = s.need; f[6] = s.vec; f[7] = s.iters; f[8] = s.lpr; f[9] = s.res32; f[10] = s.w32; f[11] = s.fin_gx;
    *kernel = s.kernel;
    return s.status;
}
static int bwd(const BwdPlan &s, int64_t *f, const char **kernel) {
    f[0] = s.status; f[1] = s.gx; f[2] = s.gy; f[3] = s.gz; f[4] = s.block; f[5] = s.need; f[6] = s.inst; f[7] = s.silu; f[8] = s.io; f[9] = s.wt; f[10] = s.n_tiles + s.n_seg;
    f[11] = s.fin_gx; f[12] = s.fin2_gx; f[13] = s.n_slabs + s.n_parts; f[14] = s.ck; f[15] = s.bc; f[16] = s.pa;
    *kernel = s.kernel;
    return s.status;
}
extern "C" int plan_an(const zigma_norm_params_t *p, int64_t *f, const char **k) { return norm(plan_add_norm(*p), f, k); }
extern "C" int plan_nb(const zigma_norm_bwd_params_t *p, int64_t *f, const char **k) { return norm(plan_add_norm_bwd(*p), f, k); }
extern "C" int plan_sb(const zigma_scan_bwd_params_t *p, int64_t *f, const char **k) { return bwd(plan_scan_bwd(*p), f, k); }
extern "C" int plan_cb(const zigma_conv_bwd_params_t *p, int64_t *f, const char **k) { return bwd(plan_conv_bwd(*p), f, k); }
extern "C" int max_batch() { return kBwdMaxBatch; }
"""
_NORM_FIELDS = ("status", "gx", "gy", "gz", "block", "need", "vec", "iters", "lpr", "res32", "w32", "fin_gx")
_BWD_FIELDS = ("status", "gx", "gy", "gz", "block", "need", "inst", "silu", "io", "wt", "pieces", "fin_gx", "fin2_gx", "parts", "ck", "bc", "pa")   # pieces: tiles | segments; parts: slabs | partials


@pytest.fixture(scope="module")
def bwd_plan():
    """the four plans of zigma_amd/csrc/norm_plan.h and bwd_plan.h compiled on their own with g++ (no HIP): plan(params) -> status, grids, block,
    workspace bytes, instantiation, kernel, by the type of the parameter block"""
    from zigma_amd import _lib
    L = _compile_plan(_BWD_PLAN_DRIVER)
    by_type = {t: _plan_caller(L, t, names, fn, ctypes.c_int64) for t, fn, names in (
        (_lib.NormParams, "plan_an", _NORM_FIELDS), (_lib.NormBwdParams, "plan_nb", _NORM_FIELDS), (_lib.ScanBwdParams, "plan_sb", _BWD_FIELDS),
        (_lib.ConvBwdParams, "plan_cb", _BWD_FIELDS))}
    plan = lambda P: by_type[type(P)](P)
    plan.max_batch = L.max_batch()
    return plan


def _bwd_plan_case_table(bwd_plan):
    """the four plans (compiled) on the parameter block the product's builders fill for every case of the table: status, last kernel, and for add-norm
    the instantiation; the built library's host-only queries (no device here) answer the same.  Every case in ONE test: all that differ are reported
    together; tests/test_gpu_bwd_plan_query.py runs them one by one."""
    import bwd_plan_cases as bc
    from zigma_amd import _lib
    wrong = {}
    for name, (_, _, want) in bc.CASES.items():
        fn, P, _, _ = bc.block(name, "cpu")
        got = bwd_plan(P)
        if not (got["status"], got["kernel"]) == tuple(want) == _lib.plan(fn, P):
            wrong[name] = (got["status"], got["kernel"], _lib.plan(fn, P), tuple(want))
        elif name in bc.INSTANTIATION and (got["vec"], got["iters"], got["lpr"]) != bc.INSTANTIATION[name]:
            wrong[name] = (got["vec"], got["iters"], got["lpr"])
    assert not wrong, wrong
    assert {c[0] for c in bc.CASES.values()} == set(bc.ENTRY) and len(bc.ENTRY) == 4
    assert set(bc.INSTANTIATION) == {n for n, c in bc.CASES.items() if c[2].kernel and c[0].startswith("add_norm")}


def _bwd_plan_geometry(bwd_plan):
    """grids, blocks, dtype slots, template switches and workspace sections of the serving leaves against the closed forms of the kernels' headers"""
    import bwd_plan_cases as bc

    def geometry(name, *fields):
        got = bwd_plan(bc.block(name, "cpu")[1])
        return tuple(got[f] for f in fields)
    an = ("gx", "block", "res32", "w32")
    assert geometry("an_served_rows_4_cols_128", *an) == (1, 256, 0, 0) and geometry("an_served_rows_5_cols_128", *an) == (2, 256, 0, 0)      # 16 rows | 4 rows per workgroup
    assert geometry("an_served_full_fp32_residual", *an) == (1, 256, 1, 0) and geometry("an_served_full_fp32_residual_fp32_weight_f16", *an) == (1, 256, 1, 1)
    assert geometry("an_served_fp32_weight_16_bytes_in", *an) == (1, 256, 0, 1) and geometry("an_served_f32", *an) == (1, 256, 1, 1)
    nb = ("gx", "block", "fin_gx", "need", "res32", "w32")
    assert geometry("nb_served_cols_768", *nb) == (2, 256, 24, 2 * 2 * 768 * 4, 1, 0) and geometry("nb_served_cols_772", *nb) == (2, 256, 26, 2 * 2 * 772 * 4, 1, 0)
    assert geometry("nb_served_2049_rows_of_8_f16_no_weight_dx_only", *nb) == (512, 256, 2, 512 * 2 * 8 * 4, 0, 0)
    assert geometry("nb_served_f32_dresidual_only", "res32", "w32") == (1, 1)
    sb = ("gx", "gy", "block", "inst", "io", "pieces", "parts", "fin_gx", "fin2_gx", "ck", "bc", "pa", "need")
    from zigma_amd._lib import BF16, F16, F32
    assert geometry("sb_served_16_states", *sb) == (1, 2, 256, 4, BF16, 2, 1, 8, 5, 2 * 2 * 16 * 64, 2 * 32 * 2 * 16, 2 * 64 * 18, (4096 + 2048 + 2304) * 4)
    assert geometry("sb_served_8_states", *sb) == (1, 2, 128, 2, BF16, 2, 1, 4, 3, 2 * 2 * 8 * 64, 2 * 32 * 2 * 8, 2 * 64 * 10, (2048 + 1024 + 1280) * 4)
    assert geometry("sb_served_8_states_forward_checkpoints", "ck", "need") == (0, (1024 + 1280) * 4)
    assert geometry("sb_served_f32_33_steps", *sb) == (1, 2, 256, 4, F32, 3, 1, 9, 5, 2 * 3 * 16 * 64, 2 * 48 * 2 * 16, 2 * 64 * 18, (6144 + 3072 + 2304) * 4)
    assert geometry("sb_served_f16_reset_period_16", "io", "inst") == (F16, 4)
    cb = ("gx", "gy", "gz", "block", "inst", "silu", "io", "wt", "pieces", "parts", "fin_gx", "need")
    assert geometry("cb_served_width_4_silu_bias", *cb) == (1, 1, 2, 64, 4, 1, BF16, BF16, 1, 2, 1, 2 * 8 * 5 * 4)
    assert geometry("cb_served_width_3_no_silu", *cb) == (1, 1, 2, 64, 3, 0, BF16, BF16, 1, 2, 1, 2 * 8 * 4 * 4)
    assert geometry("cb_served_width_2_no_bias_fp32_taps", *cb) == (1, 1, 2, 64, 2, 1, BF16, F32, 1, 2, 1, 2 * 8 * 3 * 4)
    assert geometry("cb_served_f16_width_4_no_silu_fp32_taps", "inst", "silu", "io", "wt") == (4, 0, F16, F32)
    assert geometry("cb_served_129_positions_row_table", *cb) == (1, 2, 2, 64, 4, 1, BF16, BF16, 2, 4, 1, 2 * 2 * 8 * 5 * 4)


def _norm_case_block(c, lead, tail, pitch, windows):
    """the block tests/test_gpu_outer_fwd.py builds for a case of outer_fwd_cases.norm_cases(), on allocator-aligned placeholder addresses"""
    import outer_fwd_cases as oc
    from zigma_amd import _lib
    ids, es = {"f32": _lib.F32, "f16": _lib.F16, "bf16": _lib.BF16}, {"f32": 4, "f16": 2, "bf16": 2}
    u, at = oc.norm_uses(c), lead + c["align"]
    P = _lib.NormParams()
    P.rows, P.cols, P.rows_per_batch, P.flags = c["rows"], c["cols"], c["rpb"], c["flags"]
    P.x_dtype, P.res_dtype, P.w_dtype, P.mod_dtype = ids[c["xk"]], ids[c["rk"]], ids[c["wk"]], ids[c["xk"]]
    k = [0]

    def put(field, kind, stride=None):
        k[0] += 1
        setattr(P, field, k[0] * _lib.FRESH_ADDRESS + at * es[kind])
        if stride:
            setattr(P, stride, pitch)
    put("x", c["xk"], "x_row_stride")
    for use, field, kind, stride in (("branch", "branch", c["xk"], "branch_row_stride"), ("x_out", "x_out", c["xk"], "x_out_row_stride"),
                                     ("res", "residual", c["rk"], "res_row_stride"), ("res_out", "residual_out", c["rk"], "res_out_row_stride"),
                                     ("y_out", "y_out", c["xk"], "y_row_stride")):
        if u[use]:
            put(field, kind, stride)
    if c["form"] != "ln":
        put("weight", c["wk"])
    if c["form"] == "ln-wb":
        put("bias", c["wk"])
    if u["branch"] or u["mod"]:
        base = 20 * _lib.FRESH_ADDRESS + at * es[c["xk"]]
        P.mod_batch_stride = lead + c["align"] + 6 * c["cols"] + tail
        if u["mod"]:
            put("y_mod", c["xk"], "y_mod_row_stride")
            P.shift, P.scale = (base + w * c["cols"] * es[c["xk"]] for w in windows[:2])
        if u["branch"]:
            P.gate = base + windows[2] * c["cols"] * es[c["xk"]]
    return P, [es[c["xk"]], es[c["rk"]], es[c["wk"]], es[c["xk"]]]


def _add_norm_plan_agrees_with_both_hand_restatements(bwd_plan):
    """plan_add_norm()'s (VEC, ITERS, LPR) and kernel name against the two independent restatements of the selection the tests keep —
    kernel_standins._norm_instantiation (from a block) and outer_fwd_cases.norm_branch (from a case) — on every case of outer_fwd_cases.norm_cases() and on
    a seeded sweep of 4000 blocks: cols 1 ... 4200, every pitch and offset residue mod 8, every dtype slot; on its first half every operand shares one
    offset (a case of norm_branch), on its second every pointer and pitch draws its own"""
    import kernel_standins as ks
    import outer_fwd_cases as oc
    from zigma_amd import _lib

    def check(P, es, c=None):
        got = bwd_plan(P)
        try:
            inst, name = ks._norm_instantiation(P, es)
        except Exception:
            inst, name = None, None
        assert ((got["vec"], got["iters"], got["lpr"]) if got["kernel"] else None, got["kernel"]) == (inst, name), (c, got, inst, name)
        if c is not None:
            assert oc.norm_branch(c) == inst and (inst is None or oc.norm_kernel_name(c) == name), (c, inst, name)
        return inst
    seen = set()
    for c in oc.norm_cases():
        P, es = _norm_case_block(c, oc.LEAD, oc.TAIL, oc.norm_pitch(c), oc.MOD_WINDOWS)
        assert check(P, es, c) == c["branch"]
        seen.add(c["branch"])
    rng = np.random.default_rng(20251)
    kinds = [(x, r, w) for x in ("f32", "bf16", "f16") for r in ("f32", x) for w in ("f32", x)]
    for i in range(4000):
        xk, rk, wk = kinds[i % len(kinds)]
        cols = int(rng.integers(1, 4201)) if i % 4 else int(rng.integers(1, 34)) * 128
        c = dict(xk=xk, rk=rk, wk=wk, cols=cols, rows=int(rng.integers(1, 9)), rpb=1, flags=int(rng.integers(0, 2)) if i % 8 == 0 else 0,
                 align=int(rng.integers(0, 8)) if i % 3 else 0, form=oc.NORM_FORMS[i % 4], opt=oc.NORM_OPTIONS[i % 9])
        P, es = _norm_case_block(c, oc.LEAD, oc.TAIL, oc.norm_pitch(c), oc.MOD_WINDOWS)
        if i < 2000:
            seen.add(check(P, es, c))
            continue
        for field, ctype in P._fields_:           # every pointer in use and every pitch: its own residue mod 8 elements
            if ctype is _lib.vp and getattr(P, field):
                setattr(P, field, getattr(P, field) + int(rng.integers(0, 8)) * es[{"residual": 1, "residual_out": 1, "weight": 2, "bias": 2}.get(field, 0)] * (i % 2))
            elif field.endswith("_stride"):
                setattr(P, field, getattr(P, field) + int(rng.integers(0, 8)) * (i % 3 == 0))
        seen.add(check(P, es))
    assert seen == {None, (8, 2, 64), (4, 4, 64), (4, 16, 64), (1, 16, 64), (1, 64, 64)} | {(8, it, 16) for it in range(1, 9)}


def _add_norm_bwd_plan_agrees_with_the_recorded_selection(bwd_plan):
    """plan_add_norm_bwd()'s (VEC, ITERS) against bwd_fuzz_cases.norm_branch — the selection the backward sweep records per case — on every case of its table
    and on a seeded sweep: cols 1 ... 2100, every pitch pad mod 8, every dtype slot"""
    import bwd_fuzz_cases as fc
    from zigma_amd import _lib
    ids, es = {"f32": _lib.F32, "f16": _lib.F16, "bf16": _lib.BF16}, {"f32": 4, "f16": 2, "bf16": 2}

    def check(xk, rk, wk, rows, cols, pad):
        P = _lib.NormBwdParams()
        P.rows, P.cols, P.x_dtype, P.res_dtype, P.w_dtype = rows, cols, ids[xk], ids[rk], ids[wk or xk]
        P.xsum_row_stride = P.dy_row_stride = P.dres_out_row_stride = cols + pad
        P.dx_row_stride = P.dres_row_stride = cols
        for k, field in enumerate(("xsum", "dy", "dresidual_out", "dx", "dresidual", "dweight", "dbias", "workspace") + (("weight",) if wk else ())):
            setattr(P, field, (k + 1) * _lib.FRESH_ADDRESS)
        P.workspace_bytes = 1 << 40
        got = bwd_plan(P)
        want = fc.norm_branch(cols, pad)
        assert ((got["vec"], got["iters"]) if got["kernel"] else None) == want and got["status"] == (0 if want else -2), (xk, rk, wk, rows, cols, pad, got)
        return want
    seen = set()
    for c in fc.norm_cases():
        assert check(c["xk"], c["rk"], c["wk"], c["rows"], c["cols"], c["pitch_pad"]) == c["branch"]
        seen.add(c["branch"])
    rng = np.random.default_rng(20252)
    for i in range(3000):
        xk, rk, wk = fc.NORM_DTYPES[i % 9]
        seen.add(check(xk, rk, wk if i % 5 else None, int(rng.integers(1, 3000)), int(rng.integers(1, 2101)) if i % 4 else int(rng.integers(1, 526)) * 4, int(rng.integers(0, 8)) * (i % 2)))
    assert seen == set(fc.NORM_BRANCHES) | {None}


def _bwd_workspace_bytes_answer_as_the_plans_do(bwd_plan):
    """the three *_workspace_bytes exports are the `need` of their plans, and both are the closed forms of the launchers they replace (bwd_ws_layout, nb_grid,
    the conv segment count): a seeded sweep up to batch 65535, seqlen 1 ... 4097, dim in multiples of 4, and the sizes that answer 0"""
    from zigma_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(20253)
    up = lambda a, b: -(-a // b)
    pick = lambda n, *edges: int(edges[int(rng.integers(0, len(edges)))]) if rng.integers(0, 4) == 0 else int(rng.integers(1, n + 1))
    for i in range(3000):
        batch, seqlen, dim = pick(65535, 1, 65535, 0, -1), pick(4097, 1, 16, 17, 128, 129, 4096, 4097, 0), 4 * pick(1024, 1, 16, 0)
        S = _lib.ScanBwdParams()
        S.batch, S.dim, S.seqlen, S.dstate, S.checkpoints = batch, dim, seqlen, (16, 8, 16, 0)[i % 4], (None, 1 << 30)[i % 2]
        want = 0
        if min(batch, dim, seqlen, S.dstate) > 0:
            tiles, slabs = up(seqlen, 16), dim // 64
            want = 4 * ((0 if S.checkpoints else batch * slabs * tiles * S.dstate * 64) + batch * slabs * tiles * 16 * 2 * S.dstate + batch * dim * (S.dstate + 2))
        assert L.zigma_selective_scan_bwd_workspace_bytes(ctypes.byref(S)) == bwd_plan(S)["need"] == want, (batch, dim, seqlen, S.dstate)
        Cv = _lib.ConvBwdParams()
        Cv.batch, Cv.dim, Cv.seqlen, Cv.width = batch, dim, seqlen, (4, 3, 2)[i % 3]
        want = batch * up(seqlen, 128) * dim * (Cv.width + 1) * 4 if min(batch, dim, seqlen) > 0 else 0
        assert L.zigma_causal_conv1d_bwd_workspace_bytes(ctypes.byref(Cv)) == bwd_plan(Cv)["need"] == want, (batch, dim, seqlen, Cv.width)
        N = _lib.NormBwdParams()
        N.rows, N.cols = batch * (1, 7, 2048)[i % 3] if i % 11 else pick(2049, 2047, 2048, 2049, 0, -1), pick(2100, 1, 2048, 2049, 0)
        want = max(1, min(512, up(N.rows, 4))) * 2 * N.cols * 4 if N.rows > 0 and N.cols > 0 else 0
        assert L.zigma_add_norm_bwd_workspace_bytes(ctypes.byref(N)) == bwd_plan(N)["need"] == want, (N.rows, N.cols)
    for fn in ("zigma_selective_scan_bwd", "zigma_causal_conv1d_bwd", "zigma_add_norm_bwd"):
        assert getattr(L, fn + "_workspace_bytes")(None) == 0


def _backward_batch_limit_is_the_one_python_constant(bwd_plan):
    """both backward plans serve batch == _lib.GRID_DIM_MAX and refuse one more (ZIGMA_ERR_SHAPE): the constant the bindings slice the batch by, and
    z_preactivated_eligible() reads, is the plans' kBwdMaxBatch"""
    import bwd_plan_cases as bc
    from zigma_amd import _lib
    assert bwd_plan.max_batch == _lib.GRID_DIM_MAX == 65535
    for name in ("sb_served_16_states", "cb_served_width_4_silu_bias"):
        fn, P, _, _ = bc.block(name, "cpu")
        kernel = bc.CASES[name][2].kernel
        P.workspace_bytes = 1 << 50                 # (a query dereferences nothing)
        P.batch = _lib.GRID_DIM_MAX
        assert (bwd_plan(P)["status"], bwd_plan(P)["kernel"]) == (0, kernel) == _lib.plan(fn, P)
        P.batch = _lib.GRID_DIM_MAX + 1
        assert (bwd_plan(P)["status"], bwd_plan(P)["kernel"]) == (-2, None) == _lib.plan(fn, P)


def test_bwd_plans(bwd_plan, libpath):
    """add-norm in both directions and the scan and conv backward: the case table, the geometry of the serving leaves, the add-norm selections against the
    restatements the tests keep, the three size exports and the batch limit — the six checks above in ONE test, like the nine plans of
    test_outer_plan_case_table (an assertion names the check it belongs to by its frame)"""
    for check in (_bwd_plan_case_table, _bwd_plan_geometry, _add_norm_plan_agrees_with_both_hand_restatements,
                  _add_norm_bwd_plan_agrees_with_the_recorded_selection, _bwd_workspace_bytes_answer_as_the_plans_do,
                  _backward_batch_limit_is_the_one_python_constant):
        check(bwd_plan)

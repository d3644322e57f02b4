"""zigma_norm_linear_fwd without a GPU: the plan header compiled with g++ against the case table, the ctypes mirror of its parameter block against gcc, the
Python predicates against the plan on the edges of each rule, and the block's engagement rule on stand-in tensors (nothing is launched)."""
import ctypes
import os
import subprocess
import tempfile

import pytest
import torch

from conftest import ROOT
from test_host_cpu import libpath  # noqa: F401  (the module-scoped fixture: builds the library when it is not there — the predicates ask its plan query)
from norm_linear_cases import BASE, BF16, CASES, F16, F32, OK, POINTERS, make_params

_DRIVER = r"""
#include "norm_linear_plan.h"
using namespace zigma;
extern "C" int plan(const zigma_norm_linear_params_t *p, int *fields, const char **kernel) {
    const NormLinearPlan s = plan_norm_linear(*p);
    fields[0] = s.status; fields[1] = static_cast<int>(s.grid); fields[2] = static_cast<int>(s.block); fields[3] = s.ksteps;
    *kernel = s.kernel;
    return s.status;
}
extern "C" int tile(void) { return kNlTile; }
extern "C" int lds_bytes(void) { return kNlStages * kNlStageBytes + kNlWaves * kNlTok * kNlOutPitch; }
"""
FAKE = dict(x=0x10000, w=0x20000, shift=0x30000, scale=0x30500, out=0x40000)       # 16-byte aligned stand-in addresses: the plan never dereferences


@pytest.fixture(scope="module")
def plan():
    from zigma_amd import _lib
    with tempfile.TemporaryDirectory() as d:
        src, so = os.path.join(d, "plan.cpp"), os.path.join(d, "libplan.so")
        open(src, "w").write(_DRIVER)
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "zigma_amd", "csrc"),
                        src, "-o", so], check=True)
        L = ctypes.CDLL(so)
    L.plan.argtypes = [ctypes.POINTER(_lib.NormLinearParams), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_char_p)]

    def call(P):
        f, k = (ctypes.c_int * 4)(), ctypes.c_char_p()
        L.plan(ctypes.byref(P), f, ctypes.byref(k))
        return dict(status=f[0], grid=f[1], block=f[2], ksteps=f[3], kernel=k.value.decode() if k.value else None)
    call.tile, call.lds_bytes = L.tile(), L.lds_bytes()
    return call


@pytest.mark.parametrize("name,overrides,status,kernel", CASES, ids=[c[0] for c in CASES])
def test_plan_case_table(plan, name, overrides, status, kernel):
    """one call per leaf of plan_norm_linear: status, kernel string, and for the served calls the launch geometry"""
    from zigma_amd import _lib
    P = make_params(_lib.NormLinearParams, overrides, FAKE)
    got = plan(P)
    assert (got["status"], got["kernel"]) == (status, kernel), got
    if kernel is not None:
        assert got["grid"] == P.m // 128 and got["block"] == 256 and got["ksteps"] == P.k // 64 and kernel == f"norm_linear_k{P.k}", got


def test_case_table_covers_every_status_and_pointer():
    refused = [c for c in CASES if c[2] != OK]
    assert {c[2] for c in refused} == {-1, -2, -3, -4, -6}
    for ptr in POINTERS:
        assert any(c[1].get(ptr) == "null" for c in refused) and any(hasattr(c[1].get(ptr), "nbytes") for c in refused), ptr
    assert {c[3] for c in CASES if c[3]} == {"norm_linear_k512", "norm_linear_k640", "norm_linear_k768"}


def test_tile_constants(plan, libpath):  # noqa: F811
    from zigma_amd.norm_linear import norm_linear_shape_ok
    assert plan.tile == 128 and norm_linear_shape_ok(plan.tile, 512, 640, plan.tile) and not norm_linear_shape_ok(plan.tile // 2, 512, 640, plan.tile // 2)
    assert plan.lds_bytes == 67584 and 2 * plan.lds_bytes <= 160 * 1024          # two workgroups per CU


def test_ctypes_mirror_matches_the_header():
    """sizeof / offsetof of zigma_norm_linear_params_t as gcc sees include/zigma_hip.h equal the ctypes mirror"""
    from zigma_amd import _lib
    st, cname = _lib.NormLinearParams, "zigma_norm_linear_params_t"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "zigma_hip.h"', "int main(void){", f'printf("{cname} %zu\\n", sizeof({cname}));']
    lines += [f'printf("{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in st._fields_]
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "a.c"), os.path.join(d, "a.out")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = dict(l.split() for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.strip().splitlines())
    assert int(got[cname]) == ctypes.sizeof(st)
    for f, _ in st._fields_:
        assert int(got[f]) == getattr(st, f).offset, f
    assert "zigma_norm_linear_fwd" in _lib.EXPORTS


class Stand:
    """a tensor stand-in: the attributes the predicates read, no storage"""

    def __init__(self, shape, stride=None, dtype=torch.bfloat16, cuda=True, ptr=0x10000, requires_grad=False):
        self.shape = tuple(shape)
        if stride is None:
            stride, acc = [], 1
            for s in reversed(self.shape):
                stride.insert(0, acc)
                acc *= s
        self._stride, self.dtype, self.is_cuda, self._ptr, self.requires_grad = tuple(stride), dtype, cuda, ptr, requires_grad

    def dim(self):
        return len(self.shape)

    def stride(self, i):
        return self._stride[i]

    def data_ptr(self):
        return self._ptr


def _operands(B=64, L=1024, k=640, n=512, **kw):
    """x (B, L, k), to_q's weight (n, k), shift / scale as column slices of a (B, 6k) tensor; x_* / w_* / sh_* / sc_* override an attribute of one of them"""
    of = lambda prefix, **default: dict(default, **{a[len(prefix):]: v for a, v in kw.items() if a.startswith(prefix)})
    x = Stand((B, L, k), **of("x_"))
    w = Stand((n, k), **of("w_", ptr=0x20000))
    shift = Stand((B, k), **of("sh_", stride=(6 * k, 1), ptr=0x30000))
    scale = Stand((B, k), **of("sc_", stride=(6 * k, 1), ptr=0x30000 + 2 * k))
    return x, w, shift, scale


def _plan_of(plan, x, w, shift, scale):
    from zigma_amd import _lib
    P = _lib.NormLinearParams()
    P.m, P.n, P.k, P.dtype, P.flags, P.rows_per_batch, P.eps = x.shape[0] * x.shape[1], w.shape[0], x.shape[2], _lib._DT.get(x.dtype, 7), 0, x.shape[1], 1e-6
    P.x_row_stride, P.w_row_stride, P.out_row_stride, P.mod_batch_stride = x.stride(1), w.stride(0), w.shape[0], shift.stride(0)
    P.x, P.w, P.shift, P.scale, P.out = x.data_ptr(), w.data_ptr(), shift.data_ptr(), scale.data_ptr(), 0x40000
    return plan(P)


EDGES = [
    (dict(), True),
    (dict(k=512), True), (dict(k=768), True), (dict(k=576), False), (dict(k=704), False), (dict(k=1024), False),
    (dict(n=256), False), (dict(n=640), False),
    (dict(B=1, L=128), True), (dict(B=3, L=128), True), (dict(B=4, L=96), True), (dict(B=1, L=64), False), (dict(B=3, L=96), False), (dict(B=2, L=192), True),
    (dict(x_dtype=torch.float16, w_dtype=torch.float16, sh_dtype=torch.float16, sc_dtype=torch.float16), True),
    (dict(x_dtype=torch.float32, w_dtype=torch.float32, sh_dtype=torch.float32, sc_dtype=torch.float32), False),
    (dict(x_stride=(1024 * 648, 648, 1)), True), (dict(x_stride=(1024 * 644, 644, 1)), False), (dict(x_stride=(1024 * (1 << 27), 1 << 27, 1)), False),
    (dict(w_stride=(648, 1)), True), (dict(w_stride=(644, 1)), False), (dict(w_stride=(1 << 27, 1)), False),
    (dict(sh_stride=(644, 1), sc_stride=(644, 1)), False), (dict(sh_stride=(640, 1), sc_stride=(640, 1)), True), (dict(sh_stride=(0, 1), sc_stride=(0, 1)), True),
    (dict(x_ptr=0x10008), False), (dict(w_ptr=0x20002), False), (dict(sh_ptr=0x30004), False), (dict(sc_ptr=0x30008), False),
]


@pytest.mark.parametrize("kw,ok", EDGES)
def test_python_predicate_agrees_with_the_plan(plan, kw, ok, libpath):  # noqa: F811
    """norm_linear_eligible (tensors) and norm_linear_shape_ok (shapes) on the edges of each rule: True exactly where plan_norm_linear (compiled here with
    g++, independent of the built library the predicates ask) serves the call; the block norm_linear_block builds is the block that plan was asked about"""
    from zigma_amd.norm_linear import norm_linear_block, norm_linear_eligible, norm_linear_shape_ok
    x, w, shift, scale = _operands(**kw)
    assert plan(norm_linear_block(x, w, shift, scale, 1e-6, Stand((x.shape[0] * x.shape[1], w.shape[0]), ptr=0x40000))) == _plan_of(plan, x, w, shift, scale)
    with torch.no_grad():
        got = norm_linear_eligible(x, w, shift, scale)
    served = _plan_of(plan, x, w, shift, scale)["kernel"] is not None
    assert got == ok == served, (got, ok, served)
    m, L = x.shape[0] * x.shape[1], x.shape[1]
    if all(a.startswith(("B", "L", "k", "n")) for a in kw):
        assert norm_linear_shape_ok(m, w.shape[0], x.shape[2], L) == ok


def test_predicate_refuses_what_the_plan_cannot_see(libpath):  # noqa: F811
    """mixed dtypes, a bias, CPU tensors, samples in different pitches, shift / scale in different pitches, autograd"""
    from zigma_amd.norm_linear import norm_linear_eligible as el
    with torch.no_grad():
        assert el(*_operands())
        assert not el(*_operands(w_dtype=torch.float16))
        assert not el(*_operands(sc_dtype=torch.float16))
        assert not el(*_operands(), bias=Stand((512,)))
        assert not el(*_operands(x_cuda=False))
        assert not el(*_operands(x_stride=(2048 * 640, 640, 1)))
        assert not el(*_operands(sc_stride=(640, 1)))
        assert el(*_operands(x_requires_grad=True))
    with torch.enable_grad():
        assert el(*_operands())
        assert not el(*_operands(x_requires_grad=True)) and not el(*_operands(w_requires_grad=True)) and not el(*_operands(sh_requires_grad=True))


class _ToQ:
    def __init__(self, w, bias=None):
        self.weight, self.bias = w, bias


def test_block_engagement_rule(monkeypatch, libpath):  # noqa: F811
    """model_zigma.fuse_norm_to_q on stand-ins: on at 65 536 tokens with no pending branch; off under routing.POLICY == "off", off below 65 536 tokens, off
    with a pending branch, under autograd, with the knob off; the new kernel is no row of the to_q role"""
    import zigma_amd.model_zigma as mz
    import zigma_amd.routing as zr

    def decide(B=64, branch=None, **kw):
        x, w, shift, scale = _operands(B=B, **kw)
        return mz.fuse_norm_to_q(mz.Pending(x, branch, None if branch is None else shift), _ToQ(w), shift, scale)

    assert mz.FUSE_NORM_TO_Q is True and mz.NORM_TO_Q_MIN_TOKENS == 65536
    with torch.no_grad():
        assert decide() and decide(B=128) and decide(k=512) and decide(k=768)
        assert not decide(B=63) and not decide(B=32) and not decide(B=16) and not decide(B=8)          # below the token floor
        assert not decide(branch=_operands()[0])
        assert not decide(x_dtype=torch.float32, w_dtype=torch.float32, sh_dtype=torch.float32, sc_dtype=torch.float32)
        assert not decide(k=1024)
        monkeypatch.setattr(zr, "POLICY", "off")
        assert not decide()
        monkeypatch.setattr(zr, "POLICY", "all")
        assert decide()
        monkeypatch.setattr(zr, "POLICY", "auto")
        monkeypatch.setattr(mz, "FUSE_NORM_TO_Q", False)
        assert not decide()
        monkeypatch.setattr(mz, "FUSE_NORM_TO_Q", True)
        x, w, shift, scale = _operands()
        assert not mz.fuse_norm_to_q(mz.Pending(x), _ToQ(w, bias=Stand((512,))), shift, scale)
    with torch.enable_grad():
        assert decide() and not decide(w_requires_grad=True) and not decide(x_requires_grad=True)
    assert zr.route("to_q", 65536, 512, 640).row == "to_q.tiled"
    assert not any("norm" in r.id or "norm" in r.kernel for r in zr.TABLE)


def test_knob_is_registered(monkeypatch):
    """FUSE_NORM_TO_Q answers to ZIGMA_KNOBS like FUSE_OUT_PROJ_ADD; no environment variable of its own"""
    import sys
    code = "import zigma_amd.model_zigma as z; print(z.FUSE_NORM_TO_Q, z.NORM_TO_Q_MIN_TOKENS)"
    env = dict(os.environ, ZIGMA_KNOBS="model_zigma.FUSE_NORM_TO_Q=False,model_zigma.NORM_TO_Q_MIN_TOKENS=16384")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.split() == ["False", "16384"], (out.stdout, out.stderr[-400:])
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, ZIGMA_KNOBS=""), capture_output=True, text=True)
    assert out.stdout.split() == ["True", "65536"], out.stdout


def test_build_checks_the_kernel_for_scratch():
    """every instantiation of norm_linear_kernel is under the build's no-scratch / no-spill check"""
    from zigma_amd import build
    assert "norm_linear.hip" in build.SOURCES and build.SOURCE_FLAGS["norm_linear.hip"] == build._RES and "norm_linear_kernel" in build.NO_SCRATCH_KERNELS
    ok = "a.hip:1:0: remark: Function Name: _ZN5zigma2nl18norm_linear_kernelILi10ENS_4BF16EEEv\na.hip:1:0: remark:     ScratchSize [bytes/lane]: 0\na.hip:1:0: remark:     VGPRs Spill: 0\n"
    assert build.check_no_scratch(ok, "a.hip") == 1
    with pytest.raises(RuntimeError):
        build.check_no_scratch(ok.replace("VGPRs Spill: 0", "VGPRs Spill: 3"), "a.hip")
    with pytest.raises(RuntimeError):
        build.check_no_scratch(ok.replace("bytes/lane]: 0", "bytes/lane]: 64"), "a.hip")

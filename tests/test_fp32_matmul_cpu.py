"""CPU tests of the fp32-by-bf16-splitting projection's host side: the parameter block's layout, the exported symbol, the refusals that need
no device, fp32_matmul.split / reference, linear.plan on stand-ins, the knob and the weight-plane cache (no GPU, no kernel launch)."""
import ctypes
import os
import subprocess
import sys
import tempfile

import pytest
import torch

from conftest import ROOT
from fp32_matmul_cases import EXACT, exact_case, random_case

F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(scope="module")
def libpath():
    from zigma_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.LIB_PATH


@pytest.fixture
def mode():
    """sets fp32_matmul.PRECISION for one test and puts "highest" back"""
    import zigma_amd
    yield zigma_amd.set_float32_matmul_precision
    zigma_amd.set_float32_matmul_precision("highest")


def test_split_params_match_the_header():
    """sizeof / offsetof of zigma_linear_split_params_t, as gcc sees include/zigma_hip.h, equal the ctypes mirror"""
    from zigma_amd import _lib
    cname, st = "zigma_linear_split_params_t", _lib.LinearSplitParams
    assert [f for f, _ in st._fields_] == ["m", "n", "k", "passes", "flags", "x_row_stride", "w_hi_row_stride", "w_lo_row_stride", "out_row_stride",
                                           "x", "w_hi", "w_lo", "bias", "out"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "zigma_hip.h"', "int main(void){", f'printf("{cname} %zu\\n", sizeof({cname}));']
    for f, _ in st._fields_:
        lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    lines.append('printf("abi %d\\n", ZIGMA_ABI_VERSION);')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "a.c"), os.path.join(d, "a.out")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    got = dict(l.split() for l in out.strip().splitlines())
    assert int(got[cname]) == ctypes.sizeof(st)
    for f, _ in st._fields_:
        assert int(got[f"{cname}.{f}"]) == getattr(st, f).offset, f
    assert int(got["abi"]) == 11                                        # an entry point added, no existing block changed


def test_split_symbol_is_exported(libpath):
    from zigma_amd import _lib
    L = ctypes.CDLL(libpath)
    assert hasattr(L, "zigma_linear_f32_split") and "zigma_linear_f32_split" in _lib.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "zigma_hip.h")).read()
    assert "int zigma_linear_f32_split(const zigma_linear_split_params_t *p, void *stream);" in hdr


def test_split_refusals_without_a_device(libpath):
    """every refusal is decided before anything touches the device (the pointers here are made-up addresses: nothing may read them)"""
    from zigma_amd import _lib
    L = _lib.lib()
    call = lambda P: L.zigma_linear_f32_split(ctypes.byref(P), None)
    assert L.zigma_linear_f32_split(None, None) == -1                       # ZIGMA_ERR_NULL
    assert call(_lib.LinearSplitParams()) == -1                             # a block without pointers

    def block(**kw):
        P = _lib.LinearSplitParams()
        P.m, P.n, P.k, P.passes = 0, 128, 64, 3
        P.x_row_stride, P.w_hi_row_stride, P.w_lo_row_stride, P.out_row_stride = 64, 64, 64, 128
        P.x, P.w_hi, P.w_lo, P.out = 0x7f0000000000, 0x7f0000100000, 0x7f0000200000, 0x7f0000300000
        for k, v in kw.items():
            setattr(P, k, v)
        return P
    assert call(block()) == 0                                               # m == 0: ZIGMA_OK without a launch
    assert call(block(w_lo=None)) == -1 and call(block(w_lo=None, passes=1)) == 0
    assert call(block(passes=2)) == -6 and call(block(flags=1)) == -6       # ZIGMA_ERR_UNSUPPORTED
    for bad in (dict(k=96, x_row_stride=96, w_hi_row_stride=96, w_lo_row_stride=96), dict(n=200, out_row_stride=200), dict(m=-8), dict(m=4), dict(x_row_stride=32)):
        assert call(block(**bad)) == -2, bad                                # ZIGMA_ERR_SHAPE
    for bad in (dict(x=0x7f0000000004), dict(out=0x7f0000300008), dict(w_hi=0x7f0000100002), dict(bias=0x7f0000400004), dict(x_row_stride=66),
                dict(w_lo_row_stride=68), dict(out_row_stride=130)):
        assert call(block(**bad)) == -4, bad                                # ZIGMA_ERR_STRIDE


def test_split_definition():
    from zigma_amd.fp32_matmul import split
    g = torch.Generator().manual_seed(7)
    # every fp32 with at most 16 significant bits is hi + lo exactly: 16-bit integers scaled by powers of two, both signs
    mant = torch.randint(1, 2 ** 16, (200_000,), generator=g).double()
    a = (mant * torch.pow(2.0, torch.randint(-60, 60, mant.shape, generator=g).double()) * (torch.randint(0, 2, mant.shape, generator=g) * 2 - 1)).float()
    hi, lo = split(a)
    assert hi.dtype == BF16 and lo.dtype == BF16 and torch.equal(hi.double() + lo.double(), a.double())
    # random normals: |a - hi - lo| <= 2^-16 |a| (hi leaves at most 2^-9 |a|, lo at most 2^-9 of that ... half an ulp each: 2^-18; the bound is the issue's)
    a = torch.randn(500_000, generator=g) * torch.pow(2.0, torch.randint(-20, 20, (500_000,), generator=g).float())
    hi, lo = split(a)
    assert bool(((a.double() - hi.double() - lo.double()).abs() <= 2.0 ** -16 * a.double().abs()).all())
    assert torch.equal(hi, a.to(BF16)) and torch.equal(lo, (a - hi.float()).to(BF16))
    # the clamp at the top of the range: a finite value never becomes infinite, and hi + lo still carries 16 bits of it
    big = torch.tensor([3.4028234663852886e38, -3.4028234663852886e38, 3.3961775e38, 3.3895313892515355e38, 3.39e38, -3.4e38])
    hi, lo = split(big)
    assert bool(torch.isfinite(hi.float()).all()) and bool(torch.isinf(big.to(BF16).float())[:3].all())
    assert torch.equal(hi.float().abs(), torch.full((6,), 3.3895313892515355e38))
    assert torch.equal(lo, (big - hi.float()).to(BF16)) and bool(((big.double() - hi.double() - lo.double()).abs() <= 2.0 ** -16 * big.double().abs()).all())
    # non-finite inputs: hi = bf16(a), lo = 0
    nf = torch.tensor([float("inf"), float("-inf"), float("nan"), 1.5])
    hi, lo = split(nf)
    assert hi[0] == float("inf") and hi[1] == float("-inf") and bool(torch.isnan(hi[2])) and torch.equal(lo.float(), torch.zeros(4)) and hi[3] == 1.5


@pytest.mark.parametrize("i", range(len(EXACT)))
def test_reference_on_the_exact_cases(i):
    from zigma_amd.fp32_matmul import reference
    c = exact_case(i)
    for m in ("high", "medium"):
        assert torch.equal(reference(c["x"], c["w"], None, m), c[m].double()), (EXACT[i], m)
    assert torch.equal(reference(c["x"], c["w"], None, "highest"), c["full"].double())
    b = torch.arange(c["w"].shape[0]).float()
    assert torch.equal(reference(c["x"], c["w"], b, "high"), c["high"].double() + b.double())


def test_reference_errors_on_random_operands():
    """the torch model alone against float64, in the GPU test's bounds (what is left of them is the kernel's fp32 accumulation)"""
    from zigma_amd.fp32_matmul import reference
    for i in (0, 1, 5):
        x, w, b = random_case(i)
        ref = reference(x, w, b, "highest")
        bound = x.double().abs() @ w.double().abs().t()
        eh, em = (reference(x, w, b, m) - ref for m in ("high", "medium"))
        assert bool((eh.abs() <= 2.0 ** -14 * bound).all()) and bool((em.abs() <= 2.0 ** -6 * bound).all())
        assert float(eh.norm() / ref.norm()) <= float(em.norm() / ref.norm()) / 64 and float(em.norm() / ref.norm()) <= 4e-3


class Stand:
    """what linear.plan reads of a tensor: device side, dtype, shape, strides, alignment, autograd"""

    def __init__(self, *shape, dtype=F32, pitch=None, ptr=0x7f0000000000, is_cuda=True, requires_grad=False):
        self.is_cuda, self.dtype, self.shape, self.requires_grad = is_cuda, dtype, torch.Size(shape), requires_grad
        st = [1]
        for s in reversed(shape[1:]):
            st.insert(0, st[0] * s)
        self._contig = tuple(st)
        if pitch is not None:
            st[-2] = pitch
        self._st, self._ptr = tuple(st), ptr

    def stride(self, i=None):
        return self._st if i is None else self._st[i]

    def dim(self):
        return len(self.shape)

    def numel(self):
        n = 1
        for s in self.shape:
            n *= s
        return n

    def is_contiguous(self):
        return self._st == self._contig

    def data_ptr(self):
        return self._ptr


# role -> (n, k) at E = 640; text: the batched K / V of two blocks; train: in_proj again
ROLE_SHAPES = {"in_proj": (2560, 640), "out_proj": (640, 1280), "to_q": (512, 640), "to_out": (640, 512), "text": (2048, 640), "train": (2560, 640)}


def test_plan_routes_fp32_calls_only_when_asked(mode, monkeypatch, libpath):
    import zigma_amd.routing as zr
    from zigma_amd import fp32_matmul as fm
    from zigma_amd.linear import plan
    assert fm.PRECISION == "highest" and set(ROLE_SHAPES) == set(zr.ROLES) and {"split3", "split1"} <= set(zr.KERNELS)
    today = zr.Route("library", False, "not-16bit-inference")
    calls = {role: (Stand(8, 256, k), Stand(n, k), Stand(n) if role == "to_out" else None) for role, (n, k) in ROLE_SHAPES.items()}
    for role, (x, w, b) in calls.items():
        assert plan(role, x, w, b) == today and fm.split_eligible(x, w, b)
    for m, kern in (("high", "split3"), ("medium", "split1")):
        mode(m)
        for role, (x, w, b) in calls.items():
            r = plan(role, x, w, b, residual=Stand(8, 256, w.shape[0]), gate=Stand(8, w.shape[0]))
            assert r == zr.Route(kern, False, "fp32." + m), (role, r)
            assert zr.kernel_name(r) == f"linear_split{kern[-1]}_"
    mode("high")
    n, k = ROLE_SHAPES["in_proj"]
    x, w = calls["in_proj"][:2]
    refused = {
        "mixed dtypes": (Stand(8, 256, k), Stand(n, k, dtype=BF16), None),
        "16-bit x": (Stand(8, 256, k, dtype=torch.float16), Stand(n, k), None),
        "bf16 bias": (x, w, Stand(n, dtype=BF16)),
        "CPU tensors": (Stand(8, 256, k, is_cuda=False), Stand(n, k, is_cuda=False), None),
        "requires_grad": (x, Stand(n, k, requires_grad=True), None),
        "k % 64": (Stand(8, 256, 96), Stand(n, 96), None),
        "n % 128": (Stand(8, 256, k), Stand(200, k), None),
        "tokens % 8": (Stand(3, 7, k), w, None),
        "a misaligned pointer": (Stand(8, 256, k, ptr=0x7f0000000004), w, None),
        "a misaligned row pitch": (Stand(2048, k, pitch=k + 2), w, None),
        "a misaligned bias": (x, w, Stand(n, ptr=0x7f0000000008)),
    }
    with torch.enable_grad():
        for why, (xx, ww, bb) in refused.items():
            assert not fm.split_eligible(xx, ww, bb) and plan("in_proj", xx, ww, bb).kernel == "library", why
    with torch.no_grad():                                                   # (without autograd requires_grad does not matter, as for linear_eligible)
        assert plan("in_proj", x, Stand(n, k, requires_grad=True)).kernel == "split3"
    assert plan("in_proj", Stand(2048, k, pitch=k + 64), w).kernel == "split3"          # a 2-D view of wider rows passes
    monkeypatch.setattr(zr, "POLICY", "off")
    assert plan("in_proj", x, w) == today
    monkeypatch.setattr(zr, "POLICY", "auto")
    # 16-bit calls do not read the mode
    xb, wb = Stand(8, 8192, 640, dtype=BF16), Stand(2560, 640, dtype=BF16)
    assert plan("in_proj", xb, wb) == zr.Route("ws", False, "in_proj.ws")
    # real CPU tensors keep F.linear, bit for bit
    from zigma_amd.linear import project
    xc, wc = torch.randn(8, 64), torch.randn(128, 64)
    assert torch.equal(project("in_proj", xc, wc), torch.nn.functional.linear(xc, wc))


def test_precision_setter(mode):
    import zigma_amd
    from zigma_amd import fp32_matmul as fm
    assert zigma_amd.get_float32_matmul_precision() == "highest"
    for m in ("high", "medium", "highest"):
        mode(m)
        assert zigma_amd.get_float32_matmul_precision() == m == fm.PRECISION
    with pytest.raises(ValueError):
        mode("tf32")
    assert fm.PRECISION == "highest"
    before = torch.get_float32_matmul_precision()
    mode("high")
    assert torch.get_float32_matmul_precision() == before                  # torch's global setting is neither read nor written
    with pytest.raises(ValueError):
        fm.linear_split(torch.zeros(8, 64), torch.zeros(128, 64), mode="highest")


def test_precision_knob_from_the_environment():
    code = "import zigma_amd.model_zigma, zigma_amd; print(zigma_amd.get_float32_matmul_precision())"
    run = lambda spec, c=code: subprocess.run([sys.executable, "-c", c], cwd=ROOT, env=dict(os.environ, ZIGMA_KNOBS=spec), capture_output=True, text=True)
    for spec, want in (("fp32_matmul.PRECISION=high", "high"), ("", "highest"), ("fp32_matmul.PRECISION=medium", "medium")):
        out = run(spec)
        assert out.returncode == 0 and out.stdout.split() == [want], (spec, out.stdout, out.stderr[-400:])
    bad = run("fp32_matmul.NO_SUCH=1")
    assert bad.returncode != 0 and "no knob" in bad.stderr
    bad = run("fp32_matmul.PRECISION=tf32")
    assert bad.returncode != 0 and "PRECISION" in bad.stderr
    bad = run("linear.X=1")                                                 # linear stays a module without knobs
    assert bad.returncode != 0 and "names no module with knobs" in bad.stderr


def test_weight_plane_cache():
    from zigma_amd import fp32_matmul as fm
    fm.clear_cache()
    stats = lambda: (fm.CACHE_STATS["hit"], fm.CACHE_STATS["miss"])
    w = torch.randn(128, 64)
    h0, m0 = stats()
    hi, lo = fm.split_weight(w)
    assert stats() == (h0, m0 + 1) and hi.is_contiguous() and lo.is_contiguous()
    ref_hi, ref_lo = fm.split(w)
    assert torch.equal(hi, ref_hi) and torch.equal(lo, ref_lo)
    hi2, lo2 = fm.split_weight(w)
    assert stats() == (h0 + 1, m0 + 1) and hi2 is hi and lo2 is lo          # the same tensor: a hit
    w.add_(0)                                                               # a version bump: a miss, and the stale entry is replaced
    fm.split_weight(w)
    assert stats() == (h0 + 1, m0 + 2) and len(fm._CACHE) == 1
    w.mul_(2)
    hi3, lo3 = fm.split_weight(w)
    assert torch.equal(hi3.float() + lo3.float(), (hi.float() + lo.float()) * 2) and len(fm._CACHE) == 1
    for _ in range(50):                                                     # in-place updates never grow it
        w.add_(1)
        fm.split_weight(w)
    assert len(fm._CACHE) == 1
    keep = [torch.randn(128, 64) for _ in range(5)]
    for t in keep:
        fm.split_weight(t)
    assert len(fm._CACHE) == 6
    for _ in range(20):                                                     # weights that die take their entries along
        fm.split_weight(torch.randn(256, 64))
    assert len(fm._CACHE) == 6
    del keep, t
    assert len(fm._CACHE) == 1
    wt = w.t()                                                              # another stride of the same storage: another key, the same slot
    fm.split_weight(wt)
    assert len(fm._CACHE) == 1 and fm.split_weight(wt)[0].shape == (64, 128)
    del w, wt
    assert len(fm._CACHE) == 0

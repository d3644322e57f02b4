"""CPU tests of the weight-gradient entry point's host side: the parameter block's layout, the exported symbols, and wgrad.plan_wgrad on
stand-ins (no GPU, no compute calls into the library)."""
import ctypes
import os
import subprocess
import tempfile

import pytest
import torch

from conftest import ROOT


@pytest.fixture(scope="module")
def libpath():
    from zigma_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.LIB_PATH


def test_wgrad_params_match_the_header():
    """sizeof / offsetof of zigma_linear_wgrad_params_t, as gcc sees include/zigma_hip.h, equal the ctypes mirror"""
    from zigma_amd import _lib
    cname, st = "zigma_linear_wgrad_params_t", _lib.LinearWgradParams
    assert [f for f, _ in st._fields_] == ["m", "n", "k", "dtype", "out_dtype", "slabs", "flags", "dy_row_stride", "x_row_stride", "out_row_stride",
                                           "dy", "x", "out", "workspace", "workspace_bytes"]
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
    assert int(got["abi"]) == 11                                        # entry points added, no existing block changed


def test_wgrad_symbols_are_exported(libpath):
    from zigma_amd import _lib
    L = ctypes.CDLL(libpath)
    for name in ("zigma_linear_wgrad", "zigma_linear_wgrad_workspace_bytes"):
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "zigma_hip.h")).read()
    assert "int zigma_linear_wgrad(const zigma_linear_wgrad_params_t *p, void *stream);" in hdr
    assert "int64_t zigma_linear_wgrad_workspace_bytes(const zigma_linear_wgrad_params_t *p);" in hdr


def test_wgrad_workspace_bytes_and_refusals_without_a_device(libpath):
    """the workspace query is host arithmetic: slabs x n x k fp32 partials (0 for one slab), 0 for a block the entry point would refuse; the entry
    point itself refuses a block without pointers before it touches the device"""
    from zigma_amd import _lib
    L = _lib.lib()
    P = _lib.LinearWgradParams()
    P.m, P.n, P.k, P.dtype, P.out_dtype = 65536, 72, 1280, _lib.BF16, _lib.BF16
    auto = L.zigma_linear_wgrad_workspace_bytes(ctypes.byref(P))
    assert auto > 0 and auto % (72 * 1280 * 4) == 0 and 65536 // (auto // (72 * 1280 * 4)) >= 256
    P.slabs = 3
    assert L.zigma_linear_wgrad_workspace_bytes(ctypes.byref(P)) == 3 * 72 * 1280 * 4
    P.slabs = 1
    assert L.zigma_linear_wgrad_workspace_bytes(ctypes.byref(P)) == 0
    P.slabs, P.m = 0, 200
    assert L.zigma_linear_wgrad_workspace_bytes(ctypes.byref(P)) == 0       # one slab: the GEMM kernel writes out itself
    P.n = 100
    assert L.zigma_linear_wgrad_workspace_bytes(ctypes.byref(P)) == 0
    assert L.zigma_linear_wgrad(ctypes.byref(P), None) == -1                # ZIGMA_ERR_NULL
    assert L.zigma_linear_wgrad(None, None) == -1


class Stand:
    """what plan_wgrad reads of a tensor: is_cuda, dtype, shape, stride, data_ptr (like wgrad._ContiguousLike)"""

    def __init__(self, m, w, dtype=torch.bfloat16, pitch=None, ptr=0x7f0000000000, is_cuda=True):
        self.is_cuda, self.dtype, self.shape = is_cuda, dtype, torch.Size((m, w))
        self._st, self._ptr = (pitch or w, 1), ptr

    def stride(self, i=None):
        return self._st if i is None else self._st[i]

    def dim(self):
        return 2

    def data_ptr(self):
        return self._ptr


BLOCK = {"in_proj": (2560, 640), "out_proj": (640, 1280), "to_q": (512, 640), "to_out": (640, 512), "x_proj": (72, 1280), "dt_proj": (1280, 40)}


@pytest.mark.parametrize("policy", ["auto", "off"])
def test_plan_wgrad_rows_and_limits(policy, monkeypatch):
    import zigma_amd.routing as zr
    from zigma_amd import wgrad as wg
    monkeypatch.setattr(zr, "POLICY", policy)                            # the plan does not read it
    monkeypatch.setattr(wg, "OWN_WGRAD", True)
    ids = [r.id for r in wg.PLAN_TABLE]
    assert len(set(ids)) == len(ids) and all(r.path in ("own", "bmm") and r.why for r in wg.PLAN_TABLE)
    want_row = {"in_proj": "dense", "out_proj": "dense", "to_q": "dense", "to_out": "dense", "x_proj": "skinny_n", "dt_proj": "skinny_k"}
    by_id = {r.id: r for r in wg.PLAN_TABLE}
    for tokens in (65536, 16384):
        for name, (n, k) in BLOCK.items():
            dy, x = Stand(tokens, n), Stand(tokens, k, pitch=72 if name == "dt_proj" else None)
            row = wg.plan_row(dy, x)
            assert row is not None and row.id == want_row[name], (tokens, name, row)
            assert wg.plan_wgrad(dy, x) == by_id[want_row[name]].path
    good = (Stand(65536, 72), Stand(65536, 1280))
    assert wg.plan_row(*good).id == "skinny_n" and wg.plan_wgrad(*good) == by_id["skinny_n"].path
    # a 512-token Mamba inner (the small training tests) falls on the same two rows
    assert wg.plan_row(Stand(512, 48), Stand(512, 256)).id == "skinny_n" and wg.plan_row(Stand(512, 256), Stand(512, 16, pitch=48)).id == "skinny_k"
    assert wg.plan_row(Stand(200, 72), Stand(200, 1280)).id == "few_tokens"
    refused = {
        "mixed dtypes": (Stand(65536, 72), Stand(65536, 1280, dtype=torch.float16)),
        "fp32": (Stand(65536, 72, dtype=torch.float32), Stand(65536, 1280, dtype=torch.float32)),
        "n = 100": (Stand(65536, 100, pitch=104), Stand(65536, 1280)),
        "row stride 36": (Stand(65536, 32, pitch=36), Stand(65536, 1280)),
        "pointer off by 2 bytes": (Stand(65536, 72), Stand(65536, 1280, ptr=0x7f0000000002)),
        "CPU": (Stand(65536, 72, is_cuda=False), Stand(65536, 1280, is_cuda=False)),
        "row stride below the width": (Stand(65536, 72, pitch=64), Stand(65536, 1280)),
        "different m": (Stand(65536, 72), Stand(65528, 1280)),
    }
    for why, (dy, x) in refused.items():
        assert wg.plan_row(dy, x) is None and wg.plan_wgrad(dy, x) == "bmm", why
    # the knob: False never, "all" wherever the tensor-level limits hold (and still never outside them)
    dense = (Stand(65536, 2560), Stand(65536, 640))
    monkeypatch.setattr(wg, "OWN_WGRAD", False)
    assert wg.plan_wgrad(*good) == "bmm"
    monkeypatch.setattr(wg, "OWN_WGRAD", "all")
    assert wg.plan_wgrad(*dense) == "own" and wg.plan_wgrad(*good) == "own"
    assert all(wg.plan_wgrad(dy, x) == "bmm" for dy, x in refused.values())
    # real CPU tensors keep the path they had
    monkeypatch.setattr(wg, "OWN_WGRAD", True)
    dy, x = torch.randn(512, 72).bfloat16(), torch.randn(512, 128).bfloat16()
    assert wg.plan_wgrad(dy, x) == "bmm"
    assert torch.equal(wg.wgrad(dy, x), dy.t() @ x)


def test_wgrad_knob_from_the_environment():
    import sys
    code = "import zigma_amd.wgrad as w; print(w.OWN_WGRAD)"
    for spec, want in (("wgrad.OWN_WGRAD=False", "False"), ("", "True"), ("wgrad.OWN_WGRAD=all", "all")):
        out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, ZIGMA_KNOBS=spec), capture_output=True, text=True)
        assert out.returncode == 0 and out.stdout.split() == [want], (spec, out.stdout, out.stderr[-400:])
    bad = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, ZIGMA_KNOBS="wgrad.NO_SUCH=1"), capture_output=True, text=True)
    assert bad.returncode != 0 and "no knob" in bad.stderr

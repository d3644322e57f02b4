"""The dispatch tables of the Mamba inner's four front entry points (tests/front_plan_cases.py, plans of zigma_amd/csrc/front_plan.h) through the library
on the GPU: status and zigma_last_kernel() of every case; a refusal or an empty call launches nothing (outputs pre-filled with NaN stay NaN, the last
kernel stays what it was); every served case against float64 on the same operands, under the bound the kernel's own test uses:
  conv                          test_gpu_parity.py::test_conv_tok_gather_vs_oracle — bf16: norm-wise < 1e-3 against the reference rounded to bf16 and
                                allclose(rtol 1e-2, atol 5e-2); fp32: norm-wise < 1e-5
  conv_x_proj, x_proj, dt_proj  fwd_fuzz_cases.bound_of, norm-wise and row by row (test_gpu_fwd_fuzz._report)
A plan field mapped to the wrong template instantiation or grid computes something else, or leaves rows unwritten (NaN)."""
import ctypes

import numpy as np
import pytest
import torch

import front_plan_cases as fpc
import fwd_fuzz_cases as fc
from conftest import rel_err
from test_gpu_fwd_fuzz import _report

pytestmark = pytest.mark.gpu
DEV = "cuda"
KIND = {torch.bfloat16: "bf16", torch.float16: "f16", torch.float32: "f32"}


def _launch(fn, P):
    from zigma_amd import _lib
    before = _lib.last_kernel()
    asked = _lib.plan(fn, P)                                    # the host-only query first: it must foretell the launch and report nothing itself
    assert _lib.last_kernel() == before
    rc = getattr(_lib.lib(), fn)(ctypes.byref(P), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    after = _lib.last_kernel()
    assert asked == (rc, after if asked[1] is not None else None) and (asked[1] is not None or after == before), (asked, rc, before, after)
    return rc, before, after


@pytest.mark.parametrize("name", sorted(fpc.CASES))
def test_front_dispatch_case_table(name):
    entry, _, want = fpc.CASES[name]
    (rc, before, after), o = fpc.call(name, DEV, _launch)
    assert rc == want.status
    if want.kernel is None:
        assert after == before and all(bool(torch.isnan(t).all()) for t in o["outs"].values())      # nothing reported, nothing written
        return
    assert after == want.kernel
    ref = fpc.reference(name, o)
    for key, out in o["outs"].items():
        got, r = out.detach().double().cpu().numpy(), ref[key].numpy()
        if entry != "conv":
            _report(name, key, got.reshape(r.shape), r, fc.bound_of(dict(id=name, kind=KIND[o["kind"]]), key))
            continue
        assert np.isfinite(got).all(), (name, "an element was left unwritten")
        if o["kind"] == torch.bfloat16:
            r = ref[key].float().bfloat16().double().numpy()
            e = rel_err(got, r)
            print(f"{name}: {after} rel err {e:.3e}")
            assert e < 1e-3 and np.allclose(got, r, rtol=1e-2, atol=5e-2), (name, e)
        else:
            e = rel_err(got, r)
            print(f"{name}: {after} rel err {e:.3e}")
            assert e < 1e-5, (name, e)

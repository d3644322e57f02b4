"""Add-norm in both directions and the scan and conv backward after their bindings build a block first, on the cases of tests/bwd_plan_cases.py.  A served
case: the parameter block that reached the launch is field for field the block the product's builder fills on the case's own outputs — the one that was
asked about — but for the addresses of the tensors the wrapper allocates, and the kernel that served it is the plan's.  A refused or empty case: the
launch returns the plan's status and every output keeps its bits."""
import ctypes

import pytest
import torch

import bwd_plan_cases as bc

pytestmark = pytest.mark.gpu
DEV = "cuda"
SERVED = sorted(n for n, c in bc.CASES.items() if c[2].kernel)
UNSERVED = sorted(n for n, c in bc.CASES.items() if not c[2].kernel)


@pytest.fixture
def trace():
    from zigma_amd import _lib
    _lib.lib()
    _lib.TRACE = []
    yield _lib.TRACE
    _lib.TRACE = None


@pytest.mark.parametrize("name", SERVED)
def test_served_case_launches_the_block_that_was_asked_about(name, trace):
    from zigma_amd import _lib
    entry, case, want = bc.CASES[name]
    own = any(k in case for k in bc.OWN_LAYOUT)
    with torch.no_grad():
        fn, asked, _, call = bc.block(name, DEV)
        assert _lib.plan(fn, asked) == tuple(want)
        before = bytes(asked)
        if own:
            _lib.call(fn, asked, torch.device(DEV))
        else:
            call()
    torch.cuda.synchronize()
    assert [t[:2] for t in trace] == [(fn, want.kernel)] and _lib.last_kernel() == want.kernel
    launched, asked = trace[0][2], type(asked).from_buffer_copy(before)
    for field, _ in launched._fields_:
        a, b = getattr(asked, field), getattr(launched, field)
        if field in bc.ALLOCATED[entry] and not own:
            assert (a is None) == (b is None) and (b is None or b % 16 == 0), (field, a, b)
        else:
            assert a == b, (field, a, b)
    assert _lib.plan(fn, launched) == tuple(want)


@pytest.mark.parametrize("name", UNSERVED)
def test_refused_or_empty_case_returns_the_plans_status_and_writes_nothing(name):
    from zigma_amd import _lib
    want = bc.CASES[name][2]
    fn, P, outs, _ = bc.block(name, DEV)
    outs = {k: t for k, t in outs.items() if t is not None}
    before = {k: t.clone() for k, t in outs.items()}
    torch.cuda.synchronize()
    assert _lib.plan(fn, P) == tuple(want)
    rc = getattr(_lib.lib(), fn)(ctypes.byref(P), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == want.status
    for k, t in outs.items():
        same = torch.equal(t, before[k]) if t.dtype == torch.uint8 else bool(torch.isnan(t).all())
        assert same, (k, "a call that launches nothing wrote")

"""The operators around the blocks, cross-attention, the glue backward and the weight gradient after their predicates ask the library's plans, on the
cases of tests/outer_plan_cases.py.  A served case: the parameter block that reached the launch is byte for byte the block that was asked about — the one
the predicate accepted and handed on, or the one the builder fills on placeholders — once the addresses of the tensors the wrapper allocates are set, and
the kernel that served it is the plan's.  A refused or empty case: the launch returns the plan's status and every output keeps its bits."""
import ctypes

import pytest
import torch

import outer_plan_cases as oc

pytestmark = pytest.mark.gpu
DEV = "cuda"
SERVED = sorted(n for n, c in oc.CASES.items() if c[2].kernel)
UNSERVED = sorted(n for n, c in oc.CASES.items() if not c[2].kernel)
OWN_LAYOUT = ("out_off", "out_pitch")       # cases whose output has a layout the wrappers do not allocate: launched on the case's own block


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
    entry, case, want = oc.CASES[name]
    fn = oc.ENTRY[entry]
    builder, predicate, wrapper = oc.product(entry)
    with torch.no_grad():
        if any(k in case for k in OWN_LAYOUT):
            _, asked, _ = oc.block(name, DEV)
            before = bytes(asked)
            _lib.call(fn, asked, torch.device(DEV))
        else:
            args, kwargs, _ = oc.operands(name, DEV)
            asked = predicate(*args, **kwargs) if predicate else builder(*args, **kwargs)
            assert asked, "the predicate refuses a case the table serves"
            assert _lib.plan(fn, asked) == tuple(want)
            before = bytes(asked)
            if predicate:
                wrapper(*args, **kwargs, block=asked)
            else:
                wrapper(*args, **kwargs)
    torch.cuda.synchronize()
    assert [t[:2] for t in trace] == [(fn, want.kernel)] and _lib.last_kernel() == want.kernel
    launched, asked = trace[0][2], type(asked).from_buffer_copy(before)
    for field, _ in launched._fields_:
        a, b = getattr(asked, field), getattr(launched, field)
        if field in oc.ALLOCATED[entry] and not any(k in case for k in OWN_LAYOUT):
            assert (a is None) == (b is None) and (b is None or b % 16 == 0), (field, a, b)
        else:
            assert a == b, (field, a, b)
    assert _lib.plan(fn, launched) == tuple(want)


@pytest.mark.parametrize("name", UNSERVED)
def test_refused_or_empty_case_returns_the_plans_status_and_writes_nothing(name):
    from zigma_amd import _lib
    want = oc.CASES[name][2]
    fn, P, outs = oc.block(name, DEV)
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

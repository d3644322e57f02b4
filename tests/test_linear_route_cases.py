"""linear.plan and the three predicates beside its walk give what they gave before they asked the library (tests/linear_route_cases.py: the tables
recorded on the parent commit).  No GPU: descriptors stand for the tensors, and the predicates ask the built library's host-only plan queries."""
import pytest

import linear_route_cases as lrc
from test_host_cpu import libpath  # noqa: F401  (the module-scoped fixture: builds the library when it is not there)


def test_plan_matches_the_parent_commit(libpath):  # noqa: F811
    """every case of the table in ONE test (the table has 551 of them): all the cases that differ are reported together"""
    from zigma_amd import routing
    from zigma_amd.linear import plan
    got = {name: lrc.call(plan, case) for name, case in lrc.CASES.items()}
    wrong = {name: (got[name], lrc.EXPECTED[name]) for name in lrc.CASES if got[name] != lrc.EXPECTED[name]}
    assert not wrong, wrong
    assert all(routing.Route(*got[name]) == routing.Route(*lrc.EXPECTED[name]) for name in lrc.CASES)


@pytest.mark.parametrize("cases,accepted,call,module,predicate", [
    (lrc.GATED_CASES, lrc.GATED_ACCEPTED, lrc.call_gated, "linear", "gated_residual_eligible"),
    (lrc.NORM_LINEAR_CASES, lrc.NORM_LINEAR_ACCEPTED, lrc.call_norm_linear, "norm_linear", "norm_linear_eligible"),
    (lrc.SPLIT_CASES, lrc.SPLIT_ACCEPTED, lrc.call_split, "fp32_matmul", "split_eligible")], ids=["gated_residual", "norm_linear", "split"])
def test_predicates_match_the_parent_commit(cases, accepted, call, module, predicate, libpath):  # noqa: F811
    import importlib
    fn = getattr(importlib.import_module("zigma_amd." + module), predicate)
    assert {name for name, c in cases.items() if call(fn, c)} == accepted


def test_the_table_covers_every_choice():
    assert set(lrc.EXPECTED) == set(lrc.CASES)
    routes = list(lrc.EXPECTED.values())
    assert {r[0] for r in routes} == {"ws", "ws128", "sm", "tiled", "tiled_halves", "split3", "split1", "library"}
    assert {r[2].split(".")[0] for r in routes} >= {"in_proj", "out_proj", "to_q", "to_out", "text", "train", "policy", "fp32", "autograd", "not-16bit-inference"}
    assert any(r[1] for r in routes)
    for cases, accepted in ((lrc.GATED_CASES, lrc.GATED_ACCEPTED), (lrc.NORM_LINEAR_CASES, lrc.NORM_LINEAR_ACCEPTED), (lrc.SPLIT_CASES, lrc.SPLIT_ACCEPTED)):
        assert accepted < set(cases)

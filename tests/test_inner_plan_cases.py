"""plan_inner on the shipped shapes gives what it gave before its predicates asked the library (tests/inner_plan_cases.py: the table recorded on the parent
commit).  No GPU: the predicates ask the built library's host-only plan queries."""
import pytest

import inner_plan_cases as ipc
from test_host_cpu import libpath  # noqa: F401  (the module-scoped fixture: builds the library when it is not there)


@pytest.mark.parametrize("name", sorted(ipc.CASES))
def test_plan_inner_matches_the_parent_commit(name, libpath):  # noqa: F811
    from zigma_amd.selective_scan_interface import InnerPlan, plan_inner
    assert ipc.call(plan_inner, ipc.CASES[name]) == InnerPlan(*ipc.EXPECTED[name])


def test_the_table_covers_every_choice():
    assert set(ipc.EXPECTED) == set(ipc.CASES)
    plans = list(ipc.EXPECTED.values())
    assert {p[0] for p in plans} == {"conv_x_proj", "conv+x_proj", "conv+linear"}
    assert {p[1] for p in plans} == {"in_scan", "in_split", "kernel", "linear"}
    assert any(p[2] for p in plans) and any(p[3] for p in plans)

"""Registers K36's stream-order cases and refusal rows EARLY, as tests/test_k35_tables_cpu.py does
for K35 and for the same reason.

tests/test_memory_bounds_gpu.py lists the cases of ``stream_order_cases.CASES`` when pytest collects
it, and its last test wants every entry point of include/ffn_hip.h reached by one of them under the
guarded placement.  pytest collects the files of a directory in the order of their names, and
``test_memory_bounds_gpu.py`` comes before ``test_mesh_cast_gpu.py``: the cases of K36 have to be in
the table by then.  This module's name sorts in front of it, and importing it is what registers
them.  Existing test files are not changed for K36."""

from tests import refusal_cases_mesh_cast  # noqa: F401
from tests import stream_order_cases_mesh_cast  # noqa: F401

ENTRY_POINTS = ["mesh_cast_boxes", "mesh_cast_tree", "mesh_cast", "mesh_cast_shade"]


def test_this_module_is_collected_before_the_memory_bounds_tests():
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    names = sorted(name for name in os.listdir(here)
                   if name.startswith("test_") and name.endswith(".py"))
    assert names.index(os.path.basename(__file__)) < names.index("test_memory_bounds_cpu.py")
    assert names.index(os.path.basename(__file__)) < names.index("test_memory_bounds_gpu.py")


def test_the_cases_are_in_the_table():
    from tests.stream_order_cases import CASES
    names = [case.name for case in CASES]
    reached = {entry for case in CASES for entry in case.reaches}
    for name in ENTRY_POINTS:
        assert names.count(name) == 1
        assert "ffn_" + name in reached


def test_the_rows_are_in_the_table():
    from tests import refusal_cases as rc
    assert set(ENTRY_POINTS) <= set(rc.ROWS) and set(ENTRY_POINTS) <= set(rc.subjects())

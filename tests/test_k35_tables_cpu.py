"""Registers K35's stream-order cases and refusal rows EARLY.

tests/test_memory_bounds_gpu.py lists the cases of ``stream_order_cases.CASES`` when pytest collects
it, and its last test wants every entry point of include/ffn_hip.h reached by one of them under the
guarded placement.  pytest collects the files of a directory in the order of their names, and
``test_memory_bounds_gpu.py`` comes before ``test_mesh_interp_cpu.py``: the cases of K35 have to be
in the table by then.  This module's name sorts in front of it, and importing it is what registers
them.  (K32 to K34 are imported by tests/test_memory_bounds_gpu.py itself; existing test files are
not changed for K35.)"""

from tests import refusal_cases_mesh_interp  # noqa: F401
from tests import stream_order_cases_mesh_interp  # noqa: F401


def test_this_module_is_collected_before_the_memory_bounds_tests():
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    names = sorted(name for name in os.listdir(here)
                   if name.startswith("test_") and name.endswith(".py"))
    assert names.index(os.path.basename(__file__)) < names.index("test_memory_bounds_cpu.py")


def test_the_cases_are_in_the_table():
    from tests.stream_order_cases import CASES
    names = [case.name for case in CASES]
    assert names.count("mesh_interp_face_grads") == 1
    assert names.count("mesh_interp_vertex_grad") == 1

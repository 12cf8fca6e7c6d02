"""Every entry point of include/ffn_hip.h that takes a ``stream`` has a stream-order case
(tests/stream_order_cases.py, run on the GPU by tests/test_stream_order_gpu.py).  A new entry
point without one fails here, on any machine: the table is imported without a GPU or the library
and the header is parsed as ``_lib.declared_symbols`` parses it."""

from tests import stream_helpers
from tests.stream_order_cases import CASES, UNREACHED


def test_the_header_is_parsed():
    from fourier_feature_nets_amd import _lib
    names = stream_helpers.stream_entry_points()
    declared = set(_lib.declared_symbols())
    assert names and set(names) <= declared
    # the entry points without a stream are host functions: sizes, limits, versions, tables
    assert "ffn_abi_version" not in names and "ffn_octree_grad_workspace_bytes" not in names
    assert "ffn_raygen_nearfar" in names and "ffn_mesh_raster_resolve" in names


def test_every_stream_taking_entry_point_has_a_case():
    names = set(stream_helpers.stream_entry_points())
    reached = set()
    for case in CASES:
        assert case.reaches, "%s declares no entry point" % case.name
        assert case.decoy or case.clear_only
        reached |= set(case.reaches)
    assert len(UNREACHED) <= 3 and all(UNREACHED.values()), "at most three, each with its reason"
    assert not (set(UNREACHED) & reached), "listed as unreached and reached"
    assert set(UNREACHED) <= names
    unknown = sorted(reached - names)
    assert not unknown, "cases declare entry points the header does not have: %s" % unknown
    missing = sorted(names - reached - set(UNREACHED))
    assert not missing, ("no stream-order case reaches %s: add one to tests/stream_order_cases.py"
                         % missing)


def test_case_names_are_unique():
    names = [case.name for case in CASES]
    assert len(names) == len(set(names))

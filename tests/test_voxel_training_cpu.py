"""Host side of voxel training: the train_voxels.py parser against the reference's
(tests/golden/cli_defaults_voxels.json from make_fit_schedule_voxels.py), the Voxels training
surface (parameter order, no `program` attribute) and the new exports."""

import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def test_train_voxels_parser_equals_the_reference():
    from scripts import _cli
    with open(os.path.join(HERE, "golden", "cli_defaults_voxels.json")) as f:
        ref = json.load(f)["train_voxels"]
    from tests.golden.make_fit_schedule_voxels import CLI_ARGV
    mine = vars(_cli.build_parser("t", _cli.VOXELS).parse_args(CLI_ARGV))
    assert mine == ref


def test_voxels_has_no_program_attribute():
    """RaySampler._can_fuse_focus and Raycaster._can_fuse pick the fused MLP kernels by
    hasattr(model, "program"): a Voxels opacity model must not take that path."""
    import fourier_feature_nets_amd as ffn
    model = ffn.Voxels(4, 1.0)
    assert not hasattr(model, "program")
    model.invalidate_packed()                 # a no-op the training engine calls


def test_dense_params_follow_the_state_dict_order():
    """The flat training buffer and the Adam moments line up with the reference's
    Adam(model.parameters()): voxels, then bias -- the order of its state_dict (the keys recorded
    in tests/golden/fit_schedule_voxels.npz)."""
    import numpy as np
    import fourier_feature_nets_amd as ffn
    model = ffn.Voxels(4, 1.0)
    params = model._dense_params()
    assert [p is q for p, q in zip(params, model.parameters())] == [True, True]
    g = np.load(os.path.join(HERE, "golden", "fit_schedule_voxels.npz"))
    ref_keys = [k[len("init/"):] for k in g.files if k.startswith("init/")]
    assert list(model.state_dict()) == ref_keys == ["voxels", "bias"]
    assert [tuple(p.shape) for p in params] == [(1, 4, 4, 4, 4), (1, 4)]


def test_new_symbols_are_exported():
    import fourier_feature_nets_amd as ffn
    from fourier_feature_nets_amd import _lib, ops
    assert "ffn_voxels_backward" in _lib.declared_symbols()
    assert "ffn_voxels_backward_workspace" in _lib.declared_symbols()
    assert "VoxelProgram" in ffn.__all__ and callable(ops.voxels_backward)
    lib = _lib.load()
    lib.ffn_voxels_backward            # noqa: B018 -- the library exports it
    # the workspace query is host logic: it sizes the buffers and refuses bad shapes
    small = ops.voxels_backward_workspace_bytes(1000, 16)
    assert small >= 4 * 16 ** 3 * 2 + 32 * 1000
    assert ops.voxels_backward_workspace_bytes(2000, 16) > small
    import pytest
    for n, side in [(-1, 16), (10, 0), (10, 1025), ((1 << 30) + 1, 8)]:
        with pytest.raises(_lib.FfnError):
            ops.voxels_backward_workspace_bytes(n, side)


def test_voxel_program_sizes():
    import fourier_feature_nets_amd as ffn
    prog = ffn.VoxelProgram(ffn.Voxels(8, 1.5))
    assert prog.num_grad_floats == 4 * 8 ** 3 + 4
    assert prog.plan_blocks(65) == 3
    assert prog.saved_floats(4096) * 4 >= ffn.ops.voxels_backward_workspace_bytes(4096, 8)

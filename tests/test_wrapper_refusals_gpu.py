"""The argument contract (tests/test_wrapper_refusals_cpu.py) on device tensors, for the wrappers
where a late refusal would cost most: those that work in place or take their outputs from the
caller, and those with several launches.  ``_lib.call`` is replaced by a hook that records the entry
point and raises -- it never forwards, so no kernel of the library runs here, with good arguments or
bad.  Per wrapper: the valid call passes every check and arrives at the hook; a mutated call raises,
the hook has seen no entry point (not even the first launch of several), and every tensor handed
in holds the bits it held."""

import pytest
import torch

from tests import refusal_cases as rc
from tests import stream_helpers as sh

pytestmark = pytest.mark.gpu

IN_PLACE = ["focus_sample_merge", "ycrcb_to_rgb_u8", "regression_train", "regression_eval",
            "clip_adam", "mse_loss", "voxels_backward", "octree_project", "octree_project_sh",
            "occupancy_from_octree", "MlpProgram.backward"]
SEVERAL_LAUNCHES = ["occupancy_compact", "octree_structure", "octree_mesh_faces", "octree_refine",
                    "octree_render_volume_backward", "MlpProgram.forward", "MlpProgram.render"]
GPU_ONLY = ["MlpProgram.forward16", "MlpProgram.pack", "MlpProgram.pack16"]


def _patterned(kwargs, marked):
    """Bits worth keeping: every tensor of an unmarked row gets a pattern (a marked row's values
    are what its checks read)."""
    if marked:
        return kwargs
    for value in kwargs.values():
        if torch.is_tensor(value) and value.numel():
            flat = torch.arange(value.numel(), device=value.device) % 251
            value.copy_(flat.reshape(value.shape).to(value.dtype))
    return kwargs


@pytest.mark.parametrize("subject", IN_PLACE + SEVERAL_LAUNCHES + GPU_ONLY)
def test_a_mutated_call_raises_before_the_first_launch(subject, monkeypatch):
    row = rc.ROWS[subject]
    device = torch.device("cuda", torch.cuda.current_device())
    kwargs = _patterned(row.build(rc.factory(device, True)), row.marked)
    fn, kwargs = row.target(kwargs)
    torch.cuda.synchronize()
    hook = rc.Hook().install(monkeypatch)
    kept = {name: value.clone() for name, value in kwargs.items() if torch.is_tensor(value)}

    kind, error = rc.outcome(fn, kwargs, hook)
    if subject == "MlpProgram.forward16" and isinstance(error, NotImplementedError):
        hook.seen.append("(a chain without split-bf16 kernels)")
    else:
        assert kind == rc.REACHED, "the valid call is %s: %r" % (kind, error)
    assert len(hook.seen) == 1, hook.seen       # the first launch, and nothing after the hook raised

    refused = 0
    for name, mutation, changed in rc.mutations(row, fn, kwargs):
        before = len(hook.seen)
        kind, error = rc.outcome(fn, changed, hook)
        where = "%s: %s = %s" % (subject, name, mutation)
        if (subject, name, mutation) in rc.ACCEPTED or mutation in row.defines.get(name, ()):
            assert kind == rc.REACHED, "%s is a legal call and is %s: %r" % (where, kind, error)
            continue
        assert kind == rc.REFUSED, "%s is %s: %r" % (where, kind, error)
        assert len(hook.seen) == before, "%s reached %s" % (where, hook.seen[before:])
        assert isinstance(error, ValueError) or mutation == "None", "%s: %r" % (where, error)
        assert rc.names_it(row, name, error), "%s: %s" % (where, error)
        refused += 1
    assert refused > 0 or not kept
    torch.cuda.synchronize()
    for name, value in kept.items():
        assert sh.same_bits(kwargs[name], value), "%s: %s changed" % (subject, name)

"""The stream-order cases of K33's three entry points, in the style of K32's.

tests/stream_order_cases.py is left as it is: importing this module appends the three cases to its
``CASES`` (the ``case`` decorator does), once.  tests/test_mesh_texture_cpu.py and
tests/test_mesh_texture_gpu.py import it, and pytest imports every test module before it runs a
test, so in a run that collects either of them -- the whole suite, or a marker selection of it --
tests/test_stream_order_cpu.py finds a case for all three entry points and
tests/test_stream_order_gpu.py, collected after them, runs the cases in both scenarios.  A run of
one of the stream-order files ALONE does not import this module; add
``tests/test_mesh_texture_cpu.py`` to such a command line."""

from tests.stream_order_cases import _f, _ops, _rng, _t, case
from tests.stream_order_cases_mesh_fit import _mesh_grad_state

TEX_H, TEX_W = 8, 4


def _mesh_texture_state(dev):
    """K31a-c of the ``mesh_raster`` case's scene -> (record, ids, triangles, uvs, width, height),
    structural apart from the uvs."""
    import numpy as np
    from tests import mesh_raster_reference as ref
    record, ids, _, _, width, height = _mesh_grad_state(dev)
    _, triangles, _, uvs = ref.scene(165, 65)
    return record, ids, _t(triangles, dev, np.int32), _t(uvs, dev, np.float32), width, height


def _mesh_taps_state(dev):
    """K33a and the sort on the default stream -> (tap_texel, tap_weight, sorted_texels, order)."""
    import torch
    record, ids, triangles, uvs, width, height = _mesh_texture_state(dev)
    tap_texel, tap_weight = _ops().mesh_texture_taps(record, ids, triangles, uvs, TEX_H, TEX_W,
                                                     width, height)
    sorted_texels, order = torch.sort(tap_texel.reshape(-1), stable=True)
    torch.cuda.synchronize()
    return tap_texel, tap_weight, sorted_texels.contiguous(), order.to(torch.int32).contiguous()


@case("mesh_texture_taps", ["uvs"], ["mesh_texture_taps"])
def _mesh_texture_taps(dev):
    record, ids, triangles, uvs, width, height = _mesh_texture_state(dev)
    live = dict(uvs=uvs)
    return live, lambda v: list(_ops().mesh_texture_taps(record, ids, triangles, v["uvs"], TEX_H,
                                                         TEX_W, width, height))


@case("mesh_texture_gather", ["texture"], ["mesh_texture_gather"])
def _mesh_texture_gather(dev):
    tap_texel, tap_weight, _, _ = _mesh_taps_state(dev)
    live = dict(texture=_t(_f(_rng(42), TEX_H * TEX_W, 3), dev))
    return live, lambda v: list(_ops().mesh_texture_gather(tap_texel, tap_weight, v["texture"],
                                                           (0.25, 0.5, 0.75)))


@case("mesh_texture_grad", ["d_color"], ["mesh_texture_grad"])
def _mesh_texture_grad(dev):
    tap_texel, tap_weight, sorted_texels, order = _mesh_taps_state(dev)
    live = dict(d_color=_t(_f(_rng(43), tap_texel.shape[0], 3, lo=-1, hi=1), dev))

    def run(v):
        ops = _ops()
        grad, weight = ops.mesh_texture_grad(sorted_texels, order, tap_weight, v["d_color"],
                                             TEX_H * TEX_W)
        again = ops.mesh_texture_grad(sorted_texels, order, tap_weight, v["d_color"],
                                      TEX_H * TEX_W, grad.clone(), weight.clone(),
                                      accumulate=True)
        return [grad, weight] + list(again)
    return live, run

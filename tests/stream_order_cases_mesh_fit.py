"""The stream-order cases of K32's two entry points, in the style of the ``mesh_raster`` case.

tests/stream_order_cases.py is left as it is: importing this module appends the two cases to its
``CASES`` (the ``case`` decorator does), once.  tests/test_mesh_fit_cpu.py and
tests/test_mesh_fit_gpu.py import it, and pytest imports every test module before it runs a test, so
in a run that collects either of them -- the whole suite, or a marker selection of it --
tests/test_stream_order_cpu.py finds a case for both entry points and tests/test_stream_order_gpu.py,
collected after them, runs the two cases in both scenarios.  A run of one of the stream-order files
ALONE does not import this module; add ``tests/test_mesh_fit_cpu.py`` to such a command line."""

from tests.stream_order_cases import _f, _ops, _rng, _t, case


def _mesh_grad_state(dev):
    """K31a-c of the ``mesh_raster`` case's scene on the default stream -> what K32 reads of it:
    (record, ids, corner_order, vertex_starts, width, height), structural."""
    import numpy as np
    import torch
    from fourier_feature_nets_amd import vertex_adjacency
    from fourier_feature_nets_amd.cameras import projection_matrices
    from tests import mesh_raster_reference as ref
    vertices, triangles, colors, _ = ref.scene(165, 65)
    width, height = 24, 20
    proj = projection_matrices([ref.camera(width, height)])[0]
    ops = _ops()
    vertices, triangles = _t(vertices, dev, np.float32), _t(triangles, dev, np.int32)
    record, _, counts = ops.mesh_raster_setup(vertices, triangles, proj, width, height)
    offsets, total = ops.mesh_raster_offsets(counts)
    zbuf = torch.full((width * height,), ops.MESH_RASTER_EMPTY, dtype=torch.int64, device=dev)
    ops.mesh_raster_draw(record, offsets, 0, total, width, height, zbuf)
    ids = ops.mesh_raster_resolve(zbuf, record, vertices, triangles, _t(colors, dev, np.float32),
                                  None, None, (0, 0, 0), (0, 0, 0), width, height)[3]
    assert int((ids >= 0).sum()) > 64
    order, starts = vertex_adjacency(triangles, vertices.shape[0], dev)
    torch.cuda.synchronize()
    return record, ids, order, starts, width, height


@case("mesh_raster_face_sums", ["d_color"], ["mesh_raster_face_sums"])
def _mesh_raster_face_sums(dev):
    record, ids, _, _, width, height = _mesh_grad_state(dev)
    live = dict(d_color=_t(_f(_rng(40), width * height, 3, lo=-1, hi=1), dev))
    return live, lambda v: [_ops().mesh_raster_face_sums(record, ids, v["d_color"], width, height)]


@case("mesh_vertex_gather", ["face_sums"], ["mesh_vertex_gather"])
def _mesh_vertex_gather(dev):
    record, ids, order, starts, width, height = _mesh_grad_state(dev)
    d_color = _t(_f(_rng(41), width * height, 3, lo=-1, hi=1), dev)
    live = dict(face_sums=_ops().mesh_raster_face_sums(record, ids, d_color, width, height))

    def run(v):
        ops = _ops()
        grad, weight = ops.mesh_vertex_gather(v["face_sums"], order, starts)
        again = ops.mesh_vertex_gather(v["face_sums"], order, starts, grad.clone(), weight.clone(),
                                       accumulate=True)
        return [grad, weight] + list(again)
    return live, run

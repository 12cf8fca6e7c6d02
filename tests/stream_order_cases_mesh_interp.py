"""The stream-order cases of K35's two entry points, in the style of K34's.

tests/stream_order_cases.py is left as it is: importing this module appends the two cases to its
``CASES`` (the ``case`` decorator does), once.  tests/test_k35_tables_cpu.py,
tests/test_mesh_interp_cpu.py and tests/test_mesh_interp_gpu.py import it, and pytest imports every
test module before it runs a test, so in a run that collects them -- the whole suite, or a marker
selection of it -- tests/test_stream_order_cpu.py finds a case for both entry points and
tests/test_stream_order_gpu.py, collected after them, runs the cases in both scenarios.
tests/test_memory_bounds_gpu.py lists its cases when it is collected, which is BEFORE
``test_mesh_*``: tests/test_k35_tables_cpu.py sorts in front of it for that reason, so that the two
cases run under the guarded placement there too.  A run of one of the stream-order or memory-bounds
files ALONE does not import this module; add ``tests/test_mesh_interp_cpu.py`` to such a command
line."""

from tests.stream_order_cases import _f, _ops, _rng, _t, case


def _mesh_interp_state(dev):
    """K31a-c of the ``mesh_raster`` case's scene on the default stream -> what K35 reads of it:
    dict(record, ids, colors, vertices, triangles, proj, order, starts, width, height)."""
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
    colors = _t(colors, dev, np.float32)
    record, _, counts = ops.mesh_raster_setup(vertices, triangles, proj, width, height)
    offsets, total = ops.mesh_raster_offsets(counts)
    zbuf = torch.full((width * height,), ops.MESH_RASTER_EMPTY, dtype=torch.int64, device=dev)
    ops.mesh_raster_draw(record, offsets, 0, total, width, height, zbuf)
    _, _, _, ids = ops.mesh_raster_resolve(zbuf, record, vertices, triangles, colors, None, None,
                                           (0, 0, 0), (0, 0, 0), width, height)
    assert int((ids >= 0).sum()) > 64
    order, starts = vertex_adjacency(triangles, vertices.shape[0], dev)
    torch.cuda.synchronize()
    return dict(record=record, ids=ids, colors=colors, vertices=vertices, triangles=triangles,
                proj=proj, order=order, starts=starts, width=width, height=height)


@case("mesh_interp_face_grads", ["d_color"], ["mesh_interp_face_grads"])
def _mesh_interp_face_grads(dev):
    s = _mesh_interp_state(dev)
    n = s["width"] * s["height"]
    live = dict(d_color=_t(_f(_rng(51), n, 3, lo=-1, hi=1), dev))
    return live, lambda v: [_ops().mesh_interp_face_grads(
        s["record"], s["ids"], v["d_color"], s["colors"], s["triangles"], s["width"], s["height"])]


@case("mesh_interp_vertex_grad", ["face_grads"], ["mesh_interp_vertex_grad"])
def _mesh_interp_vertex_grad(dev):
    import torch
    s = _mesh_interp_state(dev)
    n = s["width"] * s["height"]
    face_grads = _ops().mesh_interp_face_grads(
        s["record"], s["ids"], _t(_f(_rng(52), n, 3, lo=-1, hi=1), dev), s["colors"],
        s["triangles"], s["width"], s["height"])
    assert int((face_grads != 0).any(1).sum()) > 8
    torch.cuda.synchronize()
    live = dict(face_grads=face_grads)

    def run(v):
        ops = _ops()
        grad = ops.mesh_interp_vertex_grad(v["face_grads"], s["order"], s["starts"], s["vertices"],
                                           s["proj"])
        again = ops.mesh_interp_vertex_grad(v["face_grads"], s["order"], s["starts"],
                                            s["vertices"], s["proj"], grad.clone(),
                                            accumulate=True)
        return [grad, again]
    return live, run

"""The stream-order cases of K34's four entry points, in the style of K33's.

tests/stream_order_cases.py is left as it is: importing this module appends the four cases to its
``CASES`` (the ``case`` decorator does), once.  tests/test_mesh_aa_cpu.py and
tests/test_mesh_aa_gpu.py import it, and pytest imports every test module before it runs a test, so
in a run that collects either of them -- the whole suite, or a marker selection of it --
tests/test_stream_order_cpu.py finds a case for all four entry points and
tests/test_stream_order_gpu.py, collected after them, runs the cases in both scenarios.  A run of
one of the stream-order files ALONE does not import this module; add ``tests/test_mesh_aa_cpu.py``
to such a command line."""

from tests.stream_order_cases import _f, _ops, _rng, _t, case


def _mesh_aa_state(dev):
    """K31a-c of the ``mesh_raster`` case's scene on the default stream -> what K34 reads of it:
    dict(record, zbuf, ids, color, alpha, opposite, vertices, triangles, proj, width, height)."""
    import numpy as np
    import torch
    from fourier_feature_nets_amd import edge_opposites
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
    color, alpha, _, ids = ops.mesh_raster_resolve(
        zbuf, record, vertices, triangles, _t(colors, dev, np.float32), None, None, (0, 0, 0),
        (0, 0, 0), width, height)
    assert int((ids >= 0).sum()) > 64
    torch.cuda.synchronize()
    return dict(record=record, zbuf=zbuf, ids=ids, color=color, alpha=alpha,
                opposite=edge_opposites(triangles, vertices.shape[0], dev), vertices=vertices,
                triangles=triangles, proj=proj, width=width, height=height)


def _mesh_aa_entries(dev):
    """K34b and the sort on the default stream -> (state, sorted_vertex, order, entry_grad)."""
    import torch
    s = _mesh_aa_state(dev)
    n = s["width"] * s["height"]
    _, _, entry_vertex, entry_grad = _ops().mesh_aa_backward(
        s["record"], s["zbuf"], s["ids"], s["opposite"], s["vertices"], s["triangles"], s["proj"],
        s["color"], s["alpha"], _t(_f(_rng(44), n, 3, lo=-1, hi=1), dev),
        _t(_f(_rng(45), n, lo=-1, hi=1), dev), s["width"], s["height"])
    sorted_vertex, order = torch.sort(entry_vertex, stable=True)
    assert int((entry_vertex < s["vertices"].shape[0]).sum()) > 64
    torch.cuda.synchronize()
    return s, sorted_vertex.contiguous(), order.to(torch.int32).contiguous(), entry_grad


@case("mesh_aa_forward", ["color"], ["mesh_aa_forward"])
def _mesh_aa_forward(dev):
    s = _mesh_aa_state(dev)
    live = dict(color=s["color"])
    return live, lambda v: list(_ops().mesh_aa_forward(
        s["record"], s["zbuf"], s["ids"], s["opposite"], s["vertices"], s["proj"], v["color"],
        s["alpha"], s["width"], s["height"]))


@case("mesh_aa_backward", ["g_color"], ["mesh_aa_backward"])
def _mesh_aa_backward(dev):
    s = _mesh_aa_state(dev)
    n = s["width"] * s["height"]
    g_alpha = _t(_f(_rng(47), n, lo=-1, hi=1), dev)
    live = dict(g_color=_t(_f(_rng(46), n, 3, lo=-1, hi=1), dev))
    return live, lambda v: list(_ops().mesh_aa_backward(
        s["record"], s["zbuf"], s["ids"], s["opposite"], s["vertices"], s["triangles"], s["proj"],
        s["color"], s["alpha"], v["g_color"], g_alpha, s["width"], s["height"]))


@case("mesh_aa_vertex_grad", ["entry_grad"], ["mesh_aa_vertex_grad"])
def _mesh_aa_vertex_grad(dev):
    s, sorted_vertex, order, entry_grad = _mesh_aa_entries(dev)
    live = dict(entry_grad=entry_grad)

    def run(v):
        ops = _ops()
        grad = ops.mesh_aa_vertex_grad(sorted_vertex, order, v["entry_grad"], s["vertices"],
                                       s["proj"])
        again = ops.mesh_aa_vertex_grad(sorted_vertex, order, v["entry_grad"], s["vertices"],
                                        s["proj"], grad.clone(), accumulate=True)
        return [grad, again]
    return live, run


@case("mesh_laplacian", ["values"], ["mesh_laplacian"])
def _mesh_laplacian(dev):
    import numpy as np
    from fourier_feature_nets_amd import vertex_neighbors
    rng = _rng(48)
    triangles = rng.integers(0, 300, (257, 3)).astype(np.int32)
    starts, neighbors = vertex_neighbors(triangles, 300, dev)
    live = dict(values=_t(_f(rng, 300, 3, lo=-1, hi=1), dev))

    def run(v):
        ops = _ops()
        out = ops.mesh_laplacian(v["values"], starts, neighbors, 0.75)
        again = ops.mesh_laplacian(v["values"], starts, neighbors, 0.75, out.clone(),
                                   accumulate=True)
        return [out, again]
    return live, run

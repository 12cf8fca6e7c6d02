"""The stream-order cases of K36's four entry points, in the style of K35's.

tests/stream_order_cases.py is left as it is: importing this module appends the four cases to its
``CASES`` (the ``case`` decorator does), once.  tests/test_k36_tables_cpu.py and
tests/test_mesh_cast_gpu.py import it, and pytest imports every test module before it runs a test, so
in a run that collects them -- the whole suite, or a marker selection of it --
tests/test_stream_order_cpu.py finds a case for all four entry points and
tests/test_stream_order_gpu.py, collected after them, runs the cases in both scenarios.
tests/test_memory_bounds_gpu.py lists its cases when it is collected, which is BEFORE
``test_mesh_*``: tests/test_k36_tables_cpu.py sorts in front of it for that reason, so that the
four cases run under the guarded placement there too.  A run of one of the stream-order or
memory-bounds files ALONE does not import this module; add ``tests/test_k36_tables_cpu.py`` to such
a command line.

Shapes: 65 triangles, four to a leaf (17 leaves under 5 levels, the last 15 leaf slots empty), and
300 rays: past one workgroup of 256, ragged."""

from tests.stream_order_cases import _f, _ops, _rng, _t, case

LEAF = 4
RAYS = 300


def _mesh_cast_state(dev):
    """K36a/b on the ``mesh_raster`` case's scene, on the default stream -> dict(vertices,
    triangles, colors, uvs, boxes, keys, order, nodes, pad, grid_lo, grid_scale)."""
    import numpy as np
    import torch
    from tests import mesh_cast_reference as cast_ref
    from tests import mesh_raster_reference as ref
    vertices, triangles, colors, uvs = ref.scene(165, 65)
    pad = float(cast_ref.default_pad(vertices))
    grid_lo, grid_scale = cast_ref.grid_of(vertices)
    ops = _ops()
    s = dict(vertices=_t(vertices, dev, np.float32), triangles=_t(triangles, dev, np.int32),
             colors=_t(colors, dev, np.float32), uvs=_t(uvs, dev, np.float32), pad=pad,
             grid_lo=[float(c) for c in grid_lo], grid_scale=float(grid_scale))
    s["boxes"], s["keys"] = ops.mesh_cast_boxes(s["vertices"], s["triangles"], pad, s["grid_lo"],
                                                s["grid_scale"])
    torch.cuda.synchronize()
    s["order"] = _t(cast_ref.order_of(s["keys"].cpu().numpy()), dev, np.int32)
    s["nodes"] = ops.mesh_cast_tree(s["boxes"], s["order"], LEAF)
    torch.cuda.synchronize()
    return s


def _mesh_cast_rays(dev, seed):
    from tests import mesh_cast_reference as cast_ref
    starts, directions = cast_ref.random_rays(seed, RAYS)
    return _t(starts, dev), _t(directions, dev)


@case("mesh_cast_boxes", ["vertices"], ["mesh_cast_boxes"])
def _mesh_cast_boxes(dev):
    s = _mesh_cast_state(dev)
    live = dict(vertices=s["vertices"])
    return live, lambda v: list(_ops().mesh_cast_boxes(v["vertices"], s["triangles"], s["pad"],
                                                       s["grid_lo"], s["grid_scale"]))


@case("mesh_cast_tree", ["boxes"], ["mesh_cast_tree"])
def _mesh_cast_tree(dev):
    s = _mesh_cast_state(dev)
    live = dict(boxes=s["boxes"])
    return live, lambda v: [_ops().mesh_cast_tree(v["boxes"], s["order"], LEAF)]


@case("mesh_cast", ["starts"], ["mesh_cast"])
def _mesh_cast(dev):
    import torch
    s = _mesh_cast_state(dev)
    starts, directions = _mesh_cast_rays(dev, 53)
    hit = _ops().mesh_cast(s["nodes"], s["boxes"], s["order"], s["vertices"], s["triangles"],
                           starts, directions, LEAF)[0]
    assert int((hit >= 0).sum()) > 64
    torch.cuda.synchronize()
    live = dict(starts=starts)

    def run(v):
        ops = _ops()
        mesh = (s["nodes"], s["boxes"], s["order"], s["vertices"], s["triangles"])
        return list(ops.mesh_cast(*mesh, v["starts"], directions, LEAF)) \
            + list(ops.mesh_cast(*mesh, v["starts"], directions, LEAF, 0.25, True))
    return live, run


@case("mesh_cast_shade", ["u"], ["mesh_cast_shade"])
def _mesh_cast_shade(dev):
    import numpy as np
    import torch
    from tests import mesh_raster_reference as ref
    s = _mesh_cast_state(dev)
    starts, directions = _mesh_cast_rays(dev, 54)
    hit, t, u, v = _ops().mesh_cast(s["nodes"], s["boxes"], s["order"], s["vertices"],
                                    s["triangles"], starts, directions, LEAF)
    assert int((hit >= 0).sum()) > 64
    texture = _t(ref.texture(55, 5, 7, 3), dev, np.uint8)
    torch.cuda.synchronize()
    live = dict(u=u)

    def run(w):
        ops = _ops()
        return list(ops.mesh_cast_shade(hit, t, w["u"], v, s["triangles"], s["colors"], None, None,
                                        (0.25, 0.5, 0.75))) \
            + list(ops.mesh_cast_shade(hit, t, w["u"], v, s["triangles"], None, s["uvs"], texture,
                                       (0.25, 0.5, 0.75)))
    return live, run

"""The rows of K36's four wrappers in the table of the argument-contract tests.

tests/refusal_cases.py is left as it is: importing this module adds the four rows to its ``ROWS``
(the ``row`` decorator does), once.  The test modules that import
tests/stream_order_cases_mesh_cast.py import this one too, for the same reason and with the same
consequence: a run of tests/test_wrapper_refusals_cpu.py ALONE does not have the rows; add
``tests/test_k36_tables_cpu.py`` to such a command line.  The sizes are ``refusal_cases``' own
constants; the rows read no values, are not ``gpu_only`` and add no exemption."""

from tests import refusal_cases as rc

LEAF = 4
LEVELS = 2                      # rc.F = 8 triangles, four to a leaf: two leaves under a root
NODES = (1 << LEVELS) - 1
LEAF_INTS = dict(leaf_size=(1, 64))


@rc.row("mesh_cast_boxes", defines=dict(vertices="row-1", triangles="row-1"))
def _cast_boxes(make):
    return dict(vertices=make((rc.V, 3)), triangles=make((rc.F, 3), rc.i32()), pad=0.125,
                grid_lo=(0.0, -1.0, 0.5), grid_scale=2.0)


@rc.row("mesh_cast_tree", ints=LEAF_INTS, blames=dict(boxes=("order",)))
def _cast_tree(make):
    return dict(boxes=make((rc.F, 6)), order=make((rc.F,), rc.i32()), leaf_size=LEAF)


@rc.row("mesh_cast", ints=LEAF_INTS,
        blames=dict(triangles=("boxes",), starts=("directions",)), defines=dict(vertices="row-1"))
def _cast(make):
    return dict(nodes=make((NODES, 6)), boxes=make((rc.F, 6)), order=make((rc.F,), rc.i32()),
                vertices=make((rc.V, 3)), triangles=make((rc.F, 3), rc.i32()),
                starts=make((rc.R, 3)), directions=make((rc.R, 3)), leaf_size=LEAF, t_min=0.25,
                farthest=True)


@rc.row("mesh_cast_shade", optional=("colors", "uvs", "texture"), blames=dict(hit=("t",)),
        defines=dict(triangles="row-1", colors="row-1"))
def _cast_shade(make):
    return dict(hit=make((rc.R,), rc.i32()), t=make((rc.R,)), u=make((rc.R,)), v=make((rc.R,)),
                triangles=make((rc.F, 3), rc.i32()), colors=make((rc.V, 3)), uvs=None,
                texture=None, background=(0.0, 0.5, 1.0))

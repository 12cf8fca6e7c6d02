"""The rows of K35's two wrappers in the table of the argument-contract tests.

tests/refusal_cases.py is left as it is: importing this module adds the two rows to its ``ROWS``
(the ``row`` decorator does), once.  The test modules that import
tests/stream_order_cases_mesh_interp.py import this one too, for the same reason and with the same
consequence: a run of tests/test_wrapper_refusals_cpu.py ALONE does not have the rows; add
``tests/test_mesh_interp_cpu.py`` to such a command line.  The sizes are ``refusal_cases``' own
constants; the rows read no values, are not ``gpu_only`` and add no exemption."""

from tests import refusal_cases as rc


@rc.row("mesh_interp_face_grads", ints=rc.FRAME_INTS, blames=dict(triangles=("record",)),
        defines=dict(colors="row-1"))
def _interp_face_grads(make):
    return dict(record=make((rc.F, 16), rc.i32()), ids=make((rc.W * rc.H,), rc.i32()),
                d_color=make((rc.W * rc.H, 3)), colors=make((rc.V, 3)),
                triangles=make((rc.F, 3), rc.i32()), width=rc.W, height=rc.H)


@rc.row("mesh_interp_vertex_grad",
        blames=dict(face_grads=("corner_order",), vertices=("vertex_starts", "grad")))
def _interp_vertex_grad(make):
    return dict(face_grads=make((rc.F, 9)), corner_order=make((3 * rc.F,), rc.i32()),
                vertex_starts=make((rc.V + 1,), rc.i32()), vertices=make((rc.V, 3)),
                proj=rc._proj(), grad=make((rc.V, 3)), accumulate=True)

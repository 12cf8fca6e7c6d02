"""Every kernel entry point stays inside its buffers: it writes only through its non-``const``
pointers and only within them, writes every output word its comment does not call undefined, and
reads its inputs only within their extents (the contract in the preamble of include/ffn_hip.h).

Each case of tests/stream_order_cases.py is built and run three times: once on plain torch memory
(``plain``), then under the guarded placement of tests/memory_helpers.py with fill A and with fill
B.  Under the placement every ``torch.empty`` / ``torch.zeros`` buffer of the wrappers, every
workspace an object keeps, every clone or ``torch.full`` buffer an in-place entry point works on
and every input the builders make lies between two red zones that hold the fill, and fresh
``torch.empty`` memory holds it too.  Then

* no byte of any red zone has changed (a write outside a buffer);
* the outputs under fill A are the bits of ``plain`` (the placement changes nothing);
* the outputs under fill A are the bits of those under fill B: a difference whose words equal the
  fills is an output word that was never written, any other a read outside an input;
* a hook on ``_lib.call`` holds every call to the header's ``const``: a guarded buffer reached only
  through ``const`` parameters holds the same bytes after the call, every pointer passed through a
  non-``const`` parameter lies in a guarded payload (EXCEPTIONS), and the case's ``live`` tensors
  hold the same bits after the run.

What the float64 tests of each family hold the values to is not re-derived here.  The controls
show with torch operations alone that an overrun, an unwritten word, an outside read and a
written input ARE seen, each on its own and through the whole check of a case; if they fail, the
cases prove nothing.

Measured on an MI355X (printed by the last test, not asserted): of the 2168 ``const`` device
pointers the calls of the 98 cases passed under both fills, 1364 (62.9 %) pointed into a guarded
buffer as they came; the other 804 (37.1 %: job tables, sorted arrays, linspaces and parameters
that torch made) were moved into a guarded copy for the call by the hook, none was left
unguarded.  No case wrote outside a buffer, left a defined word unwritten, read outside an input
or wrote an input.  The module takes 5 s."""

import pytest
import torch

from tests import memory_helpers as mh
from tests import stream_helpers as sh
from tests import stream_order_cases as cases
from tests import stream_order_cases_mesh_aa  # noqa: F401  (the table as the whole suite has it)
from tests import stream_order_cases_mesh_fit  # noqa: F401
from tests import stream_order_cases_mesh_texture  # noqa: F401
from tests.stream_order_cases import CASES

pytestmark = pytest.mark.gpu

# (entry point, parameter) -> why the pointer a case passes there is not a guarded buffer.  A
# written pointer that is neither guarded nor listed fails its case; a row whose pointer was
# guarded wherever the session saw it fails the last test.
EXCEPTIONS = {
    ("ffn_octree_project", "leaf_data"):
        "in place on the cases' descent step, leaf_data - 0.5 * grad: torch's subtraction "
        "allocates its result itself",
    ("ffn_octree_project_sh", "leaf_rows"):
        "in place on the cases' descent step, leaf_rows - 0.5 * grad: torch's subtraction "
        "allocates its result itself",
}

# case -> (the sentence of include/ffn_hip.h that leaves words of an output undefined,
#          outputs -> one mask of the defined words per output, or None for "all").  Such an output
# is compared on its defined words only, under both fills and with ``plain`` (whose other words are
# whatever torch.empty found); the red zones are never masked.
UNDEFINED = {
    "sample_t[wide rows]": (
        "t_out       (R, t_stride) -- the first `count` entries of each row are written",
        lambda outputs: [torch.arange(cases.S + 7) < cases.S]),
}


# A case of this module's own (the stream-order table holds none with undefined words): K2a into
# rows of 24 floats, as the focus sampler calls it before it merges its own samples in.
def _sample_t_wide(dev):
    from fourier_feature_nets_amd import ops
    live, rng = cases._sampler_state(dev, 2)
    live["noise"] = cases._t(cases._f(rng, cases.R, cases.S), dev)
    unit = torch.linspace(0, 1, cases.S, device=dev)

    def run(v):
        out = torch.empty((cases.R, cases.S + 7), dtype=torch.float32, device=dev)
        return [ops.sample_t(v["near_far"], v["ray_index"], cases.S, unit, v["noise"], 0.5, out=out)]
    return live, run


EXTRA = [cases.Case("sample_t[wide rows]", _sample_t_wide, ["near_far", "ray_index", "noise"],
                    ["sample_t"])]

_REACHED, _RAN = set(), set()
_CONST = [0, 0, 0]      # const pointer arguments seen, guarded as they came, moved for the call
_UNGUARDED_WRITTEN, _UNGUARDED_CONST = set(), set()


# ------------------------------------------------------------------------------------ controls
def _guards():
    return [mh.Guard(fill) for fill in ("A", "B")]


def test_control_a_write_just_past_a_payload_is_reported():
    for guard in _guards():
        buf = guard.buffer((257,), torch.float32, "cuda", "empty")
        other = guard.buffer((65, 48), torch.int32, "cuda", "zeros")
        assert buf.start % mh.ALIGN == 0 and guard.damage() == []
        end = buf.offset + buf.nbytes
        buf.base[end:end + 4].view(torch.float32).fill_(2.0)     # the base allocation owns it
        torch.cuda.synchronize()
        found = guard.damage()
        assert len(found) == 1 and "(257,)" in found[0] and "torch.float32" in found[0], found
        assert "1 elements of the right zone changed, 0 .. 3 bytes past the payload's end" \
            in found[0], found
        assert other.damage() is None
        other.base[other.offset - 8:other.offset - 4].view(torch.int32).fill_(7)
        assert "1 elements of the left zone changed, 8 .. 5 bytes before the payload's start" \
            in other.damage()


def test_control_b_a_payload_left_as_empty_made_it_differs_between_the_fills(monkeypatch):
    got = {}
    for guard in _guards():
        with monkeypatch.context() as patch:
            guard.patch(patch)
            got[guard.name] = [torch.empty((300, 17), device="cuda"),
                               torch.empty_like(torch.zeros(257, dtype=torch.int32, device="cuda")),
                               torch.zeros((3,), device="cuda")]
        assert len(guard.buffers) == 4 and guard.find(got[guard.name][0].data_ptr()).kind == "empty"
    for k, fills in enumerate(zip(*mh.FILLS.values())):
        assert not sh.same_bits(got["A"][k], got["B"][k])
        assert bool((got["A"][k] == fills[0]).all()) and bool((got["B"][k] == fills[1]).all())
    assert sh.same_bits(got["A"][2], got["B"][2]) and not bool(got["A"][2].any())
    assert type(torch.empty(3, device="cuda")) is torch.Tensor and torch.empty is mh._RAW["empty"]


def test_control_c_a_gather_one_element_past_an_input_sees_the_fill():
    values = torch.arange(1, 258, dtype=torch.float32, device="cuda")
    got = {}
    for guard in _guards():
        placed = guard.place(values)
        buf = guard.find(placed.data_ptr())
        assert buf is not None and buf.kind == "input" and torch.equal(placed, values)
        through_base = buf.base[buf.offset:buf.offset + buf.nbytes + 4].view(torch.float32)
        got[guard.name] = through_base[torch.arange(258, device="cuda")]
        assert guard.damage() == []
    assert torch.equal(got["A"][:257], got["B"][:257])
    assert not torch.equal(got["A"], got["B"])
    assert float(got["A"][257]) == mh.FILLS["A"][0] and float(got["B"][257]) == mh.FILLS["B"][0]


def _beyond(t, count):
    """``t`` (1-D) and the ``count`` elements behind it, through the allocation that holds it; under
    the placement those are the first of its right red zone.  On plain memory: ``t`` itself."""
    if t.untyped_storage().nbytes() < (t.storage_offset() + t.numel() + count) * t.element_size():
        return t
    return torch.empty(0, dtype=t.dtype, device=t.device).set_(
        t.untyped_storage(), t.storage_offset(), (t.numel() + count,))


_MISBEHAVIOUR = {
    "a tail store": "a write outside: (257,) torch.float32 buffer (empty), arguments of no call: "
                    "1 elements of the right zone changed, 0 .. 3 bytes past the payload's end",
    "a skipped word": "output 0 ((257,) torch.float32, from torch.empty): 1 words differ, flat "
                      "indices 256 .. 256: words that were never written",
    "a read beyond": "output 0 ((257,) torch.float32, from torch.empty): 1 words differ, flat "
                     "indices 256 .. 256: values computed from a read outside an input",
    "a written input": "the run changed its live tensors ['x']",
}


@pytest.mark.parametrize("kind", list(_MISBEHAVIOUR) + ["none"])
def test_control_d_a_case_of_torch_operations_that_misbehaves_fails_as_it_should(kind, monkeypatch):
    """The whole of ``_check`` on a case that calls no entry point: ``out = 2 x`` over 257 floats,
    right, or wrong in one of the four ways the cases are held to (every access stays inside the
    allocations of the placement)."""
    def build(dev):
        live = dict(x=cases._t(cases._f(cases._rng(50), 257, lo=1.0, hi=2.0), dev))

        def run(v):
            x, out = v["x"], torch.empty((257,), dtype=torch.float32, device=dev)
            if kind == "a skipped word":
                torch.mul(x[:256], 2.0, out=out[:256])
                if out.untyped_storage().nbytes() == 257 * 4:       # plain memory: the right answer
                    torch.mul(x[256:], 2.0, out=out[256:])
                return [out]
            torch.mul(x, 2.0, out=out)
            if kind == "a tail store" and _beyond(out, 1) is not out:
                _beyond(out, 1)[-1:].fill_(2.0)
            if kind == "a read beyond":
                out[256:] += _beyond(x, 1)[-1:] - x[256:]           # + 0 on plain memory
            if kind == "a written input":
                x[3] = 0.0
            return [out]
        return live, run
    case = cases.Case("torch only: " + kind, build, ["x"], [])
    if kind == "none":
        guard = _check(case, monkeypatch)
        assert len(guard.buffers) == 2 and not guard.reached
    else:
        with pytest.raises(AssertionError) as failure:
            _check(case, monkeypatch)
        assert _MISBEHAVIOUR[kind] in str(failure.value), str(failure.value)


# ------------------------------------------------------------------------------------ one case
def _bits(t):
    width = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]
    return t.contiguous().reshape(-1).view(width)


def _run(case, guard, hook, monkeypatch):
    """Builds and runs ``case`` (under ``guard``, or on plain memory for None) -> the clones of
    its outputs and, per output, the kind of the guarded buffer it lies in (or None)."""
    dev = torch.device("cuda:0")
    with monkeypatch.context() as patch:
        cases._MODELS.clear()               # the chains keep workspaces: built under this placement
        if guard is not None:
            guard.patch(patch)
            hook.active = guard
        try:
            live, run = case.build(dev)
            _, kept, _ = sh.take_extras(live)
            sh.keep_answers(patch, kept)
            if guard is not None:
                for key, t in live.items():
                    if torch.is_tensor(t) and guard.find(t.data_ptr()) is None:
                        live[key] = guard.place(t)
            before = {key: mh.raw_clone(t) for key, t in live.items()}
            outputs = list(run(live))
            torch.cuda.synchronize()
            kinds = [None if o is None or guard is None or guard.find(o.data_ptr()) is None
                     else guard.find(o.data_ptr()).kind for o in outputs]
            got = [None if o is None else mh.raw_clone(o) for o in outputs]
            changed = [key for key, t in live.items() if not sh.same_bits(t, before[key])]
            assert not changed, "%s: the run changed its live tensors %s" % (case.name, changed)
        finally:
            hook.active = None
            cases._MODELS.clear()
        torch.cuda.synchronize()
    return got, kinds


def _explain(k, a, b, kind, fills):
    """Why output ``k`` differs between the fills."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return "output %d: %s %s under A, %s %s under B" % (k, tuple(a.shape), a.dtype,
                                                             tuple(b.shape), b.dtype)
    where = (_bits(a) != _bits(b)).nonzero().reshape(-1)
    fill_a, fill_b = (f[0] if a.dtype.is_floating_point else f[1] for f in fills)
    is_fill = bool((a.reshape(-1)[where] == fill_a).all() and (b.reshape(-1)[where] == fill_b).all())
    if is_fill and kind == "empty":
        what = "words that were never written (they hold the fills)"
    elif is_fill:
        what = "the fills themselves, copied from outside an input or from an unwritten word"
    else:
        what = "values computed from a read outside an input (or of an unwritten word)"
    return "output %d (%s %s, from %s): %d words differ, flat indices %d .. %d: %s" % (
        k, tuple(a.shape), a.dtype, "torch.%s" % kind if kind else "a torch operation",
        where.numel(), int(where[0]), int(where[-1]), what)


def _check(case, monkeypatch):
    """The three runs of ``case`` and every assertion on them -> the guard of the run under fill A."""
    from fourier_feature_nets_amd import _lib
    for name, value in case.env.items():
        monkeypatch.setenv(name, value)
    hook = mh.Hook(_lib.call)
    monkeypatch.setattr(_lib, "call", hook)
    plain, _ = _run(case, None, hook, monkeypatch)
    guard_a, guard_b = _guards()
    got_a, kinds = _run(case, guard_a, hook, monkeypatch)
    got_b, _ = _run(case, guard_b, hook, monkeypatch)
    problems = []
    for guard in (guard_a, guard_b):
        _CONST[0] += guard.const_seen
        _CONST[1] += guard.const_guarded
        _CONST[2] += guard.const_moved
        _UNGUARDED_WRITTEN.update(guard.unguarded_written)
        _UNGUARDED_CONST.update((case.name,) + pair for pair in guard.const_unguarded)
        problems += ["fill %s, a write outside: %s" % (guard.name, d) for d in guard.damage()]
        problems += ["fill %s: %s" % (guard.name, p) for p in guard.problems]
        problems += ["fill %s: %s writes through %s, which is not a guarded buffer and not listed in "
                     "EXCEPTIONS" % (guard.name, entry, param)
                     for entry, param in sorted(guard.unguarded_written - set(EXCEPTIONS))]
        missing = sorted(set(case.reaches) - set(guard.reached))
        assert not missing, "%s does not reach %s" % (case.name, missing)
    assert len(plain) == len(got_a) == len(got_b)
    masks = UNDEFINED[case.name][1](got_a) if case.name in UNDEFINED else [None] * len(got_a)
    assert len(masks) == len(got_a)

    def defined(t, mask):
        if mask is None or t is None:
            return t
        return torch.where(mask.to(t.device).expand(t.shape), t, torch.zeros_like(t))

    problems += ["output %d is listed in UNDEFINED, but holds the same bits under both fills" % k
                 for k, mask in enumerate(masks) if mask is not None and got_a[k] is not None
                 and sh.same_bits(got_a[k], got_b[k])]
    plain, got_a, got_b = ([defined(t, m) for t, m in zip(got, masks)]
                           for got in (plain, got_a, got_b))
    problems += ["output %d differs between plain and guarded memory" % k
                 for k in sh.differing(got_a, plain)]
    for k, (a, b) in enumerate(zip(got_a, got_b)):
        if a is None or b is None:
            if not (a is None and b is None):
                problems.append("output %d is None under one fill only" % k)
        elif not sh.same_bits(a, b):
            problems.append(_explain(k, a, b, kinds[k], (mh.FILLS["A"], mh.FILLS["B"])))
    print("memory bounds: %s reached %s; %d guarded buffers; of %d const pointer arguments %d were "
          "guarded as they came and %d in a copy made for the call"
          % (case.name, ", ".join(sorted(set(guard_a.reached))), len(guard_a.buffers),
             guard_a.const_seen, guard_a.const_guarded, guard_a.const_moved))
    assert not problems, "%s:\n  %s" % (case.name, "\n  ".join(problems))
    return guard_a


@pytest.mark.parametrize("case", CASES + EXTRA, ids=[c.name for c in CASES + EXTRA])
def test_every_entry_point_stays_inside_its_buffers(case, monkeypatch):
    _REACHED.update(_check(case, monkeypatch).reached)
    _RAN.add(case.name)


def test_the_cases_reached_every_stream_taking_entry_point_under_the_guard():
    """Judged only when every case has run (and passed) in this session, as the last test of
    tests/test_stream_order_gpu.py is; a selection of cases is skipped."""
    if _CONST[0]:
        print("memory bounds: of %d const pointer arguments %d were guarded as they came (%.1f %%) and "
              "%d in a copy made for the call (%.1f %%); guarded in neither way: %s"
              % (_CONST[0], _CONST[1], 100.0 * _CONST[1] / _CONST[0], _CONST[2],
                 100.0 * _CONST[2] / _CONST[0],
                 ", ".join("%s: %s(%s)" % row for row in sorted(_UNGUARDED_CONST)) or "none"))
    if len(_RAN) < len(CASES + EXTRA):
        pytest.skip("only %d of %d cases passed in this session" % (len(_RAN), len(CASES + EXTRA)))
    missing = sorted(set(sh.stream_entry_points()) - _REACHED - set(cases.UNREACHED))
    assert not missing, "no case reached %s under the guarded placement" % missing
    stale = sorted(set(EXCEPTIONS) - _UNGUARDED_WRITTEN)
    assert not stale, "listed in EXCEPTIONS, but guarded wherever a case passed it: %s" % stale

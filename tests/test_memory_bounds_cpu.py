"""The harness of the memory-bounds tests (tests/memory_helpers.py) on its own, without a GPU: the
header parser, the guarded placement on CPU tensors with the three controls of
tests/test_memory_bounds_gpu.py, and that test's two tables against include/ffn_hip.h."""

import ast
import inspect
import re

import pytest
import torch

from tests import memory_helpers as mh
from tests import stream_helpers as sh

DTYPES = [torch.float32, torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8,
          torch.uint32, torch.bool]                 # what the wrappers hand to the library
SIZES = [1, 3, 255, 4097]


# ------------------------------------------------------------------------------------ the header
def test_every_declared_entry_point_parses():
    sigs = mh.signatures()
    indirect = set()
    assert sorted(sigs) == sh.stream_entry_points() and len(sigs) >= 105
    for name, params in sigs.items():
        names = [p.name for p in params]
        assert len(set(names)) == len(names), name
        assert params[-1].text == "void* stream", name
        for p in params:
            assert re.fullmatch(r"(const )?[A-Za-z_][A-Za-z0-9_]*\*? [A-Za-z_][A-Za-z0-9_]*", p.text), \
                "%s: %r" % (name, p.text)
            assert p.pointer == ("*" in p.text) and (not p.const or p.pointer)
        if not mh.written(name, sigs):
            indirect.add(name)
    # the two whose outputs are named by a table: the jobs of the pack (device memory) and the
    # ffn_render_out of the fused render (a host struct).  The call hook cannot see those pointers;
    # the red zones and the two fills hold their buffers like every other
    assert indirect == {"ffn_mlp_pack_jobs", "ffn_render_fused_fwd"}


def test_the_outputs_are_the_non_const_pointers():
    assert mh.written("ffn_mesh_aa_backward") == ["d_color", "d_alpha", "entry_vertex", "entry_grad"]
    assert mh.written("ffn_clip_adam")[:4] == ["params", "grads", "exp_avg", "exp_avg_sq"]
    assert mh.written("ffn_clip_adam")[4:] == ["scratch", "grad_norm_out"]
    assert mh.written("ffn_raygen_nearfar") == ["starts", "directions", "near_far", "valid"]
    assert mh.written("ffn_sample_t") == ["t_out"]
    assert mh.written("ffn_focus_sample_merge") == ["t_io"]
    assert mh.written("ffn_cdf_build") == ["cdf"]
    sigs = mh.signatures()
    const = [p.name for p in sigs["ffn_raygen_nearfar"] if p.const]
    assert const == ["unproj", "cam_pos", "points", "box_lo", "box_hi"]


def _arguments_in_ops(entry):
    """How many arguments the wrappers' ``_call(entry, ...)`` sites pass (from the source)."""
    from fourier_feature_nets_amd import ops
    counts = set()
    for node in ast.walk(ast.parse(inspect.getsource(ops))):
        if (isinstance(node, ast.Call) and getattr(node.func, "id", None) == "_call" and node.args
                and any(isinstance(c, ast.Constant) and c.value == entry
                        for c in ast.walk(node.args[0]))):
            assert not any(isinstance(a, ast.Starred) for a in node.args)
            counts.add(len(node.args) - 1)
    return counts


@pytest.mark.parametrize("entry", ["ffn_mesh_aa_backward", "ffn_clip_adam", "ffn_raygen_nearfar",
                                   "ffn_sample_t", "ffn_cdf_build"])
def test_the_parameter_count_is_what_the_wrappers_pass(entry):
    assert _arguments_in_ops(entry) == {len(mh.signatures()[entry]) - 1}    # less ``stream``


# ------------------------------------------------------------------------------------ placement
@pytest.mark.parametrize("fill", ["A", "B"])
@pytest.mark.parametrize("dtype", DTYPES, ids=[str(d) for d in DTYPES])
def test_guarded_buffers_are_placed_as_torch_empty_places_them(dtype, fill):
    guard = mh.Guard(fill, "cpu")
    want = mh.FILLS[fill][0 if dtype.is_floating_point else 1]
    for n in SIZES:
        for kind in ("empty", "zeros"):
            buf = guard.buffer((n,), dtype, "cpu", kind)
            t = buf.tensor
            assert t.shape == (n,) and t.dtype == dtype and t.is_contiguous()
            assert t.data_ptr() == buf.start and buf.start % mh.ALIGN == 0
            assert buf.nbytes == n * t.element_size() and buf.end == buf.start + buf.nbytes
            assert buf.zone == max(4096, -(-buf.nbytes // 512) * 512)
            left, right = buf.zones()
            # the zones abut the payload exactly, and lie inside the base allocation
            assert left.data_ptr() + buf.zone == buf.start and right.data_ptr() == buf.end
            assert left.data_ptr() >= buf.base.data_ptr()
            assert right.data_ptr() + buf.zone <= buf.base.data_ptr() + buf.base.numel()
            assert bool((left == want).all()) and bool((right == want).all())
            payload = mh._plain(t)
            assert bool((payload == (want if kind == "empty" else 0)).all())
            # the registry: first and last payload byte, and neither zone
            assert guard.find(buf.start) is buf and guard.find(buf.end - 1) is buf
            assert guard.find(buf.start - 1) is None and guard.find(buf.end) is None
    assert guard.damage() == []
    shaped = guard.buffer((5, 7, 3), dtype, "cpu", "zeros").tensor
    assert shaped.shape == (5, 7, 3) and shaped.is_contiguous() and shaped.dtype == dtype


def test_the_fills_are_what_the_cases_can_bear():
    for floats, integers in mh.FILLS.values():
        assert 0.0 <= floats <= 1.0 and integers in (0, 1)
        assert float(torch.tensor(floats).to(torch.bfloat16)) == floats
    assert mh.FILLS["A"][0] != mh.FILLS["B"][0] and mh.FILLS["A"][1] != mh.FILLS["B"][1]
    assert mh.FILLS["A"][0] == sh.SENTINEL


def test_the_context_guards_the_four_factories_clone_and_full(monkeypatch):
    source = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    for guard in (mh.Guard("A", "cpu"), mh.Guard("B", "cpu")):
        floats, integers = mh.FILLS[guard.name]
        with monkeypatch.context() as patch:
            guard.patch(patch)
            made = [torch.empty((3, 5), dtype=torch.float32, device="cpu"),
                    torch.empty(7, dtype=torch.int32, device=torch.device("cpu")),
                    torch.empty((), dtype=torch.float32, device="cpu"),
                    torch.zeros((2, 2), dtype=torch.int64, device="cpu"),
                    torch.empty_like(source), torch.zeros_like(source), source.clone(),
                    torch.full((5,), -1, dtype=torch.int64, device="cpu"),
                    torch.full((2, 3), 0.5, device="cpu")]
            assert len(guard.buffers) == len(made)
            assert all(guard.find(t.data_ptr()) is not None for t in made)
            assert bool((made[0] == floats).all()) and bool((made[1] == integers).all())
            assert float(made[2]) == floats and made[2].shape == ()
            assert not bool(made[3].any()) and not bool(made[5].any())
            assert bool((made[4] == floats).all()) and made[4].shape == source.shape
            assert torch.equal(made[6], source) and made[6].data_ptr() != source.data_ptr()
            assert made[7].dtype == torch.int64 and made[7].tolist() == [-1] * 5
            assert made[8].dtype == torch.float32 and bool((made[8] == 0.5).all())
            # everything else passes through
            count = len(guard.buffers)
            passed = [torch.empty((3,), dtype=torch.float32), torch.empty((0, 3), device="cpu"),
                      torch.empty((3,), device="cpu", pin_memory=False),
                      torch.zeros((3,), device="meta"), torch.empty_like(source.t()),
                      source.t().clone(), source.clone(memory_format=torch.contiguous_format),
                      torch.zeros(3, requires_grad=True, device="cpu"), torch.full((3,), 2.0),
                      torch.full((3,), 2.0, device="cpu", requires_grad=True)]
            assert len(guard.buffers) == count and len(passed) == 10
            from tests import stream_order_cases
            placed = stream_order_cases._t(source.numpy(), "cpu")
            assert guard.find(placed.data_ptr()).kind == "input" and torch.equal(placed, source)
        assert guard.damage() == []
    assert torch.empty is mh._RAW["empty"] and torch.zeros_like is mh._RAW["zeros_like"]
    assert torch.Tensor.clone is mh.raw_clone and torch.full is mh._RAW["full"]
    from tests import stream_order_cases
    assert stream_order_cases.PLACE is None
    assert mh.Guard("A", "cpu").find(stream_order_cases._t(source.numpy(), "cpu").data_ptr()) is None


# ------------------------------------------------------------------------------------ controls
def test_control_a_write_just_past_a_payload_is_reported():
    for fill in "AB":
        guard = mh.Guard(fill, "cpu")
        buf = guard.buffer((257,), torch.float32, "cpu", "empty")
        other = guard.buffer((65, 48), torch.int32, "cpu", "zeros")
        assert guard.damage() == []
        end = buf.offset + buf.nbytes
        buf.base[end:end + 4].view(torch.float32).fill_(2.0)
        found = guard.damage()
        assert len(found) == 1 and "(257,)" in found[0] and "torch.float32" in found[0], found
        assert "1 elements of the right zone changed, 0 .. 3 bytes past the payload's end" \
            in found[0], found
        last = buf.offset + buf.nbytes + buf.zone
        buf.base[last - 4:last].view(torch.float32).fill_(2.0)
        assert "2 elements of the right zone changed, 0 .. %d bytes past" % (buf.zone - 1) \
            in buf.damage()
        other.base[other.offset - 8:other.offset - 4].view(torch.int32).fill_(7)
        assert "1 elements of the left zone changed, 8 .. 5 bytes before the payload's start" \
            in other.damage()
        buf.users.add("ffn_sample_t")
        assert "arguments of ['ffn_sample_t']" in buf.damage()


def test_control_b_a_payload_left_as_empty_made_it_differs_between_the_fills(monkeypatch):
    got = {}
    for fill in "AB":
        guard = mh.Guard(fill, "cpu")
        with monkeypatch.context() as patch:
            guard.patch(patch)
            got[fill] = [torch.empty((300, 17), device="cpu"),
                         torch.empty((257,), dtype=torch.int32, device="cpu"),
                         torch.zeros((3,), device="cpu")]
    assert not sh.same_bits(got["A"][0], got["B"][0]) and not sh.same_bits(got["A"][1], got["B"][1])
    assert sh.same_bits(got["A"][2], got["B"][2])


def test_control_c_a_gather_one_element_past_an_input_sees_the_fill():
    values = torch.arange(1, 258, dtype=torch.float32)
    got = {}
    for fill in "AB":
        guard = mh.Guard(fill, "cpu")
        placed = guard.place(values)
        buf = guard.find(placed.data_ptr())
        assert buf.kind == "input" and torch.equal(placed, values)
        through_base = buf.base[buf.offset:buf.offset + buf.nbytes + 4].view(torch.float32)
        got[fill] = through_base[torch.arange(258)]
        assert guard.damage() == []
    assert torch.equal(got["A"][:257], got["B"][:257])
    assert not torch.equal(got["A"], got["B"])
    assert float(got["A"][257]) == mh.FILLS["A"][0] and float(got["B"][257]) == mh.FILLS["B"][0]


# ------------------------------------------------------------------------------------ the tables
def _header_words():
    with open(sh.HEADER) as f:
        return " ".join(f.read().replace("*", " ").split())


def test_the_exceptions_name_what_the_header_has():
    from tests.test_memory_bounds_gpu import EXCEPTIONS
    sigs = mh.signatures()
    for (entry, param), reason in EXCEPTIONS.items():
        assert entry in sigs, entry
        assert param in mh.written(entry, sigs), "%s has no written pointer %s" % (entry, param)
        assert reason and len(reason) > 20, "a reason for (%s, %s)" % (entry, param)


def test_the_undefined_words_cite_the_header():
    from tests.stream_order_cases import CASES
    from tests.test_memory_bounds_gpu import EXTRA, UNDEFINED
    names = {c.name for c in CASES + EXTRA}
    assert len(names) == len(CASES) + len(EXTRA)
    text = _header_words()
    for case, (sentence, mask) in UNDEFINED.items():
        assert case in names, case
        assert callable(mask)
        assert len(sentence) > 20 and " ".join(sentence.split()) in text, \
            "%s: the header does not say %r" % (case, sentence)

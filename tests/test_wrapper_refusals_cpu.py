"""The argument contract of the wrappers ("The argument contract"), on a machine without a
GPU: every public function of ``ops.py`` and method of ``mlp_engine.py`` that reaches the library
refuses a mis-shaped tensor with a ``ValueError`` that names the wrapper and the argument -- before
anything reaches the library, and without reading a tensor's values.

The subjects come from the code (``refusal_cases.subjects``), the valid calls from the table
(``refusal_cases.ROWS``), the mutated calls from the valid ones (``refusal_cases.mutations``).  The
arguments are ``meta`` tensors: they have shapes and no values, so a check that wants values raises
and is reported.  ``_lib.call`` is replaced by a hook that records the entry point and raises; it
never forwards.  The library must be built (as tests/test_abi_cpu.py needs it): the wrappers ask it
for workspace sizes."""

import collections
import timeit

import pytest
import torch

from tests import refusal_cases as rc
from tests import stream_helpers as sh

SUBJECTS = rc.subjects()

# the wrappers of K1 .. K11 (everything of ops.py up to ``voxels_backward``) and the two launches of
# the training step may not read values: their rows are never ``marked``
UNMARKED = ["raygen_nearfar", "sample_t", "materialise_samples", "sample_materialise", "cdf_build",
            "cdf_build_logits", "focus_sample_merge", "to_image", "ycrcb_to_rgb_u8",
            "fourier_encode", "composite_fwd", "blend_weights", "blend_weights_bwd",
            "composite_bwd", "mse_loss", "composite_train", "loss_from_partials", "loss_value",
            "regression_train", "regression_eval", "regression_loss", "regression_mse_train",
            "regression_mse_eval", "regression_mse_loss", "clip_adam", "occupancy_build",
            "occupancy_compact", "occupancy_from_octree", "scatter_logits", "gather_logits",
            "voxels_forward", "voxels_backward", "MlpProgram.forward", "MlpProgram.backward"]

# what one ``TrainEngine.train_step`` and one ``Raycaster.render`` of the benchmark's model reach
# (a hook record of both on the GPU); ``MlpProgram.pack`` takes no argument and checks nothing
STEP_SUBJECTS = ["sample_materialise", "MlpProgram.forward", "composite_train",
                 "MlpProgram.backward", "clip_adam", "loss_from_partials", "MlpProgram.render"]
HOST_BOUND_STEP_US = 2000.0     # the bf16x6 NeRF step is host-bound at about 2 ms


def missing_rows(rows, subjects=None):
    """The subjects without a row, and the rows without a subject."""
    subjects = SUBJECTS if subjects is None else subjects
    return sorted(set(subjects) - set(rows)), sorted(set(rows) - set(subjects))


def examine(row, fn, kwargs, hook, accepted=None, by_value=None):
    """Runs the valid call of ``row`` and every mutation of it -> (problems, counts)."""
    accepted = rc.ACCEPTED if accepted is None else accepted
    by_value = rc.BY_VALUE_ONLY if by_value is None else by_value
    problems, counts = [], collections.Counter()
    kind, error = rc.outcome(fn, kwargs, hook)
    if kind != rc.ACCEPTED_CALL:
        return ["the valid call is %s: %r" % (kind, error)], counts
    refused = collections.Counter()
    for name, mutation, changed in rc.mutations(row, fn, kwargs):
        counts["mutations"] += 1
        kind, error = rc.outcome(fn, changed, hook)
        where = "%s = %s" % (name, mutation)
        legal = (row.subject, name, mutation) in accepted or mutation in row.defines.get(name, ())
        if kind == rc.REACHED:
            problems.append("%s reaches the library: %s" % (where, hook.seen[-1]))
        elif kind == rc.READ_VALUES:
            problems.append("%s: a check reads a tensor's values: %r" % (where, error))
        elif kind == rc.BROKE:
            problems.append("%s is no refusal: %r" % (where, error))
        elif kind == rc.ACCEPTED_CALL:
            if not legal:
                problems.append("%s passes every check: it would be launched" % where)
            counts["legal"] += 1
        elif legal:
            problems.append("%s is listed as a legal call, and is refused: %s" % (where, error))
        elif isinstance(error, TypeError) and mutation != "None":
            problems.append("%s is a TypeError, not a ValueError: %s" % (where, error))
        elif not rc.names_it(row, name, error):
            problems.append("%s: the refusal does not name the wrapper and the argument: %s"
                            % (where, error))
        else:
            refused[name] += 1
    for name, value in kwargs.items():
        if torch.is_tensor(value) and not refused[name] and (row.subject, name) not in by_value:
            problems.append("no mutation of %s is refused" % name)
    return problems, counts


def run_row(subject, monkeypatch):
    row = rc.ROWS[subject]
    hook = rc.Hook().install(monkeypatch)
    make = rc.factory("cpu" if row.marked else "meta", row.marked)
    fn, kwargs = row.target(row.build(make))
    return examine(row, fn, kwargs, hook)


# ------------------------------------------------------------------------------------ completeness
def test_every_subject_has_a_row():
    assert len(SUBJECTS) >= 88 and "raygen_nearfar" in SUBJECTS and "MlpProgram.backward" in SUBJECTS
    # the private launch halves count through the public functions that call them
    assert "mesh_sample" in SUBJECTS and "octree_refine" in SUBJECTS
    assert "octree_visible_moments" in SUBJECTS and "octree_render_volume_sh" in SUBJECTS
    assert not [s for s in SUBJECTS if rc._private(s)]
    without_row, without_subject = missing_rows(rc.ROWS)
    assert not without_row, "wrappers without a row in tests/refusal_cases.py: %s" % without_row
    assert not without_subject, "rows of no wrapper: %s" % without_subject


def test_a_subject_removed_from_the_table_is_missed():
    rows = dict(rc.ROWS)
    del rows["composite_train"]
    assert missing_rows(rows) == (["composite_train"], [])
    source = ("def _launch(t):\n    _call('ffn_x', t)\n\n"
              "def new_wrapper(t):\n    return _launch(t)\n\n"
              "def helper(t):\n    return t\n\n"
              "class Engine:\n    def step(self, t):\n        _lib.call('ffn_y', t)\n")
    assert rc.module_subjects(source) == ["Engine.step", "new_wrapper"]
    assert missing_rows(rc.ROWS, SUBJECTS + ["new_wrapper"])[0] == ["new_wrapper"]


def test_the_first_wrappers_and_the_training_launches_read_no_values():
    marked = sorted(s for s, row in rc.ROWS.items() if row.marked)
    assert not set(marked) & set(UNMARKED), marked
    assert set(UNMARKED) <= set(SUBJECTS)
    assert marked == ["mesh_sample", "octree_carve_box_level", "octree_carve_select",
                      "octree_refine", "octree_visible_moments", "octree_visible_votes"]
    assert sorted(s for s, row in rc.ROWS.items() if row.gpu_only) == [
        "MlpProgram.forward16", "MlpProgram.pack", "MlpProgram.pack16"]


def test_sizes_that_play_different_roles_differ():
    sizes = [rc.R, rc.S, rc.T, rc.L, rc.NODES, rc.C, rc.H, rc.W, rc.P, rc.V, rc.F, rc.TEX]
    assert len(set(sizes)) == len(sizes)
    assert rc.R == 5 and rc.S == 3 and rc.T == 11 and rc.L == 7 and rc.C == 4


# ------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("subject", [s for s in SUBJECTS if s in rc.ROWS
                                     and not rc.ROWS[s].gpu_only])
def test_a_wrapper_refuses_every_mutation_before_the_library(subject, monkeypatch):
    problems, counts = run_row(subject, monkeypatch)
    assert not problems, "%s:\n  %s" % (subject, "\n  ".join(problems))
    assert counts["mutations"] > 0


def test_the_counts(monkeypatch):
    """Prints what the table holds (DESIGN.md quotes these)."""
    total = collections.Counter()
    for subject, row in rc.ROWS.items():
        if row.gpu_only:
            continue
        _, counts = run_row(subject, monkeypatch)
        total.update(counts)
    legal_by_size = sum(len(kinds) for row in rc.ROWS.values() for kinds in row.defines.values())
    print("\nargument contract: %d subjects (%d rows run here, %d on the GPU only), %d mutations, "
          "%d of them legal calls of another size, %d accepted entries, %d by-value parameters"
          % (len(SUBJECTS), sum(not r.gpu_only for r in rc.ROWS.values()),
             sum(r.gpu_only for r in rc.ROWS.values()), total["mutations"], legal_by_size,
             len(rc.ACCEPTED), len(rc.BY_VALUE_ONLY)))
    assert total["mutations"] >= 1000
    assert len(rc.ACCEPTED) <= 16 and len(rc.BY_VALUE_ONLY) <= 8


# ------------------------------------------------------------------------------------ the other forms
def _refused(call, *words):
    with pytest.raises(ValueError) as error:
        call()
    assert all(w in str(error.value) for w in words), str(error.value)


def test_the_fused_render_of_a_range_of_rays(monkeypatch):
    """``ray_index = (first id, count, valid mask)``: the range, the mask and the pixels it writes
    are plain ints."""
    hook = rc.Hook().install(monkeypatch)
    make = rc.factory("meta", False)
    kwargs = rc.ROWS["MlpProgram.render"].build(make)
    prog = kwargs.pop("_self")
    kwargs.update(t_values=None, image=make((rc.R, 3), torch.uint8), pixel_offset=4)

    def render(**change):
        return lambda: prog.render(**dict(kwargs, **change))
    good = (4, rc.R, make((rc.T,), torch.uint8))
    with pytest.raises(RuntimeError, match="but the model is on"):
        render(ray_index=good)()
    with pytest.raises(RuntimeError, match="but the model is on"):
        render(ray_index=(rc.T - rc.R, rc.R, None), pixel_offset=rc.T - rc.R)()
    _refused(render(ray_index=(rc.T - rc.R + 1, rc.R, None)), "render", "ray_index", "near_far")
    _refused(render(ray_index=(-1, rc.R, None)), "render", "ray_index")
    _refused(render(ray_index=(4, rc.R, make((4 + rc.R - 1,), torch.uint8))), "render", "valid")
    _refused(render(ray_index=(4, rc.R, make((rc.T, 1), torch.uint8))), "render", "valid")
    _refused(render(ray_index=good, pixel_offset=5), "render", "image", "pixel_offset")
    _refused(render(ray_index=good, pixel_offset=3), "render", "image", "pixel_offset")
    _refused(render(ray_index=good, image=make((rc.R - 1, 3), torch.uint8)), "render", "image")
    _refused(render(ray_index=good, starts=make((rc.T - 1, 3)), directions=make((rc.T - 1, 3))),
             "render", "starts", "near_far")
    assert not hook.seen


def test_a_chain_without_a_view_encoding_takes_no_views(monkeypatch):
    import fourier_feature_nets_amd as ffn
    from fourier_feature_nets_amd.mlp_engine import MlpProgram
    hook = rc.Hook().install(monkeypatch)
    enc, specs = ffn.PositionalFourierMLP(3, 4, 5.5)._chain(torch.device("cpu"))
    plain = MlpProgram(enc, specs, torch.device("cpu"), planning_only=True)
    assert plain.uses_views is False and rc.program("cpu").uses_views is True
    make = rc.factory("meta", False)
    positions, views = make((rc.P, 3)), make((rc.P, 3))
    saved, grads = make((plain.saved_floats(rc.P),)), make((plain.num_grad_floats,))
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        plain.forward(positions, None)
    _refused(lambda: plain.forward(positions, views, saved), "forward", "views")
    _refused(lambda: plain.backward(make((rc.P, 4)), positions, views, saved, grads),
             "backward", "views")
    _refused(lambda: plain.forward(positions.unsqueeze(0), None, saved), "forward", "positions")
    assert not hook.seen


def test_an_integer_is_an_integer():
    from fourier_feature_nets_amd import ops
    ops._want_int("w", "count", 3, 1, 3)
    for bad in (3.0, True, 0, 4, None, "3"):
        with pytest.raises(ValueError, match="w: count must be an integer in 1 .. 3"):
            ops._want_int("w", "count", bad, 1, 3)


# ------------------------------------------------------------------------------------ exemptions
def _header_words():
    with open(sh.HEADER) as f:
        return " ".join(f.read().replace("*", " ").split())


def test_the_exemptions_cite_the_header():
    text = _header_words()
    for (subject, name, mutation), sentence in rc.ACCEPTED.items():
        assert subject in rc.ROWS, subject
        assert mutation in ("row-1", "last+1", "last-1", "unsqueeze"), mutation
        assert len(sentence) > 20 and " ".join(sentence.replace("*", " ").split()) in text, \
            "%s, %s: the header does not say %r" % (subject, name, sentence)
    for (subject, name), (reason, sentence) in rc.BY_VALUE_ONLY.items():
        assert subject in rc.ROWS and len(reason) > 20
        assert " ".join(sentence.replace("*", " ").split()) in text, (subject, name)


def test_an_exemption_that_is_refused_is_reported(monkeypatch):
    """The tables cannot go stale: an entry whose call is in fact refused is a problem."""
    row = rc.ROWS["composite_fwd"]
    hook = rc.Hook().install(monkeypatch)
    fn, kwargs = row.target(row.build(rc.factory("meta", False)))
    stale = {("composite_fwd", "t", "last+1"): "x"}
    problems, _ = examine(row, fn, kwargs, hook, accepted=stale)
    assert any("listed as a legal call, and is refused" in p for p in problems), problems


# ------------------------------------------------------------------------------------ teeth
def _dummy_row(subject, fn, build, **kwargs):
    row = rc.Row(subject, build, kwargs.get("ints"), False, (), None, None)
    row.target = lambda built: (fn, dict(built))
    return row


def _pair(make):
    return dict(values=make((rc.R, 3)), index=make((rc.R,), torch.int64))


def test_teeth_a_wrapper_without_checks_is_reported(monkeypatch):
    from fourier_feature_nets_amd import _lib, ops

    def unchecked(values, index):
        ops._call("ffn_gather_logits", ops._dev(values, name="values"),
                  ops._dev(index, torch.int64, "index"))

    def straight(values, index):
        _lib.call("ffn_gather_logits", int(values.shape[0]), int(index.shape[0]))

    hook = rc.Hook().install(monkeypatch)
    row = _dummy_row("unchecked", unchecked, _pair)
    problems, _ = examine(row, unchecked, _pair(rc.factory("meta", False)), hook)
    assert sum("passes every check: it would be launched" in p for p in problems) >= 5, problems
    assert any(p.startswith("values = row-1 passes") for p in problems), problems
    assert "no mutation of values is refused" in problems and not hook.seen
    # ... and one that does not even go through ``_dev`` reaches the hook, by name
    row = _dummy_row("straight", straight, _pair)
    problems, _ = examine(row, straight, _pair(rc.factory("meta", False)), hook)
    assert problems == ["the valid call is reached: ReachedLibrary('ffn_gather_logits')"], problems
    assert hook.seen == ["ffn_gather_logits"]


def test_teeth_a_check_that_reads_values_is_reported(monkeypatch):
    from fourier_feature_nets_amd import ops

    def peeking(values, index):
        if values.dim() != 2 or index.shape != (values.shape[0],):
            raise ValueError("peeking: values (n,3) and index (n,) disagree")
        if int(index.max()) >= values.shape[0]:
            raise ValueError("peeking: index leaves values")
        ops._call("ffn_gather_logits", ops._dev(values), ops._dev(index, torch.int64))

    hook = rc.Hook().install(monkeypatch)
    row = _dummy_row("peeking", peeking, _pair)
    problems, _ = examine(row, peeking, _pair(rc.factory("meta", False)), hook)
    assert len(problems) == 1 and problems[0].startswith("the valid call is read"), problems
    # on CPU tensors, as a marked row gets them, the same wrapper passes
    problems, _ = examine(row, peeking, _pair(rc.factory("cpu", True)), hook)
    assert not [p for p in problems if "reads" in p or "read:" in p], problems


def test_teeth_a_check_that_refuses_everything_fails_the_valid_call(monkeypatch):
    def paranoid(values, index):
        raise ValueError("paranoid: values and index are never right")

    hook = rc.Hook().install(monkeypatch)
    row = _dummy_row("paranoid", paranoid, _pair)
    problems, _ = examine(row, paranoid, _pair(rc.factory("meta", False)), hook)
    assert len(problems) == 1 and problems[0].startswith("the valid call is refused"), problems


def test_every_valid_call_ends_in_the_device_refusal(monkeypatch):
    hook = rc.Hook().install(monkeypatch)
    for subject, row in rc.ROWS.items():
        if row.gpu_only:
            continue
        fn, kwargs = row.target(row.build(rc.factory("cpu" if row.marked else "meta", row.marked)))
        with pytest.raises(RuntimeError, match="must live on the GPU|but the model is on"):
            fn(**kwargs)
    assert not hook.seen


# ------------------------------------------------------------------------------------ host cost
def _valid_call_seconds(subject):
    row = rc.ROWS[subject]
    fn, kwargs = row.target(row.build(rc.factory("meta", False)))

    def call():
        try:
            fn(**kwargs)
        except RuntimeError:
            pass
    call()
    number = 2000
    return min(timeit.repeat(call, number=number, repeat=5)) / number


def test_host_cost_of_the_checks_per_training_step(monkeypatch):
    """A measurement, not a threshold: the host time of the wrappers that one training step and
    one fused render reach -- the valid ``meta`` call up to ``_dev``'s refusal -- as it is, and with
    the check helpers replaced by functions that do nothing.  The second column is NOT the parent's
    time: the wrappers a step calls once per launch (``sample_materialise``, ``composite_train``, the
    samples of ``MlpProgram.forward`` / ``.backward``) test their good case inline, and that stays.
    The comparison with the parent commit needs the parent's modules; DESIGN.md records it."""
    from fourier_feature_nets_amd import mlp_engine, ops
    rc.Hook().install(monkeypatch)
    with_checks = {s: _valid_call_seconds(s) for s in STEP_SUBJECTS}
    with monkeypatch.context() as patch:
        for module in (ops, mlp_engine):
            for name in ("_want", "_want_numel", "_want_int", "_want_tensors"):
                if hasattr(module, name):
                    patch.setattr(module, name, lambda *a, **k: None)
        without = {s: _valid_call_seconds(s) for s in STEP_SUBJECTS}
    added = {s: (with_checks[s] - without[s]) * 1e6 for s in STEP_SUBJECTS}
    total = sum(added.values())
    print("\nhost cost of the argument checks, microseconds per call (with, without, added):")
    for s in STEP_SUBJECTS:
        print("  %-24s %7.2f %7.2f %+7.2f" % (s, with_checks[s] * 1e6, without[s] * 1e6, added[s]))
    print("  sum over one step and one render: %+.2f us = %.2f %% of a host-bound step of %d us"
          % (total, 100.0 * total / HOST_BOUND_STEP_US, HOST_BOUND_STEP_US))
    assert set(STEP_SUBJECTS) <= set(SUBJECTS)

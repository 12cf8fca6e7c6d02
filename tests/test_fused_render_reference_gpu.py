"""The fused inference render (``render_fused_kernel``, ``MlpProgram.render``) against float64
(tests/fused_render_reference.py) at its compaction and launch edges.

``prog.render`` is driven directly with synthetic ray tables, so the test owns starts, directions,
near_far, ray ids, t-values and the occupancy bits.  Box [-1, 1]^3, a 256^3 grid; ray r runs along
+x from (-1, y_r, z_r), (y_r, z_r) the centre of its own (iy, iz) row of cells, near 0, far 2; sample
j sits at the centre of cell ``ix_j = floor((j + 1/2) 256 / S)``.  Every coordinate is exact in f32
and half a cell from the faces, the cells of a ray's samples are distinct, so ``keep[r, j]`` is
exactly bit (ix_j, iy_r, iz_r) and every per-ray, per-sample pattern is free.

Every output is NaN (0xAB for the u8 image, with guard rows) before the kernel runs: the outputs
``MlpProgram.render`` allocates come out of ``torch.empty``, which is wrapped for the call.

Without a grid the kernel is held to the BITS of the three-pass path (K2 -> inference forward -> K5),
with one to K5's ``KAPPA`` on the compacted sequence; the case lists below are plain data, which
tests/test_fused_render_reference_cpu.py proves to reach every branch of the launch arithmetic."""

import contextlib
import json

import numpy as np
import pytest
import torch

from tests import fused_render_reference as fr
from tests.test_layer_reference_gpu import CHAINS

pytestmark = pytest.mark.gpu

EXACT = ("holds the one-launch render kernel -- an exact-f32 kernel -- to the bits of the exact-f32 three-pass "
         "path and to K5's budget; in an opt-in arithmetic mode the models compute differently")
G = 256
BOX_MIN, BOX_SIZE = [-1.0, -1.0, -1.0], [2.0, 2.0, 2.0]
NO_GRID_S = [1, 2, 31, 32, 33, 63, 64, 65, 128, 200, 256]          # (K5 accepts S = 1)
COMPACT_S = [2, 33, 64, 65, 200, 256]
WIDE_S = [65, 200]
CHAIN_S, CHAIN_R = 33, 7
LIST_S, LIST_T = 65, 150
LIST_RANGE = (20, 100)               # (first id, count) of the range form
PATTERNS = ["none", "first", "last", "second_last", "all", "all_but_last", "even", "odd",
            "first31", "first32", "first33", "first63", "first64", "first65", "runs", "runs_b",
            "bern0.1", "bern0.5", "bern0.9"]
# neighbouring rays of a 512-wide workgroup (its two pairs of waves run in step)
WIDE_PAIRS = [("none", "all"), ("all", "none"), ("first", "all"), ("invalid", "all"), ("all", "invalid"),
              ("bern0.5", "runs")]
# the skipped runs of "runs" end where the kept count stands at 30 | 34 | 62 | 68: the kept runs
# behind them straddle slots 32 and 64
RUNS = [(True, 30), (False, 5), (True, 4), (False, 7), (True, 28), (False, 3), (True, 6), (False, 10)]
RUNS_B = [(False, 3), (True, 31), (False, 2), (True, 2), (False, 40), (True, 33), (False, 1)]


# ------------------------------------------------------------------------------------- the cases (CPU data)
def pattern_row(name, S, r):
    """(S) bool: the samples ray ``r`` keeps under pattern ``name``."""
    j = torch.arange(S)
    if name == "none":
        return j < 0
    if name in ("all", "invalid"):
        return j >= 0
    if name == "first":
        return j == 0
    if name == "last":
        return j == S - 1
    if name == "second_last":
        return j == S - 2
    if name == "all_but_last":
        return j < S - 1
    if name == "even":
        return j % 2 == 0
    if name == "odd":
        return j % 2 == 1
    if name.startswith("first"):
        return j < int(name[5:])
    if name.startswith("runs"):
        row, at = torch.zeros(S, dtype=torch.bool), 0
        for keep, n in (RUNS if name == "runs" else RUNS_B):
            row[at:at + n] = keep
            at += n
        row[at:] = True
        if name == "runs":
            row[max(S - 3, 0):] = False      # the ray's tail skipped: the final kept sample is not the last
        return row
    if name.startswith("bern"):
        gen = torch.Generator().manual_seed(1000 * S + r)
        return torch.rand(S, generator=gen) < float(name[4:])
    raise ValueError(name)


def keep_rows(names, S):
    """(R, S) bool of the rays' patterns ``names`` (one name per ray)."""
    return torch.stack([pattern_row(n, S, r) for r, n in enumerate(names)])


def no_grid_rays(teams, cus):
    return [1, 3, 5, teams * cus + 3, 2 * teams * cus + 1]


def compaction_names(cus):
    """The patterns of the compaction test's rays: every pattern in turn over two rounds of the
    narrow launch and a ragged last workgroup."""
    R = fr.NARROW_TEAMS * cus + 5
    return [PATTERNS[r % len(PATTERNS)] for r in range(R)]


def wide_names(cus, layout):
    """Ray patterns of the wide-pair test: the neighbour pairs in turn over two rounds and an odd
    count.  ``layout`` 0 is the base; 1 changes every odd ray (so the even rays meet another
    neighbour), 2 every even ray."""
    R = fr.WIDE_TEAMS * cus + 2 * len(WIDE_PAIRS) + 1
    names = [WIDE_PAIRS[(r // 2) % len(WIDE_PAIRS)][r % 2] for r in range(R)]
    swap = {"none": "all", "all": "invalid", "invalid": "first", "first": "none", "bern0.5": "none",
            "runs": "all"}
    if layout:
        names = [swap[n] if r % 2 == layout % 2 else n for r, n in enumerate(names)]
    return names


def plan_cases(cus):
    """Every launch of the tests below as (label, R, S, teams, names | None): what the CPU test runs
    ``render_plan`` over."""
    out = []
    for teams in (fr.NARROW_TEAMS, fr.WIDE_TEAMS):
        for S in NO_GRID_S:
            for R in no_grid_rays(teams, cus):
                out.append(("no_grid", R, S, teams, None))
    out.append(("chains", CHAIN_R, CHAIN_S, fr.NARROW_TEAMS, None))
    out.append(("lists", LIST_T, LIST_S, fr.NARROW_TEAMS, None))
    out.append(("lists", LIST_RANGE[1], LIST_S, fr.NARROW_TEAMS, None))      # whole workgroups only
    for S in COMPACT_S:
        names = compaction_names(cus)
        out.append(("compaction", len(names), S, fr.NARROW_TEAMS, names))
    for S in WIDE_S:
        for layout in range(3):
            names = wide_names(cus, layout)
            out.append(("wide_pairs", len(names), S, fr.WIDE_TEAMS, names))
    return out


# ------------------------------------------------------------------------------------- device helpers
def dev():
    return torch.device("cuda:0")


def cu_count():
    return torch.cuda.get_device_properties(dev()).multi_processor_count


def sample_cells(S):
    """ix_j = floor((j + 1/2) 256 / S), in integers."""
    return ((2 * torch.arange(S) + 1) * (G // 2)) // S


def ray_table(T, S):
    """T rays of the construction in the module docstring, on the device."""
    r = torch.arange(T)
    iy, iz = 64 + r % 128, 64 + r // 128
    assert int(iz.max()) < 192
    centre = lambda i: (i.double() + 0.5) / (G // 2) - 1.0      # noqa: E731
    starts = torch.stack([torch.full((T,), -1.0, dtype=torch.float64), centre(iy), centre(iz)], 1).float()
    dirs = torch.tensor([[1.0, 0.0, 0.0]]).repeat(T, 1)
    near_far = torch.stack([torch.zeros(T), torch.full((T,), 2.0)])
    ix = sample_cells(S)
    t_row = ((ix.double() + 0.5) / (G // 2)).float()
    cell = (iz[:, None] * G + iy[:, None]) * G + ix[None]        # (T, S)
    to = lambda x: x.contiguous().to(dev())                      # noqa: E731
    return dict(T=T, S=S, starts=to(starts), dirs=to(dirs), near_far=to(near_far), t_row=to(t_row),
                unit=to((t_row.double() / 2).float()), cell=cell,
                t=to(t_row[None].repeat(T, 1)))


def grid_of(tab, keep):
    import fourier_feature_nets_amd as ffn
    bits = fr.grid_bits(tab["cell"][keep], G)
    return ffn.OccupancyGrid(bits.to(dev()), BOX_MIN, BOX_SIZE, G)


def slope_model():
    """A ReLU MLP with hand-set weights: sigma logit = 3 - 4 |x|_1 (moderate density across the box),
    colour logits that vary with |x|_1."""
    import fourier_feature_nets_amd as ffn
    model = ffn.MLP(3, 4, num_channels=64)
    with torch.no_grad():
        for layer in model.layers:
            layer.weight.zero_()
            layer.bias.zero_()
        for d in range(3):
            model.layers[0].weight[2 * d, d] = 1.0
            model.layers[0].weight[2 * d + 1, d] = -1.0
        model.layers[1].weight[0, :6] = 1.0
        model.layers[2].weight[0, 0] = 1.0
        out = model.layers[3]
        out.weight[3, 0], out.bias[3] = -4.0, 3.0
        out.weight[0, 0], out.bias[0] = 1.5, -0.5
        out.weight[1, 0], out.bias[1] = -1.0, 0.7
        out.bias[2] = 0.3
    return model.to(dev()).eval()


def nan_model():
    """Finite logits for x <= 1/2, NaN beyond: two channels overflow to +inf there and the head
    subtracts them."""
    import fourier_feature_nets_amd as ffn
    model = ffn.MLP(3, 4, num_channels=64)
    with torch.no_grad():
        for layer in model.layers:
            layer.weight.zero_()
            layer.bias.zero_()
        model.layers[0].weight[0, 0], model.layers[0].bias[0] = 1.0, -0.5
        model.layers[1].weight[0, 0] = model.layers[1].weight[1, 0] = 1e30
        model.layers[2].weight[0, 0] = model.layers[2].weight[1, 1] = 1e30
        model.layers[3].weight[3, 0], model.layers[3].weight[3, 1] = 1.0, -1.0
    return model.to(dev()).eval()


_MODELS = {}


def model_of(kind):
    if kind not in _MODELS:
        if kind == "narrow":
            _MODELS[kind] = slope_model()
        elif kind == "nan":
            _MODELS[kind] = nan_model()
        else:
            from tests.test_layer_reference_gpu import _model
            _MODELS[kind] = _model("gaussian512" if kind == "wide" else kind).eval()
    return _MODELS[kind]


@contextlib.contextmanager
def filled_outputs(made):
    """Whatever ``torch.empty`` hands out inside: NaN (floats) / 0xAB.. (integers), and recorded."""
    real = torch.empty

    def empty(*args, **kwargs):
        out = real(*args, **kwargs)
        out.fill_(float("nan") if out.is_floating_point() else 0xAB)
        made.append(out)
        return out

    torch.empty = empty
    try:
        yield
    finally:
        torch.empty = real


def render(model, tab, rays, S, form="t", grid=None, made=None, t_values=None, **kw):
    """``prog.render`` of ``rays`` (ids or a (first, count, valid) range) into NaN-filled outputs."""
    count = rays[1] if isinstance(rays, tuple) else rays.shape[0]
    if t_values is None and form == "t":
        t_values = tab["t_row"][None].repeat(count, 1).contiguous()
    made = [] if made is None else made
    with filled_outputs(made):
        return model.program().render(tab["starts"], tab["dirs"], tab["near_far"], rays, S, tab["unit"],
                                      t_values, occupancy=grid, **kw)


def three_pass(model, tab, ids, S, t_values=None, flag=None):
    """K2a / K2b -> the model's inference forward -> K5: (t, positions, logits, colour, alpha, depth)."""
    from fourier_feature_nets_amd import ops
    t = t_values if t_values is not None else ops.sample_t(tab["near_far"], ids, S, tab["unit"], None, None)
    pos, views = ops.materialise_samples(tab["starts"], tab["dirs"], ids, t, True)
    with torch.no_grad():
        flat = pos.reshape(-1, 3)
        logits = model(flat, views.reshape(-1, 3)) if model.use_view else model(flat)
    logits = logits.reshape(ids.shape[0], S, 4).contiguous()
    colour, alpha, depth = ops.composite_fwd(logits, t, True, flag)
    return t, pos, views, logits, colour, alpha, depth


def flag():
    return torch.zeros((1,), dtype=torch.int32, device=dev())


def report_line(what, rep, **more):
    print("fused render reference", json.dumps(dict(test=what, worst={k: round(v, 4) for k, v in rep.worst.items()},
                                                     **more)))


def same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))


# ------------------------------------------------------------------------------------- 1. no grid: bits
@pytest.mark.exact_only(reason=EXACT)
@pytest.mark.parametrize("S", NO_GRID_S)
@pytest.mark.parametrize("kind", ["narrow", "wide"])
def test_no_grid_is_the_three_pass_render_bit_for_bit(kind, S):
    """Colour, alpha and depth of the fused kernel == K2 -> forward -> K5 in every bit, for one ray, a
    ragged workgroup, one round plus three rays and two rounds plus one, with ``unit`` and with
    explicit (sorted random, one pair equal) t-values; and within K5's budget of float64."""
    model = model_of(kind)
    prog = model.program()
    assert bool(prog.wide) == (kind == "wide") and not prog.big
    teams = fr.WIDE_TEAMS if prog.wide else fr.NARROW_TEAMS
    rep, nan = fr.new_report(), flag()
    for R in no_grid_rays(teams, cu_count()):
        tab = ray_table(R, S)
        ids = torch.arange(R, device=dev())
        gen = torch.Generator().manual_seed(S * 7 + R)
        t_rand = torch.sort(torch.rand(R, S, generator=gen) * 2.0, 1).values
        if S > 2:
            t_rand[:, 1] = t_rand[:, 2]
        for form, tv in (("unit", None), ("t", t_rand.to(dev()).contiguous())):
            key = "%s S=%d R=%d %s" % (kind, S, R, form)
            t, _, _, logits, c3, a3, d3 = three_pass(model, tab, ids, S, tv, nan)
            colour, alpha, depth = render(model, tab, ids, S, form, t_values=tv, want_depth=True, nan_flag=nan)
            assert same_bits(colour, c3) and same_bits(alpha, a3) and same_bits(depth, d3), key
            fr.measure_render(rep, {}, key, logits, t, None, colour, alpha, depth, teeth=())
    report_line("no_grid", rep, kind=kind, S=S)
    assert not rep.problems(), rep.problems()
    assert int(nan.item()) == 0


# ------------------------------------------------------------------------------------- 2. every chain
@pytest.mark.exact_only(reason=EXACT)
@pytest.mark.parametrize("name", CHAINS)
def test_every_chain_fuses_or_is_refused_untouched(name):
    """Narrow and 512-wide chains render to the three-pass bits; a chain of more than 512 channels is
    refused by name and the outputs allocated for that call still hold their NaN."""
    from fourier_feature_nets_amd._lib import FfnError
    from fourier_feature_nets_amd.mlp_engine import BIAS_LDS_FLOATS
    model = model_of(name)
    prog = model.program()
    S, R = CHAIN_S, CHAIN_R
    tab = ray_table(R, S)
    ids = torch.arange(R, device=dev())
    if name == "nerf512":            # its bias lies beyond the LDS copy, and it must fuse all the same
        assert not prog.big and prog.fwd.bias_floats > BIAS_LDS_FLOATS
    if prog.big:
        made = []
        with pytest.raises(FfnError, match="ffn_render_fused_fwd"):
            render(model, tab, ids, S, "unit", made=made, want_depth=True)
        torch.cuda.synchronize()
        floats = [x for x in made if x.is_floating_point()]
        assert sorted(tuple(x.shape) for x in floats) == [(R,), (R,), (R, 3)]
        assert all(bool(torch.isnan(x).all()) for x in floats)
        return
    rep, nan = fr.new_report(), flag()
    t, _, _, logits, c3, a3, d3 = three_pass(model, tab, ids, S, None, nan)
    colour, alpha, depth = render(model, tab, ids, S, "unit", want_depth=True, nan_flag=nan)
    assert same_bits(colour, c3) and same_bits(alpha, a3) and same_bits(depth, d3)
    fr.measure_render(rep, {}, name, logits, t, None, colour, alpha, depth, teeth=())
    report_line("chains", rep, chain=name)
    assert not rep.problems(), rep.problems()
    assert int(nan.item()) == 0


@pytest.mark.exact_only(reason=EXACT)
@pytest.mark.parametrize("why", ["S=0", "S=257", "no t"])
def test_refused_shapes_leave_their_outputs_untouched(why):
    """The entry point refuses before it launches: the outputs allocated for the call keep their NaN."""
    from fourier_feature_nets_amd._lib import FfnError
    model = model_of("narrow")
    R = 5
    tab = ray_table(R, 4)
    ids = torch.arange(R, device=dev())
    S = dict([("S=0", 0), ("S=257", 257)]).get(why, 4)
    unit = None if why == "no t" else torch.linspace(0.0, 1.0, max(S, 1), device=dev())
    made = []
    with pytest.raises(FfnError, match="ffn_render_fused_fwd"):
        render(model, dict(tab, unit=unit), ids, S, "unit", made=made, want_depth=True)
    torch.cuda.synchronize()
    floats = [x for x in made if x.is_floating_point()]
    assert sorted(tuple(x.shape) for x in floats) == [(R,), (R,), (R, 3)]
    assert all(bool(torch.isnan(x).all()) for x in floats)


# ------------------------------------------------------------------------------------- 3. compaction
def conditions(grid, keep, pos):
    """The construction's conditions, on the reference alone."""
    got, dist = fr.keep_of(pos.reshape(-1, 3), grid)
    assert float(dist.min()) >= 0.25                       # (1/2 by construction)
    assert torch.equal(got.reshape(keep.shape), keep)
    _, _, index = grid.compact(pos.reshape(-1, 3).contiguous(), None)
    packed = torch.zeros(keep.numel(), dtype=torch.bool)
    packed[index.cpu().long()] = True
    assert torch.equal(packed.reshape(keep.shape), keep)


_BITES = {}


@pytest.mark.exact_only(reason=EXACT)
@pytest.mark.parametrize("S", COMPACT_S)
def test_compaction_patterns_against_float64(S):
    """Every keep pattern over two rounds: colour and alpha within K5's ``KAPPA`` of the compacted
    float64 sequence, the depth among its candidates; the K9 path on the same rays within the same
    budgets, and the two paths within the sum of their budgets of each other."""
    compaction_case(S)


def compaction_case(S):
    import fourier_feature_nets_amd as ffn
    model = model_of("narrow")
    names = compaction_names(cu_count())
    R = len(names)
    plan = fr.render_plan(R, S, fr.NARROW_TEAMS, cu_count())
    assert plan["rounds"] >= 2 and plan["ragged"]
    tab = ray_table(R, S)
    keep = keep_rows(names, S)
    grid = grid_of(tab, keep)
    ids = torch.arange(R, device=dev())
    rep, nan = fr.new_report(), flag()
    t, pos, views, logits, _, _, _ = three_pass(model, tab, ids, S, tab["t"])
    conditions(grid, keep, pos)
    colour, alpha, depth = render(model, tab, ids, S, "t", grid, want_depth=True, nan_flag=nan)
    key = "S=%d R=%d" % (S, R)
    bites = {}
    ref = fr.measure_render(rep, bites, key, logits, t, keep.to(dev()), colour, alpha, depth)
    for tooth, case in bites.items():
        _BITES.setdefault(tooth, case)
    # the data reach both sides of the alpha cut, and weights that matter on both sides of a skipped run
    a = ref["alpha"].v
    assert float(a.min()) < 0.1 < float(a.max())
    if S >= 33:                      # (two samples have no room for kept | skipped | kept)
        big =ref["weights"].v.cpu() > 1e-3
        behind = torch.cumsum((~keep & (torch.cumsum(big, 1) > 0)).long(), 1) > 0
        assert bool((big & behind).any())
    # K9: global compaction, the forward on the packed samples, K5 over all S samples
    caster = ffn.Raycaster(model)
    caster.occupancy = grid
    with torch.no_grad():
        k9 = caster.render(ffn.RaySamples(pos, views, t, ids), True)
    rep9 = fr.new_report()
    rep9.compare("colour", key + " K9", k9.color, ref["colour"])
    rep9.compare("alpha", key + " K9", k9.alpha, ref["alpha"])
    fr.check_depth(rep9, key + " K9", ref, t, k9.depth)
    both = fr.Report(dict(colour=2 * fr.KAPPA["colour"], alpha=2 * fr.KAPPA["alpha"]))
    both.compare("colour", key + " fused - K9", colour.double() - k9.color.double() + ref["colour"].v, ref["colour"])
    both.compare("alpha", key + " fused - K9", alpha.double() - k9.alpha.double() + ref["alpha"].v, ref["alpha"])
    report_line("compaction", rep, S=S, R=R, k9={k: round(v, 4) for k, v in rep9.worst.items()},
                fused_minus_k9={k: round(v, 4) for k, v in both.worst.items()}, teeth_failed_in=bites)
    assert not rep.problems(), rep.problems()
    assert not rep9.problems(), rep9.problems()
    assert not both.problems(), both.problems()
    assert int(nan.item()) == 0
    caster.check_finite()


@pytest.mark.exact_only(reason=EXACT)
def test_every_tooth_is_failed_by_the_kernel():
    """Each changed reference is failed by the kernel's own output in at least one compaction case
    (those tests run first and record it; run on its own, this test goes through the cases itself)."""
    for S in reversed(COMPACT_S):
        if all(name in _BITES for name in fr.TEETH):
            break
        compaction_case(S)
    print("fused render reference", json.dumps(dict(test="teeth", failed_in=_BITES)))
    missing = [name for name in fr.TEETH if name not in _BITES]
    assert not missing, "the kernel passes these changed references everywhere: %s" % missing


# ------------------------------------------------------------------------------------- 4. wide pairs
@pytest.mark.exact_only(reason=EXACT)
@pytest.mark.parametrize("S", WIDE_S)
def test_wide_pairs_under_compaction(S):
    """512-wide chain: neighbouring rays with unequal block counts (none | all, m = 1 | m = S, an
    invalid ray beside a valid one), odd R, two rounds.  Within ``KAPPA`` of the compacted float64
    sequence, and a ray's bits do not depend on its neighbour."""
    model = model_of("wide")
    assert model.program().wide
    cus = cu_count()
    outs, nan = [], flag()
    rep = fr.new_report()
    for layout in range(3):
        names = wide_names(cus, layout)
        R = len(names)
        plan = fr.render_plan(R, S, fr.WIDE_TEAMS, cus)
        assert plan["rounds"] >= 2 and R % 2 == 1
        tab = ray_table(R, S)
        keep = keep_rows(names, S)
        valid = torch.tensor([n != "invalid" for n in names])
        grid = grid_of(tab, keep & valid[:, None])
        near_far = tab["near_far"].clone()
        near_far[:, ~valid.to(dev())] = float("nan")
        ranged = dict(tab, near_far=near_far)
        colour, alpha, depth = render(model, ranged, (0, R, valid.to(torch.uint8).to(dev())), S, "t", grid,
                                      want_depth=True, nan_flag=nan)
        outs.append((names, valid, colour, alpha, depth))
        # invalid rays: exactly 0
        gone = ~valid.to(dev())
        assert bool(gone.any())
        assert float(colour[gone].abs().max()) == 0.0 and float(alpha[gone].abs().max()) == 0.0
        assert float(depth[gone].abs().max()) == 0.0
        if layout == 0:
            ids = torch.arange(R, device=dev())
            t, pos, _, logits, _, _, _ = three_pass(model, tab, ids, S, tab["t"])
            conditions(grid, keep & valid[:, None], pos)
            v = valid.to(dev())
            fr.measure_render(rep, {}, "wide S=%d R=%d" % (S, R), logits[v], t[v], keep.to(dev())[v], colour[v],
                              alpha[v], depth[v], teeth=())
    base = outs[0]
    for other, parity in ((outs[1], 0), (outs[2], 1)):
        same = torch.tensor([a == b and r % 2 == parity for r, (a, b) in enumerate(zip(base[0], other[0]))])
        changed = torch.tensor([base[0][r ^ 1] != other[0][r ^ 1] if (r ^ 1) < len(base[0]) else False
                                for r in range(len(base[0]))])
        pick = (same & changed).to(dev())
        assert int(pick.sum()) > len(WIDE_PAIRS)
        for x, y in zip(base[2:], other[2:]):
            assert same_bits(x[pick], y[pick])
    report_line("wide_pairs", rep, S=S)
    assert not rep.problems(), rep.problems()
    assert int(nan.item()) == 0


# ------------------------------------------------------------------------------------- 5. ray lists and outputs
def guarded_image(rows, width):
    buf = torch.full((rows + 2, width, 3), 0xAB, dtype=torch.uint8, device=dev())
    return buf, buf[1:rows + 1]


def bytes_of(colour):
    return (colour * 255.0).to(torch.int32).to(torch.uint8)


@pytest.mark.exact_only(reason=EXACT)
def test_ray_lists_output_sets_and_the_nan_flag():
    """Under a grid: an index list with repeated and descending ids, the range form over rays whose
    ``near_far`` is NaN, the four output sets and ``pixel_offset != 0`` give the bits of the plain
    ascending list wherever they overlap (which is held to float64 here too); guard rows, invalid and
    unlisted pixels keep their 0xAB; the NaN flag stays 0 on all of it.

    The flag itself: a NaN t-value makes a NaN position, and ``occupied_at`` counts a NaN position as
    occupied whatever the cell's bit, so "a NaN t-value on a sample the grid skips" does not exist --
    the sample is evaluated and flagged in an empty cell as in an occupied one.  That a SKIPPED sample
    cannot set the flag is shown the other way round: a model whose logits are NaN for x > 1/2 leaves
    the flag 0 while the grid skips that half of the box, and sets it once one such sample is kept."""
    model = model_of("narrow")
    S, T = LIST_S, LIST_T
    tab = ray_table(T, S)
    names = [PATTERNS[(3 * r + 1) % len(PATTERNS)] for r in range(T)]
    keep = keep_rows(names, S)
    grid = grid_of(tab, keep)
    nan = flag()
    every = torch.arange(T, device=dev())
    c0, a0, d0 = render(model, tab, every, S, "t", grid, want_depth=True, nan_flag=nan)
    assert not bool(torch.isnan(c0).any() | torch.isnan(a0).any() | torch.isnan(d0).any())
    rep = fr.new_report()
    t, pos, _, logits, _, _, _ = three_pass(model, tab, every, S, tab["t"])
    conditions(grid, keep, pos)
    fr.measure_render(rep, {}, "lists S=%d R=%d" % (S, T), logits, t, keep.to(dev()), c0, a0, d0, teeth=())
    report_line("lists", rep, S=S)
    assert not rep.problems(), rep.problems()
    # an index list with descending and repeated ids
    ids = torch.cat([torch.arange(T - 1, -1, -3), torch.tensor([5, 5, 9, 5, T - 1, 0, 0])]).to(dev())
    c1, a1, d1 = render(model, tab, ids, S, "t", grid, want_depth=True, nan_flag=nan)
    assert same_bits(c1, c0[ids]) and same_bits(a1, a0[ids]) and same_bits(d1, d0[ids])
    # the range form: invalid rays carry NaN near_far; ``unit`` reproduces the t-values exactly
    (first, count), width = LIST_RANGE, 10
    valid = torch.ones(T, dtype=torch.bool)
    valid[torch.arange(T) % 5 == 2] = False
    valid[first] = valid[first + count - 1] = False
    near_far = tab["near_far"].clone()
    near_far[:, ~valid.to(dev())] = float("nan")
    ranged = dict(tab, near_far=near_far)
    spec = (first, count, valid.to(torch.uint8).to(dev()))
    inside = valid[first:first + count].to(dev())
    listed = every[first:first + count][inside]
    sets = {}
    for label, kw in (("colour", dict(want_color=True)), ("depth", dict(want_color=False, want_depth=True)),
                      ("image", dict(want_color=False, image=True)),
                      ("all", dict(want_color=True, want_depth=True, image=True))):
        buf = img = None
        if kw.pop("image", False):
            buf, img = guarded_image(count // width, width)
            kw.update(image=img, pixel_offset=first)
        c, a, d = render(model, ranged, spec, S, "unit", grid, nan_flag=nan, **kw)
        sets[label] = (c, a, d, buf, img)
    assert sets["depth"][0] is None and sets["depth"][1] is None and sets["colour"][2] is None
    assert sets["image"][:3] == (None, None, None)
    c, a, d = sets["all"][:3]
    assert float(c[~inside].abs().max()) == 0.0 and float(a[~inside].abs().max()) == 0.0
    assert float(d[~inside].abs().max()) == 0.0
    assert same_bits(c[inside], c0[listed]) and same_bits(a[inside], a0[listed]) and same_bits(d[inside], d0[listed])
    assert same_bits(sets["colour"][0], c) and same_bits(sets["colour"][1], a) and same_bits(sets["depth"][2], d)
    want = bytes_of(c)
    want[~inside] = 0xAB                                   # an invalid ray's pixel stays untouched
    for label in ("image", "all"):
        buf, img = sets[label][3:]
        assert torch.equal(img.reshape(-1, 3), want), label
        assert bool((buf[0] == 0xAB).all() and (buf[-1] == 0xAB).all()), label
    # pixel_offset: pixels land at ray - offset; the rest of the frame is untouched
    offset = 10
    buf, img = guarded_image(12, width)
    render(model, ranged, spec, S, "unit", grid, nan_flag=nan, want_color=False, image=img, pixel_offset=offset)
    frame = torch.full((12 * width, 3), 0xAB, dtype=torch.uint8, device=dev())
    frame[first - offset:first - offset + count] = want
    assert torch.equal(img.reshape(-1, 3), frame)
    assert bool((buf[0] == 0xAB).all() and (buf[-1] == 0xAB).all())
    assert int(nan.item()) == 0
    # the flag: a NaN t-value makes a NaN position, which counts as occupied whatever its cell's bit
    # (occupancy_map.h), so that sample is always evaluated and always flagged ...
    for name in ("all", "none"):
        ray = names.index(name)
        tv = tab["t"][ray:ray + 1].clone()
        tv[0, S // 2] = float("nan")
        got, _ = fr.keep_of(torch.tensor([[float("nan"), 0.0, 0.0]]), grid)
        assert bool(got[0])
        f = flag()
        render(model, tab, every[ray:ray + 1], S, "t", grid, t_values=tv, nan_flag=f)
        assert int(f.item()) != 0, name
    # ... and a sample the grid does skip cannot set it: logits that are NaN for x > 1/2
    bad = model_of("nan")
    right = (tab["t_row"].cpu() - 1.0) > 0.5
    for label, row, flagged in (("skipped", ~right, False), ("kept", ~right | (torch.arange(S) == S - 2), True)):
        g2 = grid_of(tab, row[None].repeat(T, 1))
        f = flag()
        c, a, d = render(bad, tab, every[:9], S, "t", g2, want_depth=True, nan_flag=f)
        assert (int(f.item()) != 0) == flagged, label
        assert bool(torch.isnan(c).any()) == flagged, label


# ------------------------------------------------------------------------------------- 6. frames
@pytest.mark.exact_only(reason=EXACT)
@pytest.mark.parametrize("kind", ["narrow", "wide"])
def test_frames_are_byte_identical(golden, kind):
    """``render_image`` through the fused kernel (camera 1: ``pixel_offset != 0``) == floor(255 c) of
    the fused float colours == ``ops.to_image`` of the three-pass colours, byte for byte."""
    import fourier_feature_nets_amd as ffn
    from tests.test_kernels_gpu import _load_fourier
    from tests.test_pipeline_gpu import _small_model
    from tests.test_round2_gpu import _scene_sampler
    model = _small_model(golden("training")) if kind == "narrow" else _load_fourier(golden("models"), "gaussian512")[0]
    caster = ffn.Raycaster(model)
    sampler = _scene_sampler(64)
    camera = 1
    assert caster._can_fuse(sampler) and bool(model.program().wide) == (kind == "wide")
    fused = caster.render_image(sampler, camera, 100)
    per = sampler.rays_per_camera
    with torch.no_grad():
        floats = caster.render_rays(sampler, (camera * per, per))
    inside = sampler.valid[camera * per:(camera + 1) * per] != 0
    assert bool(inside.any()) and bool((~inside).any())
    want = bytes_of(floats.color)
    want[~inside] = 0
    caster.fused_render = False
    plain = caster.render_image(sampler, camera, 100)
    assert fused.dtype == np.uint8 and fused.shape == (16, 16, 3) and fused.max() > 0
    differ_floats = int((fused.reshape(-1, 3) != want.cpu().numpy()).sum())
    differ_plain = int((fused != plain).sum())
    print("fused render reference", json.dumps(dict(test="frames", kind=kind, bytes=int(fused.size),
                                                     differ_from_fused_floats=differ_floats,
                                                     differ_from_three_pass=differ_plain)))
    assert differ_floats == 0 and differ_plain == 0

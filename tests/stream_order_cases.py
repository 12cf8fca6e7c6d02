"""The table of the stream-order tests: one entry per case, with the entry points of
include/ffn_hip.h it is declared to reach.  Importing it needs neither a GPU nor the library (the
CPU test holds the union of ``reaches`` to the header); the builders import torch when they run.

A builder returns ``(live, run)``: ``live`` maps names to device tensors (the payload named in
``decoy`` is overwritten by the harness, everything else is structural and stays as built;
``live["_decoys"]`` may hold a decoy where the flip along dimension 0 is not a valid one,
``live["_kept"]`` the answers of host-side checks (``_keep_answer``) and
``live["_check_reference"]`` a check of the default-stream answer), and
``run(live)`` issues the operation on the current stream -> its outputs.  In-place operations
work on a clone of the live tensor made inside ``run``.

Shapes: a few hundred rays (across one wave of 64 and one workgroup of 256), trees of depth 5 or
less, images of 32 x 32 or less, counts that are not zero where a zero count would return before
the later launches."""

import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class Case:
    """``decoy`` empty makes a CLEAR-ONLY case: a path that only clears its outputs (a zero count),
    whose answer no input changes.  Its teeth are the marks in fresh memory (stream_helpers): a
    clear that went astray leaves the mark in the clone, so the harness asserts that the real
    answer differs from the mark instead of from a decoy's answer."""

    def __init__(self, name, build, decoy, reaches, env=None):
        self.name, self.build, self.decoy = name, build, tuple(decoy)
        self.reaches = tuple("ffn_" + r for r in reaches)
        self.env = dict(env or {})
        self.clear_only = not self.decoy


CASES = []

# Entry points that no case reaches, with the reason.  The CPU test caps this list at three.
UNREACHED = {}


def case(name, decoy, reaches, env=None, **kwargs):
    def add(build):
        CASES.append(Case(name, (lambda dev: build(dev, **kwargs)) if kwargs else build, decoy,
                          reaches, env))
        return build
    return add


# ------------------------------------------------------------------------------------ helpers
def _rng(seed):
    import numpy as np
    return np.random.default_rng(seed)


# None, or while a guarded placement is active (tests/memory_helpers.py) what moves a tensor into
# a guarded buffer: the inputs the builders make then lie between red zones too
PLACE = None


def _t(x, dev, dtype=None):
    import numpy as np
    import torch
    x = np.ascontiguousarray(x if dtype is None else np.asarray(x).astype(dtype))
    t = torch.from_numpy(x).to(dev).contiguous()
    return t if PLACE is None else PLACE(t)


def _f(rng, *shape, lo=0.0, hi=1.0):
    import numpy as np
    return (rng.random(shape) * (hi - lo) + lo).astype(np.float32)


def _ops():
    from fourier_feature_nets_amd import ops
    return ops


def _keep_answer(live, name, answer):
    """Declares that the wrapper's host-side check ``ops.<name>`` gives, in every run of the case,
    the answer it gave when the case was built (the harness patches it in through pytest's
    monkeypatch).  Those checks read ``proj`` back from the device (is it finite?), which waits
    for the caller's stream: with the check inside the run, scenario A's delay would have drained
    before the launch."""
    live.setdefault("_kept", {})[name] = answer


def _sorted_rows(rng, rows, cols, lo=0.5, hi=4.0):
    import numpy as np
    return np.sort(_f(rng, rows, cols, lo=lo, hi=hi), axis=1)


# ------------------------------------------------------------------------------------ rays (K1, K2)
R, S = 300, 17                  # rays: past one workgroup of 256, ragged; samples per ray
TOTAL = 331                     # rays of the sampler state the batch indexes into


def _sampler_state(dev, seed):
    """starts, directions (TOTAL,3), near_far (2,TOTAL), ray_index (R,) and a flipped near_far."""
    import numpy as np
    rng = _rng(seed)
    near = _f(rng, TOTAL, lo=0.5, hi=1.5)
    far = near + _f(rng, TOTAL, lo=1.0, hi=3.0)
    near_far = np.stack([near, far])
    live = dict(starts=_t(_f(rng, TOTAL, 3, lo=-1, hi=1), dev),
                directions=_t(_f(rng, TOTAL, 3, lo=-1, hi=1), dev),
                near_far=_t(near_far, dev),
                ray_index=_t(rng.permutation(TOTAL)[:R].astype(np.int64), dev))
    live["_decoys"] = dict(near_far=_t(near_far[:, ::-1], dev))
    return live, rng


@case("raygen_nearfar", ["unproj", "cam_pos"], ["raygen_nearfar"])
def _raygen(dev):
    import numpy as np
    rng = _rng(1)
    unproj = np.tile(np.eye(4, dtype=np.float32), (3, 1, 1)) + _f(rng, 3, 4, 4, lo=-0.05, hi=0.05)
    live = dict(unproj=_t(unproj, dev), cam_pos=_t(_f(rng, 3, 3, lo=-3, hi=3), dev))
    return live, lambda v: _ops().raygen_nearfar(v["unproj"], v["cam_pos"], 11, 7, (-1, -1, -1),
                                                 (1, 1, 1))


@case("sample_t", ["near_far", "ray_index", "noise"], ["sample_t"])
def _sample_t(dev):
    import torch
    live, rng = _sampler_state(dev, 2)
    live["noise"] = _t(_f(rng, R, S), dev)
    unit = torch.linspace(0, 1, S, device=dev)
    return live, lambda v: [_ops().sample_t(v["near_far"], v["ray_index"], S, unit, v["noise"], 0.5)]


@case("materialise_samples[views]", ["starts", "directions", "ray_index", "t"],
      ["materialise_samples"], want_views=True)
@case("materialise_samples[no views]", ["starts", "directions", "ray_index", "t"],
      ["materialise_samples"], want_views=False)
def _materialise(dev, want_views):
    live, rng = _sampler_state(dev, 3)
    live["t"] = _t(_sorted_rows(rng, R, S), dev)
    return live, lambda v: _ops().materialise_samples(v["starts"], v["directions"], v["ray_index"],
                                                      v["t"], want_views)


@case("sample_materialise[views]", ["near_far", "starts", "directions", "ray_index", "noise"],
      ["sample_materialise"], want_views=True)
@case("sample_materialise[no views]", ["near_far", "starts", "directions", "ray_index", "noise"],
      ["sample_materialise"], want_views=False)
def _sample_materialise(dev, want_views):
    import torch
    live, rng = _sampler_state(dev, 4)
    live["noise"] = _t(_f(rng, R, S), dev)
    unit = torch.linspace(0, 1, S, device=dev)
    return live, lambda v: _ops().sample_materialise(
        v["near_far"], v["starts"], v["directions"], v["ray_index"], S, unit, v["noise"], None,
        want_views)


@case("cdf_build", ["t_probe", "opacity"], ["cdf_build"])
def _cdf_build(dev):
    rng = _rng(5)
    live = dict(t_probe=_t(_sorted_rows(rng, R, 9), dev), opacity=_t(_f(rng, R, 9, hi=3.0), dev))
    return live, lambda v: [_ops().cdf_build(v["t_probe"], v["opacity"])]


@case("cdf_build_logits", ["t_probe", "logits"], ["cdf_build_logits"])
def _cdf_build_logits(dev):
    rng = _rng(6)
    live = dict(t_probe=_t(_sorted_rows(rng, R, 9), dev),
                logits=_t(_f(rng, R * 9, 4, lo=-2, hi=2), dev))
    return live, lambda v: [_ops().cdf_build_logits(v["t_probe"], v["logits"])]


N_FOCUS, S_FOCUS = 8, 24


def _focus_inputs(dev, seed, rows_local):
    import numpy as np
    import torch
    live, rng = _sampler_state(dev, seed)
    ops = _ops()
    rows = R if rows_local else TOTAL
    # valid CDF rows and the uniform half of every row, made once on the default stream
    live["cdfs"] = ops.cdf_build(_t(_sorted_rows(rng, rows, N_FOCUS), dev),
                                 _t(_f(rng, rows, N_FOCUS, hi=3.0), dev))
    live["u"] = _t(_f(rng, R, N_FOCUS), dev)
    t_io = torch.zeros((R, S_FOCUS), dtype=torch.float32, device=dev)
    unit = torch.linspace(0, 1, S_FOCUS - N_FOCUS, device=dev)
    ops.sample_t(live["near_far"], live["ray_index"], S_FOCUS - N_FOCUS, unit, None, None, out=t_io)
    live["t_io"] = t_io
    torch.cuda.synchronize()
    return live, np, torch


@case("focus_sample_merge", ["near_far", "cdfs", "ray_index", "u", "t_io"], ["focus_sample_merge"],
      rows_local=False)
@case("focus_sample_merge_rows", ["near_far", "cdfs", "ray_index", "u", "t_io"],
      ["focus_sample_merge_rows"], rows_local=True)
def _focus_merge(dev, rows_local):
    live, np, torch = _focus_inputs(dev, 7, rows_local)
    unit_focus = torch.linspace(0, 1, N_FOCUS, device=dev)
    return live, lambda v: [_ops().focus_sample_merge(
        v["near_far"], v["cdfs"], v["ray_index"], v["u"], unit_focus, v["t_io"].clone(), N_FOCUS,
        rows_local)]


# ------------------------------------------------------------------------------------ K3, K8
@case("fourier_encode", ["x"], ["fourier_encode"], freqs=6)
@case("fourier_encode[copy]", ["x"], ["fourier_encode"], freqs=0)
def _encode(dev, freqs):
    rng = _rng(8)
    live = dict(x=_t(_f(rng, R, 3, lo=-1, hi=1), dev))
    b = _t(_f(rng, 3, freqs, lo=-4, hi=4), dev) if freqs else None
    a = _t(_f(rng, freqs, lo=0.5, hi=1.5), dev) if freqs else None
    return live, lambda v: [_ops().fourier_encode(v["x"], b, a, 3.14159, True)]


@case("to_image", ["colors", "pixel_index"], ["to_image"])
def _to_image(dev):
    import numpy as np
    rng = _rng(9)
    live = dict(colors=_t(_f(rng, 200, 3, hi=0.999), dev),
                pixel_index=_t(rng.permutation(17 * 15)[:200].astype(np.int64), dev))
    # flipping both would pair every colour with its own pixel again: the ids are rolled instead
    live["_decoys"] = dict(pixel_index=live["pixel_index"].roll(1))
    return live, lambda v: [_ops().to_image(v["colors"], v["pixel_index"], 17, 15)]


@case("ycrcb_to_rgb_u8", ["image"], ["ycrcb_to_rgb_u8"])
def _ycrcb(dev):
    import numpy as np
    live = dict(image=_t(_rng(10).integers(0, 256, (19, 17, 3), dtype=np.uint8), dev))
    return live, lambda v: [_ops().ycrcb_to_rgb_u8(v["image"].clone())]


# ------------------------------------------------------------------------------------ K5, K6, K7
def _composite_inputs(dev, seed):
    import numpy as np
    rng = _rng(seed)
    return dict(logits=_t(_f(rng, R, S, 4, lo=-2, hi=2), dev), t=_t(_sorted_rows(rng, R, S), dev),
                gt_colors=_t(_f(rng, TOTAL, 3), dev), gt_alphas=_t(_f(rng, TOTAL), dev),
                ray_index=_t(rng.permutation(TOTAL)[:R].astype(np.int64), dev)), rng


@case("composite_fwd[depth]", ["logits", "t"], ["composite_fwd"], depth=True)
@case("composite_fwd[no depth]", ["logits", "t"], ["composite_fwd"], depth=False)
def _composite_fwd(dev, depth):
    import torch
    live, _ = _composite_inputs(dev, 11)

    def run(v):
        flag = torch.zeros((1,), dtype=torch.int32, device=dev)
        return list(_ops().composite_fwd(v["logits"], v["t"], depth, flag)) + [flag]
    return live, run


@case("blend_weights", ["t", "sigma", "d_weights"], ["blend_weights", "blend_weights_bwd"])
def _blend(dev):
    rng = _rng(12)
    live = dict(t=_t(_sorted_rows(rng, R, S), dev), sigma=_t(_f(rng, R, S, hi=3.0), dev),
                d_weights=_t(_f(rng, R, S, lo=-1, hi=1), dev))

    def run(v):
        ops = _ops()
        return [ops.blend_weights(v["t"], v["sigma"])] + list(
            ops.blend_weights_bwd(v["t"], v["sigma"], v["d_weights"], True))
    return live, run


@case("composite_bwd", ["logits", "t", "d_color", "d_alpha"], ["composite_bwd"])
def _composite_bwd(dev):
    live, rng = _composite_inputs(dev, 13)
    live.update(d_color=_t(_f(rng, R, 3, lo=-1, hi=1), dev), d_alpha=_t(_f(rng, R, lo=-1, hi=1), dev))
    return live, lambda v: [_ops().composite_bwd(v["logits"], v["t"], v["d_color"], v["d_alpha"])]


@case("mse_loss", ["color", "alpha", "ray_index"], ["mse_loss", "loss_value"])
def _mse_loss(dev):
    live, rng = _composite_inputs(dev, 14)
    live.update(color=_t(_f(rng, R, 3), dev), alpha=_t(_f(rng, R), dev))

    def run(v):
        ops = _ops()
        sums, d_color, d_alpha = ops.mse_loss(v["color"], v["alpha"], v["gt_colors"], v["gt_alphas"],
                                              v["ray_index"], 1.0 / (3 * R), 0.1 / R)
        return [sums, d_color, d_alpha, ops.loss_value(sums, R, 0.1)]
    return live, run


@case("composite_train", ["logits", "t", "ray_index"], ["composite_train", "loss_from_partials"])
def _composite_train(dev):
    import torch
    live, _ = _composite_inputs(dev, 15)

    def run(v):
        ops = _ops()
        d_logits, partials = ops.composite_train(v["logits"], v["t"], v["gt_colors"], v["gt_alphas"],
                                                 v["ray_index"], 1.0 / (3 * R), 0.1 / R)
        sums = torch.empty((2,), dtype=torch.float32, device=dev)
        return [d_logits, partials, ops.loss_from_partials(partials, R, 0.1, sums), sums]
    return live, run


@case("clip_adam", ["params", "grads", "exp_avg", "exp_avg_sq"], ["clip_adam"])
def _clip_adam(dev):
    import torch
    rng = _rng(16)
    n = 3001                                            # three reduction blocks of 1024, ragged
    live = dict(params=_t(_f(rng, n, lo=-1, hi=1), dev), grads=_t(_f(rng, n, lo=-0.2, hi=0.2), dev),
                exp_avg=_t(_f(rng, n, lo=-0.1, hi=0.1), dev), exp_avg_sq=_t(_f(rng, n, hi=0.01), dev))

    def run(v):
        state = [v[k].clone() for k in ("params", "grads", "exp_avg", "exp_avg_sq")]
        norm = torch.empty((1,), dtype=torch.float32, device=dev)
        _ops().clip_adam(*state, step=3, lr=1e-2, weight_decay=1e-3, norm_out=norm)
        return state + [norm]
    return live, run


# ------------------------------------------------------------------------------------ K11
@case("regression", ["logits", "target"],
      ["regression_train", "regression_eval", "regression_loss"], mse=False)
@case("regression_mse", ["logits", "target"],
      ["regression_mse_train", "regression_mse_eval", "regression_mse_loss"], mse=True)
def _regression(dev, mse):
    import torch
    rng = _rng(17)
    n, c = 1000, 3
    live = dict(logits=_t(_f(rng, n, 4, lo=-2, hi=2), dev), target=_t(_f(rng, n, c), dev))

    def run(v):
        ops = _ops()
        blocks = ops.regression_blocks(n)
        d_logits = torch.empty((n, 4), dtype=torch.float32, device=dev)
        part_train = torch.empty((blocks,), dtype=torch.float32, device=dev)
        part_eval = torch.empty((blocks,), dtype=torch.float32, device=dev)
        sse, loss = (torch.empty((), dtype=torch.float32, device=dev) for _ in range(2))
        out = [d_logits, part_train, part_eval, sse, loss]
        if mse:
            ops.regression_mse_train(v["logits"], v["target"], d_logits, part_train)
            ops.regression_mse_eval(v["logits"], v["target"], part_eval)
            ops.regression_mse_loss(part_train, n * c, sse, loss)
        else:
            image = torch.empty((n, c), dtype=torch.uint8, device=dev)
            ops.regression_train(v["logits"], v["target"], d_logits, part_train)
            ops.regression_eval(v["logits"], v["target"], c, part_eval, image)
            ops.regression_loss(part_train, n * c, sse, loss)
            out.append(image)
        return out
    return live, run


# ------------------------------------------------------------------------------------ K9, K10
@case("occupancy_build[dilate]", ["logits"], ["occupancy_build"], dilate=True)
@case("occupancy_build", ["logits"], ["occupancy_build"], dilate=False)
def _occupancy_build(dev, dilate):
    # softplus(sigma) > 2.9 in one cell in forty: the dilated grid is neither empty nor full
    live = dict(logits=_t(_f(_rng(18), 9 ** 3, 4, lo=-3, hi=3), dev))
    return live, lambda v: [_ops().occupancy_build(v["logits"], 9, 2.9, dilate)]


@case("occupancy_compact", ["positions", "views", "full"],
      ["occupancy_count", "occupancy_compact", "gather_logits", "scatter_logits"])
def _occupancy_compact(dev):
    import torch
    rng = _rng(19)
    n = 700                                             # three blocks of 256, ragged
    ops = _ops()
    bits = ops.occupancy_build(_t(_f(rng, 9 ** 3, 4, lo=-3, hi=3), dev), 9, 0.7, False)
    torch.cuda.synchronize()
    live = dict(positions=_t(_f(rng, n, 3, lo=-1.2, hi=1.2), dev),
                views=_t(_f(rng, n, 3, lo=-1, hi=1), dev), full=_t(_f(rng, n, 4, lo=-2, hi=2), dev))

    def run(v):
        pos, views, index = ops.occupancy_compact(v["positions"], v["views"], (-1, -1, -1),
                                                  (2, 2, 2), 9, bits)
        assert index.shape[0] > 0
        packed = ops.gather_logits(v["full"], index)
        return [pos, views, index, packed, ops.scatter_logits(packed, index, n)]
    return live, run


# the clear and the launches follow both flags: without ``accumulate`` the raster (the bits, or
# the scratch for an odd ``dilate``) is cleared; with it and no ``dilate`` nothing is; with both
# the scratch is cleared and ORed into the bits at the end
@case("occupancy_from_octree", ["rows"], ["occupancy_from_octree"], accumulate=False, dilate=0)
@case("occupancy_from_octree[dilate]", ["rows"], ["occupancy_from_octree"], accumulate=False,
      dilate=1)
@case("occupancy_from_octree[accumulate]", ["rows"], ["occupancy_from_octree"], accumulate=True,
      dilate=0)
@case("occupancy_from_octree[accumulate, dilate]", ["rows"], ["occupancy_from_octree"],
      accumulate=True, dilate=1)
def _occupancy_from_octree(dev, accumulate, dilate):
    import numpy as np
    import torch
    from tests.occupancy_octree_helpers import THRESHOLD, densities, placement, tree
    ids = tree("mixed")
    scale, center, box_min, box_size = placement("small")
    rows = np.zeros((len(ids), 4), np.float32)
    rows[:, 3] = np.nan_to_num(densities(len(ids)), nan=3.0)
    live = dict(rows=_t(rows, dev))
    leaf_index = _t(ids, dev)
    resolution = 33
    words = (resolution ** 3 + 31) // 32
    start = _t(_rng(20).integers(0, 1 << 20, words).astype(np.int32), dev)

    def run(v):
        out = start.clone() if accumulate else None
        return [_ops().occupancy_from_octree(leaf_index, scale, center, box_min, box_size,
                                             resolution, v["rows"], 4, 3, float(THRESHOLD), dilate,
                                             out)]
    return live, run


@case("voxels_forward", ["volume", "positions"], ["voxels_forward"])
def _voxels_forward(dev):
    rng = _rng(21)
    live = dict(volume=_t(_f(rng, 4, 5, 5, 5, lo=-1, hi=1), dev),
                positions=_t(_f(rng, R, 3, lo=-1.3, hi=1.3), dev))
    bias = _t(_f(rng, 4), dev)
    return live, lambda v: [_ops().voxels_forward(v["volume"], bias, v["positions"], 5, 1.1)]


@case("voxels_backward", ["positions", "d_logits"], ["voxels_backward"])
def _voxels_backward(dev):
    rng = _rng(22)
    live = dict(positions=_t(_f(rng, R, 3, lo=-1.3, hi=1.3), dev),
                d_logits=_t(_f(rng, R, 4, lo=-1, hi=1), dev))
    return live, lambda v: _ops().voxels_backward(v["positions"], v["d_logits"], 5, 1.1)


@case("voxels_backward[no samples]", [], ["voxels_backward"])
def _voxels_backward_empty(dev):
    """n == 0: the entry point only clears d_volume and d_bias."""
    import torch
    positions = torch.zeros((0, 3), dtype=torch.float32, device=dev)
    d_logits = torch.zeros((0, 4), dtype=torch.float32, device=dev)
    return {}, lambda v: _ops().voxels_backward(positions, d_logits, 5, 1.1)


# ------------------------------------------------------------------------------------ K12, K16
@case("octree_surface_points", ["alpha", "depth", "starts", "directions", "color"],
      ["octree_surface_points"])
def _surface_points(dev):
    rng = _rng(23)
    n = 700
    live = dict(alpha=_t(_f(rng, n), dev), depth=_t(_f(rng, n, lo=0.5, hi=3), dev),
                starts=_t(_f(rng, n, 3, lo=-1, hi=1), dev),
                directions=_t(_f(rng, n, 3, lo=-1, hi=1), dev), color=_t(_f(rng, n, 3), dev))
    return live, lambda v: _ops().octree_surface_points(v["alpha"], v["depth"], v["starts"],
                                                        v["directions"], 0.5, v["color"])


@case("octree_build", ["positions", "data"],
      ["octree_path_codes", "octree_structure", "octree_interior_nodes", "octree_leaf_means",
       "octree_query", "octree_leaf_geometry"])
def _octree_build(dev):
    import torch
    rng = _rng(24)
    n, depth, scale = 700, 4, 1.0
    live = dict(positions=_t(_f(rng, n, 3, lo=-0.99, hi=0.99), dev), data=_t(_f(rng, n, 3), dev))

    def run(v):
        ops = _ops()
        codes = ops.octree_path_codes(v["positions"], (0.0, 0.0, 0.0), scale, depth)
        sorted_codes, perm = torch.sort(codes, stable=True)
        leaf_of_point, leaf_ids, leaf_start, leaf_count = ops.octree_structure(
            sorted_codes.contiguous(), perm.contiguous(), depth, 1)
        assert leaf_ids.shape[0] > 0
        means = ops.octree_leaf_means(v["data"], perm.contiguous(), leaf_start, leaf_count)
        nodes = torch.sort(ops.octree_interior_nodes(leaf_ids, depth))[0]
        leaf_index = torch.sort(leaf_ids)[0]
        found = ops.octree_query(v["positions"], scale, nodes, leaf_index)
        centers, depths = ops.octree_leaf_geometry(leaf_index, scale)
        return [codes, leaf_of_point, leaf_ids, leaf_start, leaf_count, means, nodes, found,
                centers, depths]
    return live, run


@case("octree_density", ["volume"],
      ["octree_cell_centers", "voxels_forward", "octree_density_select", "octree_bake"])
def _octree_density(dev):
    rng = _rng(25)
    depth, scale = 4, 1.0
    count = 8 ** (depth - 1)
    volume = _f(rng, 4, 5, 5, 5, lo=-3, hi=3)
    live = dict(volume=_t(volume, dev))
    bias = _t(_f(rng, 4), dev)

    def run(v):
        ops = _ops()
        centers = ops.octree_cell_centers(0, count, (0.0, 0.0, 0.0), scale, depth, dev)
        logits = ops.voxels_forward(v["volume"], bias, centers, 5, 1.0)
        codes, data = ops.octree_density_select(logits, 0, 0.05, 2.0 * scale / 2 ** (depth - 1),
                                                depth)
        assert codes.shape[0] > 0
        return [centers, logits, codes, data, ops.octree_bake(logits)]
    return live, run


@case("octree_merge_level", ["data"], ["octree_merge_level"])
def _octree_merge_level(dev):
    import numpy as np
    from tests.octree_density_helpers import hand_cases
    hand = hand_cases()["two_level"]
    depth = hand["depth"]
    codes = _t(np.asarray(hand["codes"], np.int32), dev)
    levels = _t(np.full(len(hand["codes"]), depth - 1, np.int32), dev)
    live = dict(data=_t(hand["data"], dev))
    return live, lambda v: _ops().octree_merge_level(codes, levels, v["data"], depth - 1, depth,
                                                     *hand["tol"])


# ------------------------------------------------------------------------------------ the walks
def _mixed(dev, rays=R, seed=41):
    """``mixed_tree`` (depth 5) with seeded leaf data and lattice rays: structure + payload."""
    import numpy as np
    from tests.octree_lattice_helpers import lattice_rays, mixed_tree
    from tests.octree_volume_helpers import random_leaf_data
    scale, nodes, leaves = mixed_tree()
    starts, directions = lattice_rays(scale, 5, rays, seed)
    data = random_leaf_data(scale, leaves)
    data[:, 3] *= np.float32(8.0)
    live = dict(starts=_t(starts, dev), directions=_t(directions, dev), leaf_data=_t(data, dev))
    return live, (float(scale), 5, _t(nodes, dev), _t(leaves, dev))


def _walk_case(name, reaches, decoy, call):
    @case(name, decoy, reaches)
    def build(dev):
        live, tree = _mixed(dev)
        return live, lambda v: call(_ops(), v, tree)
    return build


_walk_case("octree_walk", ["octree_walk"], ["starts", "directions"],
           lambda ops, v, tr: ops.octree_walk(v["starts"], v["directions"], *tr, 24))
_walk_case("octree_spans", ["octree_spans"], ["starts", "directions"],
           lambda ops, v, tr: ops.octree_spans(v["starts"], v["directions"], *tr, 0.25, 1.0))
_walk_case("octree_first_hit", ["octree_first_hit"], ["starts", "directions"],
           lambda ops, v, tr: ops.octree_first_hit(v["starts"], v["directions"], *tr, 0.25))
_walk_case("octree_render", ["octree_render"], ["starts", "directions", "leaf_data"],
           lambda ops, v, tr: (lambda o: list(o[:3]) + list(o[3]))(ops.octree_render(
               v["starts"], v["directions"], *tr, v["leaf_data"], 0.0, (0.1, 0.2, 0.3), "faces",
               True)))
_walk_case("octree_render_volume", ["octree_render_volume"], ["starts", "directions", "leaf_data"],
           lambda ops, v, tr: ops.octree_render_volume(v["starts"], v["directions"], *tr,
                                                       v["leaf_data"], 0.0, (0.1, 0.2, 0.3), 1e-3))
_walk_case("octree_leaf_weights", ["octree_leaf_weights"], ["starts", "directions", "leaf_data"],
           lambda ops, v, tr: [ops.octree_leaf_weights(v["starts"], v["directions"], *tr,
                                                       v["leaf_data"], 4, 3)])
_walk_case("octree_distortion", ["octree_distortion"], ["starts", "directions", "leaf_data"],
           lambda ops, v, tr: [ops.octree_distortion(v["starts"], v["directions"], *tr,
                                                     v["leaf_data"], 4, 3)])


def _missing_rays(count, scale):
    """Rays that start beyond the cube and point away from it: no leaf is taken, E == 0."""
    import numpy as np
    rng = _rng(40)
    starts = (_f(rng, count, 3, lo=3.0, hi=5.0) * np.float32(scale)).astype(np.float32)
    directions = _f(rng, count, 3, lo=0.25, hi=1.0)
    return starts, directions


def _aim_past_the_tree(live, dev, scale):
    """The real rays miss every leaf (the backwards then only clear their output), the decoy is
    the case's own rays, which take leaves: a second valid ray set of the same shape."""
    starts, directions = _missing_rays(live["starts"].shape[0], scale)
    live["_decoys"] = dict(starts=live["starts"], directions=live["directions"])
    live["starts"], live["directions"] = _t(starts, dev), _t(directions, dev)

    def cleared(want):
        assert not bool(want[0].any()), "the real rays take leaves: not the clear-only path"
    live["_check_reference"] = cleared


_BACKWARD_KINDS = [("", False, False), ("[dist]", True, False), ("[no leaf taken]", False, True),
                   ("[dist, no leaf taken]", True, True)]


def _volume_backward(dev, dist, miss):
    import torch
    live, tree = _mixed(dev)
    rng = _rng(26)
    live.update(d_color=_t(_f(rng, R, 3, lo=-1, hi=1), dev), d_alpha=_t(_f(rng, R, lo=-1, hi=1), dev))
    if miss:
        _aim_past_the_tree(live, dev, tree[0])
    ops = _ops()
    workspace = ops.OctreeGradWorkspace()               # kept between the runs, as a fit keeps it

    def run(v):
        per_ray = torch.empty((R,), dtype=torch.float32, device=dev) if dist else None
        grad = ops.octree_render_volume_backward(
            v["starts"], v["directions"], *tree, v["leaf_data"], v["d_color"], v["d_alpha"], 0.0,
            (0.1, 0.2, 0.3), 1e-3, workspace, None, 0.5 if dist else 0.0, per_ray)
        # one descent step and its projection, in place on a copy of the leaves
        stepped = v["leaf_data"] - 0.5 * grad
        return [grad, per_ray, ops.octree_project(stepped)]
    return live, run


for _tag, _dist, _miss in _BACKWARD_KINDS:
    case("octree_render_volume_backward" + _tag,
         ["starts", "directions", "leaf_data", "d_color", "d_alpha"],
         ["octree_render_volume_backward" + ("_dist" if _dist else ""), "octree_project"],
         dist=_dist, miss=_miss)(_volume_backward)


# ------------------------------------------------------------------------------------ K18, K19
def _sh(dev, degree, rays=65):
    import numpy as np
    from tests.octree_sh_helpers import case as sh_case, sh_leaf_data
    ops = _ops()
    scale, nodes, leaves, starts, directions, _, _ = sh_case("mixed4")
    file_rows = sh_leaf_data(scale, leaves, degree)
    rows = ops.octree_sh_device_layout(file_rows, degree)
    live = dict(starts=_t(starts[:rays], dev), directions=_t(directions[:rays], dev),
                leaf_rows=_t(rows, dev))
    return live, (float(scale), 4, _t(nodes, dev), _t(leaves, dev)), file_rows, np


@case("octree_render_volume_sh[1]", ["starts", "directions", "leaf_rows"],
      ["octree_render_volume_sh"], degree=1)
@case("octree_render_volume_sh[2]", ["starts", "directions", "leaf_rows"],
      ["octree_render_volume_sh"], degree=2)
def _render_sh(dev, degree):
    live, tree, _, _ = _sh(dev, degree)
    return live, lambda v: _ops().octree_render_volume_sh(
        v["starts"], v["directions"], *tree, v["leaf_rows"], degree, 0.0, (0.1, 0.2, 0.3), 1e-3)


@case("octree_sh_accumulate", ["logits", "leaf_data"], ["octree_sh_accumulate"])
def _sh_accumulate(dev):
    live, _, file_rows, np = _sh(dev, 2)
    rng = _rng(27)
    live = dict(logits=_t(_f(rng, len(file_rows), 4, lo=-2, hi=2), dev), leaf_data=_t(file_rows, dev))
    weights = _f(rng, 9, lo=-1, hi=1)
    return live, lambda v: [_ops().octree_sh_accumulate(v["logits"], v["leaf_data"].clone(),
                                                        weights, 0.25, 2)]


def _sh_backward(dev, dist, miss):
    import torch
    degree, rays = 2, 65
    live, tree, _, _ = _sh(dev, degree, rays)
    rng = _rng(28)
    live.update(d_color=_t(_f(rng, rays, 3, lo=-1, hi=1), dev),
                d_alpha=_t(_f(rng, rays, lo=-1, hi=1), dev))
    if miss:
        _aim_past_the_tree(live, dev, tree[0])
    ops = _ops()
    workspace = ops.OctreeGradSHWorkspace(degree)

    def run(v):
        per_ray = torch.empty((rays,), dtype=torch.float32, device=dev) if dist else None
        grad = ops.octree_render_volume_sh_backward(
            v["starts"], v["directions"], *tree, v["leaf_rows"], degree, v["d_color"], v["d_alpha"],
            0.0, (0.1, 0.2, 0.3), 1e-3, workspace, None, 0.5 if dist else 0.0, per_ray)
        stepped = v["leaf_rows"] - 0.5 * grad
        return [grad, per_ray, ops.octree_project_sh(stepped, degree)]
    return live, run


for _tag, _dist, _miss in _BACKWARD_KINDS:
    case("octree_render_volume_sh_backward" + _tag,
         ["starts", "directions", "leaf_rows", "d_color", "d_alpha"],
         ["octree_render_volume_sh_backward" + ("_dist" if _dist else ""), "octree_project_sh"],
         dist=_dist, miss=_miss)(_sh_backward)


# ------------------------------------------------------------------------------------ K20, K21
def _tv_plan(dev):
    """The neighbour table and the plan of ``mixed_tree``, on the default stream."""
    import torch
    from tests.octree_lattice_helpers import mixed_tree
    ops = _ops()
    _, nodes, leaves = mixed_tree()
    nodes, leaves = _t(nodes, dev), _t(leaves, dev)
    plan = ops.octree_tv_plan(ops.octree_neighbors(nodes, leaves), leaves)
    torch.cuda.synchronize()
    assert plan.num_edges > 0
    return nodes, leaves, plan


@case("octree_tv", ["rows"], ["octree_neighbors", "octree_tv"], accumulate=False)
@case("octree_tv[accumulate]", ["rows", "d_rows"], ["octree_neighbors", "octree_tv"],
      accumulate=True)
def _octree_tv(dev, accumulate):
    nodes, leaves, plan = _tv_plan(dev)
    rng = _rng(29)
    count = leaves.shape[0]
    live = dict(rows=_t(_f(rng, count, 4), dev), d_rows=_t(_f(rng, count, 4, lo=-1, hi=1), dev))
    weights = _ops().octree_tv_weights((1.0, 0.5), 4)

    def run(v):
        ops = _ops()
        table = ops.octree_neighbors(nodes, leaves)
        value, grad = ops.octree_tv(v["rows"], plan, weights, 1e-3,
                                    v["d_rows"].clone() if accumulate else None, accumulate)
        return [table, value, grad]
    return live, run


@case("octree_tv[value only]", ["rows"], ["octree_tv"])
def _octree_tv_value(dev):
    """``d_rows`` null: the entry point returns after its second launch."""
    _, leaves, plan = _tv_plan(dev)
    live = dict(rows=_t(_f(_rng(30), leaves.shape[0], 4), dev))
    weights = _ops().octree_tv_weights((1.0, 0.5), 4)
    return live, lambda v: [_ops().octree_tv(v["rows"], plan, weights, 1e-3, want_grad=False)[0]]


@case("octree_tv[no edges]", [], ["octree_neighbors", "octree_tv"])
def _octree_tv_no_edges(dev):
    """A tree of one leaf, the root: no edge, and the entry point only clears the value and the
    gradient."""
    import numpy as np
    import torch
    ops = _ops()
    nodes, leaves = _t(np.zeros(0, np.int64), dev), _t(np.zeros(1, np.int64), dev)
    plan = ops.octree_tv_plan(ops.octree_neighbors(nodes, leaves), leaves)
    torch.cuda.synchronize()
    assert plan.num_edges == 0
    rows = _t(_f(_rng(42), 1, 4), dev)
    weights = ops.octree_tv_weights((1.0, 0.5), 4)

    def run(v):
        table = ops.octree_neighbors(nodes, leaves)
        return [table] + list(ops.octree_tv(rows, plan, weights, 1e-3))
    return {}, run


@case("octree_refine", ["rows"], ["octree_refine_count", "octree_refine_scatter",
                                  "octree_interior_nodes"])
def _octree_refine(dev):
    """K21b's two launches through the launch-only halves of ``ops.octree_refine``, on the
    plumbing it derives from the ids (made here, on the default stream: the wrapper uploads a small
    table first, which waits for the caller's stream, and reads the counts back between the two)."""
    import numpy as np
    from tests.octree_lattice_helpers import mixed_tree
    _, _, leaves = mixed_tree()
    rng = _rng(31)
    num = len(leaves)
    action = rng.integers(0, 3, num).astype(np.uint8)
    first_id = np.array([(8 ** k - 1) // 7 for k in range(12)], np.int64)
    levels = np.searchsorted(first_id, leaves, side="right") - 1
    codes = (leaves - first_id[levels]) << (3 * (10 - levels))
    order = np.argsort(codes, kind="stable")
    count = int((action == 1).sum() + 8 * (action == 2).sum())
    new_depth = int(max(levels[action != 0].max(), levels[action == 2].max() + 1)) + 1
    live = dict(rows=_t(_f(rng, num, 4), dev))
    ids_c, action_c = _t(leaves[order], dev), _t(action[order], dev)
    order_dev = _t(order.astype(np.int64), dev)

    def run(v):
        ops = _ops()
        rows_c = v["rows"][order_dev].contiguous()
        flags, offsets, total = ops._octree_refine_count(action_c)
        new_ids, new_rows, parent = ops._octree_refine_scatter(action_c, flags, offsets, ids_c,
                                                               rows_c, True, 4, count)
        return [total, new_ids, parent, new_rows, ops.octree_interior_nodes(new_ids, new_depth)]
    return live, run


# ------------------------------------------------------------------------------------ K22 .. K28
@case("mesh_sample", ["vertices", "uvs", "texture"], ["mesh_sample"])
def _mesh_sample(dev):
    """Through the launch-only half of ``ops.mesh_sample``: its check reads the small arrays back
    before the launch, which would drain the caller's delay (it is run once here, at the build)."""
    import numpy as np
    import torch
    rng = _rng(32)
    num_vertices, num_triangles, n = 12, 7, 700
    triangles = np.stack([rng.permutation(num_vertices)[:3] for _ in range(num_triangles)])
    counts = rng.multinomial(n, np.full(num_triangles, 1 / num_triangles))
    offsets = _t(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), dev)
    triangles = _t(triangles.astype(np.int32), dev)
    live = dict(vertices=_t(_f(rng, num_vertices, 3, lo=-0.8, hi=0.8), dev),
                uvs=_t(_f(rng, num_vertices, 2), dev),
                texture=_t(rng.integers(0, 256, (5, 4, 3), dtype=np.uint8), dev))
    assert _ops().mesh_sample_check(live["vertices"], triangles, live["uvs"], offsets,
                                    live["texture"]) == n
    torch.cuda.synchronize()
    return live, lambda v: _ops()._mesh_sample_launch(v["vertices"], triangles, v["uvs"], offsets,
                                                      v["texture"], n, True)


def _ball_pictures(dev):
    """Nine cameras round a ball, every camera with a radius and a colour of its own (so that the
    flip along the camera axis is another valid stack with another answer): images, mask, proj."""
    import numpy as np
    import fourier_feature_nets as ffn
    from tests.carve_box_helpers import cameras9
    from tests.carve_helpers import ball_images
    cameras = cameras9(32)
    images = np.concatenate([ball_images(cameras[k:k + 1], 0.45 + 0.04 * k,
                                         (20 + 25 * k, 240 - 20 * k, 60 + 10 * k))
                             for k in range(len(cameras))])
    mask = (images[..., 3] > 0).astype(np.uint8)
    return dict(images=_t(images, dev), mask=_t(mask, dev)), _t(ffn.projection_matrices(cameras), dev)


@case("octree_carve_select", ["images", "mask"], ["octree_carve_select"])
def _carve_select(dev):
    live, proj = _ball_pictures(dev)
    args = (0, 512, (0.0, 0.0, 0.0), 1.0, 4, 128, 0, 1)
    _keep_answer(live, "octree_carve_check", _ops().octree_carve_check(
        live["images"], live["mask"], proj, *args[:2], *args[4:]))

    def run(v):
        codes, data, visited = _ops().octree_carve_select(v["images"], v["mask"], proj, *args,
                                                          1.25, True)
        assert codes.shape[0] > 0
        return [codes, data, visited]
    return live, run


@case("octree_carve_box_level[coarse]", ["images", "sat"], ["octree_carve_box_level"], finest=False)
@case("octree_carve_box_level[finest, expand]", ["images", "sat"], ["octree_carve_box_level"],
      finest=True)
def _carve_box(dev, finest):
    import numpy as np
    import torch
    import fourier_feature_nets as ffn
    from tests.carve_box_helpers import rod_scene
    # the rod, not the ball: the coarse level returns no colours, so that the decoy has to change
    # the survivors.  The summed-area tables are the payload (those of the flipped masks the
    # decoy): they are made with torch.cumsum, which waits for the caller's stream
    ops = _ops()
    cameras, images = rod_scene(32)
    mask = _t((images[..., 3] > 0).astype(np.uint8), dev)
    live = dict(images=_t(images, dev), sat=ops.octree_carve_box_tables(mask))
    live["_decoys"] = dict(sat=ops.octree_carve_box_tables(mask.flip(0).contiguous()))
    proj = _t(ffn.projection_matrices(cameras), dev)
    candidates = _t(np.arange(64, dtype=np.int32), dev)         # every cell of level 2
    level = 3 if finest else 2
    _keep_answer(live, "octree_carve_box_check", ops.octree_carve_box_check(
        live["images"], live["sat"], proj, candidates, finest, level, 4, 128, 0, 1))
    torch.cuda.synchronize()

    def run(v):
        codes, data, visited = ops.octree_carve_box_level(
            v["images"], v["sat"], proj, candidates, level, (0.0, 0.0, 0.0), 1.0, 4, 128, 0, 1,
            1.25, finest, True)
        assert codes.shape[0] > 0
        return [codes, data, visited]
    return live, run


@case("octree_visible_votes", ["images", "rows"], ["octree_visible_votes"], moments=False)
@case("octree_visible_moments", ["images", "rows"], ["octree_visible_moments"], moments=True)
def _visible(dev, moments):
    import numpy as np
    import torch
    import fourier_feature_nets as ffn
    from tests.photo_helpers import ALPHA_U8, moment_scene
    ops = _ops()
    scale, nodes, ids, dens, cameras, images = moment_scene("grid")
    rows = np.zeros((len(ids), 4), np.float32)
    rows[:, 3] = dens
    leaf_index, node_index = _t(ids, dev), _t(nodes, dev)
    centers, _ = ops.octree_leaf_geometry(leaf_index, float(scale))
    proj = _t(ffn.projection_matrices(cameras, origin=(0.0, 0.0, 0.0)), dev)
    eyes = _t(ffn.eye_positions(cameras, (0.0, 0.0, 0.0)), dev)
    live = dict(images=_t(images, dev), rows=_t(rows, dev))
    _keep_answer(live, "octree_visible_check", ops.octree_visible_check(
        centers, leaf_index, live["rows"], 4, 3, live["images"], proj, eyes, 4, ALPHA_U8, 0.01, None,
        moments))
    torch.cuda.synchronize()
    fn = ops.octree_visible_moments if moments else ops.octree_visible_votes
    return live, lambda v: [fn(centers, float(scale), 4, node_index, leaf_index, v["rows"], 4, 3,
                               v["images"], proj, eyes, ALPHA_U8, 0.01)]


@case("octree_focus_sample", ["starts", "directions", "near_far", "ray_index", "rows", "u",
                              "t_uniform"], ["octree_focus_sample"])
def _octree_focus(dev):
    import numpy as np
    from tests.octree_focus_helpers import scene, targets, uniform_samples
    s = scene("mixed")
    rng = _rng(33)
    index = rng.permutation(len(s["near"]))[:100].astype(np.int64)
    near_far = np.stack([s["near"], s["far"]])
    live = dict(starts=_t(s["starts"], dev), directions=_t(s["directions"], dev),
                near_far=_t(near_far, dev), ray_index=_t(index, dev), rows=_t(s["rows"], dev),
                u=_t(targets(100, 8, 34), dev),
                t_uniform=_t(uniform_samples(s["near"][index], s["far"][index], 9), dev))
    live["_decoys"] = dict(near_far=_t(near_far[:, ::-1], dev))
    nodes, leaves = _t(s["node_index"], dev), _t(s["leaf_index"], dev)
    return live, lambda v: _ops().octree_focus_sample(
        v["starts"], v["directions"], v["near_far"], v["ray_index"], s["center"], s["scale"],
        s["depth"], nodes, leaves, v["rows"], 4, 3, v["u"], v["t_uniform"], None, 1e-3, True)


# ------------------------------------------------------------------------------------ K30, K31
@case("octree_mesh", ["rows"], ["octree_mesh_solid", "octree_mesh_candidates",
                                "octree_mesh_vertices", "octree_mesh_face_flags",
                                "octree_mesh_faces"])
def _octree_mesh(dev):
    """The launches of ``OcTree.extract_mesh`` in its order, on device rows."""
    import numpy as np
    import torch
    from tests.octree_lattice_helpers import mixed_tree
    scale, nodes, leaves = mixed_tree()
    depth = 5
    side = float(np.float32(2.0) * np.float32(scale) / np.float32(1 << (depth - 1)))
    rng = _rng(35)
    rows = _f(rng, len(leaves), 4)
    rows[:, 3] = np.where(rng.random(len(leaves)) < 0.5, 0.05, 40.0) / side     # clear or solid
    live = dict(rows=_t(rows, dev))
    nodes, leaves = _t(nodes, dev), _t(leaves, dev)

    def run(v):
        ops = _ops()
        flags, alpha = ops.octree_mesh_solid(v["rows"], 3, None, leaves.shape[0], side, 0.5, dev)
        offsets, total, _ = ops.octree_mesh_candidate_offsets(leaves, flags, depth)
        assert total > 0
        keys, masks, samples = ops.octree_mesh_candidates(nodes, leaves, flags, offsets, 0, total,
                                                          depth)
        keys, order = torch.sort(keys)
        masks, samples = masks[order].contiguous(), samples[order].contiguous()
        vertices, colors, normals, corners = ops.octree_mesh_vertices(
            keys, masks, samples, alpha, v["rows"], (0, 1, 0), depth, float(scale), (0.0, 0.0, 0.0),
            0.5, True)
        triangles = ops.octree_mesh_faces(keys, masks, depth)
        assert triangles.shape[0] > 0
        return [flags, alpha, keys, masks, samples, vertices, colors, normals, corners, triangles]
    return live, run


@case("mesh_raster", ["vertices", "colors"], ["mesh_raster_setup", "mesh_raster_draw",
                                              "mesh_raster_resolve"])
def _mesh_raster(dev):
    import numpy as np
    import torch
    from fourier_feature_nets_amd.cameras import eye_positions, projection_matrices
    from tests import mesh_raster_reference as ref
    vertices, triangles, colors, _ = ref.scene(165, 65)
    width, height = 24, 20
    cam = ref.camera(width, height)
    proj, eye = projection_matrices([cam])[0], eye_positions([cam], (0.0, 0.0, 0.0))[0]
    live = dict(vertices=_t(vertices, dev, np.float32), colors=_t(colors, dev, np.float32))
    triangles = _t(triangles, dev, np.int32)

    def run(v):
        ops = _ops()
        record, status, counts = ops.mesh_raster_setup(v["vertices"], triangles, proj, width, height)
        offsets, total = ops.mesh_raster_offsets(counts)
        assert total > 0
        zbuf = torch.full((width * height,), ops.MESH_RASTER_EMPTY, dtype=torch.int64, device=dev)
        ops.mesh_raster_draw(record, offsets, 0, total, width, height, zbuf)
        return [record, status, counts, zbuf] + list(ops.mesh_raster_resolve(
            zbuf, record, v["vertices"], triangles, v["colors"], None, None, eye, (0.25, 0.5, 0.75),
            width, height))
    return live, run


# ------------------------------------------------------------------------------------ K4: the MLPs
_MODELS = {}


def _model(name, dev):
    """The golden chain ``name`` with weights of its own (not shared with the other test modules:
    the cases overwrite its first layer)."""
    import numpy as np
    if name not in _MODELS:
        from tests.model_loaders import load_fourier, load_nerf
        g = np.load(os.path.join(GOLDEN, "models.npz"), allow_pickle=False)
        if name == "nerf_small":
            model, _ = load_nerf(g, name, [2], False, dev)
        else:
            model, _ = load_fourier(g, name, dev)
        _MODELS[name] = model
    return _MODELS[name]


def _mlp_inputs(model, n, dev, seed):
    import numpy as np
    rng = _rng(seed + n)
    live = dict(positions=_t(_f(rng, n, 3, lo=-1, hi=1), dev),
                d_logits=_t(_f(rng, n, 4, lo=-1, hi=1) / np.float32(np.sqrt(n)), dev))
    if model.use_view:
        views = _f(rng, n, 3, lo=-1, hi=1)
        live["views"] = _t(views / np.linalg.norm(views, axis=1, keepdims=True), dev)
    return live


MLP_REACHES = {
    "f32": ["mlp_pack_jobs", "mlp_forward", "mlp_backward_data", "mlp_wgrad_units",
            "mlp_wgrad_reduce"],
    "bf16x3": ["mlp_pack_jobs", "mlp_pack_bf16_parts", "mlp_forward_bf16x3",
               "mlp_forward_bf16x3_train", "mlp_backward_data_bf16x3", "mlp_wgrad_units_bf16x3",
               "mlp_wgrad_reduce"],
    "bf16x6": ["mlp_pack_jobs", "mlp_pack_bf16_parts", "mlp_forward_bf16x6",
               "mlp_forward_bf16x6_train", "mlp_backward_data_bf16x6", "mlp_wgrad_units_bf16x6",
               "mlp_wgrad_reduce"],
    "bf16x6+f32wgrad": ["mlp_pack_jobs", "mlp_pack_bf16_parts", "mlp_forward_bf16x6",
                        "mlp_forward_bf16x6_train", "mlp_backward_data_bf16x6", "mlp_wgrad_units",
                        "mlp_wgrad_reduce"],
}


def _mlp_case(chain, n, mode):
    precision = mode.split("+")[0]
    decoy = ["w0", "positions", "d_logits"] + (["views"] if chain == "nerf_small" else [])

    @case("mlp[%s, %d, %s]" % (chain, n, mode), decoy, MLP_REACHES[mode],
          env={"FFN_BF16X6_WGRAD": "f32" if mode.endswith("f32wgrad") else "bf16x6"})
    def build(dev):
        import torch
        model = _model(chain, dev)
        prog = model.program()
        live = _mlp_inputs(model, n, dev, 36)
        live["w0"] = prog.layers[0].weight.detach()     # the parameter's own storage
        assert prog.covers(precision)

        def run(v):
            views = v.get("views")
            # the packs follow the weights: re-derived in the run, as after an optimiser step
            prog.pack()
            if precision != "f32":
                prog.pack16(parts=2 if precision == "bf16x3" else 3)
            saved = torch.empty((prog.saved_floats(n),), dtype=torch.float32, device=dev)
            grads = torch.empty((prog.num_grad_floats,), dtype=torch.float32, device=dev)
            out = [prog.forward(v["positions"], views, None, precision=precision)]
            out.append(prog.forward(v["positions"], views, saved, precision=precision))
            prog.backward(v["d_logits"], v["positions"], views, saved, grads, precision=precision)
            return out + [grads]
        return live, run
    return build


for _chain in ("positional", "nerf_small"):
    for _n in (33, 1000):
        for _mode in ("f32", "bf16x3", "bf16x6", "bf16x6+f32wgrad"):
            _mlp_case(_chain, _n, _mode)


@case("mlp_pack", ["src"], ["mlp_pack", "mlp_pack_bf16"])
def _mlp_pack(dev):
    """The per-matrix packs, which only ``ops._call`` reaches: a 64 x 48 matrix into one K block
    of 16 (bf16) / six groups of 8 (f32) columns and two tiles of 32 rows."""
    import torch
    from fourier_feature_nets_amd._lib import c_i, c_p
    rows, cols = 64, 48
    live = dict(src=_t(_f(_rng(37), rows, cols, lo=-1, hi=1), dev))
    col_map = torch.arange(cols, dtype=torch.int32, device=dev)

    def run(v):
        ops = _ops()
        groups, tiles, kblocks = cols // 8, rows // 32, cols // 16
        dst = torch.empty((groups * tiles * 256,), dtype=torch.float32, device=dev)
        ops._call("ffn_mlp_pack", ops._dev(v["src"]), c_i(rows), c_i(cols), c_i(cols), c_i(0), c_p(0),
                  ops._dev(col_map, torch.int32), c_i(groups), c_i(tiles), ops._dev(dst))
        dst16 = torch.empty((kblocks * tiles * 2 * 512,), dtype=torch.int16, device=dev)
        ops._call("ffn_mlp_pack_bf16", ops._dev(v["src"]), c_i(rows), c_i(cols), c_i(cols),
                  ops._dev(col_map, torch.int32), c_i(kblocks), c_i(tiles), c_i(0),
                  ops._dev(dst16, torch.int16))
        return [dst, dst16]
    return live, run


@case("render_fused_fwd", ["starts", "directions", "near_far", "ray_index"], ["render_fused_fwd"])
def _render_fused(dev):
    import torch
    model = _model("positional", dev)
    prog = model.program()
    live, _ = _sampler_state(dev, 38)
    unit = torch.linspace(0, 1, S, device=dev)
    return live, lambda v: prog.render(v["starts"], v["directions"], v["near_far"], v["ray_index"],
                                       S, unit, want_depth=True)


@case("focus_fused", ["starts", "directions", "near_far", "ray_index", "u", "t_io"],
      ["focus_fused"])
def _focus_fused(dev):
    model = _model("positional", dev)
    prog = model.program()
    live, np, torch = _focus_inputs(dev, 39, True)
    del live["cdfs"]
    unit_focus = torch.linspace(0, 1, N_FOCUS, device=dev)
    return live, lambda v: [prog.focus_sample(v["starts"], v["directions"], v["near_far"],
                                              v["ray_index"], S_FOCUS, N_FOCUS, unit_focus, v["u"],
                                              v["t_io"].clone())]

"""Fitting a baked octree to the training images through its own volume renderer (K17).

A density tree (``OcTree.build_from_model`` / ``bake``) holds the model's value at one point per
leaf.  ``OctreeField`` makes the leaf values a parameter: its forward is ``OcTree.render_volume``
(K15) bit for bit, its backward the gradient walk K17a and the per-leaf sums K17b
(``csrc/octree_walk.hip``, ``csrc/octree_grad.hip``), deterministic and without float atomics.
``fit_octree`` is the training loop on the kernels of the NeRF path: K6 (loss and its gradient),
K17a + K17b, K7 (clip and Adam) on the flat ``(4 L,)`` buffer, K17c (projection onto
``0 <= rgb <= 1``, ``sigma >= 0``).  A fit does not change the structure of the tree.  No counterpart
in the reference.  The loop is ``fit_loop.run``, which the mesh fits use too; ``_fit`` supplies the
seeded shuffle of the rays, one step's forward and gradient, the projection, the validation and the
``tv:`` / ``dist:`` fields of the report line.

``OctreeSHField`` and ``fit_octree_sh`` (K19) are the same for a tree with spherical-harmonic leaves
(``OcTree.bake_sh``): the parameter is the ``(L, stride)`` buffer in the device layout K18a reads,
the forward K18a, the backward K19a + K19b, the projection K19c (density ``>= 0``; the coefficients
live in logit space and are not clamped).

Both fields offer the total-variation prior of K20 (``csrc/octree_tv.hip``): ``total_variation`` is
the Charbonnier energy between leaves that touch across a face, ``tv_backward`` its gradient,
deterministic and without a host sync, and ``tv_weight`` on both fit loops adds it to the data
term's gradient.  It is off by default, and off means not entered.

``leaf_weights_over`` and ``fit_octree_adaptive`` (K21) change the structure between fits: the first
folds ``OcTree.leaf_weights`` (K21a) over every ray of a dataset, the second alternates a fit with
measure -> ``refine_actions`` -> ``OcTree.refine`` (K21b).  With ``rounds=0`` it is the plain fit.

Both fields' ``backward`` take ``dist_scale`` and ``ray_distortion`` (K29b): the gradient of the
rays' distortion (``OcTree.distortion``) folded into the two walks of the backward, and
``dist_weight`` on the fit loops passes ``dist_weight / batch`` there.  Off by default, and off means
the entry points without the term.
"""

from typing import List, NamedTuple, Tuple

import numpy as np
import torch

from . import fit_loop, ops
from .fit_loop import FitLogEntry
from .octree import OcTree, refine_actions
from .utils import RenderResult

# one round of fit_octree_adaptive: leaves_before = dropped + split + kept, leaves_after = kept +
# 8 split; weight_quantiles the (min, 25 %, 50 %, 75 %, max) of the measured per-leaf weights
RefineReport = NamedTuple("RefineReport", [("round", int), ("leaves_before", int), ("dropped", int),
                                           ("split", int), ("leaves_after", int),
                                           ("depth_before", int), ("depth_after", int),
                                           ("weight_quantiles", Tuple[float, ...])])
# starting values, untuned (see refine_actions)
PRUNE_BELOW = 1e-2
SPLIT_ABOVE = 1e-1

# Raycaster.fit's clipping (ops.clip_adam's defaults)
CLIP_VALUE = 0.1
MAX_NORM = 0.1
# of 1e-3, 1e-2 and 1e-1 tried on the depth-8 density tree of the opaque-ball model, the fastest
# descent of the training loss; 1e-1 diverges (README, profiles/r15_octree_fit_microbench.json)
LEARNING_RATE = 1e-2


class _RenderVolume(torch.autograd.Function):
    @staticmethod
    def forward(ctx, data, field, starts, directions, t_min, background, min_transmittance):
        # the field's own render: K15 for an OctreeField, K18a for an OctreeSHField
        color, alpha, depth = field._render(data, starts, directions, t_min, background,
                                            min_transmittance)
        ctx.field = field
        ctx.args = (t_min, background, min_transmittance)
        ctx.save_for_backward(data, starts, directions)
        ctx.mark_non_differentiable(depth)
        return color, alpha, depth

    @staticmethod
    def backward(ctx, d_color, d_alpha, _):
        data, starts, directions = ctx.saved_tensors
        n = starts.shape[0]
        if d_color is None:
            d_color = torch.zeros((n, 3), dtype=torch.float32, device=starts.device)
        if d_alpha is None:
            d_alpha = torch.zeros((n,), dtype=torch.float32, device=starts.device)
        grad = ctx.field.backward(starts, directions, d_color.contiguous(), d_alpha.contiguous(),
                                  *ctx.args, data=data)
        return grad, None, None, None, None, None, None


def _refuse_sh(tree: OcTree, who: str):
    if tree.sh_degree is not None:
        raise ValueError("%s: fitting SH leaves is not built into this entry (the tree has sh_degree %d); "
                         "use OctreeSHField / fit_octree_sh" % (who, tree.sh_degree))


class _TotalVariation:
    """K20 for a field: the energy and its gradient on the field's own rows.  The field supplies
    ``_tv_weights`` (its columns) and ``_tree``."""

    def total_variation(self, weights=None, eps: float = 1e-2, data=None) -> torch.Tensor:
        """K20b: the total-variation energy (``OcTree.total_variation``) of ``data`` (default: the
        parameter) as a device scalar; no host sync."""
        rows = self.data.detach() if data is None else data
        value, _ = ops.octree_tv(rows, self._tree._tv_plan(), self._tv_weights(weights), eps)
        return value

    def tv_backward(self, weights=None, eps: float = 1e-2, data=None, out=None,
                    accumulate: bool = False) -> torch.Tensor:
        """K20b + K20c: the gradient of ``total_variation`` with respect to ``data``, in its shape;
        with ``accumulate`` added to the content of ``out`` (one add per element).  ``weights``
        scale the columns, so a caller's ``tv_weight`` is passed here as it is.  Deterministic, no
        host sync."""
        rows = self.data.detach() if data is None else data
        _, grad = ops.octree_tv(rows, self._tree._tv_plan(), self._tv_weights(weights), eps, out,
                                accumulate)
        return grad


class _LeafField(_TotalVariation, torch.nn.Module):
    """What ``OctreeField`` and ``OctreeSHField`` share: the tree, its centre and device, the
    parameter ``data``, the differentiable ``forward`` and ``tree()``.  The subclass supplies the
    rows of ``data``, ``sh_degree`` (None: plain leaves), the workspace, ``_render``, ``backward``,
    ``_tv_weights``, ``_project`` and ``_file_layout``."""

    def __init__(self, tree: OcTree, rows, sh_degree, center, device, workspace):
        super().__init__()
        self.sh_degree = sh_degree
        if center is None:
            center = tree.center
        self.center = None if center is None else tuple(float(c) for c in center)
        if self.center is not None and len(self.center) != 3:
            raise ValueError("%s: center has three components" % type(self).__name__)
        if device is not None:
            tree._device = torch.device(device)
        self._tree = tree
        self.data = torch.nn.Parameter(torch.from_numpy(
            np.ascontiguousarray(rows, dtype=np.float32)).to(tree._dev()))
        self.workspace = workspace

    def forward(self, starts, directions, t_min: float = 0.0, background=(0, 0, 0),
                min_transmittance: float = 0.0) -> RenderResult:
        """``tree.render_volume`` of the current data, bit for bit, as device tensors;
        differentiable with respect to ``data`` (colour and alpha; depth has no gradient).
        starts, directions: (N,3) float32 device tensors relative to the root cube's centre."""
        self._tree._check_volume(min_transmittance)
        starts, directions, _ = self._tree._rays(starts, directions)
        background = tuple(float(v) for v in background)
        return RenderResult(*_RenderVolume.apply(self.data, self, starts, directions, float(t_min),
                                                 background, float(min_transmittance)))

    def _geometry(self):
        tree = self._tree
        return (tree._scale, tree.depth, tree._on_device("node_index"),
                tree._on_device("leaf_index"))

    def tree(self) -> OcTree:
        """A new ``OcTree`` (file layout) with the same ``sh_degree``, structure and centre and the
        current data."""
        old = self._tree
        new = OcTree(old._scale, old._node_index, old._leaf_index,
                     self._file_layout(self.data.detach().cpu().numpy()), self.sh_degree)
        new._device = old._device
        new._center = self.center
        return new


class OctreeField(_LeafField):
    """The leaf values of a baked tree as a parameter.  ``data`` (L,4) float32 ``[r, g, b, sigma]``
    on the device, initialised from ``tree.leaf_data()``."""

    def __init__(self, tree: OcTree, center=None, device=None):
        _refuse_sh(tree, "OctreeField")
        tree._check_volume(0.0)
        values = np.asarray(tree.leaf_data())[:, :4]      # further channels are never rendered
        super().__init__(tree, values, None, center, device, ops.OctreeGradWorkspace())

    def backward(self, starts, directions, d_color, d_alpha, t_min=0.0, background=(0, 0, 0),
                 min_transmittance=0.0, data=None, out=None, dist_scale=0.0,
                 ray_distortion=None) -> torch.Tensor:
        """K17a + K17b: d(data) (L,4) for upstream ``d_color`` (N,3) and ``d_alpha`` (N,).  K29b:
        ``dist_scale > 0`` adds ``dist_scale * d(sum_r D_r)/d sigma`` to the density column, and
        ``ray_distortion`` (N,) receives ``D`` per ray (``ops.octree_render_volume_backward``);
        with neither, the call is the one without the term."""
        if dist_scale == 0.0 and ray_distortion is None:
            return ops.octree_render_volume_backward(
                starts, directions, *self._geometry(), self.data.detach() if data is None else data,
                d_color, d_alpha, float(t_min), background, float(min_transmittance), self.workspace,
                out)
        return ops.octree_render_volume_backward(
            starts, directions, *self._geometry(), self.data.detach() if data is None else data,
            d_color, d_alpha, float(t_min), background, float(min_transmittance), self.workspace,
            out, dist_scale=dist_scale, ray_distortion=ray_distortion)

    def _render(self, data, starts, directions, t_min, background, min_transmittance):
        return ops.octree_render_volume(starts, directions, *self._geometry(), data, t_min,
                                        background, min_transmittance)

    def _tv_weights(self, weights):
        return ops.octree_tv_weights(weights, 4, None)

    def _project(self, data):
        return ops.octree_project(data)

    def _file_layout(self, rows):
        return rows.copy()


class OctreeSHField(_LeafField):
    """The leaf values of an SH tree (``OcTree.bake_sh``) as a parameter.  ``data`` (L, stride)
    float32 on the device in the layout K18a reads (``ops.octree_sh_device_layout``:
    ``[sigma, k_r.., k_g.., k_b.., 0 ..]``), so that a step never repacks and Adam runs on the flat
    buffer; the padding has a zero gradient and stays zero."""

    def __init__(self, tree: OcTree, center=None, device=None):
        if not isinstance(tree, OcTree) or tree.sh_degree is None:
            raise ValueError("OctreeSHField: the tree has no SH leaves (sh_degree is None); a plain "
                             "baked tree is fitted by OctreeField / fit_octree")
        tree._check_volume(0.0)
        degree = int(tree.sh_degree)
        rows = ops.octree_sh_device_layout(np.asarray(tree.leaf_data()), degree)
        super().__init__(tree, rows, degree, center, device, ops.OctreeGradSHWorkspace(degree))

    def backward(self, starts, directions, d_color, d_alpha, t_min=0.0, background=(0, 0, 0),
                 min_transmittance=0.0, data=None, out=None, dist_scale=0.0,
                 ray_distortion=None) -> torch.Tensor:
        """K19a + K19b: d(data) (L, stride) for upstream ``d_color`` (N,3) and ``d_alpha`` (N,).
        ``dist_scale`` and ``ray_distortion`` (K29b) as in ``OctreeField.backward``."""
        if dist_scale == 0.0 and ray_distortion is None:
            return ops.octree_render_volume_sh_backward(
                starts, directions, *self._geometry(), self.data.detach() if data is None else data,
                self.sh_degree, d_color, d_alpha, float(t_min), background,
                float(min_transmittance), self.workspace, out)
        return ops.octree_render_volume_sh_backward(
            starts, directions, *self._geometry(), self.data.detach() if data is None else data,
            self.sh_degree, d_color, d_alpha, float(t_min), background, float(min_transmittance),
            self.workspace, out, dist_scale=dist_scale, ray_distortion=ray_distortion)

    def _render(self, data, starts, directions, t_min, background, min_transmittance):
        return ops.octree_render_volume_sh(starts, directions, *self._geometry(), data,
                                           self.sh_degree, t_min, background, min_transmittance)

    def _tv_weights(self, weights):
        return ops.octree_tv_weights(weights, int(self.data.shape[1]), self.sh_degree)

    def _project(self, data):
        return ops.octree_project_sh(data, self.sh_degree)

    def _file_layout(self, rows):
        return ops.octree_sh_file_layout(rows, self.sh_degree)


def _validation_psnr(field, dataset, t_min, min_transmittance) -> float:
    """-10 log10 of the mean colour-MSE + alpha_weight * alpha-MSE over every ray of the
    dataset's cameras, camera by camera."""
    sampler = dataset.sampler
    per = sampler.rays_per_camera
    shift = torch.tensor(field.center, dtype=torch.float32, device=sampler.starts.device)

    def frame(camera):
        rays = torch.arange(camera * per, (camera + 1) * per, dtype=torch.int64,
                            device=sampler.starts.device)
        with torch.no_grad():
            return field(sampler.starts[rays] - shift, sampler.directions[rays], t_min, (0, 0, 0),
                         min_transmittance)

    aw = float(dataset.alpha_weight) if dataset._gt_alphas() is not None else 0.0
    return fit_loop.camera_psnr(frame, sampler.num_cameras, per, dataset, aw)


def fit_octree(tree: OcTree, train_dataset, val_dataset=None, batch_size: int = 4096,
               learning_rate: float = LEARNING_RATE, num_steps: int = 2000,
               report_interval: int = 500, center=None, t_min: float = 0.0,
               min_transmittance: float = 0.0, clip_value: float = CLIP_VALUE,
               max_norm: float = MAX_NORM, seed: int = 20080524,
               verbose: bool = True, tv_weight=None,
               tv_eps: float = 1e-2, dist_weight: float = 0.0) -> Tuple[OcTree, List[FitLogEntry]]:
    """Optimises the leaf values of a baked ``tree`` against the images of ``train_dataset`` (an
    ``ImageDataset``) through ``render_volume`` with a black background; -> (a new ``OcTree`` of the
    same structure, log).  One step: a batch of ray ids from a seeded shuffle of EVERY ray of every
    camera (as ``render_image``, the sampler's validity mask is not applied), the forward on
    ``sampler.starts - center``, K6 with the dataset's colours, alphas and ``alpha_weight``, K17a +
    K17b, K7 with ``clip_value`` / ``max_norm`` (defaults: those of ``Raycaster.fit``), K17c.  The
    log holds ``(step, loss, val_psnr)`` -- every step's training loss, ``val_psnr`` (over all rays
    of ``val_dataset``'s cameras) at steps below 10 and multiples of ``report_interval``, else NaN
    -- and report steps are printed as ``Raycaster.fit`` prints them.  The only host
    synchronisation of a step is the read-back inside K17b; the losses are fetched at the end.

    ``tv_weight = (rgb, sigma)`` switches the total-variation prior of ``OcTree.total_variation`` on
    (K20): with a non-zero entry the step adds ``tv_weight * dR/d(data)`` (``tv_backward`` with
    ``accumulate``, ``tv_eps`` the Charbonnier eps) to the gradient of the data term after K17b, then
    K7 and K17c as before -- no further host sync.  The logged ``loss`` stays the data term; report
    lines gain ``tv:``, the weighted energy.  With the default of all zeros the TV code is not
    entered and the result is today's bit for bit (``None``, the default, is all zeros: the two fit
    loops keep one signature).  ``tv_weight`` and ``tv_eps`` are checked like every other argument
    before the first step, whether the prior is on or not: ``tv_eps <= 0`` raises with a zero
    weight too.

    ``dist_weight > 0`` switches the per-ray distortion prior on (K29): the step's loss gains
    ``dist_weight * (1 / count) * sum_r D_r`` with ``D`` of ``OcTree.distortion`` over the batch's
    ``count`` rays, and its gradient -- on the densities alone -- is formed inside K17a's two walks
    (``field.backward(..., dist_scale=dist_weight / count)``): no third walk, no further host sync.
    It penalises a ray that spreads its weight along a chord, which the data term and TV do not: a
    fat hull can be thinned.  The logged ``loss`` stays the data term; report lines gain ``dist:``,
    the batch mean of ``D``.  ``dist_weight`` is checked like every other argument (finite and
    ``>= 0``); with the default 0 the term's code is not entered and the tree, the log and the
    printed lines are today's bit for bit.  Limits: ``D`` treats a leaf's weight as uniform along
    its chord, so it depends on the partition (``refine`` with splits changes it at second order);
    it is measured in world lengths; it sees the tree's own densities only; it can eat thin true
    structure behind a strong surface; ``dist_weight`` has no tuned default."""
    return _fit("fit_octree", OctreeField, tree, train_dataset, val_dataset, batch_size,
                learning_rate, num_steps, report_interval, center, t_min, min_transmittance,
                clip_value, max_norm, seed, verbose, tv_weight, tv_eps, dist_weight)


def fit_octree_sh(tree: OcTree, train_dataset, val_dataset=None, batch_size: int = 4096,
                  learning_rate: float = LEARNING_RATE, num_steps: int = 2000,
                  report_interval: int = 500, center=None, t_min: float = 0.0,
                  min_transmittance: float = 0.0, clip_value: float = CLIP_VALUE,
                  max_norm: float = MAX_NORM, seed: int = 20080524,
                  verbose: bool = True, tv_weight=None,
                  tv_eps: float = 1e-2,
                  dist_weight: float = 0.0) -> Tuple[OcTree, List[FitLogEntry]]:
    """``fit_octree`` for a tree with SH leaves (``OcTree.bake_sh``): the same arguments, defaults,
    seeded shuffle, log and report lines; -> (a new SH ``OcTree`` of the same structure and
    ``sh_degree``, log).  One step: K18a, K6, K19a + K19b, K7 on the flat ``(L stride,)`` buffer in
    the device layout, K19c (density ``>= 0``, NaN -> 0; the logit-space coefficients are not
    clamped).  The default learning rate is ``fit_octree``'s.  ``tv_weight = (band0, higher_bands,
    sigma)`` and ``tv_eps`` as in ``fit_octree`` (K20), on the rows of the device layout;
    ``dist_weight`` as in ``fit_octree`` (K29), inside K19a's two walks, with the same limits."""
    return _fit("fit_octree_sh", OctreeSHField, tree, train_dataset, val_dataset, batch_size,
                learning_rate, num_steps, report_interval, center, t_min, min_transmittance,
                clip_value, max_norm, seed, verbose, tv_weight, tv_eps, dist_weight)


def _fit(who, field_type, tree, train_dataset, val_dataset, batch_size, learning_rate, num_steps,
         report_interval, center, t_min, min_transmittance, clip_value, max_norm, seed, verbose,
         tv_weight, tv_eps, dist_weight=0.0):
    """``fit_octree`` / ``fit_octree_sh`` on ``fit_loop.run``: the checks, the seeded shuffle of all
    rays, one step's forward and gradient, the validation and the ``tv:`` / ``dist:`` report fields
    are here; the field supplies the render, the backward, the TV gradient and the projection."""
    fit_loop.check_schedule(who, "batch_size >= 1, num_steps >= 0, report_interval >= 1",
                            batch_size, num_steps, report_interval, learning_rate)
    batch_size, num_steps = int(batch_size), int(num_steps)
    if field_type is OctreeField:
        _refuse_sh(tree, who)
    elif not isinstance(tree, OcTree) or tree.sh_degree is None:
        raise ValueError("%s: the tree has no SH leaves (sh_degree is None); a plain baked tree is "
                         "fitted by fit_octree" % who)
    tree._check_volume(min_transmittance)
    dist_weight = ops.octree_check_dist_scale("%s: dist_weight" % who, dist_weight)
    dist_on = dist_weight > 0.0
    if center is None:
        center = tree.center
    if center is None:
        raise ValueError("%s: a loaded tree does not know the centre of its root cube "
                         "(the file has no place for it); pass center=" % who)
    sampler = train_dataset.sampler
    dev = sampler.starts.device
    field = field_type(tree, center, dev)
    tv_eps = ops.octree_tv_check_eps(tv_eps)
    # (refuses a tuple of the wrong shape; None is off, as the default of all zeros)
    tv_on = tv_weight is not None and bool(field._tv_weights(tv_weight).any())
    data = field.data.detach()
    shift = torch.tensor(field.center, dtype=torch.float32, device=dev)
    alphas = train_dataset._gt_alphas()
    aw = float(train_dataset.alpha_weight) if alphas is not None else 0.0
    num_rays = sampler.num_cameras * sampler.rays_per_camera
    generator = torch.Generator(device=dev)
    generator.manual_seed(int(seed))
    ray_dist = None                          # the last step's per-ray distortion, for the report

    def epoch():
        order = torch.randperm(num_rays, generator=generator, device=dev)
        return (order[start:start + batch_size] for start in range(0, num_rays, batch_size))

    def step(rays, grads):
        nonlocal ray_dist
        count = int(rays.numel())
        starts = (sampler.starts[rays] - shift).contiguous()
        directions = sampler.directions[rays].contiguous()
        color, alpha, _ = field._render(data, starts, directions, float(t_min), (0.0, 0.0, 0.0),
                                        float(min_transmittance))
        sums, d_color, d_alpha = ops.mse_loss(color, alpha, train_dataset.colors, alphas, rays,
                                              1.0 / (3 * count), aw / count)
        loss = ops.loss_value(sums, count, aw)
        if dist_on:
            ray_dist = torch.empty((count,), dtype=torch.float32, device=dev)
            field.backward(starts, directions, d_color, d_alpha, t_min, (0.0, 0.0, 0.0),
                           min_transmittance, data=data, out=grads,
                           dist_scale=dist_weight / count, ray_distortion=ray_dist)
        else:
            field.backward(starts, directions, d_color, d_alpha, t_min, (0.0, 0.0, 0.0),
                           min_transmittance, data=data, out=grads)
        if tv_on:
            field.tv_backward(tv_weight, tv_eps, data=data, out=grads, accumulate=True)
        return loss

    def fields():
        shown = []
        if tv_on:
            shown.append(("tv", float(field.total_variation(tv_weight, tv_eps, data).item())))
        if dist_on:
            shown.append(("dist", float(ray_dist.mean().item())))
        return shown

    def validate():
        return _validation_psnr(field, val_dataset, t_min, min_transmittance)

    log = fit_loop.run(data, epoch, step, field._project,
                       validate if val_dataset is not None else None, num_steps, learning_rate,
                       report_interval, clip_value, max_norm, verbose, fields)
    return field.tree(), log


def leaf_weights_over(tree: OcTree, dataset, center=None, t_min: float = 0.0,
                      min_transmittance: float = 0.0) -> np.ndarray:
    """``OcTree.leaf_weights`` (K21a) folded over every ray of every camera of ``dataset`` (an
    ``ImageDataset``), camera by camera into one buffer -> (L,) float32 numpy.  The rays are those of
    the validation PSNR of the fits: ``sampler.starts - center`` and ``sampler.directions``, the
    sampler's validity mask not applied.  ``center`` defaults to ``tree.center``, which a loaded
    tree does not have."""
    tree._check_volume(min_transmittance, "leaf_weights_over")
    if center is None:
        center = tree.center
    if center is None:
        raise ValueError("leaf_weights_over: a loaded tree does not know the centre of its root "
                         "cube (the file has no place for it); pass center=")
    center = tuple(float(c) for c in center)
    if len(center) != 3:
        raise ValueError("leaf_weights_over: center has three components")
    sampler = dataset.sampler
    per = sampler.rays_per_camera
    if sampler.num_cameras < 1 or per < 1:
        raise ValueError("leaf_weights_over: the dataset has no rays (%d cameras of %d rays)"
                         % (sampler.num_cameras, per))
    shift = torch.tensor(center, dtype=torch.float32, device=sampler.starts.device)
    out = None
    for camera in range(sampler.num_cameras):
        rays = slice(camera * per, (camera + 1) * per)
        out = tree.leaf_weights(sampler.starts[rays] - shift, sampler.directions[rays], t_min,
                                min_transmittance, out)
    return out.cpu().numpy()


def fit_octree_adaptive(tree: OcTree, train_dataset, val_dataset=None, rounds: int = 1,
                        prune_below: float = PRUNE_BELOW, split_above=SPLIT_ABOVE,
                        max_depth=None, **fit_kwargs):
    """Fits a tree and refines its structure in turns (K21); -> ``(tree, logs, reports)``.

    The fit is ``fit_octree`` or, for a tree with ``sh_degree``, ``fit_octree_sh``, called with
    ``fit_kwargs`` as they are (``num_steps`` is the length of EVERY fit).  A round is: fit,
    ``leaf_weights_over`` the training rays (with the fit's ``center``, ``t_min`` and
    ``min_transmittance``), ``refine_actions(weights, leaf_depths, prune_below, split_above,
    max_depth)``, ``OcTree.refine``; a last fit closes, so ``rounds`` rounds are ``rounds + 1``
    fits.  Every fit starts its Adam moments and its step count at zero and its seeded shuffle
    anew: the optimiser's state belongs to the leaves of one structure and is not carried across a
    refine.  ``prune_below`` / ``split_above`` default to 1e-2 / 1e-1, starting values that are
    UNTUNED; ``max_depth`` as in ``refine_actions``.

    ``logs`` is the list of the fits' logs in order, ``reports`` one ``RefineReport`` per round.
    ``rounds=0`` is one call of the plain fit: its tree and its log unchanged (``logs`` IS that log,
    not a list around it) and no reports.  A round whose action would leave no leaf raises, as
    ``refine`` does."""
    rounds = int(rounds)
    if rounds < 0:
        raise ValueError("fit_octree_adaptive: rounds >= 0, got %d" % rounds)
    if not isinstance(tree, OcTree):
        raise ValueError("fit_octree_adaptive: tree is an OcTree")
    fit = fit_octree if tree.sh_degree is None else fit_octree_sh
    if rounds == 0:
        tree, log = fit(tree, train_dataset, val_dataset, **fit_kwargs)
        return tree, log, []
    refine_actions(np.zeros(0), np.zeros(0, np.int32), prune_below, split_above, max_depth)
    center = fit_kwargs.get("center")
    center = tree.center if center is None else center
    verbose = fit_kwargs.get("verbose", True)
    logs, reports = [], []
    for number in range(rounds):
        tree, log = fit(tree, train_dataset, val_dataset, **fit_kwargs)
        logs.append(log)
        weights = leaf_weights_over(tree, train_dataset, center, fit_kwargs.get("t_min", 0.0),
                                    fit_kwargs.get("min_transmittance", 0.0))
        report, tree = refine_once(tree, weights, number, prune_below, split_above, max_depth)
        reports.append(report)
        if verbose:
            print(format_refine_report(report))
    tree, log = fit(tree, train_dataset, val_dataset, **fit_kwargs)
    logs.append(log)
    return tree, logs, reports


def refine_once(tree, weights, number, prune_below, split_above, max_depth):
    """One ``refine_actions`` + ``OcTree.refine`` on measured ``weights`` (``leaf_weights_over``) ->
    ``(RefineReport, the new tree)``; ``number`` is the report's round.  What a round of
    ``fit_octree_adaptive`` does between two fits, and all of scripts/refine_octree.py."""
    action = refine_actions(weights, tree.leaf_depths(), prune_below, split_above, max_depth)
    new, _ = tree.refine(action)
    quantiles = tuple(float(q) for q in np.quantile(weights.astype(np.float64),
                                                    [0.0, 0.25, 0.5, 0.75, 1.0]))
    report = RefineReport(number, tree.num_leaves, int((action == ops.OCTREE_DROP).sum()),
                          int((action == ops.OCTREE_SPLIT).sum()), new.num_leaves, tree.depth,
                          new.depth, quantiles)
    return report, new


def format_refine_report(report: RefineReport) -> str:
    """One line for a ``RefineReport``, as ``fit_octree_adaptive`` and scripts/refine_octree.py print it."""
    return ("refine {}: leaves {} -> {} (dropped {}, split {}), depth {} -> {}, weight quantiles "
            "min/25/50/75/max {}".format(report.round, report.leaves_before, report.leaves_after,
                                         report.dropped, report.split, report.depth_before,
                                         report.depth_after,
                                         " ".join("%.3g" % q for q in report.weight_quantiles)))

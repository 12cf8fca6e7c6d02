"""Opt-in empty-space skipping for rendering.

The reference renders every sample of every ray; its only spatial acceleration structure is a
CPU octree used by the lecture visualisations (octree.py:418-501, voxelize_model.py:65-88 builds
one from depth maps).  Here an occupancy grid is built on the GPU from the density model itself
and ``Raycaster.render`` (inference only) runs the fused MLP on the samples that fall into
occupied cells.  Skipped samples get sigma = softplus(-100) = 0, so compositing is unchanged.
This is new behaviour: parity with the full render is PSNR-level (see tests), never used for
training, and off unless ``Raycaster.occupancy`` is set.
"""

from typing import Optional

import numpy as np
import torch

from . import ops


class OccupancyGrid:
    """resolution^3 bits over the sampler's bounding box."""

    def __init__(self, bits: torch.Tensor, box_min, box_size, resolution: int):
        self.bits = bits
        self.box_min = [float(v) for v in box_min]
        self.box_size = [float(v) for v in box_size]
        self.resolution = int(resolution)

    @staticmethod
    def box_of(bounds: np.ndarray):
        """Axis-aligned box of a ``bounds`` transform (ray_sampler.py:101-104: the unit cube
        [-0.5, 0.5]^3 through the 4x4 matrix)."""
        corners = np.array([[x, y, z, 1.0] for x in (-0.5, 0.5) for y in (-0.5, 0.5)
                            for z in (-0.5, 0.5)], dtype=np.float64)
        world = (np.asarray(bounds, dtype=np.float64) @ corners.T).T[:, :3]
        lo, hi = world.min(axis=0), world.max(axis=0)
        return lo, hi - lo

    @staticmethod
    def cell_centres(bounds: np.ndarray, resolution: int, device) -> torch.Tensor:
        """(G^3,3) world positions of the cell centres, x fastest (the bit order)."""
        lo, size = OccupancyGrid.box_of(bounds)
        g = int(resolution)
        axis = [torch.arange(g, dtype=torch.float32, device=device).add_(0.5).mul_(float(size[d]) / g)
                .add_(float(lo[d])) for d in range(3)]
        zz, yy, xx = torch.meshgrid(axis[2], axis[1], axis[0], indexing="ij")
        return torch.stack([xx, yy, zz], dim=-1).reshape(-1, 3).contiguous()

    @classmethod
    def from_logits(cls, logits: torch.Tensor, bounds: np.ndarray, resolution: int,
                    sigma_threshold: float = 0.01, dilate: bool = True) -> "OccupancyGrid":
        """Grid from precomputed (G^3,4) raw outputs at ``cell_centres`` (any density source:
        a voxelised model, an analytic scene)."""
        lo, size = cls.box_of(bounds)
        bits = ops.occupancy_build(logits.contiguous(), int(resolution), float(sigma_threshold),
                                   bool(dilate))
        return cls(bits, lo, size, int(resolution))

    @classmethod
    def from_model(cls, model, bounds: np.ndarray, resolution: int = 128,
                   sigma_threshold: float = 0.01, dilate: bool = True,
                   batch_size: int = 1 << 21) -> "OccupancyGrid":
        """Evaluates the model's density at the cell centres (view direction +z for models
        that take one: sigma does not depend on it in nerf_model.py:118-119)."""
        device = next(model.parameters()).device
        lo, size = cls.box_of(bounds)
        g = int(resolution)
        axis = [torch.arange(g, dtype=torch.float32, device=device).add_(0.5).mul_(float(size[d]) / g)
                .add_(float(lo[d])) for d in range(3)]
        zz, yy, xx = torch.meshgrid(axis[2], axis[1], axis[0], indexing="ij")   # x fastest
        centres = torch.stack([xx, yy, zz], dim=-1).reshape(-1, 3).contiguous()
        logits = torch.empty((centres.shape[0], 4), dtype=torch.float32, device=device)
        was_training = model.training
        model.eval()
        with torch.no_grad():
            for start in range(0, centres.shape[0], batch_size):
                chunk = centres[start:start + batch_size]
                if getattr(model, "use_view", False):
                    view = torch.zeros_like(chunk)
                    view[:, 2] = 1.0
                    logits[start:start + batch_size] = model(chunk, view)
                else:
                    logits[start:start + batch_size] = model(chunk)
        model.train(was_training)
        bits = ops.occupancy_build(logits, g, float(sigma_threshold), bool(dilate))
        return cls(bits, lo, size, g)

    @classmethod
    def from_octree(cls, tree, bounds: np.ndarray, resolution: int = 128, center=None,
                    sigma_threshold: Optional[float] = None, dilate: int = 1,
                    out: Optional["OccupancyGrid"] = None) -> "OccupancyGrid":
        """Grid from an ``OcTree``'s leaves (K25): their boxes rasterised into the bits, no model
        and no cell-centre sampling involved, so a leaf smaller than a cell still marks its cell.

        ``center`` is the root cube's centre in the frame of ``bounds`` (default ``tree.center``,
        which a loaded tree does not have).  A leaf marks every cell that meets its half-open box
        in grid coordinates; every point the lookup of ``compact`` / the fused render places in
        ``[f(lo), f(hi))`` of a marking leaf is reported occupied (``ffn_occupancy_from_octree`` in
        include/ffn_hip.h states the rule).  The points left out lie within rounding of a + face:
        ``dilate`` (n passes of the 26-neighbourhood, default 1) is the slack for those and for
        structure the tree itself missed.  With ``sigma_threshold`` a leaf whose density is
        ``<= sigma_threshold`` marks nothing (a NaN density marks); plain ``[r, g, b, sigma]`` and
        SH trees alike.  A tree without a density column (the 3-channel shells of
        ``voxelize_model.py``) marks with every leaf and refuses a threshold.  ``out``: an
        ``OccupancyGrid`` over the same box and resolution to fold into (several trees, or leaf
        subsets, give the bits of one call); it is returned."""
        who = "OccupancyGrid.from_octree"
        center = tree.center if center is None else center
        if center is None:
            raise ValueError("%s: a loaded tree does not know its root cube's centre; pass "
                             "center=(x, y, z)" % who)
        center = tuple(float(np.float32(c)) for c in center)
        if len(center) != 3:
            raise ValueError("%s: center has three components" % who)
        lo, size = cls.box_of(bounds)
        g = int(resolution)
        data = tree.leaf_data()
        has_density = data is not None and np.ndim(data) == 2 and np.shape(data)[1] >= 4
        if sigma_threshold is not None and not has_density:
            raise ValueError("%s: sigma_threshold needs a density, and this tree's leaf_data %s "
                             "holds none" % (who, None if data is None else np.shape(data)))
        if out is not None:
            same = (isinstance(out, OccupancyGrid) and out.resolution == g
                    and np.array_equal(np.float32(out.box_min), np.float32(lo))
                    and np.array_equal(np.float32(out.box_size), np.float32(size)))
            if not same:
                raise ValueError("%s: out must be an OccupancyGrid over the same box and "
                                 "resolution (%s + %s at %d)" % (who, list(lo), list(size), g))
        # refuse bad arguments before any device is needed
        ops.occupancy_from_octree_check(torch.from_numpy(tree._leaf_index), tree.scale, center, lo,
                                        size, g, dilate=dilate,
                                        out=None if out is None else out.bits)
        if sigma_threshold is not None and np.isnan(float(sigma_threshold)):
            raise ValueError("%s: sigma_threshold is NaN" % who)
        rows, stride, offset = None, 4, 3
        if sigma_threshold is None:
            pass                                  # nothing of the rows is read
        elif tree.sh_degree is not None:
            rows, offset = tree._sh_rows_on_device(), 0
            stride = int(rows.shape[1])
        else:
            rows = tree._colors_on_device()
            stride = int(rows.shape[1])
        bits = ops.occupancy_from_octree(tree._on_device("leaf_index"), tree.scale, center, lo, size,
                                         g, rows, stride, offset, sigma_threshold, dilate,
                                         None if out is None else out.bits)
        if out is not None:
            return out
        return cls(bits, lo, size, g)

    @classmethod
    def from_silhouettes(cls, dataset, bounds: Optional[np.ndarray] = None, resolution: int = 128,
                         depth: int = 8, dilate: int = 1, **carve_kwargs) -> "OccupancyGrid":
        """Grid from the training images alone: ``OcTree.build_from_silhouettes`` (K23) carves the
        visual hull, ``from_octree`` rasterises it, no density threshold.  Empty-space skipping
        from step 0 of a training run then needs nothing but the dataset.

        ``bounds`` defaults to ``dataset.sampler.bounds``; the root cube is the box's centre +-
        half its longest side.  ``carve_kwargs`` go to ``build_from_silhouettes``
        (``alpha_threshold``, ``dilate``, ``max_misses``, ``min_views``, ...).

        What a hull is and is not.  It is the intersection of the silhouettes' cones: in the limit
        of many views it is conservative, it contains the object.  Concavities that no silhouette
        shows stay filled, which is harmless for skipping: those cells are evaluated and learn
        density 0.  But the default carve (``footprint="point"``) samples each cell at its centre
        only, and can lose structure thinner than a cell or than a pixel's footprint, which is NOT
        harmless: density in a cell the grid leaves empty is never trained.  ``dilate`` here (grid
        cells) and ``dilate`` / ``max_misses`` of the carve (pixels, cameras) are the slack.
        ``footprint="box"`` (K27, forwarded like every carve argument) removes that loss instead
        of padding it: a cell is carved only when a camera sees its whole projected footprint on
        the background, so every cell holding a point that no camera sees on the background is
        kept, at the price of a fatter hull; its grid holds every bit of the ``"point"`` grid."""
        from .octree import OcTree
        who = "OccupancyGrid.from_silhouettes"
        if bounds is None:
            sampler = getattr(dataset, "sampler", None)
            bounds = getattr(sampler, "bounds", None)
            if bounds is None:
                raise ValueError("%s: the dataset has no sampler.bounds; pass bounds" % who)
        for taken in ("center", "scale"):
            if taken in carve_kwargs:
                raise ValueError("%s: %s comes from bounds (the box's centre, half its longest "
                                 "side); it cannot be passed" % (who, taken))
        lo, size = cls.box_of(bounds)
        center = tuple(float(v) for v in lo + 0.5 * size)
        scale = 0.5 * float(size.max())
        tree = OcTree.build_from_silhouettes(dataset, depth, center, scale, **carve_kwargs)
        return cls.from_octree(tree, bounds, resolution, dilate=dilate)

    def fraction_occupied(self) -> float:
        """Share of cells marked occupied (diagnostic; one sync)."""
        cells = self.resolution ** 3
        words = self.bits.to(torch.int64) & 0xffffffff
        count = 0
        for shift in range(32):
            count += int(((words >> shift) & 1).sum().item())
        return count / cells

    def compact(self, positions: torch.Tensor, views: Optional[torch.Tensor]):
        return ops.occupancy_compact(positions, views, self.box_min, self.box_size,
                                     self.resolution, self.bits)

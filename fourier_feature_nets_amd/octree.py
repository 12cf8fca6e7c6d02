"""Sparse octree over a point cloud (the reference's ``OcTree``, octree.py:584-927), built and
queried by the K12 kernels of ``csrc/octree.hip`` and walked by K13 (``csrc/octree_walk.hip``).

Node ids, the ``.npz`` keys (``node_index``, ``leaf_index``, ``scale``, ``leaf_data``) and the
public signatures are the reference's, so files and calling code go both ways.  What differs:

* ``build_from_samples`` does not shift the caller's array in place (octree.py:760 does); the
  root cube's centre is used for the build and, like the reference, not stored: ``query`` takes
  positions relative to that centre.
* a tree whose only leaf is the root reports that leaf with the real ``scale`` (the reference
  substitutes a stand-in leaf of scale 1, octree.py:864-866, and its ``query`` fails on such a
  tree); ``query`` answers 0 inside the cube.
* inputs the reference fails on raise ``ValueError``: no leaf at all (``depth == 1`` with fewer
  than ``min_leaf_size`` points), an empty cloud, a depth the path codes cannot hold.
* node centres are always the f32 chain ``c +- scale / 2^k`` of a freshly built reference tree.
  (A tree the reference has *loaded* carries a Python-float scale and descends in f64; the two
  can differ for a position within an f32 rounding of a splitting plane.)
* ``intersect`` and ``build_from_mesh`` are not part of this path.  ``walk`` is the GPU
  counterpart of ``intersect`` (same arguments, same ``Path`` layout); against the reference's
  ``_trace_ray_path`` (octree.py:418-482) it differs in three ways:

  - no nudge: the reference advances by ``t += 1e-5`` steps and records the nudged ``t``, so
    its stops lie one or more such steps above the plane crossings that ``walk`` records, and
    it can step over a region whose chord is a few nudges long.  ``walk`` moves from region to
    region on integer cell coordinates and records the crossing itself.
  - zero direction components: the reference replaces them by 1e-8 (octree.py:728).  Here such a
    component constrains nothing when the start lies inside that slab of the root cube, and
    the ray misses otherwise.
  - misses: every leaf is -1 and the ``t_stops`` row is not meaningful (the reference fills it
    with the far crossing of a cube the ray never enters).  NaN rays and an all-zero direction
    are misses.

* ``spans`` and ``center`` have no counterpart in the reference.
* ``first_hit`` / ``render`` / ``render_image`` (K14) have none either: the reference looks at a
  voxelized model through scenepic (voxelize_model.py:90-110).  The leaves of such a tree are opaque
  surface cells with one colour each, so the render is the first leaf a ray meets.  The file format
  has no place for the root cube's centre; a caller that loads a tree passes it (``center=``).
* ``bake`` / ``render_volume`` / ``render_image(mode="volume")`` (K15) have none either.  ``bake``
  evaluates a trained model at the leaf centres and stores its own colour and density
  (``[sigmoid(rgb), softplus(sigma)]``, as ``Raycaster.render`` activates them) in every leaf;
  ``render_volume`` composites them front to back along the ray's whole chord through the tree, so
  soft edges, thin structure and the transmittance left for the background survive.  A leaf of
  ``bake`` holds one colour: the view dependence of a model with ``use_view`` is baked for one fixed
  view direction.  ``bake_sh`` keeps it.
* ``bake_sh`` / ``sh_degree`` (K18) have none either.  A leaf of an SH tree holds ``B = (degree +
  1)^2`` spherical-harmonic coefficients per colour channel, in logit space, and a density:
  ``leaf_data`` is ``(L, 3 B + 1)``, ``[k_r0 .. k_r(B-1), k_g0 .., k_b0 .., sigma]``, and the colour a
  ray sees is ``sigmoid(sum_b k_cb Y_b(u))`` for its unit direction ``u`` (``sh_basis``).
  ``bake_sh`` projects a model onto the basis from ``num_views`` directions on a Fibonacci sphere;
  ``render_volume`` of a tree whose ``sh_degree`` is set evaluates the basis once per ray.  The
  degree travels in the file as one more key, ``sh_degree``, that the reference's ``load`` ignores;
  it is never inferred from the channel count.  Fitting SH leaves (K17 for them) is not built.
* ``build_from_model`` (K16) has none either: the reference can only voxelize the depth renders
  of a model (voxelize_model.py), a one-cell shell that is nearly transparent once baked.
  ``build_from_model`` evaluates the model at the centre of every finest cell, chunk by chunk in
  path-code order, keeps the cells whose opacity along one side exceeds ``alpha_threshold``, stores
  what ``bake`` would store, and can merge siblings that agree.  One sample per cell: structure
  thinner than a finest cell can be missed.  Measured on one MI355X with the opaque-ball voxel
  model (profiles/r14_octree_density_microbench.json), depth 8 / 10: 100 408 / 6 270 096 leaves,
  the build 4.0 / 176 ms wall (model 0.20 / 3.0 ms, K16a + K16b 0.51 / 11.5 ms on the device);
  against the model's render, where its alpha is >= 0.99, the tree reaches 37.0 / 50.9 dB (the
  baked shell tree 8.0 / 6.2 dB).  Over all pixels both stay near 6 dB: 99 % of that error lies
  where the model's alpha is < 0.01, where ``Raycaster.render`` adds the colour of its last
  sample (width 1e10, opacity 1) and an octree frame shows the background.  Kernel times under
  rocprofv3 and ``--precision bf16x6`` are unmeasured.

* fitting lives in ``octree_fit.py`` (K17): ``OctreeField`` makes the leaf values of a baked tree a
  parameter whose forward is ``render_volume`` bit for bit and whose backward is the gradient walk
  plus deterministic per-leaf sums; ``fit_octree`` optimises them against a dataset's images.  A
  fit keeps the structure of the tree; ``leaf_weights`` / ``refine`` (K21) change it between fits.
  No counterpart in the reference.

* ``leaf_weights`` / ``refine`` / ``refine_actions`` (K21) have none either (the reference's ``prune``,
  kept as it is, merges the deepest level into its parents).  ``leaf_weights`` measures per leaf the
  largest compositing weight ``w = T a`` any ray of a set gives it, on ``render_volume``'s own walk
  (an integer maximum over f32 bit patterns: the same bits for the same rays in any order, in one
  call or many).  ``refine`` rebuilds the tree from one decision per leaf -- drop, keep, split into
  eight children that inherit the leaf's row bit for bit -- and says where every new leaf came
  from; ``refine_actions`` is the threshold policy between the two.  Splitting changes no render
  beyond rounding: ``exp(-s L1) exp(-s L2) = exp(-s (L1 + L2))``.  ``octree_fit.fit_octree_adaptive``
  alternates fitting and refining.

* ``neighbors`` / ``total_variation`` (K20) have none either: the face adjacency of the sparse tree
  (per leaf and direction the leaf of equal size or coarser on the other side; finer neighbours hold
  the adjacency from their side) and the Charbonnier total-variation energy of ``leaf_data`` over
  every pair of touching leaves, the prior that ``fit_octree`` / ``fit_octree_sh`` switch on with
  ``tv_weight``.  Every face counts the same: no weight for its area or the centres' distance.

* ``build_from_triangles`` (K22) is the reference's ``build_from_mesh`` from the point where the
  file has been read: it takes the arrays of a textured mesh, draws the surface samples on the GPU
  (``csrc/mesh.hip``: the reference's Basu-Owen points, barycentric interpolation and bilinear
  texture lookup, operation by operation) and hands the cloud to ``build_from_samples`` without
  a visit to the host.  The per-triangle counts come from a seeded multinomial (``mesh.py``), so
  a seed names a tree; the reference draws them unseeded.  ``build_from_mesh(path)`` itself stays
  a stub (trimesh is not a dependency); ``mesh.load_obj`` reads an OBJ and
  ``scripts/mesh_to_octree.py`` is the path-taking entry.

* ``build_from_silhouettes`` (K23, ``csrc/carve.hip``) has none either: nothing in the reference
  gets a tree from a dataset alone.  It is the grid loop of ``build_from_model`` with the model
  replaced by a projection: the centre of every finest cell goes into every camera
  (``cameras.projection_matrices``), a cell that lands on the background of a silhouette is carved
  away, and a survivor starts with the mean colour of the pixels it lands on and one density for
  all, so that ``images -> carve -> fit_octree[_adaptive] -> render_octree`` has no MLP in it.
  A point sample per cell, not a conservative test; the colour ignores occlusion; the hull of few
  views is fatter than the object.  Measured on one MI355X with the torus dataset of
  ``scripts/make_mesh_npz.py`` and all 120 cameras (profiles/r21_octree_carve_microbench.json),
  depth 8 / 10: 346 484 / 22 177 601 leaves, the build 7.4 / 525 ms wall, K23 with its scan and
  scatter 0.35 / 14.9 ms on the device; carved from 116 cameras at depth 8 and fitted for 300
  steps, 4 held-out cameras go from 24.4 to 27.3 dB (the mesh's own depth-8 tree: 28.0 dB).
  Kernel times under rocprofv3 are unmeasured.  ``footprint="box"`` (K27, ``csrc/carve_box.hip``)
  is the conservative test beside it: a camera refutes a cell only when the padded rectangle
  round the cell's projected centre and corners lies on the image and on the background, so thin
  structure survives, and the carve runs coarse to fine over the children of survivors.

* ``visible_moments`` / ``carve_photo`` / ``photo_actions`` (K28, a twelfth mode of
  ``csrc/octree_walk.hip``) have none either: voxel colouring on the sparse tree.  K24's walk with
  the squares of the seen bytes beside their sums gives every leaf a colour variance over the
  cameras that see it; ``photo_actions`` is the integer policy that drops a leaf whose cameras
  disagree; ``carve_photo`` sweeps -- moments, policy, ``refine`` -- until a sweep drops nothing.
  The one step that removes hull volume no silhouette refutes.  ``build_from_silhouettes(...,
  photo_threshold=T)`` runs it between the carve and the colouring; off by default.

* ``extract_mesh`` (K30, ``csrc/octree_mesh.hip``) has none either: the reference hands its leaf
  cubes to scenepic.  It is the way out of the tree: the boundary between solid and empty finest
  cells as a closed, consistently wound triangle mesh with per-vertex colours and normals, vertices
  on the block surface or moved onto the opacity threshold (surface nets).  ``mesh.save_obj`` writes
  it and ``scripts/octree_to_mesh.py`` is the path-taking entry.  Coplanar quads of a coarse leaf
  are not merged, there are no UVs, and an SH tree keeps its band-0 colour only.

The tree itself (three small arrays) lives on the host as numpy; ``load`` / ``state_dict`` /
``save`` / ``prune`` need no GPU.  Building, ``query``, ``walk``, ``spans``, ``first_hit``, ``render``,
``bake``, ``bake_sh``, ``build_from_model``, ``build_from_silhouettes``, ``render_volume``,
``leaf_centers``, ``leaf_depths``, ``neighbors``, ``total_variation``, ``leaf_weights``, ``refine``,
``visible_votes``, ``visible_moments``, ``carve_photo`` and ``extract_mesh`` run on the GPU and
raise without one;
``refine_actions`` and ``photo_actions`` are numpy.
"""

import os
from typing import Dict, NamedTuple, Optional, Tuple, Union

import numpy as np
import torch

from . import ops
from .utils import RenderResult


def _as_index(ids) -> np.ndarray:
    if isinstance(ids, (set, frozenset)):
        ids = sorted(ids)
    return np.unique(np.asarray(ids, dtype=np.int64).reshape(-1))


def _id_depths(ids: np.ndarray) -> np.ndarray:
    depth = np.zeros(ids.shape, np.int32)
    ids = ids.copy()
    while (ids > 0).any():
        live = ids > 0
        depth[live] += 1
        ids[live] = (ids[live] - 1) >> 3
    return depth


SH_Y0 = 0.28209479177387814
SH_Y1 = 0.4886025119029199
SH_Y2 = (1.0925484305920792, 0.31539156525252005, 0.5462742152960396)


def _sh_bases(degree) -> int:
    """(degree + 1)^2 for the degrees an SH tree can have."""
    if isinstance(degree, (bool, float)) or degree not in (1, 2):
        raise ValueError("OcTree: sh_degree is 1 or 2, got %r" % (degree,))
    return (int(degree) + 1) ** 2


def sh_view_directions(num_views: int) -> np.ndarray:
    """``num_views`` unit vectors on a Fibonacci sphere, float64 (V,3): ``z`` at the midpoints of V
    equal slices of [-1, 1], the azimuth advancing by the golden angle.  Deterministic."""
    num_views = int(num_views)
    if num_views < 1:
        raise ValueError("sh_view_directions: num_views >= 1, got %d" % num_views)
    i = np.arange(num_views, dtype=np.float64)
    z = 1.0 - (2.0 * i + 1.0) / num_views
    radius = np.sqrt(np.maximum(1.0 - z * z, 0.0))
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack([radius * np.cos(phi), radius * np.sin(phi), z], 1)


def sh_basis(directions, degree: int) -> np.ndarray:
    """The real SH basis of bands 0 .. degree at unit vectors ``directions`` (V,3) or (3,): float64
    (V, B), in the order and with the signs K18a uses (include/ffn_hip.h)."""
    bases = _sh_bases(degree)
    u = np.asarray(directions, np.float64).reshape(-1, 3)
    x, y, z = u[:, 0], u[:, 1], u[:, 2]
    out = np.empty((len(u), bases))
    out[:, 0] = SH_Y0
    out[:, 1] = -SH_Y1 * y
    out[:, 2] = SH_Y1 * z
    out[:, 3] = -SH_Y1 * x
    if degree == 2:
        out[:, 4] = SH_Y2[0] * x * y
        out[:, 5] = -SH_Y2[0] * y * z
        out[:, 6] = SH_Y2[1] * (2 * z * z - x * x - y * y)
        out[:, 7] = -SH_Y2[0] * x * z
        out[:, 8] = SH_Y2[2] * (x * x - y * y)
    return out


def refine_actions(weights, depths, prune_below: float = 1e-2, split_above=1e-1,
                   max_depth: Optional[int] = None) -> np.ndarray:
    """The threshold policy of K21, pure numpy: per leaf 0 (drop) where ``weight < prune_below``,
    2 (split) where ``weight >= split_above`` and ``depth < max_depth - 1``, 1 (keep) otherwise ->
    (L,) uint8 for ``OcTree.refine``.  ``weights`` (L,) from ``OcTree.leaf_weights``, ``depths`` (L,)
    from ``leaf_depths()`` (the root has depth 0).  ``max_depth`` is the depth the refined tree may
    reach, at most and by default ``ops.octree_max_depth()``: a leaf at level ``max_depth - 1`` is
    kept, not split.  ``split_above=None`` never splits; ``prune_below > split_above`` raises (a leaf
    could be asked to go and to split).  A NaN weight is kept.  The defaults 1e-2 / 1e-1 are
    starting values and UNTUNED."""
    weights = np.asarray(weights, dtype=np.float64).reshape(-1)
    depths = np.asarray(depths).reshape(-1)
    if weights.shape != depths.shape:
        raise ValueError("refine_actions: weights %s and depths %s must have one entry per leaf"
                         % (weights.shape, depths.shape))
    prune_below = float(prune_below)
    limit = ops.octree_max_depth()       # a host function of the library: no GPU needed
    max_depth = limit if max_depth is None else int(max_depth)
    if max_depth < 1 or max_depth > limit:
        raise ValueError("refine_actions: max_depth %d is outside what the path codes hold "
                         "(1 .. %d)" % (max_depth, limit))
    if prune_below != prune_below or (split_above is not None and not
                                      prune_below <= float(split_above)):       # NaN fails too
        raise ValueError("refine_actions: prune_below %r must not exceed split_above %r"
                         % (prune_below, split_above))
    action = np.full(weights.shape, ops.OCTREE_KEEP, np.uint8)
    if split_above is not None:
        action[(weights >= float(split_above)) & (depths < max_depth - 1)] = ops.OCTREE_SPLIT
    action[weights < prune_below] = ops.OCTREE_DROP
    return action


def photo_actions(moments, threshold: float, min_views: int = 2) -> np.ndarray:
    """The photo-consistency policy of K28, pure numpy and integers only: per leaf 0 (drop) where
    at least ``min_views`` cameras see it and the pixels they see there disagree, 1 (keep)
    otherwise -> (L,) uint8 for ``OcTree.refine``.  ``moments`` (L,8) uint32 from
    ``OcTree.visible_moments``: ``[sum_r, sum_g, sum_b, n, sq_r, sq_g, sq_b, 0]``.  With
    ``Q = sq_r + sq_g + sq_b``, ``S = sum_r^2 + sum_g^2 + sum_b^2`` (int64) and
    ``limit = ceil(3 (255 threshold)^2)`` (float64, then an integer) a leaf is dropped iff
    ``n >= min_views`` and ``n Q - S > limit n^2``; equality keeps.  In words: the mean over the
    three channels of the per-channel variance of the seeing cameras' pixels exceeds
    ``threshold^2``, colours in [0, 1].  Every product stays below 2^50 for the 66 051 cameras a
    moments buffer holds.  Raises ``ValueError`` for a ``threshold`` outside [0, 1] (NaN too),
    ``min_views < 2``, moments of another shape or dtype, a count above 66 051, sums that no ``count``
    bytes can give and a nonzero eighth field."""
    threshold = float(threshold)
    if not 0.0 <= threshold <= 1.0:          # NaN fails too
        raise ValueError("photo_actions: threshold must lie in [0, 1], got %r" % threshold)
    if isinstance(min_views, bool) or int(min_views) != min_views or min_views < 2:
        raise ValueError("photo_actions: min_views must be an integer >= 2 (one camera has no "
                         "spread), got %r" % (min_views,))
    moments = np.asarray(moments)
    if moments.ndim != 2 or moments.shape[1] != 8 or moments.dtype != np.uint32:
        raise ValueError("photo_actions: moments must be (L, 8) uint32, got %s %s"
                         % (moments.dtype, moments.shape))
    if moments[:, 7].any():
        raise ValueError("photo_actions: the eighth field of moments must be 0 (a carry out of "
                         "sq_b: more than %d cameras in one buffer?)"
                         % ops.OCTREE_MOMENTS_MAX_CAMERAS)
    wide = moments.astype(np.int64)
    n = wide[:, 3]
    if n.max(initial=0) > ops.OCTREE_MOMENTS_MAX_CAMERAS:
        raise ValueError("photo_actions: a count of moments is %d; at most %d cameras fold into "
                         "one buffer" % (int(n.max()), ops.OCTREE_MOMENTS_MAX_CAMERAS))
    if (wide[:, :3] > 255 * n[:, None]).any() or (wide[:, 4:7] > 65025 * n[:, None]).any():
        raise ValueError("photo_actions: a sum of moments exceeds 255 count, or a sum of squares "
                         "255^2 count: not the moments of bytes")
    limit = int(np.ceil(3.0 * (255.0 * threshold) ** 2))
    spread = wide[:, 4:7].sum(1)
    left, squares, right = n * spread, (wide[:, :3] ** 2).sum(1), limit * n * n
    assert max(left.max(initial=0), squares.max(initial=0), right.max(initial=0)) < 1 << 50
    action = np.full(len(moments), ops.OCTREE_KEEP, np.uint8)
    action[(n >= int(min_views)) & (left - squares > right)] = ops.OCTREE_DROP
    return action


PhotoSweep = NamedTuple("PhotoSweep", [("leaves", int), ("seen", int), ("judged", int),
                                       ("dropped", int)])


class PhotoReport(list):
    """What ``OcTree.carve_photo`` did: one ``PhotoSweep(leaves, seen, judged, dropped)`` per sweep
    -- the leaves before it, those some camera saw (``count > 0``), those judged
    (``count >= min_views``) and those dropped -- and ``converged``: whether the loop ended on a
    sweep that dropped nothing (``False`` after ``max_sweeps`` sweeps that all dropped, and for
    ``max_sweeps = 0``)."""

    converged = False


Path = NamedTuple("Path", [("t_stops", np.ndarray), ("leaves", np.ndarray)])
Hit = NamedTuple("Hit", [("leaves", np.ndarray), ("t", np.ndarray), ("faces", np.ndarray)])
SurfaceMesh = NamedTuple("SurfaceMesh", [("vertices", np.ndarray), ("triangles", np.ndarray),
                                         ("colors", Optional[np.ndarray]),
                                         ("normals", np.ndarray), ("corners", np.ndarray),
                                         ("masks", np.ndarray)])


class OcTree:
    """Class representing an OcTree datastructure."""

    def __init__(self, scale: float, node_ids, leaf_ids, leaf_data: np.ndarray = None,
                 sh_degree: Optional[int] = None):
        """``node_ids`` / ``leaf_ids``: sets (as the reference takes) or arrays of node ids; the
        children of node i have the ids 8 i + 1 .. 8 i + 8.  ``sh_degree``: 1 or 2 when
        ``leaf_data`` (L, 3 (degree + 1)^2 + 1) holds SH coefficients (see ``bake_sh``)."""
        self._device = None
        self._point_leaf = None
        self._center = None
        self._update(node_ids, leaf_ids, scale)
        self._leaf_data = leaf_data
        self._sh_degree = None
        if sh_degree is not None:
            channels = 3 * _sh_bases(sh_degree) + 1
            if leaf_data is None or np.ndim(leaf_data) != 2 or np.shape(leaf_data)[1] != channels:
                raise ValueError("OcTree: sh_degree %d needs leaf_data of shape (num_leaves, %d), "
                                 "got %s" % (sh_degree, channels,
                                             None if leaf_data is None else np.shape(leaf_data)))
            self._sh_degree = int(sh_degree)

    # ------------------------------------------------------------------ host-side state
    def _update(self, node_ids, leaf_ids, scale: float):
        self._scale = float(np.float32(scale))
        self._leaf_index = _as_index(leaf_ids)
        if len(self._leaf_index) == 0:
            raise ValueError("OcTree: a tree needs at least one leaf")
        self._node_index = np.setdiff1d(_as_index(node_ids), self._leaf_index)
        self._cache = {}

    @property
    def _leaf_ids(self):
        return set(self._leaf_index.tolist())

    @property
    def _node_ids(self):
        return set(self._node_index.tolist())

    def __len__(self):
        """Counts all the nodes in the tree."""
        return len(self._node_index) + len(self._leaf_index)

    @property
    def num_leaves(self) -> int:
        """Counts the number of leaves in the tree."""
        return len(self._leaf_index)

    @property
    def scale(self) -> float:
        """Scale of the cube (side is 2 * scale)."""
        return self._scale

    @property
    def depth(self) -> int:
        """The maximum depth of the tree."""
        return int(_id_depths(self._leaf_index[-1:])[0]) + 1

    @property
    def point_leaf_ids(self) -> Optional[torch.Tensor]:
        """After ``build_from_samples``: per input point the id of the leaf it ended in, -1 for
        a dropped point (device tensor).  ``None`` for a loaded tree."""
        return self._point_leaf

    @property
    def center(self) -> Optional[Tuple[float, float, float]]:
        """After ``build_from_samples`` / ``build_from_model``: the root cube's centre in the frame
        of the build's positions (``query`` / ``walk`` take positions relative to it).  ``None`` for a loaded
        tree: like the reference, the file does not hold it."""
        return self._center

    @property
    def sh_degree(self) -> Optional[int]:
        """1 or 2 when the leaves hold spherical-harmonic coefficients (``bake_sh``): ``leaf_data``
        is ``[k_r0 .. k_r(B-1), k_g0 .., k_b0 .., sigma]`` with ``B = (sh_degree + 1)^2``.  ``None``
        otherwise; never inferred from the channel count."""
        return self._sh_degree

    def leaf_data(self) -> np.ndarray:
        """The data stored in each leaf."""
        return self._leaf_data

    @property
    def state_dict(self) -> Dict[str, np.ndarray]:
        """The state needed to reconstruct the OcTree."""
        state = {"node_index": self._node_index, "leaf_index": self._leaf_index,
                 "scale": np.float32(self._scale)}
        if self._leaf_data is not None:
            state["leaf_data"] = self._leaf_data
        if self._sh_degree is not None:
            state["sh_degree"] = np.int32(self._sh_degree)
        return state

    def save(self, path: str):
        """Saves the OcTree to the provided path."""
        np.savez(path, **self.state_dict)

    @staticmethod
    def load(path_or_data: Union[str, Dict[str, np.ndarray]]) -> "OcTree":
        """Loads an OcTree from a ``.npz`` path or a state dict (ours or the reference's).
        Returns ``None`` (with a message) when the file does not exist; no download."""
        if isinstance(path_or_data, str):
            path = path_or_data
            if not os.path.exists(path):
                path = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", "data",
                                                    path_or_data))
                if not os.path.exists(path):
                    print("Unable to find octree", path_or_data)
                    return None
            with np.load(path) as data:
                data = {key: data[key] for key in data.files}
        else:
            data = path_or_data
        leaf_data = np.asarray(data["leaf_data"]) if "leaf_data" in data else None
        sh_degree = int(data["sh_degree"]) if "sh_degree" in data else None
        return OcTree(float(data["scale"]), data["node_index"], data["leaf_index"], leaf_data,
                      sh_degree)

    def load_state(self, state_dict: Dict[str, np.ndarray]):
        """Loads the information from the state dictionary."""
        self._update(state_dict["node_index"], state_dict["leaf_index"],
                     float(state_dict["scale"]))

    def prune(self) -> "OcTree":
        """Prunes all leaves at the maximum depth: they merge into their parents, which become
        leaves holding the mean of the merged leaves' data (octree.py:629-665)."""
        depths = _id_depths(self._leaf_index)
        max_depth = self.depth - 1
        if max_depth == 0:
            raise ValueError("OcTree.prune: the root is the only leaf")
        deep = depths >= max_depth
        new_ids = np.where(deep, (self._leaf_index - 1) >> 3, self._leaf_index)
        leaf_ids, inverse = np.unique(new_ids, return_inverse=True)
        node_ids = np.setdiff1d(self._node_index, leaf_ids)
        leaf_data = None
        if self._leaf_data is not None:
            data = self._leaf_data
            sums = np.zeros((len(leaf_ids),) + data.shape[1:], data.dtype)
            np.add.at(sums, inverse, data)      # in leaf order, as the reference accumulates
            counts = np.bincount(inverse, minlength=len(leaf_ids))
            merged = np.isin(leaf_ids, new_ids[deep])
            means = sums / counts[:, None].astype(data.dtype)
            leaf_data = np.where(merged[:, None], means, sums).astype(data.dtype)
        # a mean of SH coefficient vectors is a coefficient vector
        return OcTree(self._scale, node_ids, leaf_ids, leaf_data,
                      self._sh_degree if leaf_data is not None else None)

    # ------------------------------------------------------------------ GPU side
    def _dev(self):
        return torch.device(self._device if self._device is not None else "cuda")

    def _on_device(self, name: str) -> torch.Tensor:
        dev = self._dev()
        key = (name, str(dev))
        if key not in self._cache:
            self._cache[key] = torch.from_numpy(getattr(self, "_" + name)).to(dev)
        return self._cache[key]

    def _geometry(self):
        if "geometry" not in self._cache:
            centers, depths = ops.octree_leaf_geometry(self._on_device("leaf_index"), self._scale)
            self._cache["geometry"] = (centers.cpu().numpy(), depths.cpu().numpy())
        return self._cache["geometry"]

    def _centers_on_device(self) -> torch.Tensor:
        """The array behind ``leaf_centers``, on the device (K24 reads it there)."""
        key = ("leaf_centers", str(self._dev()))
        if key not in self._cache:
            self._cache[key] = ops.octree_leaf_geometry(self._on_device("leaf_index"),
                                                        self._scale)[0]
        return self._cache[key]

    def leaf_centers(self) -> np.ndarray:
        """The Nx3 center coordinates of all leaves."""
        return self._geometry()[0]

    def leaf_depths(self) -> np.ndarray:
        """The N depths for all leaves."""
        return self._geometry()[1]

    def _neighbors_on_device(self) -> torch.Tensor:
        dev = self._dev()
        key = ("neighbors", str(dev))
        if key not in self._cache:
            self._cache[key] = ops.octree_neighbors(self._on_device("node_index"),
                                                    self._on_device("leaf_index"))
        return self._cache[key]

    def neighbors(self) -> np.ndarray:
        """(L,6) int64 (K20a): per leaf and direction ``-x, +x, -y, +y, -z, +z`` the number (its
        position in the sorted leaf ids) of the leaf of equal size or coarser across that face; -1
        at the cube's boundary, next to empty space, and where the other side is finer (the finer
        leaves hold that adjacency from their side).  Computed once and cached like the geometry."""
        if "neighbors_host" not in self._cache:
            self._cache["neighbors_host"] = \
                self._neighbors_on_device().cpu().numpy().astype(np.int64)
        return self._cache["neighbors_host"]

    def _tv_plan(self) -> "ops.OctreeTVPlan":
        """The device plan of K20b / K20c (edges, incidences sorted by leaf), made once per tree."""
        dev = self._dev()
        key = ("tv_plan", str(dev))
        if key not in self._cache:
            self._cache[key] = ops.octree_tv_plan(self._neighbors_on_device(),
                                                  self._on_device("leaf_index"))
        return self._cache[key]

    def _tv_rows(self) -> torch.Tensor:
        """``leaf_data`` as the (L, stride) rows K20b reads: ``[r, g, b, sigma]`` of a plain tree,
        the device layout of an SH tree."""
        if self._leaf_data is None:
            raise ValueError("OcTree.total_variation: the tree has no leaf_data (see OcTree.bake)")
        if self._sh_degree is not None:
            self._check_volume(0.0)
            return self._sh_rows_on_device()
        data = self._leaf_data
        if np.ndim(data) != 2 or np.shape(data)[1] < 4:
            raise ValueError("OcTree.total_variation: leaf_data must be (num_leaves, C >= 4) to "
                             "hold a colour and a density, got %s" % (np.shape(data),))
        rows = self._colors_on_device()
        return rows if rows.shape[1] == 4 else rows[:, :4].contiguous()

    def total_variation(self, weights=None, eps: float = 1e-2) -> float:
        """The total-variation energy of the tree's own ``leaf_data`` (K20b): the mean over the pairs
        of leaves that touch across a face (``neighbors``; every pair once) of ``sum_c w_c
        (sqrt(d_c^2 + eps^2) - eps)``, ``d`` the difference of the two leaves' values -- Charbonnier,
        smooth at 0 and linear for a jump.  Plain tree: ``weights = (rgb, sigma)``, default ``(1,
        1)``; SH tree: ``weights = (band0, higher_bands, sigma)``, default ``(1, 1, 1)``.  0 for a
        tree without touching leaves.  There is no geometric weight: a face counts the same whatever
        its area or the distance of the two centres."""
        eps = ops.octree_tv_check_eps(eps)
        if self._leaf_data is None:
            raise ValueError("OcTree.total_variation: the tree has no leaf_data (see OcTree.bake)")
        stride = 4 if self._sh_degree is None else \
            (ops.octree_sh_channels(self._sh_degree) + 3) // 4 * 4
        lam = ops.octree_tv_weights(weights, stride, self._sh_degree)
        rows = self._tv_rows()
        value, _ = ops.octree_tv(rows, self._tv_plan(), lam, eps)
        return float(value.item())

    def extract_mesh(self, alpha_threshold: float = 0.5, placement: str = "surface_nets",
                     center=None, solid=None, batch_size: int = 1 << 22) -> SurfaceMesh:
        """The tree's surface as a coloured triangle mesh (K30, ``csrc/octree_mesh.hip``): the
        boundary between solid and empty finest cells, closed (it closes at the cube's faces) and
        wound so that normals point from solid to empty.  No counterpart in the reference, which
        hands its leaf cubes to scenepic.

        With ``n = 2^(depth-1)`` finest cells per axis and ``side = 2 scale / n``, every finest cell
        has an opacity ``a``: inside a leaf with a density ``a = 1 - exp(-sigma side)`` (the FINEST
        side whatever the leaf's level, as in ``build_from_model``; column 3 of a plain tree with
        ``C >= 4``, the density of an SH tree; 0 for a negative or NaN density), 0 in empty space.
        A cell is solid when ``a > alpha_threshold``.  A tree whose ``leaf_data`` has exactly 3
        columns (a voxelized shell, a mesh-built colour tree) or none has ``a = 1`` in every leaf
        and the threshold 0.5 whatever was passed; so has a call with ``solid``, a bool (L,) array
        in sorted-leaf order that replaces the rule (``tree.leaf_weights(...) > w``, say): ``a`` is
        then 1 or 0.

        Vertices are the cell corners ``c = (i, j, k)`` that touch both a solid and an empty cell,
        ordered by ``(i (n+1) + j)(n+1) + k``; each boundary face of a cell is one quad of two
        triangles (a coarse leaf's face is ``k^2`` unit quads: coplanar quads are not merged).
        ``placement="corners"`` puts a vertex at ``center + (c - n/2) side``, the exact block
        surface; ``"surface_nets"`` moves it by up to half a cell to the mean of the threshold
        crossings on the twelve edges between its eight cells.  ``center`` defaults to the tree's
        own, or to zeros.  -> ``SurfaceMesh`` of numpy arrays: ``vertices`` (V,3) f32, ``triangles``
        (F,3) int32, ``colors`` (V,3) f32 -- the mean ``rgb`` of the solid cells round the vertex --
        or None for a tree without ``leaf_data``, ``normals`` (V,3) f32 (minus the normalised
        opacity gradient over the eight cells), ``corners`` (V,3) int32 and ``masks`` (V,) uint8
        (bit ``4 dx + 2 dy + dz`` set when cell ``c - 1 + (dx, dy, dz)`` is solid).  A tree with no
        solid leaf gives empty arrays.

        An SH tree is coloured with its band-0 colour ``sigmoid(k_c0 Y_00)``: the view dependence
        is dropped.  Candidates (the corners on the surfaces of solid leaves) are processed
        ``batch_size`` at a time, which bounds the memory by the chunk and the output; the result
        does not depend on it."""
        who = "OcTree.extract_mesh"
        try:
            threshold, surface_nets = ops.octree_mesh_check(alpha_threshold, placement)
        except ValueError as err:
            raise ValueError(str(err).replace("octree mesh", who)) from None
        if isinstance(batch_size, (bool, float)) or int(batch_size) < 1:
            raise ValueError("%s: batch_size >= 1, got %r" % (who, batch_size))
        num = self.num_leaves
        if solid is not None:
            is_tensor = torch.is_tensor(solid)
            kind = solid.dtype if is_tensor else np.asarray(solid).dtype
            if kind != (torch.bool if is_tensor else np.dtype(bool)):
                raise TypeError("%s: solid must be a bool array, got %s" % (who, kind))
            if tuple(solid.shape if is_tensor else np.shape(solid)) != (num,):
                raise ValueError("%s: solid must be (num_leaves,) = (%d,), got %s"
                                 % (who, num, tuple(np.shape(solid))))
        data = self._leaf_data
        has_density = False
        if data is not None:
            if np.ndim(data) != 2 or np.shape(data)[0] != num or np.shape(data)[1] < 3:
                raise ValueError("%s: leaf_data must be (num_leaves, 3) colours or (num_leaves, "
                                 "C >= 4) with a density, got %s" % (who, np.shape(data),))
            if self._sh_degree is not None:
                self._check_volume(0.0, who)
            has_density = np.shape(data)[1] >= 4
        if center is None:
            center = self._center if self._center is not None else (0.0, 0.0, 0.0)
        center = tuple(float(np.float32(c)) for c in center)
        if len(center) != 3 or not all(np.isfinite(center)):
            raise ValueError("%s: center has three finite components" % who)
        depth = self.depth
        cells = 1 << (depth - 1)
        side = float(np.float32(2.0) * np.float32(self._scale) / np.float32(cells))

        dev = self._dev()
        if depth > ops.octree_mesh_max_depth():
            raise ValueError("%s: a tree of depth %d is deeper than the corner keys hold (%d)"
                             % (who, depth, ops.octree_mesh_max_depth()))
        rows, sigma_offset, color = None, 0, None
        if data is not None:
            if self._sh_degree is not None:
                rows, color = self._sh_rows_on_device(), (1, _sh_bases(self._sh_degree), 1)
            else:
                rows, sigma_offset, color = self._colors_on_device(), 3, (0, 1, 0)
        if solid is not None:
            solid = (solid if torch.is_tensor(solid) else torch.from_numpy(
                np.ascontiguousarray(solid))).to(dev).to(torch.uint8).contiguous()
        if solid is not None or not has_density:
            threshold = 0.5
        node_index, leaf_index = self._on_device("node_index"), self._on_device("leaf_index")
        flags, alpha = ops.octree_mesh_solid(rows if has_density else None, sigma_offset, solid,
                                             num, side, threshold, dev)
        offsets, total, top_level = ops.octree_mesh_candidate_offsets(leaf_index, flags, depth)
        if top_level > depth - 1:          # cannot happen: depth is read off the deepest id
            raise ValueError("%s: a leaf at level %d in a tree of depth %d"
                             % (who, top_level, depth))
        step = min(int(batch_size), ops.octree_max_points())
        parts = [ops.octree_mesh_candidates(node_index, leaf_index, flags, offsets, first,
                                            min(step, total - first), depth)
                 for first in range(0, total, step)]
        if parts:
            keys, masks, samples = [torch.cat(p) for p in zip(*parts)]
        else:
            keys = torch.empty((0,), dtype=torch.int64, device=dev)
            masks = torch.empty((0,), dtype=torch.uint8, device=dev)
            samples = torch.empty((0, 8), dtype=torch.int32, device=dev)
        # the keys are unique: sorting them, and the payload with them, is integer plumbing
        keys, order = torch.sort(keys)
        masks, samples = masks[order].contiguous(), samples[order].contiguous()
        vertices, colors, normals, corners = ops.octree_mesh_vertices(
            keys, masks, samples, alpha, rows, color, depth, self._scale, center, threshold,
            surface_nets)
        triangles = ops.octree_mesh_faces(keys, masks, depth)
        return SurfaceMesh(vertices.cpu().numpy(), triangles.cpu().numpy(),
                           None if colors is None else colors.cpu().numpy(),
                           normals.cpu().numpy(), corners.cpu().numpy(), masks.cpu().numpy())

    def query(self, positions):
        """Index into the sorted leaf ids of the leaf containing each position, -1 outside the
        cube or in an empty region.  positions: (N,3) or (3,), numpy (-> numpy int64) or a
        device tensor (-> device tensor)."""
        assert positions.shape[-1] == 3
        assert len(positions.shape) <= 2
        as_numpy = not torch.is_tensor(positions)
        if as_numpy:
            positions = torch.from_numpy(np.ascontiguousarray(positions, dtype=np.float32))
            positions = positions.to(self._dev())
        elif self._device is None:
            self._device = positions.device
        positions = positions.reshape(-1, 3).to(torch.float32).contiguous()
        result = ops.octree_query(positions, self._scale, self._on_device("node_index"),
                                  self._on_device("leaf_index"))
        return result.cpu().numpy() if as_numpy else result

    def _rays(self, starts, directions):
        """The shape rules of the reference's ``intersect`` (octree.py:718-726); -> float32 (N,3)
        device tensors and whether the caller passed numpy."""
        assert starts.shape[-1] == 3
        assert directions.shape[-1] == 3
        assert len(starts.shape) <= 2
        assert len(directions.shape) <= 2
        assert len(starts.shape) == len(directions.shape)
        as_numpy = not torch.is_tensor(starts)
        if torch.is_tensor(directions) == as_numpy:
            raise TypeError("OcTree: starts and directions must both be numpy arrays or both be "
                            "tensors")
        if self.depth > ops.octree_max_depth():
            raise ValueError("OcTree: a tree of depth %d is deeper than the ray walk's cell "
                             "coordinates hold (%d)" % (self.depth, ops.octree_max_depth()))
        if as_numpy:
            dev = self._dev()
            starts = torch.from_numpy(np.ascontiguousarray(starts, dtype=np.float32)).to(dev)
            directions = torch.from_numpy(np.ascontiguousarray(directions,
                                                               dtype=np.float32)).to(dev)
        else:
            if self._device is None:
                self._device = starts.device
            directions = directions.to(starts.device)
        starts = starts.reshape(-1, 3).to(torch.float32).contiguous()
        directions = directions.reshape(-1, 3).to(torch.float32).contiguous()
        assert starts.shape == directions.shape
        return starts, directions, as_numpy

    def walk(self, starts, directions, max_length: int) -> Path:
        """The regions every ray crosses, in order: the GPU counterpart of the reference's
        ``intersect`` (octree.py:707-731), in its ``Path`` layout.

        starts, directions: (N,3) or (3,), relative to the root cube's centre; numpy (-> numpy)
        or device tensors (-> device tensors).  ``t_stops`` (N,max_length) float32: the t at
        which the ray enters its k-th region (a leaf or a maximal empty cell) along the whole
        chord through the cube; ``leaves`` (N,max_length) int64: the region's index into the
        sorted leaf ids, -1 for empty space.  At most ``max_length - 1`` stops are written; the
        rest hold the cube's exit t and -1.  A ray that misses the cube has every leaf -1."""
        starts, directions, as_numpy = self._rays(starts, directions)
        t_stops, leaves = ops.octree_walk(starts, directions, self._scale, self.depth,
                                          self._on_device("node_index"),
                                          self._on_device("leaf_index"), int(max_length))
        if as_numpy:
            return Path(t_stops.cpu().numpy(), leaves.cpu().numpy())
        return Path(t_stops, leaves)

    def spans(self, starts, directions, t_min: float = 0.0, pad: float = 1):
        """Per ray the span ``[t_in, t_out]`` that holds every leaf the ray crosses after
        ``t_min``, widened at both ends by ``pad`` sides of a finest cell (measured along the
        ray), and ``hit``: whether there is such a leaf.  Inputs as for ``walk``; -> (t_in, t_out
        float32, hit bool), each (N,)."""
        starts, directions, as_numpy = self._rays(starts, directions)
        t_in, t_out, hit = ops.octree_spans(starts, directions, self._scale, self.depth,
                                            self._on_device("node_index"),
                                            self._on_device("leaf_index"), float(t_min),
                                            float(pad))
        hit = hit != 0
        if as_numpy:
            return t_in.cpu().numpy(), t_out.cpu().numpy(), hit.cpu().numpy()
        return t_in, t_out, hit

    def first_hit(self, starts, directions, t_min: float = 0.0) -> Hit:
        """Per ray the first leaf that ends after ``t_min`` (K14; the walk stops there).  Inputs
        as for ``walk``.  -> ``Hit``: ``leaves`` (N,) int64 index into the sorted leaf ids, -1
        without a hit; ``t`` (N,) float32 ``max(entry t, t_min)``, 0 on a miss; ``faces`` (N,) int8,
        the face the ray enters the leaf through: ``2 * axis + (d[axis] > 0 ? 0 : 1)`` (0 / 2 / 4:
        outward normal -x / -y / -z, 1 / 3 / 5: +x / +y / +z), 6 when the entry lies before
        ``t_min`` (the ray starts inside the leaf), -1 on a miss."""
        starts, directions, as_numpy = self._rays(starts, directions)
        hit = ops.octree_first_hit(starts, directions, self._scale, self.depth,
                                   self._on_device("node_index"), self._on_device("leaf_index"),
                                   float(t_min))
        if as_numpy:
            return Hit(*[x.cpu().numpy() for x in hit])
        return Hit(*hit)

    def _check_colors(self):
        data = self._leaf_data
        if data is None:
            raise ValueError("OcTree.render: the tree has no leaf_data to show")
        if np.ndim(data) != 2 or np.shape(data)[1] < 3:
            raise ValueError("OcTree.render: leaf_data must be (num_leaves, C >= 3) to hold a "
                             "colour, got %s" % (np.shape(data),))

    def _check_volume(self, min_transmittance, who="OcTree.render_volume"):
        data = self._leaf_data
        if data is None:
            raise ValueError("%s: the tree has no leaf_data to composite (see OcTree.bake)" % who)
        if np.ndim(data) != 2 or np.shape(data)[1] < 4:
            raise ValueError("%s: leaf_data must be (num_leaves, C >= 4) to hold a colour and a "
                             "density, got %s (see OcTree.bake)" % (who, np.shape(data),))
        if not 0.0 <= float(min_transmittance) < 1.0:        # NaN fails too
            raise ValueError("%s: min_transmittance must lie in [0, 1), got %r"
                             % (who, min_transmittance,))
        if self._sh_degree is not None:
            channels = 3 * _sh_bases(self._sh_degree) + 1
            if np.shape(data)[1] != channels:
                raise ValueError("%s: sh_degree %d needs leaf_data of shape (num_leaves, %d), got "
                                 "%s" % (who, self._sh_degree, channels, np.shape(data)))

    def _sh_rows_on_device(self) -> torch.Tensor:
        """The SH ``leaf_data`` in the layout K18a reads (``ops.octree_sh_device_layout``: density
        first, rows padded to whole 16-byte loads) on the device, made once, cached like
        ``leaf_data_f32``."""
        dev = self._dev()
        key = ("leaf_data_sh", str(dev))
        if key not in self._cache:
            self._cache[key] = torch.from_numpy(
                ops.octree_sh_device_layout(self._leaf_data, self._sh_degree)).to(dev)
        return self._cache[key]

    def _colors_on_device(self) -> torch.Tensor:
        """``leaf_data`` as float32 on the device, cast once (a tree the reference saved, or a
        pruned one, holds float64); ``_update`` drops it with the rest of the cache."""
        self._check_colors()
        data = self._leaf_data
        dev = self._dev()
        key = ("leaf_data_f32", str(dev))
        if key not in self._cache:
            self._cache[key] = torch.from_numpy(
                np.ascontiguousarray(data, dtype=np.float32)).to(dev)
        return self._cache[key]

    def render(self, starts, directions, t_min: float = 0.0, background=(0, 0, 0),
               shading: str = "flat") -> RenderResult:
        """The tree as ``first_hit`` sees it, shaded in the same launch.  -> ``RenderResult``:
        ``color`` (N,3) the hit leaf's first three ``leaf_data`` channels (``shading="faces"``:
        times one factor per axis pair of the entry face, cube shading) or ``background``;
        ``alpha`` (N,) 1 on a hit, 0 otherwise; ``depth`` (N,) the hit's t.  Inputs as for
        ``walk``; numpy in gives numpy out."""
        if shading not in ops.OCTREE_SHADING:
            raise ValueError("OcTree.render: shading is 'flat' or 'faces', got %r" % (shading,))
        self._check_colors()                     # before any device is needed
        starts, directions, as_numpy = self._rays(starts, directions)
        out = RenderResult(*ops.octree_render(
            starts, directions, self._scale, self.depth, self._on_device("node_index"),
            self._on_device("leaf_index"), self._colors_on_device(), float(t_min), background,
            shading))
        return out.numpy() if as_numpy else out

    def render_volume(self, starts, directions, t_min: float = 0.0, background=(0, 0, 0),
                      min_transmittance: float = 0.0) -> RenderResult:
        """A baked tree (``bake``) composited front to back (K15).  ``leaf_data`` holds
        ``[r, g, b, sigma]`` per leaf, ``sigma`` per unit of world length.  Over the leaves a ray
        crosses after ``t_min``, in order: ``a = 1 - exp(-sigma * chord)``, ``w = T * a``,
        ``T *= 1 - a``.  -> ``RenderResult``: ``color`` (N,3) ``sum(w * rgb) + T * background``;
        ``alpha`` (N,) ``1 - T``; ``depth`` (N,) the ``max(entry t, t_min)`` of the leaf with the
        largest ``w`` (the first of equals), 0 when nothing is in the way.  The walk of a ray ends
        once ``T <= min_transmittance``.  Rescaling ``directions`` does not change the result.
        Inputs as for ``walk``; numpy in gives numpy out.

        A tree whose ``sh_degree`` is set (``bake_sh``) takes the K18a path: the same compositing,
        with the leaf colour ``sigmoid(sum_b k_cb Y_b(u))`` for the ray's unit direction ``u =
        direction / |direction|`` (not negated), so ``alpha`` and ``depth`` are those of a plain
        tree with the same densities, bit for bit.  Without ``sh_degree`` the first four channels
        are ``[r, g, b, sigma]`` whatever the channel count."""
        self._check_volume(min_transmittance)         # before any device is needed
        starts, directions, as_numpy = self._rays(starts, directions)
        if self._sh_degree is not None:
            out = RenderResult(*ops.octree_render_volume_sh(
                starts, directions, self._scale, self.depth, self._on_device("node_index"),
                self._on_device("leaf_index"), self._sh_rows_on_device(), self._sh_degree,
                float(t_min), background, float(min_transmittance)))
            return out.numpy() if as_numpy else out
        out = RenderResult(*ops.octree_render_volume(
            starts, directions, self._scale, self.depth, self._on_device("node_index"),
            self._on_device("leaf_index"), self._colors_on_device(), float(t_min), background,
            float(min_transmittance)))
        return out.numpy() if as_numpy else out

    def leaf_weights(self, starts, directions, t_min: float = 0.0, min_transmittance: float = 0.0,
                     out=None):
        """Per leaf the largest compositing weight ``w = T * a`` that any of the rays gives it
        (K21a), on the walk and with the operations of ``render_volume``: 0 for a leaf no ray takes,
        that lies behind the ``min_transmittance`` cut of every ray, or whose density is 0, negative
        or NaN.  Works on plain and SH trees alike (the weight does not depend on colour).  Inputs as
        for ``render_volume``; -> (L,) float32, numpy for numpy rays.  With ``out`` (a (L,) float32
        device tensor, as a call with device rays returns) the maxima fold into it: the same rays
        give the same bits in any order, in one call or many."""
        self._check_volume(min_transmittance, "OcTree.leaf_weights")   # before any device is needed
        starts, directions, as_numpy = self._rays(starts, directions)
        if self._sh_degree is not None:
            rows, offset = self._sh_rows_on_device(), 0
        else:
            rows, offset = self._colors_on_device(), 3
        weights = ops.octree_leaf_weights(
            starts, directions, self._scale, self.depth, self._on_device("node_index"),
            self._on_device("leaf_index"), rows, int(rows.shape[1]), offset, float(t_min),
            float(min_transmittance), out)
        return weights.cpu().numpy() if as_numpy else weights

    def distortion(self, starts, directions, t_min: float = 0.0, min_transmittance: float = 0.0):
        """Per ray the distortion of its compositing weights (K29a): with the taken leaves of
        ``render_volume`` in walk order, their weights ``w = T * a``, chord lengths ``L`` and chord
        midpoints ``m`` (both as world lengths along the ray),
        ``D = sum_ij w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 L_i`` -- the distortion loss of
        Mip-NeRF 360 for piecewise-constant weights, small for a ray whose weight sits in one short
        interval, large for one that spreads it along a chord.  -> (R,) float32, numpy for numpy
        rays; 0 for a ray that takes no leaf.  Works on plain and SH trees alike (colour does not
        enter), and the background's share of a ray takes no part.  Inputs as for ``render_volume``.

        Limits.  ``D`` treats a leaf's weight as uniform along its chord, so it depends on the
        partition: ``refine`` with splits changes it at second order.  It is measured in world
        lengths, not in units of the cube.  It sees the tree's own densities only.  As a prior
        (``fit_octree(dist_weight=...)``) it can eat thin true structure behind a strong surface,
        and ``dist_weight`` has no tuned default."""
        self._check_volume(min_transmittance, "OcTree.distortion")     # before any device is needed
        starts, directions, as_numpy = self._rays(starts, directions)
        rows, offset = self._density_rows("OcTree.distortion")
        out = ops.octree_distortion(
            starts, directions, self._scale, self.depth, self._on_device("node_index"),
            self._on_device("leaf_index"), rows, int(rows.shape[1]), offset, float(t_min),
            float(min_transmittance))
        return out.cpu().numpy() if as_numpy else out

    def _density_rows(self, who):
        """The device rows and the density's offset in them, for the walks that read the density
        alone (K21a, K24, K26)."""
        self._check_volume(0.0, who)
        if self._sh_degree is not None:
            return self._sh_rows_on_device(), 0
        return self._colors_on_device(), 3

    def focus_samples(self, starts, directions, near_far, ray_index, u, t_uniform=None,
                      center=None, min_mass: float = 1e-3, return_mass: bool = False):
        """Focus samples from the tree's own compositing weights (K26; the reference has no
        counterpart: its focus samples come from a coarse model probed at ``n_focus`` points per
        ray).  ``starts``, ``directions`` (N,3) and ``near_far`` (2,N) are a sampler's per-ray state
        in WORLD coordinates, float32 device tensors; ``ray_index`` (R,) int64 picks the batch;
        ``center`` is the root cube's centre (default: the tree's own, which a loaded tree does not
        have).  ``u`` (R, n_focus) in [0,1] is ASCENDING in every row.  Along ray r, over the
        leaves it crosses inside ``[near, far]``, the walk forms ``render_volume``'s weights
        ``w = T * a`` and their running sum, whose total is the ray's mass M; target ``u * M`` lands
        in the leaf where the sum passes it, linearly between the leaf's two crossings.
        ``t_uniform`` (R, n_uniform): the rays' ascending uniform samples, merged in.
        -> t (R, n_uniform + n_focus) float32, every row ascending: ``sort(cat(uniform, focus))``;
        with ``return_mass`` also M (R,).

        A ray with M < ``min_mass`` (or that misses the cube, or without near < far) gets the
        uniform fall-back ``near + u * (far - near)``.

        Limits.  The CDF is piecewise linear inside a leaf, and a leaf has ONE density: the samples
        are as fine as the tree.  Focus samples never land in empty regions -- where the tree has no
        leaf (or a leaf of density 0) only the uniform half of a sampler still looks.
        ``min_mass = 1e-3`` is an untuned starting value.  Works for plain and SH trees (only the
        density is read)."""
        who = "OcTree.focus_samples"
        data = self._leaf_data
        if data is None or np.ndim(data) != 2 or np.shape(data)[1] < 4:
            raise ValueError("%s: the tree has no density column (leaf_data must be (num_leaves, "
                             "C >= 4), [r, g, b, sigma] or SH rows; see OcTree.bake, "
                             "build_from_silhouettes)" % who)
        if not float(min_mass) >= 0.0:       # NaN fails too
            raise ValueError("%s: min_mass must be >= 0, got %r" % (who, min_mass))
        if self.depth > ops.octree_max_depth():
            raise ValueError("OcTree: a tree of depth %d is deeper than the ray walk's cell "
                             "coordinates hold (%d)" % (self.depth, ops.octree_max_depth()))
        center = self._visible_center(who, center)
        if self._device is None and torch.is_tensor(starts) and starts.is_cuda:
            self._device = starts.device
        rows, offset = self._density_rows(who)
        out = ops.octree_focus_sample(
            starts, directions, near_far, ray_index, center, self._scale, self.depth,
            self._on_device("node_index"), self._on_device("leaf_index"), rows,
            int(rows.shape[1]), offset, u, t_uniform, None, float(min_mass), bool(return_mass))
        return out

    @staticmethod
    def _visible_arguments(who, dataset, alpha_threshold):
        """What ``visible_votes`` checks of its dataset and ``alpha_threshold`` before any device is
        needed (``_check_volume`` has min_transmittance, the op the camera limit) -> images
        (C,H,W,4) uint8, cameras, alpha_u8."""
        alpha_threshold = float(alpha_threshold)
        if not 0.0 <= alpha_threshold <= 1.0:        # NaN fails too
            raise ValueError("%s: alpha_threshold must lie in [0, 1], got %r"
                             % (who, alpha_threshold))
        images = np.asarray(dataset.images)
        if images.ndim != 4 or images.shape[-1] != 4 or images.dtype != np.uint8:
            raise ValueError("%s: dataset.images must be (C,H,W,4) uint8 with an alpha channel, "
                             "got %s %s" % (who, images.dtype, images.shape))
        if getattr(dataset, "color_space", "RGB") != "RGB":
            raise ValueError("%s: dataset.color_space must be RGB, got %r"
                             % (who, dataset.color_space))
        cameras = list(dataset.cameras)
        if len(cameras) != len(images) or not cameras:
            raise ValueError("%s: dataset has %d cameras for %d images"
                             % (who, len(cameras), len(images)))
        return images, cameras, min(max(int(np.ceil(alpha_threshold * 255)), 1), 255)

    def _visible_votes_on_device(self, images, cameras, alpha_u8, center, min_transmittance):
        return self._visible_pairs_on_device(ops.octree_visible_votes, images, cameras, alpha_u8,
                                             center, min_transmittance)

    def _visible_moments_on_device(self, images, cameras, alpha_u8, center, min_transmittance):
        return self._visible_pairs_on_device(ops.octree_visible_moments, images, cameras,
                                             alpha_u8, center, min_transmittance)

    def _visible_pairs_on_device(self, op, images, cameras, alpha_u8, center, min_transmittance):
        from .cameras import eye_positions, projection_matrices
        dev = self._dev()
        if self._sh_degree is not None:
            rows, offset = self._sh_rows_on_device(), 0
        else:
            rows, offset = self._colors_on_device(), 3
        images_u8 = images if torch.is_tensor(images) else \
            torch.from_numpy(np.ascontiguousarray(images)).to(dev)
        proj = torch.from_numpy(projection_matrices(cameras, origin=center)).to(dev)
        eyes = torch.from_numpy(eye_positions(cameras, center)).to(dev)
        return op(
            self._centers_on_device(), self._scale, self.depth, self._on_device("node_index"),
            self._on_device("leaf_index"), rows, int(rows.shape[1]), offset, images_u8, proj, eyes,
            alpha_u8, float(min_transmittance))

    def _visible_center(self, who, center):
        center = self._center if center is None else center
        if center is None:
            raise ValueError("%s: a loaded tree does not know its root cube's centre; pass "
                             "center=(x, y, z)" % who)
        center = tuple(float(np.float32(c)) for c in center)
        if len(center) != 3:
            raise ValueError("%s: center has three components" % who)
        return center

    def visible_votes(self, dataset, center=None, alpha_threshold: float = 0.5,
                      min_transmittance: float = 0.3) -> np.ndarray:
        """Per leaf the pixels of the cameras that can see it (K24; no counterpart in the
        reference) -> (L,4) uint32 numpy ``[sum_r, sum_g, sum_b, count]``.  ``dataset`` gives
        ``images`` ((C,H,W,4) uint8 RGBA, colour space RGB) and ``cameras``; ``center`` is the root
        cube's centre (default: the tree's own, which a loaded tree does not have).  Camera c
        votes for leaf l when the leaf's centre projects, as ``build_from_silhouettes`` projects a
        cell, onto a pixel of image c whose own alpha is ``>= ceil(alpha_threshold * 255)``
        (clamped to 1 .. 255; no grown mask), and the ray from the camera's position to the centre
        reaches the leaf before its transmittance -- ``render_volume``'s, over the leaves in
        front, from the tree's own densities -- falls to ``min_transmittance`` or below.  Works on
        plain and SH trees alike (only the density is read).  Integer sums: the same bits in any
        order of the cameras."""
        who = "OcTree.visible_votes"
        self._check_volume(min_transmittance, who)           # before any device is needed
        images, cameras, alpha_u8 = OcTree._visible_arguments(who, dataset, alpha_threshold)
        center = self._visible_center(who, center)
        return self._visible_votes_on_device(images, cameras, alpha_u8, center,
                                             min_transmittance).cpu().numpy()

    def color_from_images(self, dataset, center=None, alpha_threshold: float = 0.5,
                          min_transmittance: float = 0.3) -> Tuple["OcTree", np.ndarray]:
        """A NEW tree whose leaves take the mean colour of the cameras that can see them (K24,
        ``visible_votes``) -> ``(tree, counts)``; ``counts`` (L,) uint32 numpy is the number of
        cameras that voted per leaf.  A leaf with ``count > 0`` gets ``sum / (float)(255 count)``,
        one f32 division per channel as ``build_from_silhouettes`` divides; a leaf no camera saw
        keeps its colour.  Structure, densities and any further channels, scale, centre and device
        carry over; this tree is not modified.  An SH tree is refused: its leaves hold
        coefficients, not a colour (``visible_votes`` works on it and returns the sums).

        The limits: one ray per (leaf, camera) pair, aimed at the leaf's centre, so a leaf whose
        centre is hidden counts as hidden however much of it shows.  Opacity is judged from the
        tree's own densities: a tree that is transparent hides nothing, and one whose cells are
        opaque where the object is not hides too much.  ``min_transmittance = 0.3`` is an untuned
        starting value: it lies between the 0.5 and the 0.25 that one and two whole cells of a
        fresh carve (``cell_opacity = 0.5``) leave, so rays along the lattice do not sit on the
        threshold."""
        who = "OcTree.color_from_images"
        if self._sh_degree is not None:
            raise ValueError("%s: the leaves of an SH tree hold coefficients, not a colour; "
                             "OcTree.visible_votes gives the cameras' sums for it" % who)
        self._check_volume(min_transmittance, who)           # before any device is needed
        images, cameras, alpha_u8 = OcTree._visible_arguments(who, dataset, alpha_threshold)
        center = self._visible_center(who, center)
        votes = self._visible_votes_on_device(images, cameras, alpha_u8, center,
                                              min_transmittance).cpu().numpy()
        data = np.array(self._leaf_data, dtype=np.float32, copy=True)
        data[:, :3] = OcTree._vote_colors(votes, data[:, :3])
        tree = OcTree(self._scale, self._node_index, self._leaf_index, data)
        tree._device = self._device
        tree._center = self._center
        return tree, votes[:, 3].copy()

    @staticmethod
    def _vote_colors(votes: np.ndarray, colors: np.ndarray) -> np.ndarray:
        """(L,3) float32: ``sum / (float)(255 count)`` where ``count > 0`` (both operands exact in
        f32, one division), ``colors`` elsewhere."""
        seen = votes[:, 3] > 0
        out = np.array(colors, dtype=np.float32, copy=True)
        denominator = (np.uint32(255) * votes[seen, 3]).astype(np.float32)
        out[seen] = votes[seen, :3].astype(np.float32) / denominator[:, None]
        return out

    def visible_moments(self, dataset, center=None, alpha_threshold: float = 0.5,
                        min_transmittance: float = 0.3) -> np.ndarray:
        """``visible_votes`` with the second moments (K28a; no counterpart in the reference) ->
        (L,8) uint32 numpy ``[sum_r, sum_g, sum_b, count, sq_r, sq_g, sq_b, 0]``: the same
        arguments and the same (leaf, camera) pairs, the first four fields are the votes bit for
        bit, and ``sq_c`` is the sum of the squares of the bytes the seeing cameras hold there, so
        that a leaf has a colour variance as well as a mean (``photo_actions``).  Works on plain
        and SH trees alike (only the density is read).  Integer sums: the same bits in any order
        of the cameras.  At most 66 051 cameras (``255^2 C < 2^32``)."""
        who = "OcTree.visible_moments"
        self._check_volume(min_transmittance, who)           # before any device is needed
        images, cameras, alpha_u8 = OcTree._visible_arguments(who, dataset, alpha_threshold)
        OcTree._check_moments_cameras(who, cameras)
        center = self._visible_center(who, center)
        return self._visible_moments_on_device(images, cameras, alpha_u8, center,
                                               min_transmittance).cpu().numpy()

    @staticmethod
    def _check_moments_cameras(who, cameras):
        if len(cameras) > ops.OCTREE_MOMENTS_MAX_CAMERAS:
            raise ValueError("%s: dataset has %d cameras; at most %d fold into one moments buffer "
                             "(255^2 * C must stay below 2^32)"
                             % (who, len(cameras), ops.OCTREE_MOMENTS_MAX_CAMERAS))

    def carve_photo(self, dataset, center=None, threshold: float = 0.1, min_views: int = 2,
                    max_sweeps: int = 16, alpha_threshold: float = 0.5,
                    min_transmittance: float = 0.3,
                    recolor: bool = False) -> Tuple["OcTree", "PhotoReport"]:
        """Carves by photo-consistency (K28; the classic voxel colouring / space carving, no
        counterpart in the reference): a NEW tree without the leaves whose seeing cameras disagree
        on their colour -> ``(tree, report)``, ``report`` a ``PhotoReport``.  Each sweep takes
        fresh ``visible_moments`` of the tree as it stands over all leaves and all cameras, then
        ``photo_actions(moments, threshold, min_views)``, then ``refine`` (drops only).  All
        decisions of a sweep come from one tree, so the result does not depend on the order of the
        leaves.  A drop can expose leaves behind it, which the next sweep judges; the loop stops
        after a sweep that drops nothing (``report.converged``) or after ``max_sweeps``.  A sweep
        that would drop every leaf raises ``ValueError`` (raise ``threshold``).  ``max_sweeps=0``
        returns a tree equal to this one bit for bit.  ``dataset``, ``center``,
        ``alpha_threshold`` and ``min_transmittance`` as for ``visible_votes``.

        ``recolor=True`` gives every leaf of the FINAL tree that some camera sees
        ``sum / (float)(255 count)`` as ``color_from_images`` does (the last sweep's moments when
        it dropped nothing, one more call otherwise); an SH tree is refused with it, for
        ``color_from_images``' reason, and accepted without.  Densities, the other channels,
        scale, centre, ``sh_degree`` and device carry over through ``refine``; this tree is not
        modified.

        The limits.  One ray per (leaf, camera) pair at the leaf's centre, to the nearest pixel:
        the colour a camera holds for a leaf is one sample, and a leaf whose centre is hidden
        counts as hidden.  Opacity is judged from the tree's own densities (``color_from_images``).
        A smooth or uniform texture cannot refute anything: phantom cells in front of a surface of
        one colour stay.  Specular or badly exposed views, and colour that changes within a cell's
        footprint, refute TRUE cells.  The guarantee of the box carve ("a cell containing a point
        no camera sees on the background is kept") is given up wherever the threshold fires.
        ``threshold = 0.1`` (the root of the mean channel variance, colours in [0, 1]) is an
        untuned starting value."""
        who = "OcTree.carve_photo"
        if recolor and self._sh_degree is not None:
            raise ValueError("%s: the leaves of an SH tree hold coefficients, not a colour; "
                             "recolor=False carves it, OcTree.visible_votes gives the cameras' "
                             "sums for it" % who)
        self._check_volume(min_transmittance, who)           # before any device is needed
        images, cameras, alpha_u8 = OcTree._visible_arguments(who, dataset, alpha_threshold)
        OcTree._check_moments_cameras(who, cameras)
        center = self._visible_center(who, center)
        try:
            photo_actions(np.zeros((0, 8), np.uint32), threshold, min_views)
        except ValueError as err:
            raise ValueError("%s: %s" % (who, str(err).split(": ", 1)[1])) from None
        if isinstance(max_sweeps, bool) or int(max_sweeps) != max_sweeps or max_sweeps < 0:
            raise ValueError("%s: max_sweeps must be an integer >= 0, got %r" % (who, max_sweeps))
        tree, report, moments, _ = self._photo_sweeps(
            who, images, cameras, alpha_u8, center, threshold, int(min_views), int(max_sweeps),
            float(min_transmittance), bool(recolor))
        data = tree._leaf_data
        if recolor:
            data = np.array(data, dtype=np.float32, copy=True)
            data[:, :3] = OcTree._vote_colors(moments[:, :4], data[:, :3])
        out = OcTree(tree._scale, tree._node_index.copy(), tree._leaf_index.copy(),
                     np.array(data, copy=True), tree._sh_degree)
        out._device = self._device
        out._center = self._center
        return out, report

    def _photo_sweeps(self, who, images, cameras, alpha_u8, center, threshold, min_views,
                      max_sweeps, min_transmittance, want_moments=False):
        """The loop of ``carve_photo`` -> the last tree (this one when nothing was dropped), the
        report, the last tree's moments (``None`` unless ``want_moments`` or the last sweep was
        its) and, per leaf of the last tree, the number of the leaf of THIS tree it was."""
        tree, report, last = self, PhotoReport(), None
        origin = np.arange(self.num_leaves, dtype=np.int64)
        if not torch.is_tensor(images):          # once for all sweeps
            images = torch.from_numpy(np.ascontiguousarray(images)).to(self._dev())
        for _ in range(max_sweeps):
            moments = tree._visible_moments_on_device(images, cameras, alpha_u8, center,
                                                      min_transmittance).cpu().numpy()
            action = photo_actions(moments, threshold, min_views)
            dropped = int((action == ops.OCTREE_DROP).sum())
            report.append(PhotoSweep(tree.num_leaves, int((moments[:, 3] > 0).sum()),
                                     int((moments[:, 3] >= min_views).sum()), dropped))
            if dropped == 0:
                report.converged, last = True, moments
                break
            if dropped == tree.num_leaves:
                raise ValueError("%s: sweep %d would drop every one of the %d leaves: threshold "
                                 "%r refutes them all, raise it"
                                 % (who, len(report), tree.num_leaves, threshold))
            tree, parent = tree.refine(action)
            origin = origin[parent]
        if want_moments and last is None:
            last = tree._visible_moments_on_device(images, cameras, alpha_u8, center,
                                                   min_transmittance).cpu().numpy()
        return tree, report, last, origin

    def refine(self, action) -> Tuple["OcTree", np.ndarray]:
        """A NEW tree from one decision per leaf (K21b): ``action`` (L,) with 0 drop, 1 keep, 2 split
        into the eight children, which inherit the leaf's ``leaf_data`` row bit for bit (see
        ``refine_actions``).  -> ``(tree, parent)``; ``parent`` (L',) int64 numpy is the number of
        the leaf of THIS tree that a new leaf is or came from.  ``leaf_data`` (or its absence),
        ``sh_degree``, ``scale``, the centre and the device carry over; caches start empty.  All ones
        gives this tree's ``node_index``, ``leaf_index`` and ``leaf_data`` again.  Interior nodes
        whose leaves are all dropped go with them.  Raises ``ValueError`` when no leaf would be
        left, when a leaf at level ``ops.octree_max_depth() - 1`` is to split (the ray walk holds
        11 levels), for an action of the wrong length or with a value above 2, and when the new
        leaf count could reach 2^31.  This tree is not modified."""
        action = np.asarray(action)
        if action.dtype.kind not in "iub":
            raise ValueError("OcTree.refine: action holds the integers 0, 1, 2, got dtype %s"
                             % action.dtype)
        ops.octree_refine_check_action(action, self.num_leaves)
        if len(action) and (int(action.max()) > ops.OCTREE_SPLIT or int(action.min()) < 0):
            raise ValueError("OcTree.refine: an action is 0 (drop), 1 (keep) or 2 (split), got "
                             "values in [%d, %d]" % (int(action.min()), int(action.max())))
        if not (action != ops.OCTREE_DROP).any():
            raise ValueError("OcTree.refine: the action leaves no leaf; a tree needs at least one")
        split = action == ops.OCTREE_SPLIT
        if split.any():
            deepest = int(_id_depths(self._leaf_index[split]).max())
            limit = ops.octree_max_depth()
            if deepest >= limit - 1:
                raise ValueError("OcTree.refine: a leaf at level %d cannot split: the tree would be "
                                 "deeper than the ray walk's limit of %d levels "
                                 "(octree_max_depth())" % (deepest, limit))
        dev = self._dev()
        rows = None
        data = self._leaf_data
        if data is not None:
            data = np.ascontiguousarray(data)
            # (K21b moves float32 rows; anything else, a float64 file of the reference say, is
            # gathered on the host by ``parent`` below)
            if data.dtype == np.float32 and data.ndim == 2 and len(data) == self.num_leaves:
                rows = torch.from_numpy(data).to(dev)
        leaf_ids, node_ids, rows, parent = ops.octree_refine(
            self._on_device("leaf_index"), rows,
            torch.from_numpy(np.ascontiguousarray(action, dtype=np.uint8)).to(dev), self.depth)
        parent = parent.cpu().numpy().astype(np.int64)
        if rows is not None:
            data = rows.cpu().numpy()
        elif data is not None:
            data = data[parent]
        tree = OcTree(self._scale, node_ids.cpu().numpy(), leaf_ids.cpu().numpy(), data,
                      self._sh_degree)
        tree._device = self._device
        tree._center = self._center
        return tree, parent

    def bake(self, model, center=None, view=(0, 0, 1), batch_size: int = 1 << 20) -> "OcTree":
        """A NEW tree of the same structure and centre whose ``leaf_data`` (L,4) float32 holds the
        model's own colour and density at every leaf's centre: ``[sigmoid(r), sigmoid(g),
        sigmoid(b), softplus(sigma)]`` of the model's logits, bit for bit what ``Raycaster.render``
        makes of them.  This tree is not modified.

        ``model`` is evaluated in eval mode without gradients, ``batch_size`` leaves at a time, at
        ``leaf_centers() + center``; ``center`` defaults to ``tree.center``, which a loaded tree
        does not have.  A model with ``use_view`` is given the fixed direction ``view`` for every
        leaf: a leaf holds one colour, so the view dependence of such a model is lost
        (``bake_sh`` keeps it).  The result is a plain tree (``sh_degree`` is ``None``)."""
        if center is None:
            center = self._center
        if center is None:
            raise ValueError("OcTree.bake: a loaded tree does not know the centre of its root "
                             "cube (the file has no place for it); pass center=")
        center = tuple(float(c) for c in center)
        batch_size = int(batch_size)
        if len(center) != 3 or batch_size < 1:
            raise ValueError("OcTree.bake: center has three components and batch_size is >= 1")
        device = next(model.parameters()).device
        if self._device is None:
            self._device = device
        points = torch.from_numpy(self.leaf_centers()).to(device)
        points = points + torch.tensor(center, dtype=torch.float32, device=device)
        use_view = bool(getattr(model, "use_view", False))
        if use_view:
            direction = torch.tensor([float(v) for v in view], dtype=torch.float32, device=device)
        was_training = model.training
        model.eval()
        baked = []
        try:
            with torch.no_grad():
                for start in range(0, points.shape[0], batch_size):
                    batch = points[start:start + batch_size].contiguous()
                    if use_view:
                        logits = model(batch, direction.expand(batch.shape[0], 3).contiguous())
                    else:
                        logits = model(batch)
                    baked.append(ops.octree_bake(logits.reshape(-1, 4).to(torch.float32)
                                                 .contiguous()))
        finally:
            model.train(was_training)
        tree = OcTree(self._scale, self._node_index, self._leaf_index,
                      torch.cat(baked).cpu().numpy())
        tree._device = self._device
        tree._center = center
        return tree

    def bake_sh(self, model, degree: int = 2, num_views: int = 64, center=None,
                batch_size: int = 1 << 20) -> "OcTree":
        """A NEW tree of the same structure and centre with ``sh_degree = degree`` whose
        ``leaf_data`` (L, 3 B + 1) float32, ``B = (degree + 1)^2``, holds per leaf and colour channel
        the SH coefficients of the model's colour LOGIT over the view direction, and the density
        (K18b).  This tree is not modified.

        A model with ``use_view`` is evaluated as ``bake`` evaluates it, once per direction
        ``v_j`` of ``sh_view_directions(num_views)`` (every leaf of a batch gets ``v_j``), and
        view j adds ``P[b, j] * logit[c]`` to coefficient ``k[c B + b]``, ``P`` the float32 cast of
        the float64 pseudo-inverse of ``sh_basis(views, degree)``: the least-squares fit of the
        logits over the views.  The density is the mean over the views of ``softplus(sigma)``.
        ``num_views >= 2 B``.  The (L, V, 4) logits are never held.

        A model without ``use_view`` is evaluated once: band 0 is ``logit / Y_0`` and the other
        bands are zero, the density what ``bake`` stores."""
        bases = _sh_bases(degree)
        degree = int(degree)
        num_views = int(num_views)
        if num_views < 2 * bases:
            raise ValueError("OcTree.bake_sh: degree %d needs num_views >= %d, got %d"
                             % (degree, 2 * bases, num_views))
        if center is None:
            center = self._center
        if center is None:
            raise ValueError("OcTree.bake: a loaded tree does not know the centre of its root "
                             "cube (the file has no place for it); pass center=")
        center = tuple(float(c) for c in center)
        batch_size = int(batch_size)
        if len(center) != 3 or batch_size < 1:
            raise ValueError("OcTree.bake_sh: center has three components and batch_size is >= 1")
        device = next(model.parameters()).device
        if self._device is None:
            self._device = device
        points = torch.from_numpy(self.leaf_centers()).to(device)
        points = points + torch.tensor(center, dtype=torch.float32, device=device)
        count = points.shape[0]
        use_view = bool(getattr(model, "use_view", False))
        views = sh_view_directions(num_views)
        project = np.linalg.pinv(sh_basis(views, degree)).astype(np.float32)      # (B, V)
        data = torch.zeros((count, 3 * bases + 1), dtype=torch.float32, device=device)
        was_training = model.training
        model.eval()
        try:
            with torch.no_grad():
                if use_view:
                    inv_views = float(np.float32(1.0 / num_views))
                    for j in range(num_views):
                        direction = torch.tensor(views[j], dtype=torch.float32, device=device)
                        for start in range(0, count, batch_size):
                            batch = points[start:start + batch_size].contiguous()
                            logits = model(batch, direction.expand(batch.shape[0], 3).contiguous())
                            ops.octree_sh_accumulate(
                                logits.reshape(-1, 4).to(torch.float32).contiguous(),
                                data[start:start + batch_size], project[:, j], inv_views, degree)
                else:
                    # a device tensor, not a Python number: a true f32 division, not a product
                    # with the reciprocal
                    y0 = torch.tensor(SH_Y0, dtype=torch.float32, device=device)
                    for start in range(0, count, batch_size):
                        batch = points[start:start + batch_size].contiguous()
                        logits = model(batch).reshape(-1, 4).to(torch.float32).contiguous()
                        rows = data[start:start + batch_size]
                        # layout only: band 0 of a constant is the constant over Y_0
                        rows[:, 0:3 * bases:bases] = logits[:, :3] / y0
                        rows[:, 3 * bases] = ops.octree_bake(logits)[:, 3]
        finally:
            model.train(was_training)
        tree = OcTree(self._scale, self._node_index, self._leaf_index, data.cpu().numpy(), degree)
        tree._device = self._device
        tree._center = center
        return tree

    def render_image(self, sampler, index: int, center=None, t_min: float = 0.0,
                     background=(0, 0, 0), shading: str = "flat", include_depth: bool = False,
                     mode: str = "first_hit", min_transmittance: float = 0.0):
        """(H,W,3) uint8 frame of the sampler's camera ``index % num_cameras``, as
        ``Raycaster.render_image`` returns it; with ``include_depth`` also the (H,W) float32
        alpha and depth maps.  Every ray of the camera is used -- the octree is the geometry, the
        sampler's validity mask is not applied.  ``center``: the root cube's centre in the
        sampler's frame; defaults to ``tree.center``, which a loaded tree does not have.
        ``mode``: ``"first_hit"`` (``render``) or ``"volume"`` (``render_volume`` of a baked tree,
        with ``min_transmittance``; its shading is ``"flat"``)."""
        if mode not in ("first_hit", "volume"):
            raise ValueError("OcTree.render_image: mode is 'first_hit' or 'volume', got %r"
                             % (mode,))
        if mode == "volume":
            if shading != "flat":
                raise ValueError("OcTree.render_image: mode='volume' has no face shading; "
                                 "shading must be 'flat', got %r" % (shading,))
            self._check_volume(min_transmittance)
        if center is None:
            center = self._center
        if center is None:
            raise ValueError("OcTree.render_image: a loaded tree does not know the centre of its "
                             "root cube (the file has no place for it); pass center=")
        camera = index % sampler.num_cameras
        first = camera * sampler.rays_per_camera
        rays = slice(first, first + sampler.rays_per_camera)
        shift = torch.tensor([float(c) for c in center], dtype=torch.float32,
                             device=sampler.starts.device)
        if mode == "volume":
            color, alpha, depth = self.render_volume(sampler.starts[rays] - shift,
                                                     sampler.directions[rays], t_min, background,
                                                     min_transmittance)
        else:
            color, alpha, depth = self.render(sampler.starts[rays] - shift,
                                              sampler.directions[rays], t_min, background, shading)
        pixels = torch.arange(sampler.rays_per_camera, dtype=torch.int64, device=color.device)
        image = ops.to_image(color, pixels, sampler.image_width, sampler.image_height)
        image = image.cpu().numpy()
        if not include_depth:
            return image
        shape = (sampler.image_height, sampler.image_width)
        return image, alpha.reshape(shape).cpu().numpy(), depth.reshape(shape).cpu().numpy()

    def intersect(self, starts, directions, max_length: int):
        raise NotImplementedError("OcTree.intersect (the ray walker of the lecture animations) "
                                  "is not part of the HIP path")

    @staticmethod
    def build_from_mesh(mesh_path: str, voxel_depth: int, min_leaf_size: int,
                        up_dir=(0, 1, 0)) -> "OcTree":
        raise NotImplementedError("OcTree.build_from_mesh needs trimesh and is not part of the "
                                  "HIP path; sample the mesh and call build_from_samples")

    @staticmethod
    def build_from_triangles(vertices, triangles, uvs, texture, voxel_depth: int,
                             min_leaf_size: int, up_dir=(0, 1, 0), seed: int = 0) -> "OcTree":
        """Builds a colour OcTree from a textured triangle mesh: the reference's
        ``build_from_mesh`` (octree.py:807-853) from the point where trimesh has read the file.

        vertices (V,3), triangles (F,3) integers, uvs (V,2), texture (H,W,C) uint8 with C >= 3 and
        row 0 at the top of the image (``mesh.load_obj`` and ``mesh.procedural_torus`` return
        exactly these).  The vertices are normalised (``mesh.normalize_points`` with ``up_dir``),
        ``8^(voxel_depth - 2) * min_leaf_size`` surface samples are spread over the triangles by
        area (``mesh.triangle_counts`` with ``seed``; the reference draws them unseeded) and drawn
        by K22 with the texture flipped vertically, so that ``v = 0`` is the bottom row of the
        image; ``build_from_samples`` takes the cloud as it lies on the GPU."""
        from . import mesh
        voxel_depth, min_leaf_size = int(voxel_depth), int(min_leaf_size)
        limit = ops.octree_max_depth()
        if voxel_depth < 2 or voxel_depth > limit or min_leaf_size < 1:
            raise ValueError("OcTree.build_from_triangles: 2 <= voxel_depth <= %d and "
                             "min_leaf_size >= 1, got %d and %d"
                             % (limit, voxel_depth, min_leaf_size))
        texture = texture.cpu().numpy() if torch.is_tensor(texture) else np.asarray(texture)
        if texture.ndim != 3:
            raise ValueError("OcTree.build_from_triangles: texture must be (H,W,C), got %s"
                             % (texture.shape,))
        num_points = (8 ** (voxel_depth - 2)) * min_leaf_size
        if num_points > ops.octree_max_points():
            raise ValueError("OcTree.build_from_triangles: 8^(voxel_depth - 2) * min_leaf_size = "
                             "%d samples; at most %d are supported"
                             % (num_points, ops.octree_max_points()))
        points = mesh.normalize_points(vertices, up_dir)
        counts = mesh.triangle_counts(points, triangles, num_points, seed)
        positions, colors = mesh.sample_mesh(points, triangles, uvs,
                                             np.ascontiguousarray(texture[::-1]), counts)
        return OcTree.build_from_samples(positions, voxel_depth, min_leaf_size, colors)

    @staticmethod
    def build_from_model(model, depth: int, center=(0, 0, 0), scale: float = 1.0,
                         alpha_threshold: float = 0.01, merge_tolerance=None, view=(0, 0, 1),
                         batch_size: int = 1 << 20) -> "OcTree":
        """Builds a tree with a leaf wherever a trained model has density (K16; no counterpart in
        the reference, whose voxelize_model.py builds the shell of the depth renders).

        The root cube is ``center +- scale``.  Every cell of the finest grid (level ``depth - 1``,
        ``2^(depth-1)`` per axis, ``depth`` as in ``build_from_samples``) is evaluated once at its
        centre, ``batch_size`` consecutive path codes at a time, so the dense grid is never held.
        ``model`` is called as ``bake`` calls it (eval mode, no gradients, the fixed ``view`` for a
        model with ``use_view``).  A cell becomes a leaf iff ``sigma * side > tau`` in f32, with
        ``sigma`` the baked density, ``side = 2 scale / 2^(depth-1)`` and ``tau =
        -log1p(-alpha_threshold)``: the cell's opacity along one side exceeds ``alpha_threshold``
        (0 <= alpha_threshold < 1).  ``leaf_data`` is (L,4) float32 ``[sigmoid(rgb),
        softplus(sigma)]``, what ``bake`` stores: without merging,
        ``tree.bake(model, view=view).leaf_data()`` is ``tree.leaf_data()`` bit for bit.

        ``merge_tolerance``: ``None``, one float (all four channels) or ``(rgb_tol, sigma_tol)``.
        When given, eight sibling leaves whose channels all lie within the tolerance of their mean
        become their parent, which holds the mean; one pass per level from the finest up, so
        merges cascade.

        One sample per finest cell: structure thinner than a cell can be missed, and a leaf holds
        one colour (see ``bake``)."""
        depth, center, scale, batch_size, tolerances = OcTree._grid_arguments(
            "OcTree.build_from_model", "center and view have three components",
            depth, center, scale, batch_size, merge_tolerance)
        alpha_threshold = float(alpha_threshold)
        if not 0.0 <= alpha_threshold < 1.0:        # NaN fails too
            raise ValueError("OcTree.build_from_model: alpha_threshold must lie in [0, 1), got %r"
                             % (alpha_threshold,))
        view = tuple(float(v) for v in view)
        if len(view) != 3:
            raise ValueError("OcTree.build_from_model: center and view have three components and "
                             "batch_size is >= 1")
        tau = float(np.float32(-np.log1p(-np.float64(alpha_threshold))))
        side = float(np.float32(2.0 * scale) / np.float32(2.0 ** (depth - 1)))

        device = next(model.parameters()).device
        use_view = bool(getattr(model, "use_view", False))
        if use_view:
            direction = torch.tensor(view, dtype=torch.float32, device=device)
        cells = 8 ** (depth - 1)
        kept_codes, kept_data = [], []
        was_training = model.training
        model.eval()
        try:
            with torch.no_grad():
                for first in range(0, cells, batch_size):
                    count = min(batch_size, cells - first)
                    points = ops.octree_cell_centers(first, count, center, scale, depth, device)
                    if use_view:
                        logits = model(points, direction.expand(count, 3).contiguous())
                    else:
                        logits = model(points)
                    logits = logits.reshape(-1, 4).to(torch.float32).contiguous()
                    codes, data = ops.octree_density_select(logits, first, tau, side, depth)
                    if codes.shape[0] > 0:
                        kept_codes.append(codes)
                        kept_data.append(data)
        finally:
            model.train(was_training)
        if not kept_codes:
            raise ValueError("OcTree.build_from_model: no leaf (no cell of depth %d with "
                             "sigma * side > %g)" % (depth, tau))
        return OcTree._from_cells(torch.cat(kept_codes), torch.cat(kept_data), depth, scale,
                                  center, tolerances, device)

    @staticmethod
    def _grid_arguments(who, three, depth, center, scale, batch_size, merge_tolerance):
        """What the dense-grid builders check alike -> depth, center and scale as f32 values,
        batch_size, and merge_tolerance as ``None`` or ``(rgb_tol, sigma_tol)``."""
        depth = int(depth)
        limit = ops.octree_max_depth()
        if depth < 1 or depth > limit:
            raise ValueError("%s: depth %d is outside what the path codes hold (1 .. %d)"
                             % (who, depth, limit))
        center = tuple(float(np.float32(c)) for c in center)
        batch_size = int(batch_size)
        if len(center) != 3 or batch_size < 1:
            raise ValueError("%s: %s and batch_size is >= 1" % (who, three))
        scale = float(np.float32(scale))
        if not 0.0 < scale < float("inf"):
            raise ValueError("%s: scale must be positive and finite, got %r" % (who, scale))
        tolerances = None
        if merge_tolerance is not None:
            pair = np.atleast_1d(np.asarray(merge_tolerance, dtype=np.float64)).reshape(-1)
            if len(pair) == 1:
                pair = np.repeat(pair, 2)
            if len(pair) != 2 or not (pair >= 0).all():        # NaN fails too
                raise ValueError("%s: merge_tolerance is None, one float >= 0 or a pair "
                                 "(rgb_tol, sigma_tol) of them, got %r" % (who, merge_tolerance))
            tolerances = (float(pair[0]), float(pair[1]))
        return depth, center, scale, batch_size, tolerances

    @staticmethod
    def _from_cells(codes, data, depth, scale, center, tolerances, device) -> "OcTree":
        """The tail of the dense-grid builders: the kept finest cells in code order (codes (K)
        int32, data (K,4) float32 on the device) -> the optional merge passes, the ids, the
        interior nodes and the tree in id order."""
        levels = torch.full_like(codes, depth - 1)
        if tolerances is not None:
            for level in range(depth - 1, 0, -1):
                codes, levels, data = ops.octree_merge_level(codes, levels, data, level, depth,
                                                             tolerances[0], tolerances[1])
        # ids from (code, level): integer plumbing
        first_id = torch.tensor([(8 ** k - 1) // 7 for k in range(depth)], dtype=torch.int64,
                                device=device)
        wide = levels.to(torch.int64)
        leaf_ids = first_id[wide] + (codes.to(torch.int64) >> (3 * (depth - 1 - wide)))
        node_ids = ops.octree_interior_nodes(leaf_ids.contiguous(), depth)
        leaf_ids, order = torch.sort(leaf_ids)            # code order -> id order
        tree = OcTree(scale, node_ids.cpu().numpy(), leaf_ids.cpu().numpy(),
                      data[order].cpu().numpy())
        tree._device = device
        tree._center = center
        return tree

    @staticmethod
    def build_from_silhouettes(dataset, depth: int, center=(0, 0, 0), scale: float = 1.0,
                               alpha_threshold: float = 0.5, dilate: int = 1, max_misses: int = 0,
                               min_views: int = 2, cell_opacity: float = 0.5,
                               merge_tolerance=None, batch_size: int = 1 << 20,
                               color: str = "mean",
                               visible_transmittance: float = 0.3,
                               footprint: str = "point", start_level: int = 4,
                               photo_threshold: Optional[float] = None,
                               photo_min_views: int = 2, photo_max_sweeps: int = 16,
                               photo_report: Optional[list] = None) -> "OcTree":
        """Carves a tree out of the root cube from the images' silhouettes alone (K23; no
        counterpart in the reference): a starting point for ``fit_octree`` that needs neither a
        trained model nor the mesh.

        ``dataset`` gives ``images`` ((C,H,W,4) uint8 RGBA, colour space RGB) and ``cameras``.  The
        root cube is ``center +- scale`` and the grid that of ``build_from_model``: every cell of
        level ``depth - 1`` is looked at once, ``batch_size`` consecutive path codes at a time.  A
        pixel is foreground where its alpha is ``>= alpha_u8 = ceil(alpha_threshold * 255)``
        (clamped to 1 .. 255); that mask is grown by ``dilate`` pixels (a square maximum filter,
        once, before the kernel).  A cell's centre is projected into every camera to its nearest
        pixel; the cell survives iff at most ``max_misses`` of the cameras that see it see it on the
        background of the grown mask, and at least ``min_views`` cameras see it at all.  Its row is
        ``[r, g, b, sigma0]``: the mean of the pixels it projects to whose own alpha is
        ``>= alpha_u8`` (grey 0.5 if none), and ``sigma0 = -log1p(-cell_opacity) / side``, so that
        one cell side starts at opacity ``cell_opacity`` (0 <= cell_opacity < 1).
        ``merge_tolerance`` as for ``build_from_model``.

        The limits: one sample per cell, at its centre, so structure thinner than a cell or than
        a pixel's footprint can be carved away (``dilate`` and ``max_misses`` are the slack).  The
        colour ignores occlusion: cameras on the far side of the object vote into the mean.  The
        hull of few views is fatter than the object, and concavities that no silhouette shows
        stay filled.  The defaults ``cell_opacity``, ``dilate`` and ``min_views`` are untuned
        starting values.

        ``color="visible"`` answers the second limit (K24): the carved cells, unmerged, form a tree
        first; every cell that some camera can see through that tree (``visible_votes`` with the
        same ``alpha_threshold`` and ``min_transmittance = visible_transmittance``) takes the mean
        of those cameras alone, a cell none sees keeps the mean of all; then the merge passes run
        as usual.  ``color="mean"`` is the tree described above, bit for bit.  The limits of
        ``color_from_images`` apply.

        ``footprint="box"`` answers the first limit (K27, ``csrc/carve_box.hip``).  A camera
        refutes a cell only when it sees all of it (centre and eight corners in front) and the
        bounding rectangle of their nearest pixels, widened by ``1 + (depth - 1 - level)`` pixels,
        lies wholly inside the image and holds no foreground pixel of the grown mask.  Such a test
        is conservative, so the carve runs coarse to fine: it starts from every cell of level
        ``min(start_level, depth - 1)``, tests at most ``batch_size`` candidates per call (one
        read-back each) and looks only at the children of survivors; ``min_views`` applies at the
        finest level.  Every ``start_level`` gives the same tree.  Guaranteed: with
        ``max_misses = 0`` a finest cell is kept if it contains a point that no camera sees on the
        background of the grown mask (and ``min_views`` cameras see the cell).  Not guaranteed:
        the hull is fatter than the point carve's by the cell's footprint plus the pad (more than a
        cell where a pixel is wider than a cell); a cell kept only through its footprint, whose
        centre projects onto no foreground pixel in any camera, starts grey until
        ``color="visible"`` or a fit colours it; and a cell that is partly off an image cannot be
        refuted by that camera at all.  A cell both footprints keep has the same row bit for bit.  ``footprint="point"``
        (the default) is the carve described first, bit for bit, and ignores ``start_level``.

        ``photo_threshold`` answers the third limit (K28).  ``None`` (the default) is the method
        described so far, bit for bit.  Otherwise the carved cells, unmerged, form a tree and
        ``carve_photo(dataset, center, photo_threshold, photo_min_views, photo_max_sweeps,
        alpha_threshold, min_transmittance=visible_transmittance)`` thins it: cells whose seeing
        cameras disagree on their colour go, sweep by sweep.  That comes before the
        ``color="visible"`` votes, which are then taken from the thinned tree, and before the merge
        passes.  ``photo_report``, an empty ``PhotoReport``, receives the sweeps and the
        ``converged`` flag.  The limits of ``carve_photo`` apply; where the threshold fires, the
        guarantee of ``footprint="box"`` is given up."""
        who = "OcTree.build_from_silhouettes"
        depth, center, scale, batch_size, tolerances = OcTree._grid_arguments(
            who, "center has three components", depth, center, scale, batch_size,
            merge_tolerance)
        alpha_threshold, cell_opacity = float(alpha_threshold), float(cell_opacity)
        if not 0.0 <= alpha_threshold <= 1.0:        # NaN fails too
            raise ValueError("%s: alpha_threshold must lie in [0, 1], got %r"
                             % (who, alpha_threshold))
        if not 0.0 <= cell_opacity < 1.0:
            raise ValueError("%s: cell_opacity must lie in [0, 1), got %r" % (who, cell_opacity))
        if color not in ("mean", "visible"):
            raise ValueError("%s: color is 'mean' or 'visible', got %r" % (who, color))
        if (color == "visible" or photo_threshold is not None) and \
                not 0.0 <= float(visible_transmittance) < 1.0:
            raise ValueError("%s: visible_transmittance must lie in [0, 1), got %r"
                             % (who, visible_transmittance))
        if photo_threshold is not None:
            try:
                photo_actions(np.zeros((0, 8), np.uint32), photo_threshold, photo_min_views)
            except ValueError as err:
                raise ValueError("%s: photo_%s" % (who, str(err).split(": ", 1)[1])) from None
            if isinstance(photo_max_sweeps, bool) or int(photo_max_sweeps) != photo_max_sweeps \
                    or photo_max_sweeps < 0:
                raise ValueError("%s: photo_max_sweeps must be an integer >= 0, got %r"
                                 % (who, photo_max_sweeps))
        dilate, max_misses, min_views = int(dilate), int(max_misses), int(min_views)
        if dilate < 0 or max_misses < 0 or min_views < 0:
            raise ValueError("%s: dilate, max_misses and min_views must be >= 0, got %d, %d and %d"
                             % (who, dilate, max_misses, min_views))
        if footprint not in ("point", "box"):
            raise ValueError("%s: footprint is 'point' or 'box', got %r" % (who, footprint))
        if footprint == "box":
            if isinstance(start_level, bool) or int(start_level) != start_level or start_level < 0:
                raise ValueError("%s: start_level must be an integer >= 0, got %r"
                                 % (who, start_level))
            start_level = min(int(start_level), depth - 1)
        images = np.asarray(dataset.images)
        if images.ndim != 4 or images.shape[-1] != 4 or images.dtype != np.uint8:
            raise ValueError("%s: dataset.images must be (C,H,W,4) uint8 with an alpha channel, "
                             "got %s %s" % (who, images.dtype, images.shape))
        if getattr(dataset, "color_space", "RGB") != "RGB":
            raise ValueError("%s: dataset.color_space must be RGB, got %r"
                             % (who, dataset.color_space))
        cameras = list(dataset.cameras)
        if len(cameras) != len(images) or not cameras:
            raise ValueError("%s: dataset has %d cameras for %d images"
                             % (who, len(cameras), len(images)))
        from .cameras import projection_matrices
        alpha_u8 = min(max(int(np.ceil(alpha_threshold * 255)), 1), 255)
        side = float(np.float32(2.0 * scale) / np.float32(2.0 ** (depth - 1)))
        sigma0 = float(np.float32(-np.log1p(-np.float64(cell_opacity)) / np.float64(side)))

        sampler = getattr(dataset, "sampler", None)
        device = torch.device(getattr(sampler, "device", None) or "cuda")
        images_u8 = torch.from_numpy(np.ascontiguousarray(images)).to(device)
        proj = torch.from_numpy(projection_matrices(cameras)).to(device)
        mask = (images_u8[..., 3] >= alpha_u8).to(torch.float32)
        if dilate > 0:      # maxima of 0 / 1: exact
            mask = torch.nn.functional.max_pool2d(mask[:, None], 2 * dilate + 1, stride=1,
                                                  padding=dilate)[:, 0]
        mask_u8 = mask.to(torch.uint8).contiguous()
        cells = 8 ** (depth - 1)
        kept_codes, kept_data = [], []
        if footprint == "box":
            kept_codes, kept_data = OcTree._carve_box_levels(
                images_u8, mask_u8, proj, center, scale, depth, alpha_u8, max_misses, min_views,
                sigma0, start_level, batch_size)
        for first in range(0, cells if footprint == "point" else 0, batch_size):
            count = min(batch_size, cells - first)
            codes, data = ops.octree_carve_select(images_u8, mask_u8, proj, first, count, center,
                                                  scale, depth, alpha_u8, max_misses, min_views,
                                                  sigma0)
            if codes.shape[0] > 0:
                kept_codes.append(codes)
                kept_data.append(data)
        if not kept_codes:
            raise ValueError("%s: no leaf (every cell of depth %d is carved away or seen by fewer "
                             "than %d cameras)" % (who, depth, min_views))
        codes, data = torch.cat(kept_codes), torch.cat(kept_data)
        if photo_threshold is not None:
            # the unmerged tree again: leaf k is cell k, and `origin` names the cells that are left
            OcTree._check_moments_cameras(who, cameras)
            hull = OcTree._from_cells(codes, data, depth, scale, center, None, device)
            _, report, _, origin = hull._photo_sweeps(
                who, images_u8, cameras, alpha_u8, center, photo_threshold, int(photo_min_views),
                int(photo_max_sweeps), float(visible_transmittance))
            if photo_report is not None:
                photo_report.extend(report)
                photo_report.converged = report.converged
            origin = torch.from_numpy(origin).to(device)
            codes, data = codes[origin].contiguous(), data[origin].contiguous()
        if color == "visible":
            # the unmerged tree: every leaf on the finest level, where id order is code order
            hull = OcTree._from_cells(codes, data, depth, scale, center, None, device)
            votes = hull._visible_votes_on_device(images_u8, cameras, alpha_u8, center,
                                                  float(visible_transmittance)).cpu().numpy()
            rows = data.cpu().numpy()
            rows[:, :3] = OcTree._vote_colors(votes, rows[:, :3])
            data = torch.from_numpy(rows).to(device)
        return OcTree._from_cells(codes, data, depth, scale, center, tolerances, device)

    @staticmethod
    def _carve_box_levels(images_u8, mask_u8, proj, center, scale, depth, alpha_u8, max_misses,
                          min_views, sigma0, start_level, batch_size, trace=None):
        """The coarse-to-fine loop of ``build_from_silhouettes(footprint="box")``: every cell of
        level ``start_level``, then level by level the children of the survivors, at most
        ``batch_size`` candidates per call of K27.  -> lists of the kept finest cells' codes and
        rows, chunk by chunk in code order (empty when nothing survives).  ``trace``, a list, gets
        one ``(level, candidates, survivors)`` per level."""
        sat = ops.octree_carve_box_tables(mask_u8)
        device = images_u8.device

        def test(candidates, level, expand):
            return ops.octree_carve_box_level(images_u8, sat, proj, candidates, level, center,
                                              scale, depth, alpha_u8, max_misses, min_views,
                                              sigma0, expand=expand)

        parts, tested = [], 8 ** start_level
        for first in range(0, tested, batch_size):
            count = min(batch_size, tested - first)
            codes = torch.arange(first, first + count, dtype=torch.int32, device=device)
            parts.append(test(codes, start_level, False))
        for level in range(start_level, depth):
            parts = [(c, d) for c, d in parts if c.shape[0] > 0]
            if trace is not None:
                trace.append((level, tested, sum(c.shape[0] for c, _ in parts)))
            if level == depth - 1 or not parts:
                break
            parents = torch.cat([c for c, _ in parts])
            parts, tested = [], 8 * parents.shape[0]
            if batch_size >= 8:     # the kernel expands eight children per parent itself
                step = batch_size // 8
                for first in range(0, parents.shape[0], step):
                    parts.append(test(parents[first:first + step].contiguous(), level + 1, True))
            else:
                children = ((parents[:, None] << 3)
                            | torch.arange(8, dtype=torch.int32, device=device)).reshape(-1)
                for first in range(0, tested, batch_size):
                    parts.append(test(children[first:first + batch_size].contiguous(), level + 1,
                                      False))
        return [c for c, _ in parts], [d for _, d in parts]

    @staticmethod
    def build_from_samples(positions, depth: int, min_leaf_size: int, data=None) -> "OcTree":
        """Builds a sparse OcTree from position samples (octree.py:733-806) on the GPU.

        positions (N,3) and data (N,C): numpy arrays or device tensors.  The leaves hold the
        mean of their points' data.  The caller's positions are left as they are."""
        depth = int(depth)
        limit = ops.octree_max_depth()
        if depth < 1 or depth > limit:
            raise ValueError("OcTree.build_from_samples: depth %d is outside what the path codes "
                             "hold (1 .. %d)" % (depth, limit))

        def to_device(x, device):
            if torch.is_tensor(x):
                return x.to(torch.float32).contiguous()
            return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(device)

        device = positions.device if torch.is_tensor(positions) else torch.device("cuda")
        pos = to_device(positions, device).reshape(-1, 3)
        n = pos.shape[0]
        if n == 0:
            raise ValueError("OcTree.build_from_samples: empty point cloud")
        # the root cube in the reference's f32 arithmetic (octree.py:756-759)
        min_pos, max_pos = pos.amin(0), pos.amax(0)
        cube = torch.cat([0.5 * (min_pos + max_pos), ((max_pos - min_pos).max() * 0.5)[None]])
        cx, cy, cz, scale = [float(v) for v in cube.cpu()]

        codes = ops.octree_path_codes(pos, (cx, cy, cz), scale, depth)
        codes, perm = torch.sort(codes, stable=True)     # key sort: plumbing
        point_leaf, leaf_ids, leaf_start, leaf_count = ops.octree_structure(
            codes, perm, depth, int(min_leaf_size))
        if leaf_ids.shape[0] == 0:
            raise ValueError("OcTree.build_from_samples: no leaf (%d points, min_leaf_size %d, "
                             "depth %d)" % (n, min_leaf_size, depth))
        node_ids = ops.octree_interior_nodes(leaf_ids, depth)
        leaf_ids, order = torch.sort(leaf_ids)            # code order -> id order
        leaf_data = None
        if data is not None:
            values = to_device(data, device).reshape(n, -1)
            leaf_data = ops.octree_leaf_means(values, perm, leaf_start[order].contiguous(),
                                              leaf_count[order].contiguous()).cpu().numpy()
        tree = OcTree(scale, node_ids.cpu().numpy(), leaf_ids.cpu().numpy(), leaf_data)
        tree._device = device
        tree._point_leaf = point_leaf
        tree._center = (cx, cy, cz)
        return tree

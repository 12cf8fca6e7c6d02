"""MI355X-native NeRF volume rendering behind the ``fourier_feature_nets`` class surface.

Everything numeric runs in hand-written gfx950 kernels (``csrc/``) reached through the C ABI
of ``include/ffn_hip.h``; this package is the host-side mirror of the reference's Python API
for that path.  There is no CPU fallback: using a model or sampler without a GPU raises.
"""

from .cameras import CameraInfo, Resolution, eye_positions, orbit, projection_matrices
from .caster import LogEntry, Raycaster, TrainEngine
from .dataset import ImageDataset, RayDataset
from .frames import FrameSink
from .occupancy import OccupancyGrid
from .octree import (OcTree, PhotoReport, PhotoSweep, SurfaceMesh, photo_actions,
                     refine_actions)
from .octree_fit import (FitLogEntry, OctreeField, OctreeSHField, RefineReport, fit_octree,
                         fit_octree_adaptive, fit_octree_sh, leaf_weights_over)
from .pixel_dataset import PixelData, PixelDataset
from .regression import RegressionEngine
from .signal_dataset import SignalData, SignalDataset
from .mesh import (MeshBVH, MeshHit, MeshTaps, bake_vertex_colors, build_mesh_bvh, cast_rays,
                   color_mesh_from_images, edge_opposites,
                   fit_mesh_colors, fit_mesh_geometry, fit_mesh_texture, load_obj,
                   mesh_spans, mesh_texture_taps, normalize_points, procedural_torus, render_mesh,
                   render_mesh_backward, render_mesh_geometry_backward, render_mesh_image,
                   render_mesh_rays, render_mesh_texture, render_mesh_texture_backward, sample_mesh, save_obj,
                   texture_mesh_from_images, texture_to_uint8, triangle_counts, unwrap_mesh,
                   vertex_adjacency, vertex_neighbors)
from .models import (
    BasicFourierMLP,
    FourierFeatureMLP,
    GaussianFourierMLP,
    MLP,
    NeRF,
    PositionalFourierMLP,
)
from .sampler import RaySampler, RaySamples
from .utils import (
    ETABar,
    RenderResult,
    calculate_blend_weights,
    exponential_lr_decay,
    linspace,
    load_model,
)
from .visualizers import ActivationVisualizer, EvaluationVisualizer, OrbitVideoVisualizer, Visualizer
from .voxels import VoxelProgram, Voxels

__version__ = "0.1.0"

__all__ = ["__version__", "ActivationVisualizer", "BasicFourierMLP", "CameraInfo", "ETABar", "EvaluationVisualizer", "FitLogEntry", "FourierFeatureMLP", "FrameSink",
           "GaussianFourierMLP", "ImageDataset", "LogEntry", "MLP", "MeshBVH", "MeshHit", "MeshTaps", "NeRF",
           "OcTree", "OccupancyGrid", "OctreeField", "OctreeSHField", "OrbitVideoVisualizer", "PhotoReport", "PhotoSweep", "PixelData", "PixelDataset", "PositionalFourierMLP", "RayDataset", "RaySampler", "RaySamples", "Raycaster", "RefineReport", "RegressionEngine",
           "RenderResult", "Resolution", "SignalData", "SignalDataset", "SurfaceMesh", "TrainEngine", "Visualizer", "VoxelProgram", "Voxels", "bake_vertex_colors", "build_mesh_bvh", "calculate_blend_weights", "cast_rays", "color_mesh_from_images", "edge_opposites",
           "exponential_lr_decay", "eye_positions", "fit_mesh_colors", "fit_mesh_geometry", "fit_mesh_texture", "fit_octree", "fit_octree_adaptive", "fit_octree_sh", "leaf_weights_over",
           "linspace", "load_model", "load_obj", "mesh_spans", "mesh_texture_taps", "normalize_points", "orbit", "photo_actions", "procedural_torus",
           "projection_matrices", "refine_actions", "render_mesh", "render_mesh_backward", "render_mesh_geometry_backward", "render_mesh_image", "render_mesh_rays", "render_mesh_texture", "render_mesh_texture_backward", "sample_mesh", "save_obj",
           "texture_mesh_from_images", "texture_to_uint8", "triangle_counts", "unwrap_mesh", "vertex_adjacency", "vertex_neighbors"]

"""K31 on the GPU: the rasteriser's three kernels against the numpy restatement of their contract
(tests/mesh_raster_reference.py), bit for bit on ids, alpha, colour and depth -- hipcc rounds f32
``/`` and ``sqrtf`` correctly, so the depth needs no budget of its own; the shapes, placements and
colour paths the contract names; the same bits over chunks, calls and triangle orders; the image
of a block mesh against the project's own first-hit walk of the tree it came from; the scripts as
programs."""

import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import mesh_raster_reference as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "make_mesh_npz_octree.json")


def on_gpu(x, dtype):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


def device_raster(vertices, triangles, proj, eye, width, height, colors=None, uvs=None,
                  texture=None, background=(0, 0, 0), batch_size=1 << 22):
    from fourier_feature_nets_amd import mesh
    out = mesh.rasterize_mesh(on_gpu(vertices, "float32"), on_gpu(triangles, "int32"), proj, eye,
                              width, height, on_gpu(colors, "float32"), on_gpu(uvs, "float32"),
                              on_gpu(texture, "uint8"), background, batch_size)
    return tuple(t.cpu().numpy() for t in out[:5]) + (out[5],)


def assert_same_bits(got, want):
    """(color, alpha, depth, ids, status, box pixels) of the device against the restatement's."""
    for name, g, w in zip(("color", "alpha", "depth"), got, want):
        assert g.dtype == np.float32 and g.shape == w.shape, name
        np.testing.assert_array_equal(g.view(np.uint32), w.view(np.uint32), err_msg=name)
    assert got[3].dtype == np.int32
    np.testing.assert_array_equal(got[3], want[3])
    np.testing.assert_array_equal(got[4], want[4])
    assert got[5] == int(want[5].sum())


def both(*args, **kwargs):
    batch = kwargs.pop("batch_size", 1 << 22)
    got = device_raster(*args, batch_size=batch, **kwargs)
    want = ref.raster(*args, **kwargs)
    assert_same_bits(got, want)
    return got


def view(width, height, focal=None):
    from fourier_feature_nets_amd.cameras import eye_positions, projection_matrices
    cam = ref.camera(width, height, focal=focal)
    return projection_matrices([cam])[0], eye_positions([cam], (0.0, 0.0, 0.0))[0]


# F of 1, 63, 64, 65 and 257 (around one wave and past one block of set-up threads), on every image
# shape the contract names; the one-pixel-wide and one-pixel-high images keep a 48-pixel focal length
@pytest.mark.parametrize("count,width,height,focal", [
    (1, 24, 20, None), (63, 64, 48, None), (64, 65, 33, None), (65, 24, 20, None),
    (257, 64, 48, None), (65, 1, 48, 66.0), (63, 65, 1, 66.0), (257, 65, 33, None)])
def test_the_image_is_the_restatements_bit_for_bit(count, width, height, focal):
    vertices, triangles, colors, _ = ref.scene(100 + count, count)
    proj, eye = view(width, height, focal)
    color, alpha, depth, ids, status, total = both(vertices, triangles, proj, eye, width, height,
                                                   colors=colors, background=(0.25, 0.5, 0.75))
    assert alpha.any() and (ids[alpha == 0] == -1).all() and not depth[alpha == 0].any()
    np.testing.assert_array_equal(color[alpha == 0], np.float32([[0.25, 0.5, 0.75]])
                                  .repeat((alpha == 0).sum(), 0))


@pytest.mark.parametrize("batch", [64, 100, 4096])
def test_chunks_give_the_bits_of_one_launch(batch):
    """The boxes of 60 random triangles hold up to 400 pixels each and 8052 together, more than a
    chunk of 4096 and no multiple of any chunk: chunks start and end inside boxes."""
    vertices, triangles, colors, _ = ref.scene(0, 60)
    proj, eye = view(64, 48)
    whole = both(vertices, triangles, proj, eye, 64, 48, colors=colors)
    assert whole[5] > 4096 and whole[5] % batch != 0
    chunked = both(vertices, triangles, proj, eye, 64, 48, colors=colors, batch_size=batch)
    for a, b in zip(whole[:5], chunked[:5]):
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("boxes,total", [([(1, 1)], 1), ([(15, 17)], 255), ([(16, 16)], 256),
                                         ([(16, 16), (1, 1)], 257)])
def test_box_pixel_totals_round_one_block(boxes, total):
    """Triangles whose boxes hold ``total`` pixels together: one thread, one short of a block of
    256, one block, one block and a thread."""
    groups, x = [], 2.0
    for bw, bh in boxes:
        # corners strictly inside the outermost pixels' cells: the box is bw x bh
        groups.append(ref.flat([(x - 0.25, 1.75), (x + bw - 0.75, 1.8), (x + 0.1, bh + 1.25)]))
        x += bw + 2
    vertices = np.concatenate(groups)
    triangles = np.arange(len(vertices), dtype=np.int32).reshape(-1, 3)
    out = both(vertices, triangles, ref.PIXEL_PROJ, ref.ORIGIN, 40, 24, colors=ref.grey(vertices))
    assert out[5] == total and out[1].any()


def test_placements_get_their_status_and_stay_on_the_image():
    width, height = 64, 48
    vertices, triangles, expected = ref.placement_scene(width, height)
    color, alpha, depth, ids, status, _ = both(vertices, triangles, ref.PIXEL_PROJ, ref.ORIGIN,
                                               width, height, colors=ref.grey(vertices))
    np.testing.assert_array_equal(status, expected)
    drawn = set(ids[ids >= 0].tolist())
    # the four border crossers, the vertex-on-a-centre triangle and the first of the tied pair are
    # seen; the second of the pair and the sliver cover nothing that is theirs
    assert drawn == {0, 1, 2, 3, 13, 14}
    image = ids.reshape(height, width)
    assert (image[:, 0] == 0).any() and (image[:, -1] == 1).any()
    assert (image[0] == 2).any() and (image[-1] == 3).any()
    assert image[10, 30] == 13                       # the vertex (30, 10) itself
    assert alpha.sum() == (ids >= 0).sum() and np.isfinite(color).all() and np.isfinite(depth).all()


def test_shared_edges_and_coincident_triangles():
    vertices, triangles = ref.quad_scene()
    _, alpha, _, ids, _, _ = both(vertices, triangles, ref.PIXEL_PROJ, ref.ORIGIN, 16, 14,
                                  colors=ref.grey(vertices))
    assert alpha.sum() == 63 and (ids.reshape(14, 16)[[3, 6, 9], [2, 6, 10]] == 0).all()
    twice = np.array([[0, 1, 2], [0, 1, 2], [1, 2, 0]], np.int32)
    for order in ([0, 1, 2], [2, 1, 0]):
        _, alpha, _, ids, _, _ = both(vertices, twice[order], ref.PIXEL_PROJ, ref.ORIGIN, 16, 14,
                                      colors=ref.grey(vertices))
        assert set(ids[alpha > 0].tolist()) == {0}
    out = both(ref.SLIVER, np.array([[0, 1, 2]], np.int32), ref.PIXEL_PROJ, ref.ORIGIN, 32, 32,
               colors=ref.grey(ref.SLIVER))
    assert out[5] == 20 and not out[1].any()


@pytest.mark.parametrize("shape", [(1, 1, 3), (5, 4, 3), (7, 3, 4)])
def test_textures_with_uvs_outside_the_unit_square(shape):
    vertices, triangles, _, uvs = ref.scene(7, 20)
    assert (uvs < 0).any() and (uvs > 1).any()
    proj, eye = view(64, 48)
    texture = ref.texture(sum(shape), *shape)
    color, alpha, _, _, _, _ = both(vertices, triangles, proj, eye, 64, 48, uvs=uvs,
                                    texture=texture)
    print("covered %.3f" % alpha.mean())
    assert alpha.mean() > 0.1 and len(np.unique(color[alpha > 0], axis=0)) > (1 if shape[0] > 1 else 0)


def test_two_calls_and_a_permuted_order_give_the_same_image():
    vertices, triangles, colors, _ = ref.scene(0, 30)
    proj, eye = view(64, 48)
    first = device_raster(vertices, triangles, proj, eye, 64, 48, colors=colors)
    again = device_raster(vertices, triangles, proj, eye, 64, 48, colors=colors)
    for a, b in zip(first[:5], again[:5]):
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8))
    order = np.random.default_rng(1).permutation(len(triangles))
    moved = device_raster(vertices, triangles[order], proj, eye, 64, 48, colors=colors)
    for a, b in zip(first[:3], moved[:3]):
        np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
    # no two of these triangles tie in depth on a pixel (they are in general position), so the ids
    # follow the permutation everywhere
    hit = first[3] >= 0
    np.testing.assert_array_equal(order[moved[3][hit]], first[3][hit])
    np.testing.assert_array_equal(moved[4], first[4][order])


def test_render_mesh_is_the_kernels_and_supersample_one_is_the_plain_call():
    from fourier_feature_nets_amd import render_mesh, render_mesh_image
    from fourier_feature_nets_amd.cameras import eye_positions, projection_matrices
    cam = ref.camera(24, 20)
    vertices, triangles, colors, uvs = ref.scene(2, 10)
    texture = ref.texture(3, 5, 4, 3)
    proj, eye = projection_matrices([cam])[0], eye_positions([cam], (0.0, 0.0, 0.0))[0]
    want = ref.raster(vertices, triangles, proj, eye, 24, 20, colors=colors)
    out, ids, report = render_mesh(vertices, triangles, cam, colors=colors, return_ids=True)
    assert isinstance(out.color, np.ndarray)
    assert_same_bits(tuple(out) + (ids, want[4], int(want[5].sum())), want)
    assert report == {"drawn": 10, "behind": 0, "clipped": 0, "degenerate": 0, "off_image": 0,
                      "box_pixels": int(want[5].sum())}
    # row 0 of the texture is the top of the image: v = 0 reads the LAST row, as K22 is handed it
    want = ref.raster(vertices, triangles, proj, eye, 24, 20, uvs=uvs, texture=texture[::-1])
    tensors, _ = render_mesh(torch.from_numpy(vertices).cuda(), torch.from_numpy(triangles),
                             cam, uvs=torch.from_numpy(uvs), texture=torch.from_numpy(texture),
                             supersample=1, batch_size=100)
    assert tensors.color.is_cuda
    for g, w in zip(tensors, want[:3]):
        np.testing.assert_array_equal(g.cpu().numpy().view(np.uint32), w.view(np.uint32))
    image, alpha, depth = render_mesh_image(vertices, triangles, cam, uvs=uvs, texture=texture,
                                            include_depth=True)
    assert image.dtype == np.uint8 and image.shape == (20, 24, 3)
    np.testing.assert_array_equal(image, (want[0] * np.float32(255)).astype(np.uint8).reshape(20, 24, 3))
    np.testing.assert_array_equal(alpha, want[1].reshape(20, 24))
    np.testing.assert_array_equal(depth, want[2].reshape(20, 24))
    # supersample 3 is the 72 x 60 image of S P, averaged
    from fourier_feature_nets_amd import mesh
    fine = ref.raster(vertices, triangles, mesh.supersample_projection(cam, 3), eye, 72, 60,
                      colors=colors)
    mean = mesh.supersample_reduce(*[torch.from_numpy(x) for x in fine[:3]], 24, 20, 3)
    out, _ = render_mesh(vertices, triangles, cam, colors=colors, supersample=3)
    np.testing.assert_array_equal(out.alpha, mean[1].numpy())
    np.testing.assert_allclose(out.color, mean[0].numpy(), rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(out.depth, mean[2].numpy(), rtol=1e-6)


def test_clipped_triangles_are_counted_and_warned_about():
    from fourier_feature_nets_amd import mesh
    from fourier_feature_nets_amd.cameras import projection_matrices
    vertices, triangles, colors, _ = ref.scene(0, 30)
    cam = ref.camera(64, 48, distance=0.3)            # inside the scene: triangles cross w = 0
    status = ref.setup(vertices, triangles, projection_matrices([cam])[0], 64, 48)["status"]
    tally = np.bincount(status, minlength=5).tolist()
    assert tally[ref.CLIPPED] > 0 and tally[ref.BEHIND] > 0
    mesh._warned_clipped = False
    with pytest.warns(UserWarning, match="no near-plane clipping"):
        _, report = mesh.render_mesh(vertices, triangles, cam, colors=colors)
    assert [report[k] for k in ("drawn", "behind", "clipped", "degenerate", "off_image")] == tally


@pytest.mark.parametrize("name,offset", [("cuboid", (1.0, 0.25, -0.5)), ("touching", (0.4, 0.4, 0.6))])
def test_a_block_mesh_looks_like_the_first_hit_walk_of_its_tree(name, offset):
    """``extract_mesh(placement="corners")`` of a tree of opaque leaves is the tree's block surface;
    K31's picture of it and ``OcTree.render`` of the tree from the same camera show the same
    silhouette and the same distances.

    alpha: equal on every decided pixel -- one whose centre is at least 1/128 px from every
    float64-projected edge of the mesh (the snap to 1/256 px moves an edge by less); at most 2 % of
    the pixels may be undecided, a condition of the test.

    depth: both are the distance from the eye to a cube face along the pixel's ray.  K31's is that
    of the unsnapped face at a screen point within 1/500 px of the centre in x and y
    (test_mesh_raster_cpu.py derives this), so it lies between the float64 plane distances at the
    four corners of that box, [low, high], up to 1e-5 relative for its ~20 f32 roundings.  The
    walk's t = (plane - o) / d is three roundings on lattice planes that are exact, with an f32 unit
    direction off by at most 2 ulp per component: below 1e-5 relative as well.  Budget:
    (high - low) + 2e-5 t.  Worst observed share of the budget: 0.41 (cuboid, 612 pixels) and 0.34
    (touching, 456 pixels); the test prints it."""
    from tests.octree_mesh_cases import case
    from fourier_feature_nets_amd import render_mesh
    from fourier_feature_nets_amd.octree import OcTree
    c = case(name)
    tree = OcTree(c.scale, c.nodes, c.leaves, c.leaf_data, c.sh_degree)
    width, height = 64, 48
    cam = ref.camera(width, height, distance=4.5 if name == "cuboid" else 3.0)
    surface = tree.extract_mesh(placement="corners", center=offset)
    out, ids, report = render_mesh(surface.vertices, surface.triangles, cam, colors=surface.colors,
                                   return_ids=True)
    assert report["clipped"] == report["behind"] == 0
    py, px = np.divmod(np.arange(width * height), width)
    rays = cam.raycast(np.stack([px, py], -1).astype(np.float32))
    walk = tree.render(rays.origin - np.float32(offset), rays.direction)
    near_edge = ref.edge_distance64(surface.vertices, surface.triangles, cam.intrinsics,
                                    cam.extrinsics, width, height) < 1 / 128
    print("undecided %.4f covered %.4f" % (near_edge.mean(), out.alpha.mean()))
    assert near_edge.mean() <= 0.02 and out.alpha.mean() >= 0.05
    decided = ~near_edge
    np.testing.assert_array_equal(out.alpha[decided], walk.alpha[decided])
    hit = np.flatnonzero(decided & (out.alpha > 0))
    snap = 1 / 500
    corners = [ref.plane_distance64(surface.vertices, surface.triangles, ids[hit], cam.intrinsics,
                                    cam.extrinsics, px[hit] + dx, py[hit] + dy)
               for dx in (-snap, snap) for dy in (-snap, snap)]
    budget = (np.max(corners, 0) - np.min(corners, 0)) + 2e-5 * walk.depth[hit]
    share = np.abs(out.depth[hit].astype(np.float64) - walk.depth[hit]) / budget
    print("worst share of the depth budget %.3f over %d pixels" % (share.max(), len(hit)))
    assert share.max() <= 1.0


def write_textured_obj(path, texture_path, vertices, triangles, uvs, texture):
    from PIL import Image
    Image.fromarray(texture).save(texture_path)
    lines = ["v %.9g %.9g %.9g" % tuple(v) for v in vertices.tolist()]
    lines += ["vt %.9g %.9g" % tuple(t) for t in uvs.tolist()]
    lines += ["f " + " ".join("%d/%d" % (i + 1, i + 1) for i in face) for face in triangles.tolist()]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def run_script(name, *args):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", name)] + list(args),
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    return out.stdout


def test_the_scripts_draw_the_torus_in_fresh_processes(tmp_path):
    """make_mesh_npz.py --render mesh writes the frames render_mesh_image gives, and
    render_mesh.py, given the same torus as an OBJ, draws the held-out frame again."""
    import fourier_feature_nets_amd as ffn
    from bench import synthetic_rig
    data = str(tmp_path / "torus.npz")
    run_script("make_mesh_npz.py", data, "--render", "mesh", "--size", "32", "--cameras", "3")
    vertices, triangles, uvs, texture = ffn.procedural_torus()
    points = ffn.normalize_points(vertices)
    intr, poses = synthetic_rig(3, 32)
    order = torch.randperm(3, generator=torch.Generator().manual_seed(0)).numpy()
    with np.load(data) as blob:
        images, extrinsics, splits = blob["images"], blob["extrinsics"], blob["split_counts"]
    assert images.shape == (3, 32, 32, 4) and images.dtype == np.uint8
    assert splits.tolist() == [1, 1, 1]
    np.testing.assert_array_equal(extrinsics, np.stack(poses)[order])
    for slot, index in enumerate(order):
        cam = ffn.CameraInfo.create("c", ffn.Resolution(32, 32), intr, poses[index])
        color, alpha, _ = ffn.render_mesh_image(points, triangles, cam, uvs=uvs, texture=texture,
                                                include_depth=True)
        np.testing.assert_array_equal(images[slot, ..., :3], color)
        np.testing.assert_array_equal(images[slot, ..., 3], np.rint(255 * alpha).astype(np.uint8))
    assert 0.05 < (images[..., 3] > 0).mean() < 0.9

    smooth = str(tmp_path / "smooth.npz")
    run_script("make_mesh_npz.py", smooth, "--render", "mesh", "--supersample", "2", "--size", "32",
               "--cameras", "3")
    with np.load(smooth) as blob:
        partial = blob["images"][..., 3]
    assert set(np.unique(partial).tolist()) <= {0, 64, 128, 191, 255} and (partial == 128).any()

    obj, png, frames = str(tmp_path / "torus.obj"), str(tmp_path / "torus.png"), str(tmp_path / "out")
    write_textured_obj(obj, png, vertices, triangles, uvs, texture)
    text = run_script("render_mesh.py", obj, data, frames, "--normalize", "--texture", png)
    assert "camera 0 (" in text and "mean psnr over 1 cameras:" in text
    assert float(text.strip().rsplit(" ", 1)[-1]) > 40.0
    from PIL import Image
    assert np.asarray(Image.open(os.path.join(frames, "frame_00000.png"))).shape == (32, 32, 3)


def test_render_octree_is_still_the_default_and_writes_the_recorded_bytes(tmp_path):
    """``--render octree`` and no ``--render`` at all write the same arrays, and they hash to what
    the script wrote before it had the option (tests/golden/make_mesh_npz_octree.json)."""
    digests = []
    for extra in ([], ["--render", "octree"]):
        path = str(tmp_path / ("o%d.npz" % len(extra)))
        run_script("make_mesh_npz.py", path, "--size", "32", "--cameras", "3", "--voxel-depth", "6",
                   *extra)
        sha = hashlib.sha256()
        with np.load(path) as blob:
            assert sorted(blob.files) == ["bounds", "extrinsics", "images", "intrinsics",
                                          "split_counts"]
            for key in sorted(blob.files):
                sha.update(key.encode() + str(blob[key].dtype).encode() + str(blob[key].shape).encode())
                sha.update(np.ascontiguousarray(blob[key]).tobytes())
        digests.append(sha.hexdigest())
    print("sha256", digests[0])
    with open(GOLDEN) as f:
        assert digests == [json.load(f)["sha256"]] * 2

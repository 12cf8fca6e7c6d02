"""The numpy restatement of K33 (csrc/mesh_texture.hip), on top of tests/mesh_raster_reference.py.

``taps``, ``gather`` and ``grad`` follow the contract of include/ffn_hip.h operation for operation:
every value a numpy float32, every product and add one rounded f32 operation in the header's order,
the rows of a texel found by ``searchsorted`` in the stably sorted tap slots and added in that order
from 0.0f.  They have to give the kernels' bits.  ``sort_taps`` is the stable argsort
``mesh.mesh_texture_taps`` makes; ``texture_from_images`` restates ``texture_mesh_from_images`` and
``unwrap`` restates ``unwrap_mesh`` triangle by triangle, in plain loops.

``gamma`` and the ``*_budget`` functions are the error budgets of the float64 identities the tests
hold K33 to, counted from the f32 roundings of the contract (derived where they stand).

Nothing here needs a GPU.
"""

import numpy as np

from tests import mesh_raster_reference as R

F32 = np.float32
U = 2.0 ** -24                      # the unit roundoff of f32


# ------------------------------------------------------------------------------- the kernels
def lookup_taps(u, v, tex_height, tex_width):
    """The index and weight arithmetic of K22's lookup -> (texel (n,4) int64, weight (n,4) f32) in
    the order 00, 01, 10, 11."""
    with np.errstate(all="ignore"):
        col, row = u * F32(tex_width), v * F32(tex_height)
        fj, fi = np.floor(col), np.floor(row)
        dj, di = col - fj, row - fi

        def clamp(index, last):
            return np.fmin(np.fmax(index, F32(0.0)), F32(last)).astype(np.int64)

        j0, j1 = clamp(fj, tex_width - 1), clamp(fj + F32(1.0), tex_width - 1)
        i0, i1 = clamp(fi, tex_height - 1), clamp(fi + F32(1.0), tex_height - 1)
        one = F32(1.0)
        weight = np.stack([(one - di) * (one - dj), (one - di) * dj, di * (one - dj), di * dj], -1)
    texel = np.stack([i0 * tex_width + j0, i0 * tex_width + j1, i1 * tex_width + j0,
                      i1 * tex_width + j1], -1)
    return texel, weight.astype(F32)


def taps(state, ids, uvs, tex_height, tex_width, width):
    """K33a -> (tap_texel (P,4) int32, tap_weight (P,4) f32).  ``state`` from ``R.setup`` (its
    ``ids`` are the clamped vertex ids); ``ids`` (P,) int32 of K31c, or foreign."""
    uvs = np.asarray(uvs, dtype=F32)
    ids = np.asarray(ids)
    num = len(ids)
    tap_texel = np.full((num, 4), -1, dtype=np.int32)
    tap_weight = np.zeros((num, 4), dtype=F32)
    hit = np.flatnonzero((ids >= 0) & (ids < len(state["ids"])))
    if len(hit) == 0:
        return tap_texel, tap_weight
    f = ids[hit].astype(np.int64)
    _, q, depth_w = R.terms(state["X"][f], state["Y"][f], state["w"][f], hit % width, hit // width)
    corner = state["ids"][f]
    with np.errstate(all="ignore"):
        b = [q[i] * depth_w for i in range(3)]
        u, v = [(uvs[corner[:, 0], j] * b[0] + uvs[corner[:, 1], j] * b[1])
                + uvs[corner[:, 2], j] * b[2] for j in range(2)]
    texel, weight = lookup_taps(u, v, tex_height, tex_width)
    tap_texel[hit] = texel
    tap_weight[hit] = weight
    return tap_texel, tap_weight


def gather(tap_texel, tap_weight, texture, background=(0, 0, 0)):
    """K33b -> (color (P,3), alpha (P,)) f32.  ``texture`` (T,3) f32."""
    texture = np.asarray(texture, dtype=F32).reshape(-1, 3)
    num = len(tap_texel)
    color = np.tile(np.asarray(background, dtype=F32), (num, 1))
    alpha = np.zeros(num, dtype=F32)
    hit = np.flatnonzero(tap_texel[:, 0] >= 0)
    texel, weight = tap_texel[hit].astype(np.int64), tap_weight[hit]
    inside = (texel >= 0) & (texel < len(texture))
    with np.errstate(all="ignore"):
        term = [np.where(inside[:, k, None],
                         weight[:, k, None] * texture[np.where(inside[:, k], texel[:, k], 0)],
                         F32(0.0)) for k in range(4)]
        color[hit] = ((term[0] + term[1]) + term[2]) + term[3]
    alpha[hit] = 1.0
    return color, alpha


def sort_taps(tap_texel):
    """-> (sorted_texels (4P,) int32, tap_order (4P,) int32): the slots 4 p + k stably sorted."""
    flat = np.asarray(tap_texel, dtype=np.int32).reshape(-1)
    order = np.argsort(flat, kind="stable")
    return flat[order], order.astype(np.int32)


def rows_of(sorted_texels, num_texels):
    """The first and one-past-last slot of every texel's row -> (begin (T,), end (T,))."""
    texels = np.arange(num_texels)
    return (np.searchsorted(sorted_texels, texels, side="left"),
            np.searchsorted(sorted_texels, texels + 1, side="left"))


def grad(sorted_texels, tap_order, tap_weight, d_color, num_texels, grad=None, weight=None,
         accumulate=False):
    """K33c -> (grad (T,3), weight (T,)) f32; with ``accumulate`` ``out = out + value``."""
    d_color = np.asarray(d_color, dtype=F32)
    flat_weight = np.asarray(tap_weight, dtype=F32).reshape(-1)
    slots = len(flat_weight)
    g = np.zeros((num_texels, 3), dtype=F32)
    w = np.zeros(num_texels, dtype=F32)
    begin, end = rows_of(sorted_texels, num_texels)
    with np.errstate(all="ignore"):
        for t in range(num_texels):
            for s in tap_order[begin[t]:end[t]]:
                if not 0 <= s < slots:
                    continue
                value = flat_weight[s]
                if not value > 0:
                    continue
                g[t] = g[t] + value * d_color[s // 4]
                w[t] = w[t] + value
        if accumulate:
            return grad + g, weight + w
    return g, w


def camera_taps(vertices, triangles, uvs, proj, width, height, size, hidden=None):
    """``mesh.mesh_texture_taps`` -> (tap_texel, tap_weight, sorted_texels, tap_order, state, ids)."""
    from tests import mesh_raster_grad_reference as Rg
    state, ids = Rg.raster_ids(vertices, triangles, proj, width, height)
    if hidden is not None:
        ids = np.where(hidden, -1, ids).astype(np.int32)
    tap_texel, tap_weight = taps(state, ids, uvs, size[0], size[1], width)
    return (tap_texel, tap_weight) + sort_taps(tap_texel) + (state, ids)


def texture_from_images(vertices, triangles, uvs, projections, images, size, texture=None,
                        alpha_threshold=0.5):
    """``texture_mesh_from_images`` on (C,H,W,3 or 4) uint8 images and their (3,4) projections ->
    (texture (H,W,3), weights (H,W)) f32."""
    height, width = images.shape[1:3]
    num_texels = size[0] * size[1]
    alpha_u8 = min(max(int(np.ceil(float(alpha_threshold) * 255)), 1), 255)
    total, weights = None, None
    for proj, frame in zip(projections, images):
        hidden = frame[..., 3].reshape(-1) < alpha_u8 if frame.shape[-1] == 4 else None
        _, tap_weight, sorted_texels, order, _, _ = camera_taps(vertices, triangles, uvs, proj,
                                                                width, height, size, hidden)
        rgb = (frame[..., :3].astype(F32) / 255).reshape(-1, 3)
        total, weights = grad(sorted_texels, order, tap_weight, rgb, num_texels, total, weights,
                              accumulate=total is not None)
    out = np.full((num_texels, 3), 0.5, dtype=F32) if texture is None else \
        np.array(texture, dtype=F32).reshape(-1, 3)
    seen = weights > 0
    out[seen] = total[seen] / weights[seen][:, None]
    return out.reshape(tuple(size) + (3,)), weights.reshape(tuple(size))


# ------------------------------------------------------------------------------- the atlas
def atlas_size(num_tiles, tile):
    side = 1
    while side < tile:
        side *= 2
    width = height = side
    while (width // tile) * (height // tile) < num_tiles:
        if width == height:
            width *= 2
        else:
            height *= 2
    return height, width


def unwrap(triangles, tile):
    """``unwrap_mesh`` triangle by triangle -> (triangles' (F,3), texel coordinates (V',2) float64,
    vertex_map (V',), tile_of (F,), (height, width))."""
    triangles = [tuple(int(i) for i in t) for t in np.asarray(triangles)]
    lo, hi = 0.5, tile - 1.5
    new_triangles, local, vertex_map, tile_of, tiles = [], [], [], [], 0
    f = 0
    while f < len(triangles):
        a = triangles[f]
        b = triangles[f + 1] if f % 2 == 0 and f + 1 < len(triangles) else None
        pair = (b is not None and len(set(a)) == 3 and len(set(b)) == 3
                and len(set(a) & set(b)) == 2)
        first = len(vertex_map)
        vertex_map.extend(a)
        if not pair:
            local.extend([(lo, lo), (hi, lo), (lo, hi)])
            new_triangles.append((first, first + 1, first + 2))
            tile_of.append(tiles)
            f += 1
        else:
            alone = [i for i in range(3) if a[i] not in b][0]
            spot = {(alone + 0) % 3: (lo, lo), (alone + 1) % 3: (hi, lo), (alone + 2) % 3: (lo, hi)}
            local.extend([spot[0], spot[1], spot[2]])
            new_triangles.append((first, first + 1, first + 2))
            other = [j for j in range(3) if b[j] not in a][0]
            vertex_map.append(b[other])
            local.append((hi, hi))
            new_triangles.append(tuple(first + 3 if j == other else first + a.index(b[j])
                                       for j in range(3)))
            tile_of.extend([tiles, tiles])
            f += 2
        tiles += 1
    height, width = atlas_size(tiles, tile)
    per_row = width // tile
    texel = np.zeros((len(vertex_map), 2))
    for face, number in zip(new_triangles, tile_of):
        for vertex in face:
            texel[vertex] = (local[vertex][0] + tile * (number % per_row),
                             local[vertex][1] + tile * (number // per_row))
    return (np.array(new_triangles, np.int32), texel, np.array(vertex_map, np.int32),
            np.array(tile_of), (height, width))


# ------------------------------------------------------------------------------- budgets
def gamma(n):
    """Higham's gamma_n = n u / (1 - n u): the relative error n f32 roundings leave at most."""
    return n * U / (1.0 - n * U)


def longest_row(sorted_texels, num_texels):
    begin, end = rows_of(sorted_texels, num_texels)
    return int((end - begin).max())


def partition_budget():
    """|w00 + w01 + w10 + w11 - 1| in float64 at a covered pixel with finite UVs.  di = row -
    floor(row) and dj are exact f32 subtractions in [0, 1).  A weight rounds 1 - di, 1 - dj and
    their product: it is within gamma_3 of the real (1 - di)(1 - dj), and so are the other three of
    theirs.  The four real products are >= 0 and sum to 1 exactly: gamma_3, and 1e-15 for the
    float64 sum."""
    return gamma(3) + 1e-15


def weight_budget(covered, depth):
    """|sum_t weight_t - covered pixels|.  A pixel's four weights are within gamma_3 of reals that
    sum to 1 (``partition_budget``); every weight then passes at most ``depth`` f32 adds (the
    longest texel row; a skipped zero weight adds nothing): gamma_{3 + depth} per pixel."""
    return (gamma(3 + depth) + 1e-13) * covered


def adjoint_budget(tap_texel, tap_weight, texture, g, depth):
    """|sum_p color[p] . g[p] - sum_t texture[t] . grad[t]| is at most this.  Both sides are sums of
    the reals w t g with the same f32 w.  On the left K33b rounds the product w t and at most three
    adds: gamma_4 of the term's size.  On the right K33c rounds the product w g and every add the
    term passes after it, at most ``depth``, the longest texel row: gamma_{1 + depth}.  So the two
    differ by at most gamma_{4 + depth} A, A = sum |w t g| in float64; the float64 sums add
    1e-13 A."""
    texture = np.asarray(texture, dtype=np.float64).reshape(-1, 3)
    hit = np.flatnonzero(tap_texel[:, 0] >= 0)
    size = 0.0
    for k in range(4):
        size += float((tap_weight[hit, k].astype(np.float64)[:, None]
                       * np.abs(texture[tap_texel[hit, k]])
                       * np.abs(np.asarray(g, dtype=np.float64)[hit])).sum())
    return (gamma(4 + depth) + 1e-13) * size


def splat_budget(depth, constant):
    """|sum_t / weight_t - c| per channel when every image holds the one colour c > 0.  ``depth``
    is the most adds a term passes: the longest texel row of any camera plus the number of cameras
    (one accumulate add each).  The numerator adds w c with one product and ``depth`` adds, the
    denominator w with ``depth`` adds, all terms >= 0, and the quotient rounds once:
    gamma_{2 + 2 depth} of c."""
    return gamma(2 + 2 * depth) * np.abs(np.asarray(constant, dtype=np.float64))


def quantisation_budget():
    """|K31c's colour through ``texture_to_uint8`` - K33b's colour| for texels in [0, 1].  The byte
    q = floor(fl(fl(255 x) + 0.5)): the two roundings move the argument by at most 2 u 256, so
    |q / 255 - x| <= 0.5 / 255 + 512 u / 255 < 0.5 / 255 + 3 u.  The weights are >= 0 and sum to at
    most 1 + gamma_3, so the real blends differ by (0.5 / 255 + 3 u)(1 + gamma_3).  K33b rounds a
    product and three adds (gamma_4 of at most 1 + gamma_3), K31c a product, three adds and the
    division (gamma_5 of the same): in all less than 0.5 / 255 + gamma_14."""
    return 0.5 / 255 + gamma(14)

"""Hand-worked leaf lists for the K16 merge passes, shared by the CPU tests (against the numpy
restatement) and the GPU tests (against the kernels)."""

import numpy as np

F = np.float32
ROW = F([0.25, 0.5, 0.75, 4.0])
EXACT_TOL = F(7 * 2.0 ** -10)


def _constant(codes):
    return np.repeat(ROW[None, :], len(codes), 0).astype(F)


def _one_off(sigma):
    """Eight siblings of value 1, child 7 with density ``sigma``."""
    data = np.ones((8, 4), F)
    data[7, 3] = sigma
    return data


def hand_cases():
    """name -> dict(depth, codes, data, tol=(rgb, sigma), leaves, nodes[, mean]): finest-level
    codes and their data in, the expected sorted ids out.

    * two_level: octant 0 full and constant, and the two far corners of octant 7: the geometry of
      ``octree_walk_helpers.two_level_tree``.
    * constant: the full 4 x 4 x 4 grid, one value: 64 -> 8 -> the root leaf.
    * seven: child 7 of the group is missing; nothing merges whatever the tolerance.
    * exact: child 7 has density 1 + 2^-7: sum 8 + 2^-7, mean 1 + 2^-10, every step exact in f32;
      child 7 is 7 * 2^-10 off, the others 2^-10.  With sigma_tol = 7 * 2^-10 the group merges.
    * below: the same data, the tolerance one f32 below: no merge.
    * above: the tolerance of ``exact``, child 7 one f32 further away (1 + 2^-7 + 2^-23: the sum
      rounds to the same 8 + 2^-7, so the mean stays and the offset is 7 * 2^-10 + 2^-23, which is
      an f32): no merge.
    * nan: a NaN colour in an otherwise constant group: no merge.
    * mixed: depth 4; cells 0 and 2 .. 7 of the first octant's level-2 children are full, cell 1
      holds one finest leaf.  After the first pass the eight consecutive entries from cell 0 on
      are children 0 .. 7 of one parent with a level-2 head and tail, but entry 1 is one level
      deeper: no second merge."""
    quarter = np.arange(8)
    mixed = np.concatenate([np.arange(0, 9), np.arange(16, 64)])
    nan = _constant(quarter)
    nan[3, 1] = np.nan
    sigma = F(1 + 2.0 ** -7)
    return {
        "two_level": dict(depth=3, codes=np.concatenate([quarter, [56, 63]]),
                          data=np.concatenate([_constant(quarter), F([[0, 0, 1, 9], [1, 0, 0, 7]])]),
                          tol=(0.0, 0.0), leaves=[1, 65, 72], nodes=[0, 8]),
        "constant": dict(depth=3, codes=np.arange(64), data=_constant(np.arange(64)),
                         tol=(0.0, 0.0), leaves=[0], nodes=[], mean=ROW),
        "seven": dict(depth=3, codes=np.arange(7), data=_constant(np.arange(7)), tol=(1e9, 1e9),
                      leaves=list(range(9, 16)), nodes=[0, 1]),
        "exact": dict(depth=2, codes=quarter, data=_one_off(sigma), tol=(0.0, float(EXACT_TOL)),
                      leaves=[0], nodes=[], mean=F([1, 1, 1, 1 + 2.0 ** -10])),
        "below": dict(depth=2, codes=quarter, data=_one_off(sigma),
                      tol=(0.0, float(np.nextafter(EXACT_TOL, F(0)))),
                      leaves=list(range(1, 9)), nodes=[0]),
        "above": dict(depth=2, codes=quarter, data=_one_off(np.nextafter(sigma, F(2))),
                      tol=(0.0, float(EXACT_TOL)), leaves=list(range(1, 9)), nodes=[0]),
        "nan": dict(depth=2, codes=quarter, data=nan, tol=(1e9, 1e9), leaves=list(range(1, 9)),
                    nodes=[0]),
        "mixed": dict(depth=4, codes=mixed, data=_constant(mixed), tol=(0.0, 0.0),
                      leaves=[9, 11, 12, 13, 14, 15, 16, 81], nodes=[0, 1, 10]),
    }


def blob_field(depth=5, seed=11):
    """All 8^(depth-1) cells in code order, activated values: a few constant-valued axis-aligned
    blocks (which merge, at several levels), noise elsewhere (which does not), and a share of
    empty cells.  -> data (N,4) f32."""
    rng = np.random.default_rng(seed)
    side = 2 ** (depth - 1)
    grid = rng.random((side, side, side, 4), dtype=F)
    grid[..., 3] *= F(8)
    grid[rng.random((side, side, side)) < 0.3, 3] = 0            # empty cells
    grid[0:8, 0:8, 0:8] = F([0.125, 0.25, 0.375, 5.0])                # a whole level-1 octant
    grid[8:12, 4:8, 12:16] = F([0.9, 0.8, 0.7, 3.0])             # a level-2 cell
    grid[12:14, 2:4, 6:8] = F([0.5, 0.5, 0.5, 2.0])              # a level-3 cell
    grid[9:13, 9:13, 9:13] = F([0.4, 0.6, 0.2, 6.0])             # aligned to nothing coarse
    grid[10, 10, 10, 0] += F(0.001)                              # within a loose tolerance
    # code order: 3 bits per level, root first, 4 [x] + 2 [y] + [z]
    ix, iy, iz = np.meshgrid(np.arange(side), np.arange(side), np.arange(side), indexing="ij")
    code = np.zeros_like(ix)
    for level in range(depth - 1):
        bit = depth - 2 - level
        code = (code << 3) | (((ix >> bit) & 1) << 2) | (((iy >> bit) & 1) << 1) | ((iz >> bit) & 1)
    data = np.empty((side ** 3, 4), F)
    data[code.reshape(-1)] = grid.reshape(-1, 4)
    return data

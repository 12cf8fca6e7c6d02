"""Float64 reference of the fused inference render (csrc/mlp.hip ``render_fused_kernel``, entry
``ffn_render_fused_fwd``, host side ``MlpProgram.render``) with the error budget of K5
(tests/composite_reference.py), and the host image of its launch arithmetic.

Without an occupancy grid the kernel composites a ray's S samples exactly like K5, and
``render_reference(logits, t)`` is ``composite_forward``.  With a grid the wave first compacts the
ray's occupied samples (ballot / popcount ranks into a slot list) and then evaluates this sequence,
which ``render_reference(logits, t, keep)`` follows step by step:

* only the m kept samples enter, in ray order: slot k holds the k-th kept position ``j_k``;
* each has its OWN ``delta = fl(t[j + 1] - t[j])`` from the full row, not the distance to the next
  kept sample: the skipped samples between them have ``sigma = 0``, weight 0 and transmittance
  factor ``min(1, 1 + 1e-10) = 1``, so leaving them out changes nothing else;
* a sample is "last" (``delta = 1e10``, excluded from alpha and from the depth pick) only if it is
  the ray's last POSITION ``j == S - 1``, wherever it lands in the slot list;
* rows of 64 slots run over the compacted order: ``ceil(m / 64)`` rows, so the running sums are
  ``rows + 6`` levels deep, with rows counted on m and not on S;
* the depth is ``t[j]`` of the picked sample's POSITION; a ray without a kept inner sample (m = 0
  among them) reports ``t[S - 1]``, colour 0 and alpha 0.

The budget counts only the operations performed on the m kept samples: the padding slots up to
the row end are inactive lanes, which the kernel gives ``alpha = 0`` and ``tau = 1`` without any
arithmetic.

Teeth (``TEETH``): references with one deliberate change that a correct kernel's output must fail
somewhere in the data.

``keep_of`` is the float64 image of ``occupied_at`` (csrc/occupancy_map.h), ``render_plan`` the host
image of the launch arithmetic of ``ffn_render_fused_fwd``.
"""

import torch

from tests import composite_reference as cr
from tests.composite_reference import KAPPA, U, V, WAVE, Report  # noqa: F401  (re-exported)

TEETH = ("next_kept_delta", "last_kept_is_last", "mask_ignored", "slot_depth", "dropped_tail")
TEETH_DOC = dict(next_kept_delta="delta = t of the next kept sample - t[j] instead of t[j + 1] - t[j]",
                 last_kept_is_last="the final kept sample gets delta 1e10 and leaves alpha and depth",
                 mask_ignored="skipped samples contribute (every sample evaluated)",
                 slot_depth="depth = t[slot] of the pick instead of t[position]",
                 dropped_tail="the last m mod 32 kept samples are lost")
NARROW_TEAMS, WIDE_TEAMS = 4, 2      # rays a workgroup renders at a time (waves / pairs of waves)


def new_report():
    return Report(KAPPA, TEETH_DOC)


# ------------------------------------------------------------------------------------- render
def render_reference(logits, t, keep=None, variant=None):
    """The fused render of (R, S, 4) f32 logits and (R, S) f32 t (any device), ``keep`` (R, S) bool =
    the samples in occupied cells (None: no grid, every sample).  -> dict of V ``colour`` (R, 3),
    ``alpha`` (R), ``weights`` (R, S) by ray position (0 where skipped) and the bool ``candidates``
    (R, S): the POSITIONS whose t the kernel may report as depth; ``m`` (R) kept samples."""
    assert variant is None or variant in TEETH, variant
    lg, tt = logits.double(), t.double()
    R, S = tt.shape
    dev = tt.device
    pos = torch.arange(S, device=dev)[None].expand(R, S)
    if keep is None or variant == "mask_ignored":
        keep = torch.ones((R, S), dtype=torch.bool, device=dev)
    keep = keep.to(dev)
    kept = keep.sum(1)
    m = kept - kept % 32 if variant == "dropped_tail" else kept
    # slot k <- the k-th kept position (distinct keys: a stable order)
    order = torch.where(keep, pos, pos + S).argsort(1)
    active = pos < m[:, None]
    lgc = torch.gather(lg, 1, order[..., None].expand(R, S, 4))
    lgc = torch.where(active[..., None], lgc, 0.0)
    last = active & (order == S - 1)
    if variant == "last_kept_is_last":
        last = last | (active & (pos == m[:, None] - 1))
    succ = (order + 1).clamp_max(S - 1)
    if variant == "next_kept_delta":
        nxt = torch.cat([order[:, 1:], order[:, -1:]], 1)
        succ = torch.where(pos + 1 < kept[:, None], nxt, succ)
    d = tt.gather(1, succ) - tt.gather(1, order)
    zero = torch.zeros_like(d)
    own = active & ~last
    dl = V.rounded(d, zero)
    delta = V(torch.where(last, 1e10, torch.where(own, dl.v, 0.0)), torch.where(own, dl.b, 0.0))
    rgb = [cr.sigmoid(V(lgc[..., c])) for c in range(3)]
    sg = cr.softplus(lgc[..., 3])
    sigma = V(torch.where(active, sg.v, 0.0), torch.where(active, sg.b, 0.0))
    wt = cr.weights(sigma, delta)
    # an inactive lane's weight is 0 without arithmetic (its tau is 1 exactly: T is unaffected)
    w = V(torch.where(active, wt["w"].v, 0.0), torch.where(active, wt["w"].b, 0.0))
    depth = ((m + 63) // 64 + WAVE).double()
    colour = V.stack([cr.vsum(w.exact_mul(c), 1, depth) for c in rgb], 1)
    w_in = V(torch.where(own, w.v, 0.0), torch.where(own, w.b, 0.0))
    alpha = cr.vsum(w_in, 1, depth)
    by_pos = lambda x: torch.zeros_like(x).scatter(1, order, x)        # noqa: E731
    w_pos = V(by_pos(w.v), by_pos(w.b))
    if variant == "slot_depth":          # the pick's slot number read as a position
        cand = cr.depth_candidates(dict(wt=dict(w=w), alpha=alpha), own)
    else:
        cand = cr.depth_candidates(dict(wt=dict(w=w_pos), alpha=alpha), by_pos(own))
    return dict(colour=colour, alpha=alpha, weights=w_pos, candidates=cand, m=kept, keep=keep,
                variant=variant)


def masked_reference(logits, t, keep):
    """The same quantity evaluated the other way: the full-length K5 reference with ``sigma := 0``
    exactly at the skipped samples."""
    lg, tt = logits.double(), t.double()
    R, S = tt.shape
    keep = keep.to(tt.device)
    rgb = [cr.sigmoid(V(lg[..., c])) for c in range(3)]
    sg = cr.softplus(lg[..., 3])
    sigma = V(torch.where(keep, sg.v, 0.0), torch.where(keep, sg.b, 0.0))
    wt = cr.weights(sigma, cr._delta(tt, None))
    w = wt["w"]
    depth = cr.rows_of(S) + WAVE
    colour = V.stack([cr.vsum(w.exact_mul(c), 1, depth) for c in rgb], 1)
    inner = torch.arange(S, device=tt.device)[None] < S - 1
    alpha = cr.vsum(V(torch.where(inner, w.v, 0.0), torch.where(inner, w.b, 0.0)), 1, depth)
    cand = cr.depth_candidates(dict(wt=dict(w=w), alpha=alpha))
    return dict(colour=colour, alpha=alpha, weights=w, candidates=cand)


def depth_ok(candidates, t, depth):
    """(R) bool: the reported depth is the t of a candidate position, bit for bit."""
    return (candidates & (t.double().to(depth.device) == depth.double()[:, None])).any(1)


def check_depth(rep, key, ref, t, depth):
    ok = depth_ok(ref["candidates"], t, depth)
    if not bool(ok.all()):
        bad = int((~ok).nonzero()[0, 0])
        rep.failures.append("depth %s: %d of %d rays report a t no candidate sample has, first ray %d: %r (m = %d)"
                            % (key, int((~ok).sum()), ok.numel(), bad, float(depth[bad]), int(ref["m"][bad])))


def measure_render(rep, bites, key, logits, t, keep, colour, alpha, depth, teeth=TEETH):
    """Holds the kernel's colour / alpha (None: not asked for) to ``KAPPA`` and its depth to the
    candidates; ``bites[tooth]`` = the first case ``key`` in which the kernel's output fails the
    changed reference (colour or alpha beyond the bound of an element the change moves beyond it, or
    a depth no changed candidate has).  -> the reference."""
    ref = render_reference(logits, t, keep)
    if colour is not None:
        rep.compare("colour", key, colour, ref["colour"])
    if alpha is not None:
        rep.compare("alpha", key, alpha, ref["alpha"])
    if depth is not None:
        check_depth(rep, key, ref, t, depth)
    for name in teeth:
        alt = render_reference(logits, t, keep, name)
        one = Report(KAPPA, TEETH_DOC)
        if colour is not None:
            one.tooth("colour", name, colour, ref["colour"], alt["colour"])
        if alpha is not None:
            one.tooth("alpha", name, alpha, ref["alpha"], alt["alpha"])
        bit = any(v["exceeds"] and v["ratio"] > 1.0 for v in one.teeth.values())
        if depth is not None and not bool(depth_ok(alt["candidates"], t, depth).all()):
            bit = True
        if bit:
            bites.setdefault(name, key)
    return ref


# ------------------------------------------------------------------------------------- occupancy
def keep_of(positions, grid):
    """``occupied_at`` of (N, 3) f32 positions in ``grid`` (``bits`` int32 words, ``box_min``,
    ``box_size``, ``resolution``; an ``OccupancyGrid`` or anything shaped like one) -> (keep (N) bool,
    dist (N, 3) float64).  The grid coordinate is ``fl(fl(x - min) * inv)`` with
    ``inv = fl(G / size)``, clamped to [0, G - 1] and truncated; cell (ix, iy, iz) is bit ``cell & 31``
    of word ``cell >> 5``, ``cell = (iz G + iy) G + ix`` (x fastest).  A NaN coordinate counts as
    occupied.  ``dist``: how far each (unclamped) coordinate lies from the nearest cell face, in cells
    -- at 0 the cell, and with it the mask, hangs on a rounding."""
    p = positions.detach().cpu().float().reshape(-1, 3)
    G = int(grid.resolution)
    lo = torch.tensor([float(v) for v in grid.box_min], dtype=torch.float32)
    size = torch.tensor([float(v) for v in grid.box_size], dtype=torch.float32)
    inv = torch.tensor(float(G), dtype=torch.float32) / size
    f = (p - lo) * inv                                   # two f32 roundings
    nan = torch.isnan(f).any(1)
    idx = torch.nan_to_num(f.clamp(0.0, float(G - 1)), nan=0.0).to(torch.int64)     # truncation
    cell = (idx[:, 2] * G + idx[:, 1]) * G + idx[:, 0]
    words = grid.bits.detach().cpu().to(torch.int64) & 0xffffffff
    bit = (words[cell >> 5] >> (cell & 31)) & 1
    fd = f.double()
    frac = fd - torch.floor(fd)
    return nan | (bit != 0), torch.minimum(frac, 1.0 - frac)


def grid_bits(cells, resolution):
    """int32 words (CPU) of a G^3 grid whose set bits are the int64 cell numbers ``cells``."""
    G = int(resolution)
    words = torch.zeros(((G ** 3 + 31) // 32,), dtype=torch.int64)
    cells = torch.unique(cells.reshape(-1).to(torch.int64))
    words.index_put_((cells >> 5,), torch.ones_like(cells) << (cells & 31), accumulate=True)
    words = torch.where(words >= 2 ** 31, words - 2 ** 32, words)
    return words.to(torch.int32)


# ------------------------------------------------------------------------------------- launch plan
def render_plan(R, S, teams, cus, m=None):
    """Host image of the launch arithmetic of ``ffn_render_fused_fwd`` for ``R`` rays of ``S`` samples:
    ``teams`` rays per workgroup at a time (4 waves, narrow; 2 pairs of waves, 512-wide), one
    workgroup per CU at most.  With ``m`` (a ray's kept samples) also that ray's ``nblk`` 32-sample
    blocks, its ``rows`` of the composite scan and the lanes of its last block that recompute slot
    m - 1 (``tail_lanes``)."""
    assert R >= 1 and 1 <= S <= 256 and teams in (NARROW_TEAMS, WIDE_TEAMS) and cus >= 1
    grid = min(-(-R // teams), cus)
    per_round = grid * teams
    rounds = -(-R // per_round)
    plan = dict(wide=teams == WIDE_TEAMS, grid=grid, rays_per_round=per_round, rounds=rounds,
                ragged=R % teams != 0, idle_teams=rounds * per_round - R, mask_passes=-(-S // 64))
    if m is not None:
        assert 0 <= m <= S
        nblk = (m + 31) >> 5
        plan.update(m=m, nblk=nblk, rows=(nblk + 1) // 2, tail_lanes=(32 * nblk - m),
                    half_row=nblk % 2 == 1)
    return plan


def ray_place(r, plan):
    """(round, workgroup, team) that renders ray ``r`` of the launch."""
    if plan["wide"]:
        return r // 2 // plan["grid"], r // 2 % plan["grid"], r % 2
    rnd, rest = divmod(r, plan["rays_per_round"])
    return rnd, rest // NARROW_TEAMS, rest % NARROW_TEAMS


def pair_plan(m_a, m_b):
    """The two pairs of a 512-wide workgroup run ``max(nblk)`` passes; the pair with fewer blocks
    pads with ``dummy`` passes on a dummy sample whose results are ignored."""
    na, nb = (m_a + 31) >> 5, (m_b + 31) >> 5
    passes = max(na, nb)
    return dict(nblk=(na, nb), passes=passes, dummy=(passes - na, passes - nb))

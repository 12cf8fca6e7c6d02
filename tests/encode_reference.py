"""Exact references of the standalone Fourier encoder (K3) and the u8 pixel writers (K8 and the
fused render kernel's image output).  Plain torch / numpy; nothing here needs a GPU.

K3 is held to ``|got - ref| <= kappa * 2^-24 * terms`` against float64, ``terms`` being
``|a| (|s| sum_d |x_d B_dk| + 1)`` for a trig column and ``|x|`` for a pass-through column: the
formula, the code (``layer_reference._features``) and the kappa of the fused kernels' features,
because K3 runs the same ``fast_sincos_n`` after the same mul / fma / fma argument chain.

K8's reference does what the kernels do: a byte is ``trunc(float32(c) * float32(255))``, one
float32 multiply and a truncation.  Against ``floor(float64(c) * 255)`` that differs in the
TRUNCATION, not in the rounding of the product: for a float32 ``c`` in [0, 1] the rounded
product never reaches a level the exact one is below.  (The float32 just below ``m / 255`` is
``rho`` ulps below it, ``rho = rot(m) / 255 >= 128 / 255`` with ``rot(m)`` the 8 bits of ``m``
rotated until the top one is set, because 1 / 255 repeats with period 8 and 24 = 3 * 8; its
product with 255 is ``rho * 255 / 256 >= 1 / 2`` ulp(m) below ``m``, and exactly 1 / 2 only for
a power of two, where that is one whole spacing.)  So on float32 colours in [0, 1 + 2^-23] the
two agree byte for byte and the bytes can be required exactly; the only value of the
quantisation ladder on which they part is the float32 just below 0, which truncates to 0 and
floors to -1 (``to_image_bytes`` against ``to_image_bytes_float64`` on ``quantisation_ladder``).

``encode_plan`` restates K3's launch arithmetic so that the tests can PROVE their shape list
reaches every branch of it; it is never an expected value of anything.
"""

import types

import numpy as np
import torch

from tests import layer_reference as lr

U = lr.U
# kappa of the fused kernels' features, not chosen anew: K3 runs the same arithmetic.  Worst ratio
# |err| / (2^-24 terms) of K3 on an MI355X over every case of tests/test_encode_reference_gpu.py
# after the value (the 33 M elements of F = 255 at 65 553 rows; 2.72 at angles up to 4500 rad;
# the fused kernels measure 2.96 .. 3.00 on their smaller batches)
KAPPA = lr.KAPPA["f32"]["features"]        # 6.0  [3.12]

TILE_BYTES = 64 * 1024          # most dynamic LDS a block may take
GROUP_BYTES = 32 * 1024         # what a block normally assembles
MAX_GROUP = 128                 # rows per block pass
STATIC_LDS_BYTES = 3 * MAX_GROUP * 4        # the kernel's staged points
MAX_GRID = 4096                 # blocks; more groups than that take the grid-stride loop


# ------------------------------------------------------------------------------------------ K3
def encode_features(x, b, a, scale, include_input):
    """(ref, terms), both float64 ``(N, 2F[+3])`` in the natural order ``[a cos | a sin | x]``.
    ``a=None`` means ones; ``b=None`` or ``F == 0`` means the output is ``x``."""
    x = x.double()
    freq = 0 if b is None else int(b.shape[1])
    if freq > 0 and a is None:
        a = torch.ones((freq,), dtype=torch.float64, device=x.device)
    enc = types.SimpleNamespace(scale=float(scale), num_freq=freq, b=b, a=a,
                                include_input=bool(include_input) or freq == 0)
    return lr._features(enc, x)


def check_features(key, got, ref, terms, kappa=KAPPA):
    """(worst |err| / (2^-24 terms), failures) of ``got`` against ``encode_features``' pair."""
    stage = lr._Stage("K3", kappa)
    assert tuple(got.shape) == tuple(ref.shape), "%s: shape %s, expected %s" % (key, tuple(got.shape), tuple(ref.shape))
    stage.compare(key, got.double(), ref, terms)
    return stage.worst, stage.failures


def encode_plan(freq, include_input, lds_limit=None):
    """The launch plan of ``ffn_fourier_encode`` for ``freq`` frequencies, or None where the entry
    point refuses (a row wider than four rows of the 64 KB tile; with ``lds_limit``, a workgroup
    whose tile plus static LDS exceeds it).  ``freq == 0`` is a device-to-device copy."""
    if freq < 0:
        return None
    if freq == 0:
        return dict(copy=True, width=3, group=MAX_GROUP)
    width = 2 * freq + (3 if include_input else 0)
    group = GROUP_BYTES // (4 * width) // 4 * 4
    rule = "32KB"
    if group > MAX_GROUP:
        group, rule = MAX_GROUP, "cap"
    if group < 4:
        group, rule = (4, "64KB") if TILE_BYTES // (4 * width) // 4 * 4 >= 4 else (0, None)
    if group < 4:
        return None
    dynamic = group * width * 4
    if lds_limit is not None and dynamic + STATIC_LDS_BYTES > lds_limit:
        return None
    pairs = (freq + 1) // 2
    per = max(pairs, 3 if include_input else 0)
    lanes = min(per, 256)
    spb = 256 // lanes
    return dict(copy=False, width=width, group=group, rule=rule, lds_dynamic=dynamic,
                lds_static=STATIC_LDS_BYTES, lds=dynamic + STATIC_LDS_BYTES, pairs=pairs, per=per,
                lanes=lanes, spb=spb, idle=256 - spb * lanes, slots=-(-per // lanes),
                repeats_frequency=freq % 2 == 1, repeats_pair=per > pairs)


def grid_strides(freq, include_input, n):
    """True where ``n`` rows are more groups than the grid has blocks."""
    plan = encode_plan(freq, include_input)
    return -(-n // plan["group"]) > MAX_GRID


def block_diagonal_b(freq):
    """(3, freq) B as NeRF builds it: input d feeds frequencies d L .. d L + L - 1 only, octaves
    from 1 to (just under) 2^10."""
    assert freq % 3 == 0 and freq > 0
    per = freq // 3
    octaves = 2.0 ** (10.0 * torch.arange(per, dtype=torch.float64) / per)
    b = torch.zeros((3, freq), dtype=torch.float64)
    for d in range(3):
        b[d, d * per:(d + 1) * per] = octaves
    return b.float()


# the shape list of tests/test_encode_reference_gpu.py (tests/test_encode_reference_cpu.py proves
# that it reaches every branch of the plan)
FREQS = [0, 1, 2, 3, 4, 5, 6, 7, 10, 85, 255, 256, 257, 511, 512, 513, 1023, 1025]
ROW_SWEEP_FREQS = [3, 63, 257]                  # with pass-through: widths 9, 129, 517, all odd
LIMIT_SHAPES = [(2000, True), (2046, True), (2048, False)]        # n = 5
TOO_WIDE = [(2047, True), (2049, False)]
GRID_STRIDE = [(1, False, 4096 * 128 + 129), (255, False, 4096 * 16 + 17)]


def ragged_rows(freq, include_input):
    """The one ragged row count every frequency count is run at: two whole groups and three rows
    (n mod 4 = 3: with an odd width the last group ends in the scalar store tail)."""
    return 2 * encode_plan(freq, include_input)["group"] + 3


def row_sweep(freq, include_input=True):
    group = encode_plan(freq, include_input)["group"]
    return [0, 1, 2, 3, 4, 5, group - 1, group, group + 1, 2 * group + 3]


def shape_cases():
    """Every (freq, include_input, n) the shape tests run, refusals excluded."""
    cases = [(f, inc, ragged_rows(f, inc)) for f in FREQS for inc in (False, True)]
    cases += [(f, True, n) for f in ROW_SWEEP_FREQS for n in row_sweep(f)]
    cases += [(f, inc, 5) for f, inc in LIMIT_SHAPES]
    cases += GRID_STRIDE
    return cases


# ------------------------------------------------------------------------------------------ K8
def to_image_bytes(colors, pixel_index, width, height):
    """(H, W, 3) uint8: zeros, scatter ``float32(colors) * float32(255)``, truncate through int32.
    Defined for colours in [0, 256/255)."""
    colors = np.asarray(colors)
    px = np.zeros((height * width, 3), np.float32)
    px[np.asarray(pixel_index, np.int64)] = colors.astype(np.float32) * np.float32(255)
    return px.astype(np.int32).astype(np.uint8).reshape(height, width, 3)


def to_image_bytes_float64(colors, pixel_index, width, height):
    """The same with the product in float64 and a floor: what K8 is NOT."""
    px = np.zeros((height * width, 3), np.float64)
    px[np.asarray(pixel_index, np.int64)] = np.asarray(colors).astype(np.float64) * 255.0
    return np.floor(px).astype(np.int32).astype(np.uint8).reshape(height, width, 3)


def quantisation_ladder(clip=True):
    """The 256 levels k / 255 in float32 and their two float32 neighbours, clipped to
    [0, 1 + 2^-23] (``clip=False``: with the negative neighbour of 0, outside K8's domain):
    (768,) float32."""
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    below = np.nextafter(k, np.float32(-1), dtype=np.float32)
    above = np.nextafter(k, np.float32(2), dtype=np.float32)
    ladder = np.stack([below, k, above], 1).reshape(-1)
    if not clip:
        return ladder
    return np.clip(ladder, np.float32(0), np.float32(1) + np.float32(2.0 ** -23)).astype(np.float32)

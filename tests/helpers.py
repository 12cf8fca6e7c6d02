"""Shared helpers for the test-suite (deterministic fills, camera rigs, a host-independent exp)."""

import math
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def formula_fill(shape, salt):
    """Same closed-form fill tests/golden/make_goldens.py used for full-size models."""
    n = int(np.prod(shape))
    fan_in = shape[-1] if len(shape) > 1 else shape[0]
    h = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(salt * 40503 + 12345))
    h = (h % np.uint64(2 ** 32)) >> np.uint64(8)
    vals = (h.astype(np.float64) / 2 ** 24 * 2 - 1) / np.sqrt(fan_in)
    return vals.astype(np.float32).reshape(shape)


def look_at_camera(eye, width, height, fov_deg=40.0):
    """Camera-to-world pose looking at the origin (x right, y down, z forward)."""
    eye = np.asarray(eye, np.float32)
    fwd = -eye / np.linalg.norm(eye)
    up = np.array([0, 1, 0], np.float32)
    if abs(np.dot(fwd, up)) > 0.95:
        up = np.array([1, 0, 0], np.float32)
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    ext = np.eye(4, dtype=np.float32)
    ext[:3, 0], ext[:3, 1], ext[:3, 2], ext[:3, 3] = right, down, fwd, eye
    focal = 0.5 * width / np.tan(0.5 * np.deg2rad(fov_deg))
    intr = np.array([[focal, 0, width / 2], [0, focal, height / 2], [0, 0, 1]], np.float32)
    return intr, ext


def portable_exp(x):
    """float32 exp of a float32 array from IEEE double adds and multiplies only (reduction by
    ln 2 in two parts, a degree-14 Taylor polynomial, exact scaling by 2^k), rounded once to
    float32: the same bits on every host, whichever exp kernel its math library dispatches to."""
    x = np.clip(np.asarray(x, np.float32).astype(np.float64), -200.0, 100.0)
    k = np.rint(x * (1.0 / math.log(2.0)))
    r = (x - k * 6.93147180369123816490e-01) - k * 1.90821492927058770002e-10
    p = np.full_like(r, 1.0 / math.factorial(14))
    for i in range(13, -1, -1):
        p = p * r + 1.0 / math.factorial(i)
    with np.errstate(over="ignore", invalid="ignore"):      # (inf above 88.7; NaN stays NaN)
        return np.ldexp(p, k.astype(np.int32)).astype(np.float32)


_EXP_PINS = None


def captured_exp_values(x):
    """float32 exp of `x` as the host that captured tests/golden computed it: `portable_exp`,
    except at the inputs tests/golden/exp_pins.npz lists (make_exp_pins.py), where that host's
    torch.exp (its math library's vector exp is not correctly rounded, and picks its kernel by
    host CPU) gave other bits."""
    global _EXP_PINS
    if _EXP_PINS is None:
        with np.load(os.path.join(GOLDEN, "exp_pins.npz"), allow_pickle=False) as g:
            _EXP_PINS = g["input_bits"], g["exp"]
    keys, vals = _EXP_PINS
    x = np.ascontiguousarray(x, np.float32)
    y = portable_exp(x).reshape(-1)
    bits = x.reshape(-1).view(np.int32)
    at = np.minimum(np.searchsorted(keys, bits), len(keys) - 1)
    hit = keys[at] == bits
    y[hit] = vals[at[hit]]
    return y.reshape(x.shape)


class _CapturedExp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        y = torch.from_numpy(captured_exp_values(x.detach().numpy()))
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, grad):
        (y,) = ctx.saved_tensors
        return grad * y                  # (ATen's exp backward: grad * result)


def captured_exp(x):
    """Drop-in for torch.exp on float32 CPU tensors, autograd included, with the values of
    `captured_exp_values`."""
    if x.dtype != torch.float32 or x.device.type != "cpu":
        raise TypeError("captured_exp covers float32 CPU tensors, not %s on %s" % (x.dtype, x.device))
    return _CapturedExp.apply(x)

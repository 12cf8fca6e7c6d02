"""The training loop of the explicit-buffer fits: ``fit_octree`` / ``fit_octree_sh`` (K17, K19),
``fit_mesh_colors`` (K32), ``fit_mesh_texture`` (K33) and ``fit_mesh_geometry`` (K34) all optimise
one plain float32 buffer against an ``ImageDataset`` with K7 (``ops.clip_adam``), and ``run`` is
that loop once; a fit supplies what is its own as plain callables.  ``report_line`` is the line a report step prints,
shared with ``Raycaster.fit``; ``check_schedule`` the refusals the fits have in common, made before
a fit touches the device; ``camera_psnr`` their validation.  Host code only: no kernel of its own.
"""

import time
from typing import List, NamedTuple, Sequence, Tuple

import numpy as np
import torch

from . import ops

FitLogEntry = NamedTuple("FitLogEntry", [("step", int), ("loss", float), ("val_psnr", float)])


def check_schedule(who: str, rule: str, batch, num_steps, report_interval, learning_rate) -> None:
    """The refusals the fits share, under the caller's name: ``batch >= 1`` (the caller's batch
    size, whatever it counts), ``num_steps >= 0``, ``report_interval >= 1`` -- ``rule`` is the
    caller's sentence for the three -- and a positive ``learning_rate`` (NaN is refused).  No
    device."""
    if int(batch) < 1 or int(num_steps) < 0 or int(report_interval) < 1:
        raise ValueError("%s: %s" % (who, rule))
    if not learning_rate > 0:
        raise ValueError("%s: learning_rate must be positive, got %r" % (who, learning_rate))


def report_line(step: int, num_steps: int, report_interval: int, start_time: float, now: float,
                fields: Sequence[Tuple[str, float]], learning_rate: float) -> str:
    """``0000500 0.001234 s/step name: value ... lr: 1.00e-02 eta: <date>``: the seconds per step
    since ``start_time`` and the time the run ends at that pace, 0 and ``N/A`` while
    ``step < report_interval``; ``fields`` are ``(name, value)`` in the caller's order."""
    per_step = (now - start_time) / step if step >= report_interval else 0
    eta = "N/A" if not per_step else time.strftime(
        "%a, %d %b %Y %H:%M:%S +0000", time.gmtime(now + (num_steps - step) * per_step))
    return " ".join(["{:07}".format(step), "{:2f} s/step".format(per_step)]
                    + ["{}: {:2f}".format(name, value) for name, value in fields]
                    + ["lr: {:.2e}".format(learning_rate), "eta:", eta])


def camera_psnr(frame, num_cameras: int, per: int, dataset, alpha_weight: float = 0.0) -> float:
    """-10 log10 of the mean colour-MSE + ``alpha_weight`` * alpha-MSE over every ray of
    ``num_cameras`` cameras of ``dataset``, camera by camera; ``frame(number) -> (color, alpha,
    ...)`` is the picture of camera ``number``, ``per`` its rays."""
    device = dataset.colors.device
    alphas = dataset._gt_alphas()
    total = torch.zeros((2,), dtype=torch.float32, device=device)
    rays = torch.arange(per, dtype=torch.int64, device=device)
    for number in range(num_cameras):
        color, alpha = frame(number)[:2]
        sums, _, _ = ops.mse_loss(color, alpha, dataset.colors, alphas, rays + number * per, 0.0,
                                  0.0, want_grad=False)
        total += sums
    count = per * num_cameras
    total = total.cpu().numpy().astype(np.float64)
    mean = total[0] / (3 * count) + alpha_weight * total[1] / count
    return float(-10.0 * np.log10(max(mean, 1e-12)))


def run(data, epoch, step, project, validate, num_steps, learning_rate, report_interval,
        clip_value, max_norm, verbose=True, fields=None) -> List[FitLogEntry]:
    """``num_steps`` steps on the contiguous float32 buffer ``data``, in place -> the log, one
    ``FitLogEntry(step, loss, val_psnr)`` per step.  The gradient buffer, the Adam moments, K7's
    scratch and the step counter are here.  ``epoch()`` returns one epoch's batches and is called
    again when they run out; the run stops in the middle of an epoch at ``num_steps``.
    ``step(batch, grads)`` writes the gradient of the batch's loss into ``grads`` (the shape of
    ``data``) and returns the loss, already reduced, as a device scalar: the losses are fetched once,
    at the end.  Then K7 (``ops.clip_adam``, step number ``k + 1``) on the flat buffer and
    ``project(data)``.  At steps below 10 and at multiples of ``report_interval`` ``validate()``
    gives the entry's ``val_psnr`` (NaN at every other step, and at all of them when ``validate``
    is None), and with ``verbose`` the ``report_line`` is printed: ``loss:``, ``val_psnr:``, then
    the ``(name, value)`` pairs ``fields()`` returns.  ``check_schedule`` is the caller's to make."""
    flat = data.view(-1)
    grads = torch.empty_like(data)
    exp_avg, exp_avg_sq = torch.zeros_like(flat), torch.zeros_like(flat)
    scratch = torch.empty(((flat.numel() + 1023) // 1024,), dtype=torch.float32,
                          device=data.device)
    losses, reports = [], {}
    start_time = time.time()
    k = 0
    while k < num_steps:
        for batch in epoch():
            if k >= num_steps:
                break
            losses.append(step(batch, grads))
            ops.clip_adam(flat, grads.view(-1), exp_avg, exp_avg_sq, k + 1, learning_rate,
                          clip_value=clip_value, max_norm=max_norm, scratch=scratch)
            project(data)
            if validate is not None and (k < 10 or k % report_interval == 0):
                reports[k] = validate()
                if verbose:
                    now = time.time()
                    shown = [("loss", float(losses[-1].item())), ("val_psnr", reports[k])]
                    shown += fields() if fields is not None else []
                    print(report_line(k, num_steps, report_interval, start_time, now, shown,
                                      learning_rate))
            k += 1
    values = torch.stack(losses).cpu().numpy() if losses else np.zeros(0, np.float32)
    return [FitLogEntry(k, float(values[k]), reports.get(k, float("nan")))
            for k in range(len(values))]

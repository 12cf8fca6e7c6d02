"""2-D image regression as a straight line of kernel launches (train_image_regression.py:179-186).

``RegressionEngine.step`` replaces the reference's
``optim.zero_grad(); out = torch.sigmoid(model(uv)); loss = 0.5 * torch.square(out - y).mean();
loss.backward(); optim.step()`` with: the fused MLP forward with saved slabs, K11
(``ffn_regression_train``: sigmoid, squared error sums and d(loss)/d(logits) in one launch), the
fused backward, and K7 (``ffn_clip_adam``) with both clips off.  Parameters, gradients and Adam
moments live in flat device buffers, as in ``TrainEngine``; the step issues no host sync.
"""

import math
from typing import Optional, Tuple

import torch
import torch.nn as nn

from . import ops


class RegressionEngine:
    """Adam (torch.optim.Adam's defaults) over the dense weights and biases of a
    ``FourierFeatureMLP``.  ``a_values`` / ``b_values`` are not trained: they have
    ``requires_grad=False`` in the reference as here, so its Adam skips them."""

    def __init__(self, model: nn.Module, beta1: float = 0.9, beta2: float = 0.999,
                 eps: float = 1e-8):
        self.model = model
        params = model._dense_params()
        device = params[0].device
        if device.type != "cuda":
            raise RuntimeError("training runs on the HIP kernels only; move the model to a GPU")
        total = sum(p.numel() for p in params)
        flat = torch.empty((total,), dtype=torch.float32, device=device)
        offset = 0
        for p in params:                      # nn.Parameters become views of one buffer
            n = p.numel()
            flat[offset:offset + n].copy_(p.data.reshape(-1))
            p.data = flat[offset:offset + n].view(p.shape)
            offset += n
        self.flat = flat
        self.grads = torch.zeros_like(flat)
        self.exp_avg = torch.zeros_like(flat)
        self.exp_avg_sq = torch.zeros_like(flat)
        self.scratch = torch.empty(((total + 1023) // 1024,), dtype=torch.float32, device=device)
        self.beta1, self.beta2, self.eps = beta1, beta2, eps
        self.device = device
        self.count = 0
        self._buffers = {}
        model.invalidate_packed()
        assert model.program().num_grad_floats == total

    def _buffer(self, name: str, shape, dtype=torch.float32) -> torch.Tensor:
        """A device buffer reused from step to step (allocated once per shape)."""
        buf = self._buffers.get(name)
        if buf is None or tuple(buf.shape) != tuple(shape) or buf.dtype != dtype:
            self._buffers[name] = buf = None
            self._buffers[name] = buf = torch.empty(shape, dtype=dtype, device=self.device)
        return buf

    @staticmethod
    def _check(inputs3: torch.Tensor, target: Optional[torch.Tensor]):
        if inputs3.dim() != 2 or inputs3.shape[1] != 3:
            raise ValueError("inputs3 must be (N,3) positions (2-D uvs padded with a zero column: "
                             "PixelDataset.train_uv3), got %s" % (tuple(inputs3.shape),))
        if target is not None and (target.dim() != 2 or target.shape[0] != inputs3.shape[0]):
            raise ValueError("target must be (N,C) for N = %d inputs, got %s"
                             % (inputs3.shape[0], tuple(target.shape)))

    def step(self, inputs3: torch.Tensor, target: torch.Tensor, lr: float) -> torch.Tensor:
        """One Adam step on 0.5 * mean((sigmoid(model(uv)) - target)^2) over all N pixels.
        ``inputs3`` (N,3), ``target`` (N,C) float32 on the model's GPU; ``lr`` from
        ``learning_rate_at``.  Returns the loss (before the update) as a device scalar."""
        self._check(inputs3, target)
        n, c = target.shape
        if n == 0:
            raise ValueError("an empty batch")
        model = self.model
        prog = model.program()
        precision = model.effective_precision(model.train_precision)
        saved = self._buffer("saved", (prog.saved_floats(n),))
        logits = prog.forward(inputs3, None, saved, precision=precision)
        d_logits = self._buffer("d_logits", (n, 4))
        partials = self._buffer("partials", (ops.regression_blocks(n),))
        ops.regression_train(logits, target, d_logits, partials)
        loss = torch.empty((), dtype=torch.float32, device=self.device)
        ops.regression_loss(partials, n * c, loss_out=loss)
        prog.backward(d_logits, inputs3, None, saved, self.grads, precision=precision)
        self.count += 1
        # the reference's loop does not clip: with both bounds at +inf K7's clamp and its norm
        # coefficient min(1, inf / (norm + 1e-6)) are the identity, bit for bit
        ops.clip_adam(self.flat, self.grads, self.exp_avg, self.exp_avg_sq, self.count, lr,
                      clip_value=math.inf, max_norm=math.inf, beta1=self.beta1, beta2=self.beta2,
                      eps=self.eps, scratch=self.scratch)
        model.invalidate_packed()
        return loss

    def evaluate(self, inputs3: torch.Tensor, target: Optional[torch.Tensor] = None,
                 want_image: bool = False) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
        """Validation forward (inference precision of the model) + K11: (sum((sigmoid - y)^2) as a
        device scalar or None without a target, (N,C) u8 (sigmoid * 255) pixels or None)."""
        self._check(inputs3, target)
        n = inputs3.shape[0]
        c = self.model.num_outputs if target is None else target.shape[1]
        model = self.model
        prog = model.program()
        mode = model.effective_precision(model.precision)
        with torch.no_grad():
            logits = prog.forward(inputs3, None, None, precision=mode)
        image = torch.empty((n, c), dtype=torch.uint8, device=self.device) if want_image else None
        sse = None
        partials = None
        if target is not None:
            partials = torch.empty((ops.regression_blocks(n),), dtype=torch.float32,
                                   device=self.device)
        ops.regression_eval(logits, target, c, partials, image)
        if target is not None:
            sse = torch.empty((), dtype=torch.float32, device=self.device)
            ops.regression_loss(partials, n * c, sse_out=sse)
        return sse, image

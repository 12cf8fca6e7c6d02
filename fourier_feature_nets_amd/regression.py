"""2-D image and 1-D signal regression as a straight line of kernel launches
(train_image_regression.py:179-186, train_signal_regression.py:153-157).

``RegressionEngine.step`` replaces the reference's
``optim.zero_grad(); out = torch.sigmoid(model(uv)); loss = 0.5 * torch.square(out - y).mean();
loss.backward(); optim.step()`` with: the fused MLP forward with saved slabs, K11
(``ffn_regression_train``: sigmoid, squared error sums and d(loss)/d(logits) in one launch), the
fused backward, and K7 (``ffn_clip_adam``) with both clips off.  Parameters, gradients and Adam
moments live in flat device buffers, as in ``TrainEngine``; the step issues no host sync.

With ``loss="linear"`` the loss is signal regression's ``(model(x) - y).square().mean()``
(train_signal_regression.py:81-85): K11b (``ffn_regression_mse_train``) takes K11's place, and
``weight_decay`` is the coupled L2 term of its ``Adam(..., weight_decay=1e-3)`` (:141), which K7
adds to the gradient as ``g + wd * p`` before the moments.
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

    LOSSES = ("sigmoid", "linear")

    def __init__(self, model: nn.Module, beta1: float = 0.9, beta2: float = 0.999,
                 eps: float = 1e-8, *, weight_decay: float = 0.0, loss: str = "sigmoid"):
        """``loss``: "sigmoid" = 0.5 * mean((sigmoid(z) - y)^2) (image regression, K11) or
        "linear" = mean((z - y)^2) (signal regression, K11b).  ``weight_decay``: torch.optim.Adam's
        coupled L2 term."""
        if loss not in self.LOSSES:
            raise ValueError("loss must be one of %s, not %r" % (self.LOSSES, loss))
        self.model = model
        params = model._dense_params()
        device = params[0].device
        if device.type != "cuda":
            raise RuntimeError("training runs on the HIP kernels only; move the model to a GPU")
        model.check_params(device)          # before the copies into the flat buffer
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
        self.weight_decay = float(weight_decay)
        self.loss = loss
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
        """One Adam step on the engine's loss over all N inputs: 0.5 * mean((sigmoid(model(uv)) -
        target)^2), or mean((model(x) - target)^2) for ``loss="linear"``.  ``inputs3`` (N,3),
        ``target`` (N,C) float32 on the model's GPU; ``lr`` from ``learning_rate_at`` (or constant).
        Returns the loss (before the update) as a device scalar."""
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
        loss = torch.empty((), dtype=torch.float32, device=self.device)
        if self.loss == "linear":
            ops.regression_mse_train(logits, target, d_logits, partials)
            ops.regression_mse_loss(partials, n * c, loss_out=loss)
        else:
            ops.regression_train(logits, target, d_logits, partials)
            ops.regression_loss(partials, n * c, loss_out=loss)
        prog.backward(d_logits, inputs3, None, saved, self.grads, precision=precision)
        self.count += 1
        # the reference's loop does not clip: with both bounds at +inf K7's clamp is the identity
        # and its norm coefficient exactly 1 (even where the f32 sum of squares overflows)
        ops.clip_adam(self.flat, self.grads, self.exp_avg, self.exp_avg_sq, self.count, lr,
                      weight_decay=self.weight_decay, clip_value=math.inf, max_norm=math.inf, beta1=self.beta1, beta2=self.beta2,
                      eps=self.eps, scratch=self.scratch)
        model.invalidate_packed()
        return loss

    def evaluate(self, inputs3: torch.Tensor, target: Optional[torch.Tensor] = None,
                 want_image: bool = False) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
        """Validation forward (inference precision of the model) + K11: (sum((sigmoid - y)^2) as a
        device scalar or None without a target, (N,C) u8 (sigmoid * 255) pixels or None).
        ``loss="linear"``: K11b, (sum((z - y)^2), None); a target is required, there is no image."""
        sse, image, _ = self._evaluate(inputs3, target, want_image, False)
        return sse, image

    def validation_loss(self, inputs3: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        """The engine's loss of the model's inference forward over (inputs3, target), as a device
        scalar: mean((z - y)^2) for ``loss="linear"`` (train_signal_regression.py:88-95),
        0.5 * mean((sigmoid(z) - y)^2) otherwise."""
        if target is None:
            raise ValueError("validation_loss needs a target")
        return self._evaluate(inputs3, target, False, True)[2]

    def _evaluate(self, inputs3, target, want_image, want_loss):
        self._check(inputs3, target)
        linear = self.loss == "linear"
        if linear and (target is None or want_image):
            raise ValueError("the linear loss evaluates against a target and renders no image")
        n = inputs3.shape[0]
        c = self.model.num_outputs if target is None else target.shape[1]
        model = self.model
        prog = model.program()
        mode = model.effective_precision(model.precision)
        with torch.no_grad():
            logits = prog.forward(inputs3, None, None, precision=mode)
        image = torch.empty((n, c), dtype=torch.uint8, device=self.device) if want_image else None
        sse = loss = None
        partials = None
        if target is not None:
            partials = torch.empty((ops.regression_blocks(n),), dtype=torch.float32,
                                   device=self.device)
        if linear:
            ops.regression_mse_eval(logits, target, partials)
        else:
            ops.regression_eval(logits, target, c, partials, image)
        if target is not None:
            sse = torch.empty((), dtype=torch.float32, device=self.device)
            loss = torch.empty((), dtype=torch.float32, device=self.device) if want_loss else None
            (ops.regression_mse_loss if linear else ops.regression_loss)(
                partials, n * c, sse_out=sse, loss_out=loss)
        return sse, image, loss

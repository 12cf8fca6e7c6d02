"""Radiance-field models behind the reference's class surface, computed by the fused HIP MLP.

Constructor signatures, attribute names, state-dict keys/shapes and the checkpoint format
mirror ``fourier_feature_models.py:10-191`` and ``nerf_model.py:12-135`` of the reference so
that its scripts and checkpoints see a drop-in.  ``forward`` does not run ATen GEMMs: it hands
the whole layer chain to ``MlpProgram`` (fourier_feature_nets_amd/mlp_engine.py) and raises
when the module is not on a GPU.
"""

import math
import os
from typing import List, Optional, Sequence

import torch
import torch.nn as nn

from .mlp_engine import DenseSpec, EncodingSpec, MlpProgram
from .sampler import _notice_once


class _FusedChainFunction(torch.autograd.Function):
    """logits = chain(positions[, views]); backward = dgrad + wgrad + reduce kernels."""

    @staticmethod
    def forward(ctx, module, grad_mode, positions, views, *params):
        prog = module.program()
        if grad_mode and (positions.requires_grad or (views is not None and views.requires_grad)):
            raise NotImplementedError(
                "gradients w.r.t. sample positions / view directions are not produced by the "
                "fused kernels (the volume-rendering path never needs them); detach the inputs")
        positions = positions.contiguous()
        views = None if views is None else views.contiguous()
        # grad mode is sampled by the caller: inside Function.forward it is always off, and
        # needs_input_grad stays true for parameters even under torch.no_grad()
        track = grad_mode and any(ctx.needs_input_grad[4:])
        saved = None
        # (keep_activations: the slabs are written even without gradient tracking, and handed to
        # FourierFeatureMLP.forward, which copies the last hidden layer out of them)
        keep = bool(getattr(module, "keep_activations", False)) and positions.shape[0] > 0
        if track or keep:
            saved = torch.empty((prog.saved_floats(positions.shape[0]),), dtype=torch.float32,
                                device=positions.device)
        precision = module.effective_precision(module.train_precision) if track else "f32"
        infer_mode = module.effective_precision(module.precision)
        if keep and not track:
            precision = infer_mode
            logits = prog.forward(positions, views, saved, precision=precision)
            module._kept_slabs = saved
            saved = None
        elif not track and infer_mode == "bf16x3":
            logits = prog.forward16(positions, views)       # opt-in fast inference mode
        elif not track and infer_mode == "bf16x6":
            logits = prog.forward(positions, views, None, precision="bf16x6")   # opt-in, f32-accurate
        else:
            logits = prog.forward(positions, views, saved, precision=precision)
        if keep and track:
            module._kept_slabs = saved
        ctx.module = module
        ctx.precision = precision     # backward runs in the mode its forward ran in
        ctx.saved_acts = saved
        ctx.save_for_backward(positions, views)
        return logits

    @staticmethod
    def backward(ctx, d_logits):
        positions, views = ctx.saved_tensors
        if ctx.saved_acts is None:
            raise RuntimeError("the fused MLP frees its activation slabs in backward: a second "
                               "backward through the same forward (retain_graph=True) is not "
                               "supported -- run the forward again")
        prog = ctx.module.program()
        grads = torch.empty((prog.num_grad_floats,), dtype=torch.float32, device=positions.device)
        prog.backward(d_logits.contiguous(), positions, views, ctx.saved_acts, grads,
                      precision=ctx.precision)
        ctx.saved_acts = None
        outs = []
        for i, spec in enumerate(prog.layers):
            w0 = prog.grad_w_off[i]
            outs.append(grads[w0:w0 + spec.out * spec.ld].view(spec.out, spec.ld))
            b0 = prog.grad_b_off[i]
            # (a 0-d bias -- train_signal_regression.py:126 assigns one -- gets a 0-d gradient)
            outs.append(grads[b0:b0 + spec.out].view(spec.bias.shape))
        return (None, None, None, None) + tuple(outs)


class _FusedModel(nn.Module):
    """Shared machinery: lazily built MlpProgram, re-packed when the weights change."""

    def __init__(self):
        nn.Module.__init__(self)
        self._prog: Optional[MlpProgram] = None
        self._packed_key = None
        # "f32": exact-f32 MFMA everywhere (the parity mode).  "bf16x3": OPT-IN split-bf16
        # matrix products for INFERENCE calls (no_grad / eval renders); "bf16x6": OPT-IN
        # f32-accurate three-part split (six bf16 products per f32 product, mlp_bf16_ws.hip).
        self.precision = "f32"
        # "bf16x3" / "bf16x6": the OPT-IN split kernels for the TRAINING pass as well (forward with
        # saved activations, backward data, weight gradients -- bf16x6: full units on the three-part
        # kernel, narrow units on the exact-f32 one; FFN_BF16X6_WGRAD=f32 opts out).
        # Separately labelled wherever it is reported.
        self.train_precision = "f32"
        # FFN_PRECISION=bf16x6|bf16x3 (environment, read at construction): the arithmetic mode of
        # every model built while it is set -- how the test-suite runs the reference-golden tests of
        # the exact mode over an opt-in mode unchanged (tests/test_round5_gpu.py)
        mode = os.environ.get("FFN_PRECISION", "f32")
        if mode not in ("f32", "bf16x3", "bf16x6"):
            raise ValueError("FFN_PRECISION must be f32, bf16x3 or bf16x6, not %r" % mode)
        if mode != "f32":
            _notice_once("FFN_PRECISION=%s: every model built in this process (opacity / coarse models "
                         "included) computes in the opt-in %s mode wherever that mode has kernels for its "
                         "chain, in exact f32 elsewhere" % (mode, mode))
        self.precision = self.train_precision = mode
        # A mode that came from the ENVIRONMENT is a process-wide default: a chain it does not cover
        # (bf16x6: layers wider than 256 channels) runs the exact-f32 kernels, with a notice.  A mode
        # assigned to the attributes by hand is a request: a chain it does not cover raises.
        self._precision_is_default = mode != "f32"

    def effective_precision(self, mode: str) -> str:
        """The arithmetic a call in ``mode`` runs in (see ``_precision_is_default``)."""
        if mode == "f32" or not self._precision_is_default or self.program().covers(mode):
            return mode
        _notice_once("%s: no %s kernels for this chain (%s) -- it runs in exact f32"
                     % (type(self).__name__, mode,
                        "layers wider than 256 channels" if mode == "bf16x6" else "unfused logits heads"))
        return "f32"

    def _chain(self, device):   # -> (encodings, dense specs)
        raise NotImplementedError

    def _dense_params(self) -> List[nn.Parameter]:
        raise NotImplementedError

    def invalidate_packed(self):
        """The kernels read MFMA-operand COPIES of the weights, re-derived whenever a
        parameter's autograd version changes.  Writes that bypass the version counter --
        ``p.data.copy_()`` / ``layer.weight.data.uniform_()``, raw-pointer updates such as the
        fused optimiser kernel -- must be followed by this call, or the next forward uses stale
        copies.  ``load_state_dict`` calls it itself.  (``train()`` / ``eval()`` do not: the mode
        never changes a weight, and ``render_image`` flips it around every frame.)"""
        self._packed_key = None

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self.invalidate_packed()
        return out

    def check_params(self, device: torch.device):
        """Every dense weight / bias is a float32 tensor on ``device`` of its layer's size (a bias
        may be 0-d when its layer has one output, as train_signal_regression.py:126 makes it).
        Runs before the pack table is built: that table copies from the raw data pointers, so a
        host tensor assigned to ``layer.bias.data`` of a GPU model would hand a host pointer to a
        device copy."""
        params = self._dense_params()
        for k in range(0, len(params), 2):
            w, b = params[k], params[k + 1]
            for name, t in (("weight", w), ("bias", b)):
                if t.device != device:
                    raise RuntimeError("%s: a dense %s lives on %s, the model on %s; move it with "
                                       "the model (.to(device)) before calling it"
                                       % (type(self).__name__, name, t.device, device))
                if t.dtype != torch.float32:
                    raise TypeError("%s: a dense %s is %s; the kernels take float32"
                                    % (type(self).__name__, name, t.dtype))
            if w.dim() != 2 or w.stride(1) != 1:
                raise ValueError("%s: a dense weight must be a row-major (out, in) matrix, got "
                                 "shape %s" % (type(self).__name__, tuple(w.shape)))
            if b.dim() > 1 or b.numel() != w.shape[0] or not b.is_contiguous():
                raise ValueError("%s: a bias of shape %s for a layer of %d outputs (a (%d,) or, "
                                 "for one output, a 0-d tensor)"
                                 % (type(self).__name__, tuple(b.shape), w.shape[0], w.shape[0]))

    def program(self) -> MlpProgram:
        params = self._dense_params()
        device = params[0].device
        if device.type != "cuda":
            raise RuntimeError(
                "%s runs on the HIP kernels only: move the model to a GPU (.to('cuda')); there "
                "is no CPU fallback" % type(self).__name__)
        ptrs = tuple(p.data_ptr() for p in params)
        if self._prog is None or self._prog.device != device or self._prog_ptrs != ptrs:
            # (a tensor assigned to a parameter's .data always changes its pointer: the checks run
            # whenever the pack table is rebuilt, off the per-step path)
            self.check_params(device)
            encodings, specs = self._chain(device)
            self._prog = MlpProgram(encodings, specs, device)
            self._prog_ptrs = ptrs
            self._packed_key = None
        key = tuple(p._version for p in params)
        if self._packed_key != key:
            self._prog.pack()
            self._packed_key = key
        return self._prog

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._prog = None
        return out

    def __getstate__(self):          # keep deepcopy / pickling of modules working
        state = dict(self.__dict__)
        state["_prog"] = None
        state["_packed_key"] = None
        return state


class FourierFeatureMLP(_FusedModel):
    """gamma(x) = [a cos(pi x B), a sin(pi x B)] followed by a ReLU MLP
    (reference: fourier_feature_models.py:10-89)."""

    def __init__(self, num_inputs: int, num_outputs: int, a_values: Optional[torch.Tensor],
                 b_values: Optional[torch.Tensor], layer_channels: List[int]):
        _FusedModel.__init__(self)
        self.params = {
            "num_inputs": num_inputs,
            "num_outputs": num_outputs,
            "a_values": None if a_values is None else a_values.tolist(),
            "b_values": None if b_values is None else b_values.tolist(),
            "layer_channels": layer_channels,
        }
        self.num_inputs = num_inputs
        self.num_outputs = num_outputs
        if b_values is None:
            self.a_values = None
            self.b_values = None
            width = num_inputs
        else:
            assert b_values.shape[0] == num_inputs
            assert a_values.shape[0] == b_values.shape[1]
            self.a_values = nn.Parameter(a_values, requires_grad=False)
            self.b_values = nn.Parameter(b_values, requires_grad=False)
            width = 2 * b_values.shape[1]
        self.layers = nn.ModuleList()
        for channels in layer_channels:
            self.layers.append(nn.Linear(width, channels))
            width = channels
        self.layers.append(nn.Linear(width, num_outputs))
        self.use_view = False
        self.keep_activations = False
        self.activations = []

    def _dense_params(self):
        out = []
        for layer in self.layers:
            out += [layer.weight, layer.bias]
        return out

    def _chain(self, device):
        if self.num_inputs not in (1, 2, 3) or self.num_outputs > 4:
            raise NotImplementedError("the fused kernels cover 1, 2 or 3 inputs and <= 4 outputs "
                                      "(got %d inputs, %d outputs)"
                                      % (self.num_inputs, self.num_outputs))
        # (fewer than 3 inputs: a 3-input chain with zero rows of B / zero raw-input weight
        # columns, see EncodingSpec; forward pads the positions to match)
        enc = EncodingSpec(None if self.b_values is None else self.b_values.data,
                           None if self.a_values is None else self.a_values.data,
                           math.pi, False, device, num_inputs=self.num_inputs)
        specs = []
        last = len(self.layers) - 1
        for i, layer in enumerate(self.layers):
            specs.append(DenseSpec(layer.weight, layer.bias, 0 if i == 0 else layer.in_features,
                                   0 if i == 0 else None, i != last,
                                   (0, self.num_outputs) if i == last else None))
        return [enc], specs

    def forward(self, inputs: torch.Tensor) -> torch.Tensor:
        """(..., num_inputs) positions -> (..., num_outputs) raw outputs (any leading shape, as
        the reference's matmul-based forward accepts: ``(H, W, 2)`` uv grids in image regression)."""
        self.activations.clear()
        self._kept_slabs = None
        if inputs.dim() < 1 or inputs.shape[-1] != self.num_inputs:
            raise ValueError("%s expects (..., %d) inputs, got %s"
                             % (type(self).__name__, self.num_inputs, tuple(inputs.shape)))
        lead = tuple(inputs.shape[:-1])
        flat = inputs.reshape(-1, self.num_inputs)
        if self.num_inputs < 3:      # lifted to the kernels' (N,3) positions with zero columns
            flat = torch.nn.functional.pad(flat, (0, 3 - self.num_inputs))
        out = _FusedChainFunction.apply(self, torch.is_grad_enabled(), flat, None,
                                        *self._dense_params())
        if self.keep_activations:
            # fourier_feature_models.py:70-75: the output of the last hidden layer, as a numpy
            # array on the host.  The forward pass left that layer's activation slab in HBM; this
            # is a copy of it (MlpProgram.slab_rows), not a second evaluation.
            hidden = len(self.layers) - 2
            if hidden < 0:
                raise NotImplementedError("keep_activations needs at least one hidden layer")
            n = flat.shape[0]
            if n == 0:
                rows = torch.zeros((0, self.layers[hidden].out_features))
            else:
                rows = self.program().slab_rows(self._kept_slabs, n, hidden)
            self._kept_slabs = None
            self.activations.append(rows.detach().cpu().numpy().reshape(lead + (rows.shape[-1],)))
        out = out if self.num_outputs == 4 else out[:, :self.num_outputs]
        return out if len(lead) == 1 else out.reshape(lead + (self.num_outputs,))

    def save(self, path: str):
        """Checkpoint in the reference format: state dict + "type" + "params"."""
        blob = self.state_dict()
        blob["type"] = "fourier"
        blob["params"] = self.params
        torch.save(blob, path)


class MLP(FourierFeatureMLP):
    """No encoding (fourier_feature_models.py:92-109)."""

    def __init__(self, num_inputs: int, num_outputs: int, num_layers=3, num_channels=256):
        FourierFeatureMLP.__init__(self, num_inputs, num_outputs, None, None,
                                   [num_channels] * num_layers)


class BasicFourierMLP(FourierFeatureMLP):
    """B = identity (fourier_feature_models.py:112-131)."""

    def __init__(self, num_inputs: int, num_outputs: int, num_layers=3, num_channels=256):
        FourierFeatureMLP.__init__(self, num_inputs, num_outputs, torch.ones(num_inputs),
                                   torch.eye(num_inputs), [num_channels] * num_layers)


def axis_frequencies(max_log_scale: float, num_freq: int, num_inputs: int) -> torch.Tensor:
    """(num_inputs, num_inputs*num_freq) axis-aligned frequency matrix, one block per
    frequency with columns [x f, y f, z f]; f = 2**linspace(0, max_log_scale, num_freq)."""
    freqs = 2. ** torch.linspace(0, max_log_scale, num_freq)
    out = torch.zeros((num_inputs, num_inputs * num_freq))
    for axis in range(num_inputs):
        out[axis, axis::num_inputs] = freqs
    return out


class PositionalFourierMLP(FourierFeatureMLP):
    """Axis-aligned log-spaced frequencies (fourier_feature_models.py:134-166)."""

    def __init__(self, num_inputs: int, num_outputs: int, max_log_scale: float, num_layers=3,
                 num_channels=256, embedding_size=256):
        b_values = self._encoding(max_log_scale, embedding_size, num_inputs)
        FourierFeatureMLP.__init__(self, num_inputs, num_outputs, torch.ones(b_values.shape[1]),
                                   b_values, [num_channels] * num_layers)

    @staticmethod
    def _encoding(max_log_scale: float, embedding_size: int, num_inputs: int):
        return axis_frequencies(max_log_scale, embedding_size // num_inputs, num_inputs)


class GaussianFourierMLP(FourierFeatureMLP):
    """Dense Gaussian B drawn from torch's global RNG (fourier_feature_models.py:169-191)."""

    def __init__(self, num_inputs: int, num_outputs: int, sigma: float, num_layers=3,
                 num_channels=256, embedding_size=256):
        b_values = torch.normal(0, sigma, size=(num_inputs, embedding_size))
        FourierFeatureMLP.__init__(self, num_inputs, num_outputs, torch.ones(b_values.shape[1]),
                                   b_values, [num_channels] * num_layers)


class NeRF(_FusedModel):
    """Full NeRF: ReLU trunk with skip concatenation, sigma head, linear bottleneck,
    view-dependent colour branch (reference: nerf_model.py:9-135)."""

    def __init__(self, num_layers: int, num_channels: int, max_log_scale_pos: float,
                 num_freq_pos: int, max_log_scale_view: float, num_freq_view: int,
                 skips: Sequence[int], include_inputs: bool):
        _FusedModel.__init__(self)
        self.params = {
            "num_layers": num_layers,
            "num_channels": num_channels,
            "max_log_scale_pos": max_log_scale_pos,
            "num_freq_pos": num_freq_pos,
            "max_log_scale_view": max_log_scale_view,
            "num_freq_view": num_freq_view,
            "skips": list(skips),
            "include_inputs": include_inputs,
        }
        self.pos_encoding = nn.Parameter(self._encoding(max_log_scale_pos, num_freq_pos, 3),
                                         requires_grad=False)
        self.view_encoding = nn.Parameter(self._encoding(max_log_scale_view, num_freq_view, 3),
                                          requires_grad=False)
        self.skips = set(skips)
        self.include_inputs = include_inputs
        self.use_view = True
        extra = 3 if include_inputs else 0
        enc_width = 2 * self.pos_encoding.shape[-1] + extra
        self.layers = nn.ModuleList()
        width = enc_width
        for i in range(num_layers):
            if i in self.skips:
                width += enc_width
            self.layers.append(nn.Linear(width, num_channels))
            width = num_channels
        self.opacity_out = nn.Linear(width, 1)
        self.bottleneck = nn.Linear(width, num_channels)
        self.hidden_view = nn.Linear(num_channels + 2 * self.view_encoding.shape[-1] + extra,
                                     num_channels // 2)
        self.color_out = nn.Linear(num_channels // 2, 3)

    @staticmethod
    def _encoding(max_log_scale: float, num_freq: int, num_inputs: int):
        return axis_frequencies(max_log_scale, num_freq, num_inputs)

    def _dense_params(self):
        out = []
        for layer in list(self.layers) + [self.opacity_out, self.bottleneck, self.hidden_view,
                                          self.color_out]:
            out += [layer.weight, layer.bias]
        return out

    def _chain(self, device):
        if 0 in self.skips:
            raise NotImplementedError("a skip connection into layer 0")
        enc_pos = EncodingSpec(self.pos_encoding.data, None, 1.0, self.include_inputs, device)
        enc_view = EncodingSpec(self.view_encoding.data, None, 1.0, self.include_inputs, device)
        channels = self.params["num_channels"]
        specs = []
        for i, layer in enumerate(self.layers):
            if i == 0:
                specs.append(DenseSpec(layer.weight, layer.bias, 0, 0, True))
            elif i in self.skips:
                specs.append(DenseSpec(layer.weight, layer.bias, channels, 0, True))
            else:
                specs.append(DenseSpec(layer.weight, layer.bias, channels, None, True))
        specs.append(DenseSpec(self.opacity_out.weight, self.opacity_out.bias, channels, None,
                               False, (3, 1)))
        specs.append(DenseSpec(self.bottleneck.weight, self.bottleneck.bias, channels, None, False))
        specs.append(DenseSpec(self.hidden_view.weight, self.hidden_view.bias, channels, 1, True))
        specs.append(DenseSpec(self.color_out.weight, self.color_out.bias, channels // 2, None,
                               False, (0, 3)))
        return [enc_pos, enc_view], specs

    def forward(self, position: torch.Tensor, view: torch.Tensor) -> torch.Tensor:
        """(N,3) positions and (N,3) unit view directions -> (N,4) raw [r,g,b,sigma]."""
        return _FusedChainFunction.apply(self, torch.is_grad_enabled(), position, view,
                                         *self._dense_params())

    def save(self, path: str):
        """Checkpoint in the reference format: state dict + "type" + "params"."""
        blob = self.state_dict()
        blob["type"] = "nerf"
        blob["params"] = self.params
        torch.save(blob, path)

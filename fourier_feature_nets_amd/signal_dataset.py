"""A 1-D signal as a regression dataset (reference: signal_dataset.py:11-127).

Names, signatures, the sampling (``linspace(0, 2, num_samples * sample_rate)`` in float32, every
``sample_rate``-th point for training, all of them for validation) and the axis limits follow the
reference.  Additions: ``to(device)``, and ``train_x3`` / ``val_x3``, the (N,3) positions with two
zero columns that ``RegressionEngine`` takes (the kernels' 3-input lift, mlp_engine.EncodingSpec).

``plot`` draws what the reference draws; the arrays it draws come from ``_plot_arrays`` (no figure
needed, so they can be pinned on their own).  The model runs on its own device and the results are
moved to the host.  matplotlib is imported inside ``plot`` only.
"""

from typing import Callable, NamedTuple, Union

import numpy as np
import torch


class SignalData(NamedTuple("FunctionData", [("x", torch.FloatTensor),
                                             ("y", torch.FloatTensor)])):
    """1-D Signal data with x and corresponding y values."""


def _get_limits(vals: Union[np.ndarray, torch.Tensor], stretch=1.1):
    """(min, max) of ``vals`` stretched by ``stretch`` about their midpoint (signal_dataset.py:17-22)."""
    min_x, max_x = vals.min().item(), vals.max().item()
    mid_x = 0.5 * (min_x + max_x)
    min_x = mid_x + stretch * (min_x - mid_x)
    max_x = mid_x + stretch * (max_x - mid_x)
    return min_x, max_x


def _lift(x: torch.Tensor) -> torch.Tensor:
    """(N,1) -> (N,3) float32 with zero columns: the kernels' positions (EncodingSpec's lift)."""
    return torch.nn.functional.pad(x.reshape(-1, 1).to(torch.float32), (0, 2)).contiguous()


class SignalDataset:
    """Dataset consisting of 1-d signal data."""

    def __init__(self, train_data: SignalData, val_data: SignalData):
        """``train_data`` / ``val_data``: (N,1) x and y tensors."""
        self.train_x, self.train_y = train_data
        self.val_x, self.val_y = val_data
        self.x_lim = _get_limits(self.val_x)
        self.y_lim = _get_limits(self.val_y)
        self._lifted = {}

    @staticmethod
    def create(signal: Callable[[np.ndarray], np.ndarray],
               num_samples: int, sample_rate: int) -> "SignalDataset":
        """``signal`` evaluated at ``num_samples * sample_rate`` points of [0, 2); every
        ``sample_rate``-th point is a training sample, all points are validation samples."""
        x = np.linspace(0, 2, num_samples * sample_rate, endpoint=False).astype(np.float32)
        y = signal(x)
        x = x.reshape(-1, 1)
        y = y.reshape(-1, 1)
        train_data = SignalData(torch.from_numpy(x[::sample_rate]),
                                torch.from_numpy(y[::sample_rate]))
        val_data = SignalData(torch.from_numpy(x), torch.from_numpy(y))
        return SignalDataset(train_data, val_data)

    def to(self, device) -> "SignalDataset":
        """The same dataset with its tensors on ``device``."""
        return SignalDataset(SignalData(self.train_x.to(device), self.train_y.to(device)),
                             SignalData(self.val_x.to(device), self.val_y.to(device)))

    def _lift_cached(self, name: str, x: torch.Tensor) -> torch.Tensor:
        out = self._lifted.get(name)
        if out is None:
            out = self._lifted[name] = _lift(x)
        return out

    @property
    def train_x3(self) -> torch.Tensor:
        """(N_train, 3) positions for ``RegressionEngine``: x and two zero columns."""
        return self._lift_cached("train", self.train_x)

    @property
    def val_x3(self) -> torch.Tensor:
        """(N_val, 3) positions for ``RegressionEngine``: x and two zero columns."""
        return self._lift_cached("val", self.val_x)

    def _plot_arrays(self, model, num_points: int, max_hidden: int) -> dict:
        """What ``plot`` draws (signal_dataset.py:93-127), as host arrays: ``x_vals`` /
        ``y_vals`` (predictions), ``activation`` (num_points, H) of the last hidden layer,
        ``activation_values`` = activation * w_out + b_out, ``index`` (the units drawn, widest
        range first), and per drawn unit its ``on`` mask (activation > 0)."""
        x_vals = torch.linspace(self.val_x[0, 0].cpu(), self.val_x[-1, 0].cpu(), num_points)
        device = model.layers[-1].weight.device
        was_training = model.training
        model.eval()
        model.keep_activations = True
        try:
            with torch.no_grad():
                y_vals = model(x_vals.reshape(-1, 1).to(device)).reshape(-1)
                y_vals = y_vals.cpu().numpy()
        finally:
            model.keep_activations = False
            model.train(was_training)

        slope = model.layers[-1].weight.data.detach().cpu().numpy().reshape(-1)
        bias = model.layers[-1].bias.data.item()
        activation = model.activations[-1]
        activation_values = activation * slope[np.newaxis, :] + bias
        activation_range = activation_values.max(0) - activation_values.min(0)
        index = np.argsort(activation_range)[::-1]
        index = index[:max_hidden]
        return {"x_vals": x_vals.numpy(), "y_vals": y_vals, "activation": activation,
                "activation_values": activation_values, "activation_range": activation_range,
                "index": index, "on": [activation[:, i] > 0 for i in index],
                "hidden_ylim": _get_limits(activation_values[activation > 0])}

    def plot(self, space_ax, hidden_ax, model, num_points: int, colors: np.ndarray,
             max_hidden: int):
        """Plots the model to the given matplotlib axes: on ``hidden_ax`` the ``max_hidden``
        last-layer units with the widest range, each as activation * slope + bias with its
        active points; on ``space_ax`` the validation signal, the training samples and the
        predictions at ``num_points`` points.  ``colors``: (num_points, 3) per-point colours."""
        import matplotlib.pyplot as plt

        arr = self._plot_arrays(model, num_points, max_hidden)
        x_vals, activation_values = arr["x_vals"], arr["activation_values"]
        cmap = plt.get_cmap("jet")
        for rank, (i, on_index) in enumerate(zip(arr["index"], arr["on"])):
            act_y = activation_values[:, i]
            hidden_ax.plot(x_vals, act_y, color=cmap(rank / max_hidden)[:3], zorder=1,
                           label="h{:02d}".format(i))
            hidden_ax.scatter(x_vals[on_index], act_y[on_index], color=colors[on_index],
                              marker=".", zorder=2)

        hidden_ax.set_ylim(*arr["hidden_ylim"])
        hidden_ax.legend(loc="upper right", ncol=2)
        space_ax.set_xlim(*self.x_lim)
        space_ax.set_ylim(*self.y_lim)
        space_ax.plot(self.val_x.cpu().numpy(), self.val_y.cpu().numpy(), "r-", label="val",
                      zorder=1)
        space_ax.plot(self.train_x.cpu().numpy(), self.train_y.cpu().numpy(), "go", label="train",
                      zorder=2)
        space_ax.scatter(x_vals, arr["y_vals"], color=colors, marker="P", label="pred", zorder=3)
        space_ax.legend()

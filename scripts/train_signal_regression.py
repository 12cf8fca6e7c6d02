"""Trains a 1-D Fourier-feature network to fit a signal on the MI355X path (counterpart of the
reference's train_signal_regression.py: same positionals, flags, model, loop, report lines and
log.txt).

The loop is the reference's: num_steps + 1 iterations of one full-batch Adam step each (lr 5e-4,
coupled weight decay 1e-3, no clipping, no decay); at every 50th step and the last, the model is
validated AFTER that step's update, while the printed training loss is the one computed before it.
Each step is one RegressionEngine.step with the linear MSE (fused MLP forward, K11b, fused backward,
K7) and no host sync.  Unless --no-plot is given, each report's figure is rendered with matplotlib's
Agg canvas to <results_dir>/frame_NNNNN.png (the reference shows it in a window and can record an
MP4; neither is available here).
"""

import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fourier_feature_nets_amd as ffn  # noqa: E402
from scripts import _cli  # noqa: E402

LEARNING_RATE = 5e-4      # train_signal_regression.py:119-123 (both branches)
WEIGHT_DECAY = 1e-3       # train_signal_regression.py:141
REPORT_INTERVAL = 50
MAX_FREQUENCIES = 256     # the encoder's limit (mlp_engine.EncodingSpec)


def _sections(x):
    """Which half-unit section of [0, 2) each x lies in: 0, 1, 2 or 3."""
    return np.minimum(np.floor(x * 2), 3)


def multifreq(x):
    """2 + sin(pi x) + 0.5 sin(2 pi x) - 0.2 cos(5 pi x)."""
    return 2 + np.sin(x * np.pi) + 0.5 * np.sin(2 * x * np.pi) - 0.2 * np.cos(5 * x * np.pi)


def sawtooth(x):
    """Rises with slope 1 from 0 on each half-unit section."""
    return (x - 0.5 * _sections(x)).astype(x.dtype)


def triangle(x):
    """Rises on even half-unit sections, falls on odd ones, between 0 and 0.5."""
    k = _sections(x)
    return np.where(k % 2 == 0, x - 0.5 * k, 0.5 * (k + 1) - x).astype(x.dtype)


SIGNALS = {"multifreq": multifreq, "sawtooth": sawtooth, "triangle": triangle}


def build_model(args, dataset):
    """FourierFeatureMLP(1, 1, a, b, [num_channels] * num_layers) with the output bias set to the
    mean training target the reference's way (a 0-d tensor), on the host."""
    if args.fourier:
        b_values = torch.from_numpy(
            np.arange(1, args.num_samples // 2 + 1).astype(np.float32)).reshape(1, -1)
        a_values = torch.from_numpy(1 / np.arange(1, args.num_samples // 2 + 1).astype(np.float32))
    else:
        a_values = b_values = None
    model = ffn.FourierFeatureMLP(1, 1, a_values, b_values, [args.num_channels] * args.num_layers)
    model.layers[-1].bias.data = dataset.train_y.mean()
    return model


class Frames:
    """The reference's two-panel figure (hidden-layer basis | signal space) on an Agg canvas,
    written as PNG frames."""

    def __init__(self, args):
        from matplotlib.backends.backend_agg import FigureCanvasAgg
        from matplotlib.figure import Figure
        import matplotlib.pyplot as plt
        width, height = [int(val) for val in args.resolution.split("x")]
        self.fig = Figure(figsize=(width / 100, height / 100), dpi=100)
        self.canvas = FigureCanvasAgg(self.fig)
        self.colors = plt.get_cmap("viridis")(np.linspace(0, 1, args.num_plot))[..., :3]
        self.hidden_ax = self.fig.add_subplot(121)
        self.space_ax = self.fig.add_subplot(122)
        self.args = args
        self.count = 0

    def write(self, dataset, model, val_loss, step):
        args = self.args
        self.space_ax.cla()
        self.hidden_ax.cla()
        self.hidden_ax.set_title("Hidden Layer Basis")
        self.space_ax.set_title("{}MLP {}x{} {:.3f}@{:05d}".format(
            "Fourier " if args.fourier else "", args.num_layers, args.num_channels, val_loss, step))
        dataset.plot(self.space_ax, self.hidden_ax, model, args.num_plot, self.colors,
                     args.max_hidden)
        self.fig.tight_layout()
        self.canvas.draw()
        pixels = np.ascontiguousarray(np.asarray(self.canvas.buffer_rgba())[..., :3])
        _cli.save_png(os.path.join(args.results_dir, "frame_{:05d}.png".format(self.count)), pixels)
        self.count += 1


def train_loop(engine, data, num_steps, report=None, losses=None):
    """train_signal_regression.py:153-182 without the display: ``num_steps + 1`` engine steps on
    the full training set; at every REPORT_INTERVAL-th step and the last, the validation loss
    AFTER that step's update and the training loss from BEFORE it go to
    ``report(step, train_loss, val_loss)`` and into the returned log.  ``losses``, if given,
    collects every step's training loss as a device scalar (no host sync)."""
    train_x3, train_y = data.train_x3, data.train_y
    val_x3, val_y = data.val_x3, data.val_y
    log = []
    for step in range(num_steps + 1):
        loss = engine.step(train_x3, train_y, LEARNING_RATE)
        if losses is not None:
            losses.append(loss)
        if step % REPORT_INTERVAL == 0 or step == num_steps:
            val_loss = engine.validation_loss(val_x3, val_y).item()
            if report is not None:
                report(step, loss.item(), val_loss)
            log.append((step, loss.item(), val_loss))
    return log


def main():
    args = _cli.build_parser("1-D Signal Regression", _cli.SIGNAL_REGRESSION).parse_args()
    if args.fourier and args.num_samples // 2 > MAX_FREQUENCIES:
        raise NotImplementedError("encodings with more than 256 frequencies")
    args.device, _, _, _ = _cli.setup_device(args.device, False)
    if args.make_video:
        # (train_signal_regression.py:142-148 writes an MP4 with scenepic: outside the HIP hot path)
        print("warning: --make-video is not supported on the HIP path; the frame_NNNNN.png frames "
              "are written instead", file=sys.stderr)
        args.no_plot = False
    if not args.no_plot:
        # (train_signal_regression.py:176 also shows every frame in an on-screen window)
        print("note: no on-screen progress window on the HIP path; see the frame_NNNNN.png frames",
              file=sys.stderr)

    dataset = ffn.SignalDataset.create(SIGNALS[args.signal], args.num_samples, args.sample_rate)
    model = build_model(args, dataset).to(args.device)
    os.makedirs(args.results_dir, exist_ok=True)
    frames = None if args.no_plot else Frames(args)

    engine = ffn.RegressionEngine(model, weight_decay=WEIGHT_DECAY, loss="linear")

    def report(step, train_loss, val_loss):
        if frames is not None:
            frames.write(dataset, model, val_loss, step)
        print(step, "train:", train_loss, "val:", val_loss)

    log = train_loop(engine, dataset.to(args.device), args.num_steps, report)
    with open(os.path.join(args.results_dir, "log.txt"), "w") as file:
        file.write("step\ttrain_loss\tval_loss\n")
        for i, train_loss, val_loss in log:
            file.write("{}\t{}\t{}\n".format(i, train_loss, val_loss))
    return 0


if __name__ == "__main__":
    sys.exit(main())

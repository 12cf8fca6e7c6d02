"""Generates the 1-D signal regression fixtures FROM THE REFERENCE ITSELF (only where a checkout of
the reference is available read-only at make_goldens.REFERENCE):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_signal_regression.py

- signal_regression.npz:
  - ``create/<signal>/<field>``: the reference ``SignalDataset.create`` (its own signal functions)
    for the three signals at the default 32 samples x rate 8 and at CREATE_ODD: train / val x and
    y, ``x_lim``, ``y_lim``.
  - ``<run>/...`` for each of RUNS: the reference's own ``train_signal_regression._main`` on CPU,
    ``--no-plot``, the global RNG seeded with SEED: the initial state after the 0-d bias
    assignment (``init/<key>``), every step's training loss (``loss``, float32 as printed), the
    report lines (``report_lines``, ``report_step``, ``report_train``, ``report_val``), the
    state after the update of each step in CHECKPOINTS (``state<step>/<key>``; the last is the
    final state) and the run's ``args``.
  - ``plot/...``: what the reference's ``SignalDataset.plot`` draws (real matplotlib, Agg) for the
    final state of PLOT_RUN: the hidden-basis lines' xy data and their labels in order, the
    hidden scatters' offsets, the hidden axis' y limits, and the space axis' val / train lines and
    prediction offsets.
- cli_defaults_signal_regression.json: the reference parser's defaults.
- api_signatures_signal.json: the ``SignalDataset`` / ``SignalData`` signatures.

cv2 is absent: on top of make_goldens' stand-ins, imshow / waitKey / cvtColor do nothing (the runs
are headless).  Outputs are plain data.
"""

import contextlib
import importlib.util
import inspect
import io
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

SEED = 20080524
NUM_STEPS = 10000                       # the reference's default --num-steps
CHECKPOINTS = [200, 1000, NUM_STEPS]
RUNS = {"multifreq": ["multifreq"],
        "multifreq_fourier": ["multifreq", "--fourier"],
        "sawtooth_fourier": ["sawtooth", "--fourier"],
        "triangle": ["triangle"]}
PLOT_RUN = "multifreq_fourier"
PLOT_POINTS, PLOT_HIDDEN = 48, 10       # --num_plot, --max-hidden defaults
CREATE_ODD = (20, 5)                    # a second (num_samples, sample_rate)
CLI_ARGV = ["multifreq", "out"]
SIGNAL_METHODS = ["__init__", "create", "plot"]


def _cv2_stubs():
    cv2 = sys.modules["cv2"]
    cv2.COLOR_RGB2BGR = 11
    cv2.cvtColor = lambda pixels, code: pixels
    cv2.imshow = lambda *a, **k: None
    cv2.waitKey = lambda *a, **k: -1


def _describe(fn):
    out = []
    for p in inspect.signature(fn).parameters.values():
        if p.name in ("self", "cls"):
            continue
        default = None if p.default is inspect.Parameter.empty else repr(p.default)
        out.append({"name": p.name, "kind": p.kind.name, "default": default})
    return out


def _state(model):
    return {k: v.detach().clone().numpy() for k, v in model.state_dict().items()}


def _run_training(mod, ffn_ref, argv_tail, out):
    """One _main run; returns (arrays, final model, dataset)."""
    _cv2_stubs()
    captured = {}
    cls = ffn_ref.FourierFeatureMLP
    orig_init = cls.__init__

    def init(self, *a, **k):
        orig_init(self, *a, **k)
        captured["model"] = self

    orig_create = mod.SignalDataset.create

    def create(*a, **k):
        captured["dataset"] = orig_create(*a, **k)
        return captured["dataset"]

    adam = torch.optim.Adam
    orig_adam_init, orig_step = adam.__init__, adam.step
    states, counter = {}, [0]

    def adam_init(self, *a, **k):        # train_signal_regression.py:141, after the bias assignment
        captured["init"] = _state(captured["model"])
        orig_adam_init(self, *a, **k)

    def adam_step(self, *a, **k):
        res = orig_step(self, *a, **k)
        step = counter[0]
        counter[0] += 1
        if step in CHECKPOINTS:
            states[step] = _state(captured["model"])
        return res

    losses = []
    orig_backward = torch.Tensor.backward

    def backward(self, *a, **k):
        losses.append(float(self))
        return orig_backward(self, *a, **k)

    argv = ["train_signal_regression.py"] + argv_tail[:1] + [out] + argv_tail[1:] + [
        "--no-plot", "--num-steps", str(NUM_STEPS)]
    old_argv = sys.argv
    cls.__init__, mod.SignalDataset.create, sys.argv = init, staticmethod(create), argv
    adam.__init__, adam.step, torch.Tensor.backward = adam_init, adam_step, backward
    buf = io.StringIO()
    try:
        torch.manual_seed(SEED)
        np.random.seed(SEED)
        with contextlib.redirect_stdout(buf):
            mod._main()
    finally:
        cls.__init__, mod.SignalDataset.create, sys.argv = orig_init, staticmethod(orig_create), old_argv
        adam.__init__, adam.step, torch.Tensor.backward = orig_adam_init, orig_step, orig_backward
    lines = [ln for ln in buf.getvalue().splitlines() if " train: " in ln]
    with open(os.path.join(out, "log.txt")) as f:
        log = f.read()
    arrays = {"loss": np.array(losses, np.float32),
              "report_lines": np.array(lines),
              "report_step": np.array([int(ln.split()[0]) for ln in lines], np.int64),
              "report_train": np.array([float(ln.split()[2]) for ln in lines], np.float64),
              "report_val": np.array([float(ln.split()[4]) for ln in lines], np.float64),
              "log_txt": np.array(log),
              "args": np.array(json.dumps(argv[1:]))}
    assert np.array_equal(arrays["loss"].astype(np.float64), np.array(losses))   # f32 as printed
    for key, value in captured["init"].items():
        arrays["init/" + key] = value
    for step, state in states.items():
        for key, value in state.items():
            arrays["state%d/%s" % (step, key)] = value
    return arrays, captured["model"], captured["dataset"]


def _plot_arrays(dataset, model):
    """The reference's SignalDataset.plot on a real Agg figure; the data of what it drew."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    fig = plt.figure(figsize=(12.8, 7.2), dpi=100)
    colors = plt.get_cmap("viridis")(np.linspace(0, 1, PLOT_POINTS))[..., :3]
    hidden_ax, space_ax = fig.add_subplot(121), fig.add_subplot(122)
    dataset.plot(space_ax, hidden_ax, model, PLOT_POINTS, colors, PLOT_HIDDEN)
    out = {"plot/labels": np.array([ln.get_label() for ln in hidden_ax.lines]),
           "plot/hidden_ylim": np.array(hidden_ax.get_ylim(), np.float64),
           "plot/space_xlim": np.array(space_ax.get_xlim(), np.float64),
           "plot/space_ylim": np.array(space_ax.get_ylim(), np.float64),
           "plot/val_line": np.asarray(space_ax.lines[0].get_xydata(), np.float64),
           "plot/train_line": np.asarray(space_ax.lines[1].get_xydata(), np.float64),
           "plot/pred": np.asarray(space_ax.collections[0].get_offsets(), np.float64),
           "plot/colors": colors}
    for k, ln in enumerate(hidden_ax.lines):
        out["plot/hidden_line%d" % k] = np.asarray(ln.get_xydata(), np.float64)
    for k, col in enumerate(hidden_ax.collections):
        out["plot/hidden_scatter%d" % k] = np.asarray(col.get_offsets(), np.float64)
    plt.close(fig)
    return out


def main():
    sys.path.insert(0, HERE)
    from make_goldens import REFERENCE, _install_stubs
    _install_stubs()
    _cv2_stubs()
    sys.path.insert(0, REFERENCE)
    sys.dont_write_bytecode = True
    torch.set_num_threads(4)
    import fourier_feature_nets as ffn_ref
    from fourier_feature_nets.signal_dataset import SignalData, SignalDataset

    spec = importlib.util.spec_from_file_location(
        "ref_train_signal_regression", os.path.join(REFERENCE, "train_signal_regression.py"))
    mod = importlib.util.module_from_spec(spec)
    with contextlib.redirect_stdout(io.StringIO()):
        spec.loader.exec_module(mod)

    old = sys.argv
    sys.argv = ["train_signal_regression.py"] + CLI_ARGV
    try:
        cli = {"train_signal_regression": vars(mod._parse_args())}
    finally:
        sys.argv = old
    with open(os.path.join(HERE, "cli_defaults_signal_regression.json"), "w") as f:
        json.dump(cli, f, indent=1, sort_keys=True)

    sig = {"SignalDataset": {m: _describe(getattr(SignalDataset, m)) for m in SIGNAL_METHODS},
           "SignalData_fields": list(SignalData._fields)}
    with open(os.path.join(HERE, "api_signatures_signal.json"), "w") as f:
        json.dump(sig, f, indent=1, sort_keys=True)

    blob = {"seed": np.array(SEED), "num_steps": np.array(NUM_STEPS),
            "checkpoints": np.array(CHECKPOINTS), "create_odd": np.array(CREATE_ODD)}
    functions = {"multifreq": mod._multifreq, "sawtooth": mod._sawtooth, "triangle": mod._triangle}
    for tag, (samples, rate) in (("", (32, 8)), ("_odd", CREATE_ODD)):
        for name, fn in functions.items():
            ds = SignalDataset.create(fn, samples, rate)
            pre = "create%s/%s/" % (tag, name)
            blob[pre + "train_x"], blob[pre + "train_y"] = ds.train_x.numpy(), ds.train_y.numpy()
            blob[pre + "val_x"], blob[pre + "val_y"] = ds.val_x.numpy(), ds.val_y.numpy()
            blob[pre + "x_lim"] = np.array(ds.x_lim, np.float64)
            blob[pre + "y_lim"] = np.array(ds.y_lim, np.float64)

    for run, argv_tail in RUNS.items():
        with tempfile.TemporaryDirectory() as out:
            arrays, model, dataset = _run_training(mod, ffn_ref, argv_tail, out)
        for key, value in arrays.items():
            blob["%s/%s" % (run, key)] = value
        if run == PLOT_RUN:
            blob.update(_plot_arrays(dataset, model))
        print(run, "val", arrays["report_val"][[0, 1, 4, 20, -1]].tolist())
    np.savez_compressed(os.path.join(HERE, "signal_regression.npz"), **blob)
    print("wrote signal_regression.npz, cli_defaults_signal_regression.json, "
          "api_signatures_signal.json")


if __name__ == "__main__":
    main()

"""Host side of 1-D signal regression: SignalDataset.create against the reference's own outputs
(tests/golden/signal_regression.npz), the SignalDataset / SignalData signatures and the
train_signal_regression.py parser against the reference's (tests/golden/make_signal_regression.py),
the new K11b entry points in the C header, and the parameter checks that guard the pack table."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fourier_feature_nets_amd as ffn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
SIGNALS = ["multifreq", "sawtooth", "triangle"]


@pytest.fixture(scope="module")
def sig():
    return np.load(os.path.join(GOLDEN, "signal_regression.npz"))


@pytest.mark.parametrize("tag", ["", "_odd"])
@pytest.mark.parametrize("name", SIGNALS)
def test_signal_dataset_create_matches_the_reference(sig, name, tag):
    """Samples, targets (float32 for all three signals) and axis limits, bit for bit."""
    from scripts.train_signal_regression import SIGNALS as functions
    samples, rate = (32, 8) if tag == "" else tuple(int(v) for v in sig["create_odd"])
    ds = ffn.SignalDataset.create(functions[name], samples, rate)
    pre = "create%s/%s/" % (tag, name)
    for field in ("train_x", "train_y", "val_x", "val_y"):
        got = getattr(ds, field)
        ref = sig[pre + field]
        assert got.dtype == torch.float32 and ref.dtype == np.float32, field
        assert tuple(got.shape) == ref.shape and got.shape[1] == 1, field
        assert np.array_equal(got.numpy(), ref), (name, field)
    assert ds.train_x.shape[0] == samples and ds.val_x.shape[0] == samples * rate
    assert ds.x_lim == tuple(sig[pre + "x_lim"]) and ds.y_lim == tuple(sig[pre + "y_lim"])
    # the engine's lifted positions: x and two zero columns
    x3 = ds.train_x3
    assert tuple(x3.shape) == (samples, 3) and x3.is_contiguous()
    assert torch.equal(x3[:, :1], ds.train_x) and not x3[:, 1:].any()
    moved = ds.to("cpu")
    assert torch.equal(moved.val_y, ds.val_y) and moved.y_lim == ds.y_lim


def test_signatures_match_the_reference():
    from tests.test_alias_cpu import _check
    with open(os.path.join(GOLDEN, "api_signatures_signal.json")) as f:
        api = json.load(f)
    import fourier_feature_nets as alias
    from fourier_feature_nets.signal_dataset import SignalData, SignalDataset
    assert alias.SignalDataset is SignalDataset is ffn.SignalDataset
    assert alias.SignalData is SignalData is ffn.SignalData
    for method, params in api["SignalDataset"].items():
        _check(getattr(SignalDataset, method), params, "SignalDataset." + method)
    assert list(SignalData._fields) == api["SignalData_fields"]


def test_importing_the_package_does_not_import_matplotlib():
    code = "import sys, fourier_feature_nets; assert 'matplotlib' not in sys.modules"
    res = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True,
                         timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]


def test_train_signal_regression_parser_equals_the_reference():
    from scripts import _cli
    from tests.golden.make_signal_regression import CLI_ARGV
    with open(os.path.join(GOLDEN, "cli_defaults_signal_regression.json")) as f:
        ref = json.load(f)["train_signal_regression"]
    mine = vars(_cli.build_parser("t", _cli.SIGNAL_REGRESSION).parse_args(CLI_ARGV))
    assert mine.pop("device") == "cuda"          # appended, as in the other drivers
    assert mine == ref


def test_mse_entry_points_are_declared():
    from fourier_feature_nets_amd import _lib
    names = _lib.declared_symbols()
    for name in ("ffn_regression_mse_train", "ffn_regression_mse_eval", "ffn_regression_mse_loss"):
        assert name in names, name
    assert _lib.ABI_VERSION == 3


def test_driver_builds_the_reference_model_with_a_0d_bias(sig):
    """--fourier: b = arange(1, 17) as (1, 16), a = 1 / b; the output bias is the 0-d mean of the
    training targets -- the initial state's shapes equal the fixture's."""
    import argparse
    from scripts.train_signal_regression import SIGNALS as functions, build_model
    ds = ffn.SignalDataset.create(functions["multifreq"], 32, 8)
    for fourier, run in ((False, "multifreq"), (True, "multifreq_fourier")):
        args = argparse.Namespace(fourier=fourier, num_samples=32, num_channels=64, num_layers=1)
        model = build_model(args, ds)
        state = model.state_dict()
        ref = {k[len(run) + 6:]: sig[k] for k in sig.files if k.startswith(run + "/init/")}
        assert sorted(state) == sorted(ref)
        for key, value in ref.items():
            assert tuple(state[key].shape) == value.shape, key
        assert model.layers[-1].bias.dim() == 0
        assert np.array_equal(model.layers[-1].bias.detach().numpy(), ref["layers.1.bias"])
        for key in ("a_values", "b_values"):
            if key in ref:
                assert np.array_equal(state[key].numpy(), ref[key])


def test_driver_refuses_more_frequencies_than_the_encoder_has(tmp_path):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train_signal_regression.py"),
                          "multifreq", str(tmp_path / "out"), "--fourier", "--num-samples", "514",
                          "--device", "cpu"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert res.returncode != 0
    assert "NotImplementedError: encodings with more than 256 frequencies" in res.stderr


@pytest.mark.parametrize("bad", ["shape", "dtype", "device"])
def test_parameter_checks_refuse_before_any_copy(bad):
    """check_params (run before the pack table and the engine's flat buffer are built) refuses a
    bias of the wrong size or type, and one on another device than the model."""
    model = ffn.FourierFeatureMLP(1, 1, None, None, [32])
    model.check_params(torch.device("cpu"))                      # a (1,) bias
    model.layers[-1].bias.data = torch.tensor(0.5)               # a 0-d bias
    model.check_params(torch.device("cpu"))
    if bad == "shape":
        model.layers[-1].bias.data = torch.zeros(2)
        with pytest.raises(ValueError, match="bias of shape"):
            model.check_params(torch.device("cpu"))
    elif bad == "dtype":
        model.layers[0].weight.data = model.layers[0].weight.data.double()
        with pytest.raises(TypeError, match="float32"):
            model.check_params(torch.device("cpu"))
    else:
        with pytest.raises(RuntimeError, match="lives on cpu"):
            model.check_params(torch.device("cuda", 0))

"""Host side of 2-D image regression: PixelDataset against the reference's own outputs
(tests/golden/pixel_dataset.npz), its signatures and the train_image_regression.py parser against
the reference's (tests/golden/make_image_regression.py), and the lift of 1- and 2-input chains to
the kernels' 3-input encoding (EncodingSpec column maps, operand maps, gradient layout)."""

import json
import math
import os

import numpy as np
import pytest
import torch

import fourier_feature_nets_amd as ffn
from fourier_feature_nets_amd.mlp_engine import EncodingSpec, MlpProgram

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")


@pytest.fixture(scope="module")
def pix():
    return np.load(os.path.join(GOLDEN, "pixel_dataset.npz"))


def _check_against_golden(ds, pix):
    f32 = lambda a: torch.from_numpy(np.asarray(a)).to(torch.float32)   # noqa: E731
    assert ds.train_uv.dtype == torch.float32 and ds.train_color.dtype == torch.float32
    assert torch.equal(ds.train_uv, f32(pix["train_uv"]))
    assert torch.equal(ds.val_uv, f32(pix["val_uv"]))
    # targets are float32 (the reference keeps float64): the correctly rounded k / 255
    assert torch.equal(ds.train_color, f32(pix["train_color"]))
    assert torch.equal(ds.val_color, f32(pix["val_color"]))
    assert tuple(ds.train_uv.shape) == (32, 32, 2) and tuple(ds.train_color.shape) == (32, 32, 3)
    assert np.array_equal(ds.image, pix["image"])


def test_pixel_dataset_from_array_matches_the_reference(pix):
    ds = ffn.PixelDataset.from_array(pix["source"], "RGB", 64)
    _check_against_golden(ds, pix)
    colors = torch.from_numpy(pix["colors"])
    assert np.array_equal(ds.to_image(colors), pix["to_image"])
    assert np.array_equal(ds.to_image(colors[:32 * 32], 32), pix["to_image_half"])
    assert np.array_equal(ffn.PixelDataset.generate_uvs(10, "cpu").numpy(), pix["uvs_10"])
    # PSNR against float32 targets: within 1e-4 dB of the reference's float64 ones
    for key, ref in (("colors", "psnr_colors"), ("near", "psnr_near")):
        got = ds.psnr(torch.from_numpy(pix[key]).reshape(64, 64, 3))
        assert abs(got - float(pix[ref])) < 1e-4, (key, got, float(pix[ref]))
    # the (N,3) lifted uvs the engine takes: row-major over the grid, zero third column
    uv3 = ds.train_uv3
    assert tuple(uv3.shape) == (32 * 32, 3) and uv3.is_contiguous()
    assert torch.equal(uv3[:, :2], ds.train_uv.reshape(-1, 2)) and not uv3[:, 2].any()
    assert torch.equal(ds.train_color_flat, ds.train_color.reshape(-1, 3))
    moved = ds.to("cpu")
    assert torch.equal(moved.val_color, ds.val_color) and moved.size == 64


def test_pixel_dataset_create_decodes_a_png(tmp_path, pix):
    from PIL import Image
    path = str(tmp_path / "img.png")
    Image.fromarray(pix["source"]).save(path)
    _check_against_golden(ffn.PixelDataset.create(path, "RGB", 64), pix)
    assert ffn.PixelDataset.create(str(tmp_path / "missing.png"), "RGB", 64) is None


def test_pixel_dataset_area_resize_is_the_block_mean():
    rng = np.random.RandomState(0)
    big = rng.randint(0, 256, (128, 160, 3)).astype(np.uint8)   # crop to 128 x 128, 2:1
    ds = ffn.PixelDataset.from_array(big, "RGB", 64)
    crop = big[:, 16:144].astype(np.int64)
    mean = (crop.reshape(64, 2, 64, 2, 3).sum(axis=(1, 3)) + 2) // 4
    assert np.array_equal(ds.image, mean.astype(np.uint8))
    with pytest.raises(NotImplementedError):
        ffn.PixelDataset.from_array(big, "HSV", 64)


def test_signatures_match_the_reference():
    from tests.test_alias_cpu import _check
    with open(os.path.join(GOLDEN, "api_signatures_pixels.json")) as f:
        api = json.load(f)
    import fourier_feature_nets as alias
    from fourier_feature_nets.pixel_dataset import PixelData, PixelDataset
    assert alias.PixelDataset is PixelDataset is ffn.PixelDataset
    assert PixelData is ffn.PixelData
    for method, params in api["PixelDataset"].items():
        _check(getattr(PixelDataset, method), params, "PixelDataset." + method)
    assert list(PixelData._fields) == api["PixelData_fields"]


def test_train_image_regression_parser_equals_the_reference():
    from scripts import _cli
    from tests.golden.make_image_regression import CLI_ARGV
    with open(os.path.join(GOLDEN, "cli_defaults_image_regression.json")) as f:
        ref = json.load(f)["train_image_regression"]
    mine = vars(_cli.build_parser("t", _cli.IMAGE_REGRESSION).parse_args(CLI_ARGV))
    assert mine == ref


@pytest.mark.parametrize("num_inputs", [1, 2, 3])
@pytest.mark.parametrize("freq,include", [(0, True), (5, False), (64, False), (30, True)])
def test_encoding_raw_channels_past_d_have_no_column(num_inputs, freq, include):
    b = None if freq == 0 else torch.randn(num_inputs, freq)
    enc = EncodingSpec(b, None, math.pi, include, torch.device("cpu"), num_inputs=num_inputs)
    raw = num_inputs if enc.include_input else 0
    assert enc.natural_width == 2 * freq + raw
    assert tuple(enc.b.shape) == (3, max(freq, 1))
    if b is not None:
        assert torch.equal(enc.b[:num_inputs], b) and not enc.b[num_inputs:].any()
    nat = [enc.natural_index(c) for c in range(enc.width)]
    assert sorted(n for n in nat if n >= 0) == list(range(enc.natural_width))
    for d in range(3):
        expect = 2 * freq + d if (enc.include_input and d < num_inputs) else -1
        if 2 * freq + d < enc.width:
            assert nat[2 * freq + d] == expect


def test_encoding_refuses_unsupported_input_counts():
    with pytest.raises(NotImplementedError):
        EncodingSpec(torch.zeros(4, 8), None, 1.0, False, torch.device("cpu"), num_inputs=4)
    with pytest.raises(ValueError):
        EncodingSpec(torch.zeros(3, 8), None, 1.0, False, torch.device("cpu"), num_inputs=2)
    model = ffn.FourierFeatureMLP(4, 3, torch.ones(8), torch.zeros(4, 8), [32])
    with pytest.raises(NotImplementedError, match="1, 2 or 3 inputs"):
        model._chain(torch.device("cpu"))


@pytest.mark.parametrize("make", [
    lambda d: ffn.MLP(d, 3, num_channels=64),
    lambda d: ffn.BasicFourierMLP(d, 3, num_channels=64),
    lambda d: ffn.PositionalFourierMLP(d, 3, 6, num_channels=256, embedding_size=256),
    lambda d: ffn.GaussianFourierMLP(d, 3, 10.0, num_channels=32, embedding_size=48),
])
@pytest.mark.parametrize("d", [1, 2])
def test_low_dimensional_chains_line_up_with_nn_linear(make, d):
    torch.manual_seed(0)
    model = make(d)
    enc, specs = model._chain(torch.device("cpu"))
    prog = MlpProgram(enc, specs, torch.device("cpu"), planning_only=True)
    first = model.layers[0]
    e = prog.encodings[0]
    assert first.in_features == e.natural_width            # 2F (+ D for the plain MLP)
    # the first layer's operand map: every nn.Linear column once, -1 elsewhere (zero weights)
    cmap = prog.col_maps[0].tolist()
    assert sorted(c for c in cmap if c >= 0) == list(range(first.in_features))
    assert len(cmap) == e.width
    # gradient buffer = [W0 (out x in), b0, W1, b1, ...] at nn.Linear's own shapes
    off = 0
    for i, layer in enumerate(model.layers):
        assert prog.grad_w_off[i] == off
        off += layer.weight.numel()
        assert prog.grad_b_off[i] == off
        off += layer.bias.numel()
    assert prog.num_grad_floats == off
    # the reducer writes only mapped columns: the raw channels past D appear in no reduce job's map
    raw_past_d = [c for c in range(e.width) if e.include_input and 2 * e.num_freq + d <= c < 2 * e.num_freq + 3]
    assert all(cmap[c] == -1 for c in raw_past_d)

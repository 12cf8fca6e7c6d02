"""Generates the 2-D image regression fixtures FROM THE REFERENCE ITSELF (build container only,
reference mounted read-only at /root/reference):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_image_regression.py

- image_regression.npz: the reference's own ``train_image_regression._main`` on CPU with a seeded
  global RNG, on a synthetic 64 x 64 u8 image (``synthetic_image``), NUM_STEPS steps reporting every
  REPORT, for the mlp, positional and gaussian models with CHANNELS channels and embedding size: the initial state (``<model>/init/<key>``),
  every step's train loss (``<model>/loss``), the report lines (``<model>/report_step``,
  ``/report_psnr``, ``/report_lr``) and the final state (``<model>/final/<key>``).
- pixel_dataset.npz: uv grids, training colours, ``image`` / ``to_image`` bytes and ``psnr`` values
  of the reference ``PixelDataset`` (a 64 x 80 image: centre crop, no resize).
- cli_defaults_image_regression.json: the reference parser's defaults.
- api_signatures_pixels.json: the ``PixelDataset`` / ``PixelData`` signatures.

cv2 is absent: on top of make_goldens' stand-ins, imread returns the synthetic image (BGR),
cvtColor swaps BGR <-> RGB (RGB colour space only), imwrite / imshow / waitKey do nothing.  No
resize is reached (the image is already at --image-size).  Outputs are plain data.
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

SIZE, NUM_STEPS, REPORT, SEED = 64, 40, 10, 20080524
CHANNELS = 64           # --num-channels and --embedding_size (small: the fixture stores weights)
MODELS = ["mlp", "positional", "gaussian"]
CLI_ARGV = ["img.png", "positional", "out"]
PIXEL_METHODS = ["__init__", "create", "to", "to_act_image", "to_image", "generate_uvs", "psnr"]


def synthetic_image(height=SIZE, width=SIZE):
    """(H,W,3) u8 RGB: smooth ramps, a disc, stripes of rising frequency and a little noise --
    detail that separates the Fourier-feature models from the plain MLP."""
    rng = np.random.RandomState(7)
    yy, xx = np.mgrid[0:height, 0:width].astype(np.float64)
    u, v = xx / width, yy / height
    r = 0.5 + 0.4 * np.sin(2 * np.pi * u) * np.cos(np.pi * v)
    g = np.where((u - 0.45) ** 2 + (v - 0.55) ** 2 < 0.07, 0.9, 0.2 + 0.5 * v)
    b = 0.5 + 0.45 * np.sin(2 * np.pi * (2 + 10 * u) * u) * (v > 0.5) + 0.1 * (v <= 0.5)
    img = np.stack([r, g, b], -1) * 255 + rng.randint(-6, 7, (height, width, 3))
    return np.clip(np.round(img), 0, 255).astype(np.uint8)


def _cv2_stubs(image_rgb):
    cv2 = sys.modules["cv2"]
    cv2.COLOR_BGR2RGB, cv2.COLOR_RGB2BGR, cv2.COLOR_BGR2YCrCb, cv2.COLOR_YCrCb2RGB = 10, 11, 12, 13

    def cvt(pixels, code):
        if code in (cv2.COLOR_BGR2RGB, cv2.COLOR_RGB2BGR):
            return np.ascontiguousarray(pixels[..., ::-1])
        raise NotImplementedError("colour conversion %r is not stubbed" % code)

    def resize(*a, **k):
        raise NotImplementedError("resize is not reached by these fixtures")

    cv2.imread = lambda path: np.ascontiguousarray(image_rgb[..., ::-1])
    cv2.cvtColor = cvt
    cv2.resize = resize
    cv2.imwrite = lambda *a, **k: True
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


def _run_training(mod, ffn_ref, model_name, image, out):
    """One _main run; returns the arrays for this model."""
    _cv2_stubs(image)
    cls = ffn_ref.FourierFeatureMLP
    state = {}
    orig_to = cls.to

    def to(self, *a, **k):             # the first .to() is train_image_regression.py:135
        if "init" not in state:
            state["init"] = {k2: v.detach().clone() for k2, v in self.state_dict().items()}
        return orig_to(self, *a, **k)

    losses = []
    orig_backward = torch.Tensor.backward

    def backward(self, *a, **k):
        losses.append(float(self))
        return orig_backward(self, *a, **k)

    argv = ["train_image_regression.py", "img.png", model_name, out, "--image-size", str(SIZE),
            "--num-steps", str(NUM_STEPS), "--report-interval", str(REPORT), "--device", "cpu",
            "--num-channels", str(CHANNELS), "--embedding_size", str(CHANNELS)]
    old_argv = sys.argv
    cls.to, torch.Tensor.backward, sys.argv = to, backward, argv
    buf = io.StringIO()
    try:
        torch.manual_seed(SEED)
        np.random.seed(SEED)
        with contextlib.redirect_stdout(buf):
            mod._main()
    finally:
        cls.to, torch.Tensor.backward, sys.argv = orig_to, orig_backward, old_argv
    lines = [ln for ln in buf.getvalue().splitlines() if ln.startswith("step ")]
    final = torch.load(os.path.join(out, "model.pt"), map_location="cpu")
    final.pop("type")
    params = final.pop("params")
    arrays = {"loss": np.array(losses, np.float64),
              "report_step": np.array([int(ln.split()[1]) for ln in lines], np.int64),
              "report_psnr": np.array([float(ln.split()[3]) for ln in lines], np.float64),
              "report_lr": np.array([float(ln.split()[5]) for ln in lines], np.float64),
              "report_lines": np.array(lines),
              "params": np.array(json.dumps(params))}
    for key, value in state["init"].items():
        arrays["init/" + key] = value.numpy()
    for key, value in final.items():
        arrays["final/" + key] = value.numpy()
    return arrays


def main():
    sys.path.insert(0, HERE)
    from make_goldens import REFERENCE, _install_stubs
    _install_stubs()
    sys.path.insert(0, REFERENCE)
    sys.dont_write_bytecode = True
    torch.set_num_threads(4)
    image = synthetic_image()
    _cv2_stubs(image)
    import fourier_feature_nets as ffn_ref
    from fourier_feature_nets.pixel_dataset import PixelData, PixelDataset

    spec = importlib.util.spec_from_file_location(
        "ref_train_image_regression", os.path.join(REFERENCE, "train_image_regression.py"))
    mod = importlib.util.module_from_spec(spec)
    with contextlib.redirect_stdout(io.StringIO()):
        spec.loader.exec_module(mod)

    old = sys.argv
    sys.argv = ["train_image_regression.py"] + CLI_ARGV
    try:
        cli = {"train_image_regression": vars(mod._parse_args())}
    finally:
        sys.argv = old
    with open(os.path.join(HERE, "cli_defaults_image_regression.json"), "w") as f:
        json.dump(cli, f, indent=1, sort_keys=True)

    sig = {"PixelDataset": {m: _describe(getattr(PixelDataset, m)) for m in PIXEL_METHODS},
           "PixelData_fields": list(PixelData._fields)}
    with open(os.path.join(HERE, "api_signatures_pixels.json"), "w") as f:
        json.dump(sig, f, indent=1, sort_keys=True)

    # PixelDataset: a 64 x 80 image (centre crop to 64 x 64, no resize)
    wide = synthetic_image(SIZE, SIZE + 16)
    _cv2_stubs(wide)
    ds = PixelDataset.create("img.png", "RGB", SIZE)
    rng = np.random.RandomState(3)
    colors = torch.from_numpy(rng.rand(SIZE * SIZE, 3).astype(np.float32))
    near = (ds.val_color.reshape(-1, 3) + torch.from_numpy(
        rng.normal(0, 0.05, (SIZE * SIZE, 3)))).clamp(0, 1).to(torch.float32)
    pix = {"source": wide, "train_uv": ds.train_uv.numpy(), "train_color": ds.train_color.numpy(),
           "val_uv": ds.val_uv.numpy(), "val_color": ds.val_color.numpy(), "image": ds.image,
           "colors": colors.numpy(), "to_image": ds.to_image(colors),
           "to_image_half": ds.to_image(colors[:(SIZE // 2) ** 2], SIZE // 2),
           "psnr_colors": np.array(ds.psnr(colors.reshape(SIZE, SIZE, 3))),
           "near": near.numpy(), "psnr_near": np.array(ds.psnr(near.reshape(SIZE, SIZE, 3))),
           "uvs_10": PixelDataset.generate_uvs(10, "cpu").numpy()}
    np.savez_compressed(os.path.join(HERE, "pixel_dataset.npz"), **pix)

    blob = {"image": image, "size": np.array(SIZE), "num_steps": np.array(NUM_STEPS),
            "report_interval": np.array(REPORT), "seed": np.array(SEED),
            "channels": np.array(CHANNELS)}
    for name in MODELS:
        with tempfile.TemporaryDirectory() as out:
            arrays = _run_training(mod, ffn_ref, name, image, out)
        for key, value in arrays.items():
            blob["%s/%s" % (name, key)] = value
        print(name, "psnr", arrays["report_psnr"].round(3).tolist())
    np.savez_compressed(os.path.join(HERE, "image_regression.npz"), **blob)
    print("wrote image_regression.npz, pixel_dataset.npz, cli_defaults_image_regression.json, "
          "api_signatures_pixels.json")


if __name__ == "__main__":
    main()

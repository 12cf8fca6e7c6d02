"""Trains a 2-D Fourier-feature network to predict the pixels of an image on the MI355X path
(counterpart of the reference's train_image_regression.py: same flags, same loop, same outputs
`valNNNNN.png`, `superres.png` and `model.pt`).

The loop is the reference's: num_steps + 1 iterations; at every report step (and the last) the
model is validated BEFORE that step's update; the learning rate decays before every step.  Each
step is RegressionEngine.step (fused MLP forward, K11 loss, fused backward, Adam) with no host
sync; validation is one fused forward and K11's evaluation pass, which also writes the u8 frame.
"""

import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fourier_feature_nets_amd as ffn  # noqa: E402
from fourier_feature_nets_amd import ops  # noqa: E402
from fourier_feature_nets_amd.utils import learning_rate_at  # noqa: E402
from scripts import _cli  # noqa: E402


def build_model(args):
    if args.nerf_model == "mlp":
        return ffn.MLP(2, 3, num_channels=args.num_channels)
    if args.nerf_model == "basic":
        return ffn.BasicFourierMLP(2, 3, num_channels=args.num_channels)
    if args.nerf_model == "positional":
        return ffn.PositionalFourierMLP(2, 3, max_log_scale=args.pos_max_log_scale,
                                        num_channels=args.num_channels,
                                        embedding_size=args.embedding_size)
    if args.nerf_model == "gaussian":
        return ffn.GaussianFourierMLP(2, 3, sigma=args.gauss_sigma, num_channels=args.num_channels,
                                      embedding_size=args.embedding_size)
    raise NotImplementedError("Unsupported model: {}".format(args.nerf_model))


def render(engine, dataset, uv3, size):
    """(size, size, 3) u8 RGB frame of the model's sigmoid outputs at ``uv3``, plus the sum of
    squared errors against the validation colours when ``uv3`` is the validation grid."""
    target = dataset.val_color_flat if uv3 is dataset.val_uv3 else None
    sse, image = engine.evaluate(uv3, target, want_image=True)
    if dataset.color_space == "YCrCb":
        ops.ycrcb_to_rgb_u8(image)
    return sse, image.reshape(size, size, 3).cpu().numpy()


def main():
    args = _cli.build_parser("NeRF2D Image Trainer", _cli.IMAGE_REGRESSION).parse_args()
    args.device, _, _, _ = _cli.setup_device(args.device, False)
    os.makedirs(args.results_dir, exist_ok=True)
    if args.make_video:
        # (train_image_regression.py:125-131 writes an MP4 with scenepic: outside the HIP hot path)
        print("warning: --make-video is not supported on the HIP path; the valNNNNN.png frames "
              "are written instead", file=sys.stderr)
    # (train_image_regression.py:169-171 also shows every frame in an on-screen window)
    print("note: no on-screen progress window on the HIP path; see the valNNNNN.png frames",
          file=sys.stderr)

    print("Creating dataset...")
    dataset = ffn.PixelDataset.create(args.image_path, args.color_space, args.image_size)
    if dataset is None:
        print("Dataset unavailable, exiting.")
        return 1
    dataset = dataset.to(args.device)
    model = build_model(args)

    size = args.image_size
    if args.omit_gt and not args.activations:
        width, height = size, size
    elif args.vertical:
        width, height = size, 2 * size
    else:
        width, height = 2 * size, size
    frame = np.zeros((height, width, 3), np.uint8)
    if not args.omit_gt:
        if args.vertical:
            frame[:size, :] = dataset.image
        else:
            frame[:, :size] = dataset.image

    model = model.to(args.device)
    engine = ffn.RegressionEngine(model)
    train_uv3, train_color = dataset.train_uv3, dataset.train_color_flat
    val_count = dataset.val_color_flat.numel()
    lr = args.learning_rate            # optim.param_groups[0]["lr"] as the reference prints it
    for step in range(args.num_steps + 1):
        if step % args.report_interval == 0 or step == args.num_steps:
            sse, image = render(engine, dataset, dataset.val_uv3, size)
            psnr_val = ffn.PixelDataset.psnr_from_sse(float(sse), val_count)
            print("step", step, "val:", psnr_val, "lr:", lr)
            if args.omit_gt and not args.activations:
                frame[:] = image
            elif args.vertical:
                frame[size:, :] = image
            else:
                frame[:, size:] = image
            if args.activations:
                act_image = dataset.to_act_image(model, size)
                if args.vertical:
                    frame[:size, :] = act_image
                else:
                    frame[:, :size] = act_image
            _cli.save_png(os.path.join(args.results_dir, "val{:05}.png".format(step)), frame)
        lr = learning_rate_at(args.learning_rate, step, args.decay_rate, args.decay_steps)
        engine.step(train_uv3, train_color, lr)

    # super-resolution at twice the size, on the GPU (there is no CPU fallback)
    uvs = ffn.PixelDataset.generate_uvs(size * 2, args.device).reshape(-1, 2)
    uv3 = torch.nn.functional.pad(uvs, (0, 1)).contiguous()
    _, image = render(engine, dataset, uv3, size * 2)
    _cli.save_png(os.path.join(args.results_dir, "superres.png"), image)
    model.to("cpu").save(os.path.join(args.results_dir, "model.pt"))
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""The reference's `Raycaster.fit` on a `Voxels` model (its train_voxels.py workflow, README steps
1-2) -> fit_schedule_voxels.npz, and the reference train_voxels.py parser -> cli_defaults_voxels.json.
Runs on the 20 + 10 camera 128x128 rig of make_fit_schedule.py (tests/psnr_ensemble.write_npz),
stratified with annealing, crop_steps 0, lr 0.01, 15 steps reporting every 5.  Build container
only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_fit_schedule_voxels.py

Recorded (data, not source): the initial state, every training batch the reference drew (the
dataset indices handed to `_loss`), the training losses, the LogEntry table, the report lines,
the final state."""

import contextlib
import importlib.util
import io
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

TRAIN_CAMS, VAL_CAMS, SIZE, SAMPLES, BATCH = 20, 10, 128, 64, 512
SIDE, LR, NUM_STEPS, REPORT, ANNEAL_STEPS = 32, 0.01, 14, 5, 8
DECAY_RATE, DECAY_STEPS = 0.9, 25000
CLI_ARGV = ["d.npz", "32", "out"]


def scene_file(path):
    from tests.psnr_ensemble import write_npz
    if not os.path.exists(path):
        write_npz(path, TRAIN_CAMS, VAL_CAMS, SIZE)
    return path


def main():
    sys.path.insert(0, HERE)
    from make_goldens import REFERENCE, _install_stubs
    _install_stubs()
    sys.path.insert(0, REFERENCE)
    sys.dont_write_bytecode = True
    import fourier_feature_nets as ffn

    spec = importlib.util.spec_from_file_location("ref_train_voxels",
                                                  os.path.join(REFERENCE, "train_voxels.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    old = sys.argv
    sys.argv = ["train_voxels.py"] + CLI_ARGV
    try:
        cli = {"train_voxels": vars(mod._parse_args())}
    finally:
        sys.argv = old
    with open(os.path.join(HERE, "cli_defaults_voxels.json"), "w") as f:
        json.dump(cli, f, indent=1, sort_keys=True)

    npz = scene_file("/tmp/ffn_fit_schedule_scene.npz")
    torch.manual_seed(20080524)
    np.random.seed(20080524)
    torch.set_num_threads(4)
    with contextlib.redirect_stdout(io.StringIO()):
        train = ffn.ImageDataset.load(npz, "train", SAMPLES, True, True, anneal_start=0.2,
                                      num_anneal_steps=ANNEAL_STEPS)
        val = ffn.ImageDataset.load(npz, "val", SAMPLES, True, False)
    scale = 2 / train.sampler.bounds[0, 0]            # train_voxels.py:108
    model = ffn.Voxels(SIDE, scale)
    out = {"init/" + k: v.clone().numpy() for k, v in model.state_dict().items()}
    out["scale"] = np.array(scale, np.float64)
    torch.manual_seed(777)
    np.random.seed(777)
    caster = ffn.Raycaster(model)
    batches, losses = [], []
    inner = caster._loss

    def spy(step, dataset, batch):
        value = inner(step, dataset, batch)
        if torch.is_grad_enabled() and value.requires_grad:
            batches.append(np.asarray(batch, np.int64))
            losses.append(float(value))
        return value

    caster._loss = spy
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        log = caster.fit(train, val, BATCH, LR, NUM_STEPS, 0, REPORT, DECAY_RATE, DECAY_STEPS, 0.0, [],
                         disable_aml=True)
    print(buf.getvalue())
    out["batches"] = np.stack(batches)
    out["losses"] = np.array(losses, np.float64)
    out["stdout"] = np.array(buf.getvalue())
    out["log_steps"] = np.array([e.step for e in log])
    out["log_train_psnr"] = np.array([e.train_psnr for e in log])
    out["log_val_psnr"] = np.array([e.val_psnr for e in log])
    for key, value in model.state_dict().items():
        out["final/" + key] = value.numpy()
    np.savez_compressed(os.path.join(HERE, "fit_schedule_voxels.npz"), **out)
    print(len(batches), "training steps")


if __name__ == "__main__":
    main()

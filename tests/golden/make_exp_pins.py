"""exp_pins.npz: the float32 exp of the host that captured the other fixtures, at every input the
bit-exact blend-weight / CDF tests of test_oracle_golden.py feed to torch.exp where it differs from
tests.helpers.portable_exp (a few per cent of them).  Run on that host -- there the three tests
pass with torch's own exp, which this script checks first:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_exp_pins.py
"""

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import test_oracle_golden as tog  # noqa: E402
from tests.helpers import portable_exp  # noqa: E402


def main():
    def golden(name):
        return np.load(os.path.join(HERE, name + ".npz"), allow_pickle=False)

    native, seen = torch.exp, []

    def record(x):
        seen.append(x.detach().reshape(-1).clone())
        return native(x)

    torch.exp = record
    try:
        tog.test_cdf_and_focus_sampling(golden, None)
        tog.test_blend_weights_render_and_gradient(golden, None)
        tog.test_config3_fit_schedule_nerf(None)
    finally:
        torch.exp = native
    bits = np.unique(torch.cat(seen).numpy().view(np.int32))
    x = bits.view(np.float32)
    y = native(torch.from_numpy(x)).numpy()
    keep = y.view(np.int32) != portable_exp(x).view(np.int32)
    np.savez_compressed(os.path.join(HERE, "exp_pins.npz"), input_bits=bits[keep], exp=y[keep])
    print("exp_pins.npz: %d of %d distinct inputs pinned" % (int(keep.sum()), bits.size))


if __name__ == "__main__":
    main()

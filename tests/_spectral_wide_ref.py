"""Fixtures of tests/golden/spectral_wide/ (spectral layers wider than the resident mode-mixing kernels take; recorded by
make_golden_spectral_wide.py next to them) for test_modemix_wide_cpu.py and test_modemix_wide_gpu.py."""
import os

import numpy as np
import torch

from _util import GOLDEN, Golden

SUB = "spectral_wide/"
WIDE_GOLDEN = ("sconv2d_w96x80", "sconv1d_w128x64", "sconv1d_w160x136", "sreg_w96")
# files next to the fixtures that are no fixture of their own: weights / inputs, and the second halves of the regressor's
WIDE_PARTS = tuple(n + "_in" for n in WIDE_GOLDEN) + ("sreg_w96_in2", "sreg_w96_d2")


def wide_golden(name):
    """Golden(spectral_wide/<name>); the regressor's weights and parameter gradients are stored in two files each (1 MiB
    limit per committed file): <name>_in2 holds the rest of sd/, <name>_d2 the rest of dparam/.  meta["base"] is dropped:
    test_modules_gpu.build_module hands a regressor's meta to the constructor."""
    g = Golden(SUB + name)
    for part, prefix, into in (("_in2", "sd/", g.sd), ("_d2", "dparam/", g.dparam)):
        path = os.path.join(GOLDEN, SUB + name + part + ".npz")
        if os.path.exists(path):
            z = np.load(path, allow_pickle=False)
            assert all(k.startswith(prefix) for k in z.files), (part, z.files)
            into.update({k[len(prefix):]: torch.from_numpy(np.array(z[k])) for k in z.files})
    g.meta.pop("base", None)
    return g

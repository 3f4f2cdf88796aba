"""Fixtures of tests/golden/softmax_wide/ (attention_type='softmax' at head tiles 68 and 100 wide; recorded by
make_golden_softmax_wide.py next to them) for test_softmax_wide_cpu.py and test_softmax_wide_gpu.py."""
import os

import numpy as np
import torch

from _util import GOLDEN, Golden

SUB = "softmax_wide/"
WIDE_GOLDEN = ("enc_softmax_w100", "enc_softmax_w100_replay", "enc_softmax_w68", "enc_softmax_w68_replay",
               "enc_softmax_w68_weights", "model_burgers_softmax_ex1")
# files next to the fixtures that are no fixture of their own: shared weights / inputs, and the second halves of the model's
WIDE_PARTS = ("enc_softmax_w68_in", "model_burgers_softmax_ex1_in", "model_burgers_softmax_ex1_in2",
              "model_burgers_softmax_ex1_d2")


def wide_golden(name):
    """Golden(softmax_wide/<name>); the model's weights and parameter gradients are stored in two files each (1 MiB limit
    per committed file): <name>_in2 holds the rest of sd/, <name>_d2 the rest of dparam/."""
    g = Golden(SUB + name)
    for part, prefix, into in (("_in2", "sd/", g.sd), ("_d2", "dparam/", g.dparam)):
        path = os.path.join(GOLDEN, SUB + name + part + ".npz")
        if os.path.exists(path):
            z = np.load(path, allow_pickle=False)
            assert all(k.startswith(prefix) for k in z.files), (part, z.files)
            into.update({k[len(prefix):]: torch.from_numpy(np.array(z[k])) for k in z.files})
    return g

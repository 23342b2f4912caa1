"""Generate tests/golden/cyclegan_keys.npz from the REFERENCE'S OWN definitions (runs only in the build container; helpers shared with make_golden.py).

Lifted by `ast` from cyclegan_og/models.py and instantiated on the CPU: ResidualBlock and GeneratorResNet((3, 256, 256), 9), the shape and depth of
the reference's launch scripts. The fixture holds the state_dict's key names and tensor shapes ONLY, in state_dict order: no weights, no outputs, no
reference source text. Never imported by a GPU test.
Usage:  python tests/golden/make_golden_cyclegan.py        (writes next to this file)
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import lift, save  # noqa: E402  (sets MKL_CBWR before torch starts MKL)

import numpy as np  # noqa: E402

MODELS = "/root/reference/cyclegan_og/models.py"
SHAPE, BLOCKS = (3, 256, 256), 9


def main():
    L = lift(MODELS, ["ResidualBlock", "GeneratorResNet"])
    sd = L["GeneratorResNet"](SHAPE, BLOCKS).state_dict()
    names = list(sd)
    shapes = np.zeros((len(names), 4), dtype=np.int64)           # rows padded with zeros: a bias has one dimension, a filter four
    for i, k in enumerate(names):
        shapes[i, :sd[k].dim()] = list(sd[k].shape)
    save("cyclegan_keys", names=np.array(names), shapes=shapes, input_shape=np.array(SHAPE), num_residual_blocks=np.array(BLOCKS))


if __name__ == "__main__":
    main()

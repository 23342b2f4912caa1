import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# The CPU oracle is held against tests/golden at fp32 round-off, so its CPU numerics must not depend on the host: MKL's conditional numerical
# reproducibility mode gives the same bits on any x86 CPU (test_oracle_golden.py adds oneDNN off and 8 threads; make_golden.py made the fixtures so).
# MKL reads the variable when it starts, which is after this file is imported and before any test runs.
os.environ["MKL_CBWR"] = "COMPATIBLE"

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def golden():
    import numpy as np

    def load(name):
        return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    return load

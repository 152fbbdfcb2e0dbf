#!/usr/bin/env python
"""Record the expectations of tests/test_squared_soft_posterior.py that take the host too long inside a test -- the enumerated
``log m`` of the 32-unit cases, the fp64 restatement of the Categorical case, the fp64 restated sampler on 2048 rows and the
enumerated joint of the chi-square test -- into tests/golden/sq_soft_posterior_expected.npz:

    PYTHONPATH=.:tests python scripts/record_squared_soft_posterior_expected.py

tests/test_squared_soft_posterior_restatement.py recomputes them and compares; the GPU tests read them."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import squared_soft_posterior_restatement as Q  # noqa: E402

if __name__ == "__main__":
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", Q.GOLDEN), **Q.record())

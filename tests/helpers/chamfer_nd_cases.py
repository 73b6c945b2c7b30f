"""The seeded inputs of the D-component Chamfer fixtures
(tests/golden/chamfer_nd_python_d{2,5,6}.npz), shared by the fixture maker
(tests/golden/make_chamfer_nd_golden.py) and the tests, which regenerate the
d = 3 inputs from the same seeds to anchor the new kernel to the 3-D one.

    case      (b, n, m)         seed      why
    unit      (4, 100, 200)     100 + d   the reference's unit_test.py shape; one split
    split     (3, 777, 1025)    200 + d   3 candidate splits; m = 8 * 128 + 1; n ragged
    ragged    (2, 2049, 600)    300 + d   one query past a 2048-query block; 2 splits;
                                          m % 8 != 0
    ties      (2, 64, 72)       400 + d   exact hits and bit-identical duplicates
"""
import numpy as np

DIMS = (2, 5, 6)
CASES = {"unit": (4, 100, 200, 100), "split": (3, 777, 1025, 200), "ragged": (2, 2049, 600, 300),
         "ties": (2, 64, 32, 400)}


def inputs(case: str, d: int):
    """(a (b, n, d), c (b, m, d)) float32 of one case."""
    b, n, m, seed = CASES[case]
    g = np.random.default_rng(seed + d)
    a = g.random((b, n, d), dtype=np.float32)
    c = g.random((b, m, d), dtype=np.float32)
    if case == "ties":
        c[:, :10] = a[:, :10]                              # exact hits
        c = np.concatenate([c, c, c[:, :8]], axis=1)       # bit-identical duplicates
    return a, c

"""Shapes of the sparse split route's tests (dopt_set_sparse(h, 2): the split
LSQR on a sparse A_moi), shared by the CPU pins of the oracle's behaviour on
them and the GPU suite.  Every shape is `conic_numpy_wellcond(..., pair_norm=1.0,
sparse_k=5)`: about five entries per row of A_moi, the family on which LSQR
converges (istop 1–2) well inside maxiter.

  S1  one PSD(65) — the first side the one-workgroup sparse route refuses; the
      side pads to 68 in the Dπ apply; m = 2158 is no multiple of a power-of-two
      block, so the row / column boundary of the pass kernel's outputs falls
      inside a workgroup.
  S2  every cone code; a PSD(68) (no padding) applied from global scratch beside
      a PSD(6) that stays in LDS; m = 2399.
  the small shapes are test_sparse_gpu.CONIC_ALL5 (m69 / m87, B = 4), restated
  here so that this module imports without a GPU test module.

All of these average below 12 entries per output (row or column) of A_moi, so
their products run one lane per output (sp_lanes).  LANES adds m69 at the two
other widths the pass kernel is compiled for: 15 entries per row (4 lanes per
output) and a dense A_moi (16 lanes).
"""
import functools

import numpy as np

# (name, B, n, cones, seed)
S1 = ("S1", 2, 2200, [(4, 2145), (1, 8), (3, 5)], 11)
S2 = ("S2", 2, 2450, [(0, 4), (4, 2346), (1, 12), (3, 9), (2, 7), (4, 21)], 12)
BIG = [S1, S2]
SMALL = [("m69", 4, 60, [(0, 2), (1, 30), (2, 20), (3, 8), (4, 6), (4, 3)], 42),
         ("m87", 4, 80, [(0, 5), (1, 20), (2, 10), (3, 10), (3, 6), (4, 15), (4, 21)], 41)]
M69 = SMALL[0]
# (name, B, n, cones, seed, sparse_k, lanes per output)
LANES = [("m69-k15", 4, 60, SMALL[0][3], 42, 15, 4), ("m69-dense", 4, 60, SMALL[0][3], 42, None, 16)]
SPARSE_K = {"S1": 5, "S2": 5, "m69": 5, "m87": 5, "m69-k15": 15, "m69-dense": None}

assert sum(d for _, d in S1[3]) == 2158 and 65 * 66 // 2 == 2145
assert sum(d for _, d in S2[3]) == 2399 and 68 * 69 // 2 == 2346


@functools.lru_cache(maxsize=None)
def data(name):
    """The shape's problem data (read-only: shared between tests)."""
    from diffopt_amd.synthetic import conic_numpy_wellcond
    _, B, n, cones, seed = shape(name)
    d = conic_numpy_wellcond(B, n, cones, seed, pair_norm=1.0, sparse_k=SPARSE_K[name])
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def shape(name):
    return {s[0]: s[:5] for s in BIG + SMALL + LANES}[name]


def lanes(name):
    """sp_lanes of the shape: lanes per output of the sparse products."""
    d = data(name)
    _, m, n = d["A"].shape
    e = 2.0 * np.count_nonzero(d["A"]) / (d["A"].shape[0] * (m + n))
    return 1 if e <= 12.0 else 4 if e <= 48.0 else 16

"""What the sparse split route's GPU tests (test_sparse_split_gpu.py) take for
granted about their large shapes, pinned on the CPU: on S1 and S2 the oracle's
LSQR converges in both directions (istop 1 or 2) far inside maxiter, so every
output can be held to 1e-6 and the stop codes compared.  Iteration counts are
not pinned: another summation order of the products moves a stop by one."""
import pytest

import sparse_split_cases as sc
from oracle import conic as ocn


@pytest.mark.parametrize("name", [s[0] for s in sc.BIG])
def test_oracle_converges_on_large_shapes(name):
    _, B, n, cones, _ = sc.shape(name)
    d = sc.data(name)
    assert d["A"].shape == (B, sum(k for _, k in cones), n)
    assert (d["A"] != 0).mean() < 0.01            # ≈ 5 entries per row
    for b in range(B):
        cache = ocn.Cache(d["A"][b], d["b"][b], d["c"][b], d["x"][b], d["s"][b], d["y"][b], cones)
        _, fi = ocn.forward_differentiate(cache, d["dA"][b], d["db"][b], d["dc"][b], return_info=True)
        _, ri = ocn.reverse_differentiate(cache, d["dx"][b], return_info=True)
        for it, istop in (fi[:2], ri[:2]):
            assert istop in (1, 2), (name, b, fi, ri)
            assert it < 200, (name, b, fi, ri)


def test_lane_widths_of_the_shapes():
    """sp_lanes of every shape: one lane per output on the issue's shapes, 4
    and 16 on the two LANES cases (the GPU suite runs each compiled width)."""
    for s in sc.BIG + sc.SMALL:
        assert sc.lanes(s[0]) == 1, s[0]
    assert [sc.lanes(s[0]) for s in sc.LANES] == [s[6] for s in sc.LANES] == [4, 16]

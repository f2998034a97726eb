"""Conic multi-seed calls (dopt_conic_reverse_k / dopt_conic_forward_k /
dopt_conic_lsqr_stats_k, ConicBatch.reverse_k / forward_k / lsqr_stats_k):
k LSQR sequences per solved cone program in one call; on the dense persistent
route groups of G = 4 seeds co-iterate in one workgroup and share every sweep
over A (conic_lsqrk_kernel).

The contract is bitwise: seed j's outputs, istop and iteration count equal the
single-seed call's on that seed alone, on every route.  The one tolerance is
the project's parity bar RTOL = 1e-6 against oracle/conic.py, on the m69
shape whose single-seed path test_sparse_gpu.py already holds to it."""

import numpy as np
import pytest

from oracle import conic as ocn
from test_conic_gpu import ConicBatch, SplitConicBatch, _errors, _oracle_outputs   # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
RTOL = 1e-6
G = 4   # group width of conic_lsqrk_kernel (LSQRK_G, csrc/conic.hip)
KS = [1, 3, G, G + 1, 2 * G + 1]   # a single seed, a partial, a full, a remainder group

MIXED = [(0, 3), (1, 10), (3, 6), (2, 4), (4, 6)]
M69 = [(0, 2), (1, 30), (2, 20), (3, 8), (4, 6), (4, 3)]


@pytest.fixture
def persistent(monkeypatch):
    """The route is chosen from the shape (no DOPT_CONIC_SPLIT override)."""
    monkeypatch.delenv("DOPT_CONIC_SPLIT", raising=False)


def _make(CB, d, B, n, cones, sparse=False):
    if sparse:
        import scipy.sparse as sp
        e = CB(B, n, cones, sparse=True)
        e.set_csc([sp.csc_matrix(a) for a in d["A"]], d["b"], d["c"], d["x"], d["s"], d["y"])
    else:
        e = CB(B, n, cones)
        e.set(d["A"], d["b"], d["c"], d["x"], d["s"], d["y"])
    return e


def _stats(e):
    st = e.lsqr_stats()
    return st["istop"].copy(), st["iterations"].copy()


def _check_reverse_k(e, dx):
    """reverse_k(dx) against one reverse call per seed on the same handle:
    every output and the per-seed statistics bitwise.  Returns the k-call's
    (outputs, statistics)."""
    k = dx.shape[0]
    ref = []
    for j in range(k):
        out = [np.array(a) for a in e.reverse(dx[j])]
        ref.append((out, _stats(e)))
    got = e.reverse_k(dx)
    st = e.lsqr_stats_k(k)
    for j in range(k):
        for a, b, what in zip(got, ref[j][0], ("g", "dA", "db", "dc")):
            np.testing.assert_array_equal(np.asarray(a)[j], b, err_msg=f"reverse seed {j}: {what}")
        np.testing.assert_array_equal(st["istop"][j], ref[j][1][0], err_msg=f"reverse seed {j}: istop")
        np.testing.assert_array_equal(st["iterations"][j], ref[j][1][1], err_msg=f"reverse seed {j}: iterations")
    # the single-call introspection reports seed 0
    np.testing.assert_array_equal(e.info(), ref[0][1][0])
    np.testing.assert_array_equal(e.iterations(), ref[0][1][1])
    return got, st


def _check_forward_k(e, dA, db, dc):
    k = dA.shape[0]
    ref = []
    for j in range(k):
        out = [np.array(a) for a in e.forward(dA[j], db[j], dc[j])]
        ref.append((out, _stats(e)))
    got = e.forward_k(dA, db, dc)
    st = e.lsqr_stats_k(k)
    for j in range(k):
        for a, b, what in zip(got, ref[j][0], ("out", "dx")):
            np.testing.assert_array_equal(np.asarray(a)[j], b, err_msg=f"forward seed {j}: {what}")
        np.testing.assert_array_equal(st["istop"][j], ref[j][1][0], err_msg=f"forward seed {j}: istop")
        np.testing.assert_array_equal(st["iterations"][j], ref[j][1][1], err_msg=f"forward seed {j}: iterations")
    np.testing.assert_array_equal(e.iterations(), ref[0][1][1])
    return got, st


def _normal_seeds(rng_seed, k, B, m, n):
    rng = np.random.default_rng(rng_seed)
    return (rng.standard_normal((k, B, n)), rng.standard_normal((k, B, m, n)), rng.standard_normal((k, B, m)),
            rng.standard_normal((k, B, n)))


# (b): m = 600 > PAIR_ROWS = 512, so gemv_multi's row-block loop runs twice
# (the `r0 ? g + sc : sc` accumulation); n = 30 in (a) leaves a column remainder
PERSISTENT = [("mixed cones", 3, 30, MIXED, 11, None),
              ("two row blocks", 2, 100, [(3, 25)] * 24, 14, 12)]


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("shape", PERSISTENT, ids=lambda s: s[0])
def test_bitwise_vs_single_calls_persistent(ConicBatch, persistent, shape, k):
    from diffopt_amd.synthetic import conic_numpy
    _, B, n, cones, seed, cap = shape
    m = sum(dim for _, dim in cones)
    d = conic_numpy(B, n, cones, seed)
    e = _make(ConicBatch, d, B, n, cones)
    if cap:
        e.set_maxiter(cap)
    dx, dA, db, dc = _normal_seeds(100 + k, k, B, m, n)
    _check_reverse_k(e, dx)
    _check_forward_k(e, dA, db, dc)
    e.close()


def test_bitwise_two_wide_groups_large_psd(ConicBatch, monkeypatch):
    """A PSD side of 62 on the persistent kernel (forced: its m = 1953 would
    take the split route): the three Dπ images leave LDS for two sequences'
    row partials only, so the groups are two wide; four row blocks."""
    from diffopt_amd.synthetic import conic_numpy
    monkeypatch.setenv("DOPT_CONIC_SPLIT", "0")
    cones, B, n, k = [(4, 62 * 63 // 2)], 1, 8, 3
    d = conic_numpy(B, n, cones, 31)
    e = _make(ConicBatch, d, B, n, cones)
    e.set_maxiter(4)
    dx, dA, db, dc = _normal_seeds(7, k, B, cones[0][1], n)
    _check_reverse_k(e, dx)
    _check_forward_k(e, dA, db, dc)
    e.close()


def _m69():
    from diffopt_amd.synthetic import conic_numpy_wellcond
    return conic_numpy_wellcond(4, 60, M69, 42, pair_norm=1.0)


def test_ragged_stopping(ConicBatch, persistent):
    """Five reverse sequences of one group and its remainder group that stop
    at different iterations: the data's dx, an all-zero seed, a seed below the
    reference's 1e-4 rule (both give exactly 0 with no iteration) and two
    random seeds."""
    d = _m69()
    B, n = 4, 60
    # rng seed 0: oracle.conic.reverse_differentiate(..., return_info=True) stops (istop 2) after
    #   d["dx"]: 55, 70, 75, 54   random 0: 54, 69, 75, 53   random 1: 50, 69, 73, 52   iterations
    # (problems 0..3): the counts differ within every problem
    r = np.random.default_rng(0).standard_normal((2, B, n))
    dx = np.stack([d["dx"], np.zeros((B, n)), 1e-6 * d["dx"], r[0], r[1]])
    e = _make(ConicBatch, d, B, n, M69)
    (g, dA, db, dc), st = _check_reverse_k(e, dx)
    for j in (1, 2):
        for a in (g, dA, db, dc):
            assert not np.any(np.asarray(a)[j])
        assert not np.any(st["istop"][j]) and not np.any(st["iterations"][j])
    its = st["iterations"][[0, 3, 4]]
    assert np.all(st["istop"][[0, 3, 4]] > 0)
    assert any(len(set(its[:, b])) > 1 for b in range(B)), its
    e.close()


def test_oracle_parity_scaled_seeds(ConicBatch, persistent):
    """Seeds dx·{1, 2, −4, 0.5} (tangents scaled alike): powers of two keep the
    oracle's iterates exactly scaled, so every seed meets RTOL where seed 0
    does."""
    d = _m69()
    B, n = 4, 60
    scales = [1.0, 2.0, -4.0, 0.5]
    e = _make(ConicBatch, d, B, n, M69)
    g, dA, db, dc = e.reverse_k(np.stack([s * d["dx"] for s in scales]))
    out, fdx = e.forward_k(np.stack([s * d["dA"] for s in scales]), np.stack([s * d["db"] for s in scales]),
                           np.stack([s * d["dc"] for s in scales]))
    e.close()
    worst = 0.0
    for b in range(B):
        cache = ocn.Cache(d["A"][b], d["b"][b], d["c"][b], d["x"][b], d["s"][b], d["y"][b], M69)
        for j, s in enumerate(scales):
            ref = _oracle_outputs(cache, s * d["dA"][b], s * d["db"][b], s * d["dc"][b], s * d["dx"][b])
            got = dict(fwd=out[j][b], dx=fdx[j][b], g=g[j][b], dA=dA[j][b], db=db[j][b], dc=dc[j][b])
            err = _errors(got, ref, cache)
            print(f"[parity] problem {b} scale {s}: " + " ".join(f"{k}={v:.2e}" for k, v in err.items()))
            worst = max([worst] + list(err.values()))
    assert worst <= RTOL, worst


def test_handle_reuse_across_k(ConicBatch, persistent):
    """k = 2, then 2G + 1, then 1 on one handle (workspace and info sized per
    call), then the co-iterated forward_reverse as before any _k call."""
    from diffopt_amd.synthetic import conic_numpy
    B, n, seed = 3, 30, 11
    m = sum(dim for _, dim in MIXED)
    d = conic_numpy(B, n, MIXED, seed)
    e = _make(ConicBatch, d, B, n, MIXED)
    before = e.forward_reverse(d["dx"], d["dA"], d["db"], d["dc"])
    before = [np.array(a) for a in before[0] + before[1]]
    dx = _normal_seeds(5, 2 * G + 1, B, m, n)[0]
    for k in (2, 2 * G + 1, 1):
        _check_reverse_k(e, dx[:k])
    after = e.forward_reverse(d["dx"], d["dA"], d["db"], d["dc"])
    for a, b in zip(after[0] + after[1], before):
        np.testing.assert_array_equal(np.asarray(a), b)
    e.close()


@pytest.mark.parametrize("route", ["split", "sparse"])
def test_fallback_routes_bitwise(SplitConicBatch, monkeypatch, route):
    """The split route and the sparse route: the single-seed LSQR per seed
    inside the call (no shared sweep), per-seed statistics kept."""
    from diffopt_amd.synthetic import conic_numpy
    if route == "sparse":
        monkeypatch.delenv("DOPT_CONIC_SPLIT", raising=False)
    B, n, k = 3, 30, 3
    m = sum(dim for _, dim in MIXED)
    d = conic_numpy(B, n, MIXED, 11)
    e = _make(SplitConicBatch, d, B, n, MIXED, sparse=route == "sparse")
    dx, dA, db, dc = _normal_seeds(9, k, B, m, n)
    _check_reverse_k(e, dx)
    _check_forward_k(e, dA, db, dc)
    e.close()


def test_errors(ConicBatch, persistent):
    from diffopt_amd._lib import EngineError
    from diffopt_amd.synthetic import conic_numpy
    B, n = 2, 12
    cones = [(1, 4), (3, 5), (0, 2)]
    d = conic_numpy(B, n, cones, 3)
    e = _make(ConicBatch, d, B, n, cones)
    with pytest.raises(EngineError):
        e.reverse_k(np.zeros((0, B, n)))
    with pytest.raises(EngineError):
        e.forward_k(dc=np.zeros((0, B, n)))
    with pytest.raises(EngineError):
        e.lsqr_stats_k(0)
    e.reverse_k(np.ones((3, B, n)))
    assert e.lsqr_stats_k(3)["istop"].shape == (3, B)
    with pytest.raises(EngineError):
        e.lsqr_stats_k(2)
    e.reverse(np.ones((B, n)))   # a single call: no _k statistics any more
    with pytest.raises(EngineError):
        e.lsqr_stats_k(3)
    e.close()

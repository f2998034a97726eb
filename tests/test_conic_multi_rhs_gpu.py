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
    """(istop, iterations, norms) of the last single call."""
    st = e.lsqr_stats()
    return st["istop"].copy(), st["iterations"].copy(), e.lsqr_norms()["last"].copy()


def _check_seed0_slots(e, ref0, what):
    """After a k-call the single-call getters report seed 0: stop code,
    iteration count and the four norms, bitwise."""
    st = e.lsqr_stats()
    np.testing.assert_array_equal(st["istop"], ref0[0], err_msg=f"{what}: istop of seed 0")
    np.testing.assert_array_equal(st["iterations"], ref0[1], err_msg=f"{what}: iterations of seed 0")
    np.testing.assert_array_equal(e.lsqr_norms()["last"], ref0[2], err_msg=f"{what}: norms of seed 0")


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
    _check_seed0_slots(e, ref[0][1], "reverse_k")
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
    _check_seed0_slots(e, ref[0][1], "forward_k")
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


def _slots(e):
    """Everything the single-call getters hold: both [istop | iterations]
    blocks and both norm blocks."""
    st, nr = e.lsqr_stats(), e.lsqr_norms()
    return {"last": (st["istop"].copy(), st["iterations"].copy(), nr["last"].copy()),
            "fwd": (st["fwd_istop"].copy(), st["fwd_iterations"].copy(), nr["fwd"].copy())}


def _assert_slot(got, ref, what):
    for a, b, name in zip(got, ref, ("istop", "iterations", "norms")):
        np.testing.assert_array_equal(a, b, err_msg=f"{what}: {name}")


@pytest.mark.parametrize("route", ["persistent", "split-fused", "split-six-launch", "sparse"])
def test_info_slots_across_calls(ConicBatch, monkeypatch, route):
    """forward_reverse leaves the reverse run's statistics and norms in the
    "last" slots and the forward run's in the "fwd" slots, each bitwise what
    the separate call reports; a later single call rewrites "last" only."""
    from diffopt_amd.synthetic import conic_numpy
    if route.startswith("split"):
        monkeypatch.setenv("DOPT_CONIC_SPLIT", "1")
        if route == "split-six-launch":
            monkeypatch.setenv("DOPT_SPLIT_FUSE", "0")
    else:
        monkeypatch.delenv("DOPT_CONIC_SPLIT", raising=False)
    B, n = 3, 30
    d = conic_numpy(B, n, MIXED, 11)
    e = _make(ConicBatch, d, B, n, MIXED, sparse=route == "sparse")
    e.forward_reverse(d["dx"], d["dA"], d["db"], d["dc"])
    both = _slots(e)
    e.forward(d["dA"], d["db"], d["dc"])
    fwd = _slots(e)
    _assert_slot(both["fwd"], fwd["last"], "forward_reverse's fwd slots against forward")
    _assert_slot(fwd["fwd"], both["fwd"], "fwd slots after a single forward")
    e.reverse(d["dx"])
    rev = _slots(e)
    _assert_slot(both["last"], rev["last"], "forward_reverse's last slots against reverse")
    _assert_slot(rev["fwd"], both["fwd"], "fwd slots after a single reverse")
    assert np.all(both["fwd"][1] > 0) and np.all(both["last"][1] > 0)   # both runs iterated
    e.close()


# phase counts per call as dopt_get_phase_times reports them, from a run of
# commit c059bfe (the parent of the call-table refactor): on the persistent
# route every call brackets each phase once; on the split route a _k call
# runs seed by seed, so each phase is bracketed once per seed
_ONCE = {"conic_rhs": 1, "conic_lsqr": 1, "conic_output": 1}
_PER_SEED = {"conic_rhs": 3, "conic_lsqr": 3, "conic_output": 3}
PHASE_COUNTS = {"persistent": {"reverse_k": _ONCE, "forward_k": _ONCE, "forward_reverse": _ONCE, "reverse": _ONCE,
                               "forward": _ONCE},
                "split": {"reverse_k": _PER_SEED, "forward_k": _PER_SEED, "forward_reverse": _ONCE, "reverse": _ONCE,
                          "forward": _ONCE}}


@pytest.mark.parametrize("route", ["persistent", "split"])
def test_phase_counts_per_call(ConicBatch, monkeypatch, route):
    from diffopt_amd.synthetic import conic_numpy
    if route == "split":
        monkeypatch.setenv("DOPT_CONIC_SPLIT", "1")
    else:
        monkeypatch.delenv("DOPT_CONIC_SPLIT", raising=False)
    B, n, k = 2, 30, 3
    m = sum(dim for _, dim in MIXED)
    d = conic_numpy(B, n, MIXED, 11)
    e = _make(ConicBatch, d, B, n, MIXED)
    e.factor()
    e.set_profiling(True)
    dx, dA, db, dc = _normal_seeds(3, k, B, m, n)
    calls = {"reverse_k": lambda: e.reverse_k(dx),
             "forward_k": lambda: e.forward_k(dA, db, dc),
             "forward_reverse": lambda: e.forward_reverse(dx[0], dA[0], db[0], dc[0]),
             "reverse": lambda: e.reverse(dx[0]),
             "forward": lambda: e.forward(dA[0], db[0], dc[0])}
    for name, call in calls.items():
        call()
        got = {ph: cnt for ph, (_, cnt) in e.phase_times().items()}
        print(f"[phases] {route} {name}: {got}")
        assert got == PHASE_COUNTS[route][name], (route, name, got)
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

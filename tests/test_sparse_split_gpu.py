"""The sparse split route (dopt_set_sparse(h, 2), ConicBatch(sparse="split")):
A_moi kept sparse as on the one-workgroup sparse route, LSQR as the split path
runs it — the products by conic_sp_split_pass_kernel over the CSC / CSR
arrays, Dπ one workgroup per cone, PSD sides above 64 from global scratch.

Shapes: tests/sparse_split_cases.py.  Checked against the oracle at 1e-6
(stop codes equal; iteration counts are not compared with the oracle's — one
more or less is another summation order's doing), against the dense split
route on the densified problem and the one-workgroup sparse route (two LSQR
runs that differ in summation order: DESIGN §2.4's 1e-7 where they stop at
the same iteration, 1e-6 otherwise, counts at most 2 apart), for the route's
bit identities, LSQR's edges, handle reuse and refusals."""
import functools

import numpy as np
import pytest

import sparse_split_cases as sc
from oracle import conic as ocn

pytestmark = pytest.mark.gpu
RTOL = 1e-6
STATS = ("istop", "iterations", "fwd_istop", "fwd_iterations")


def relfro(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / max(np.linalg.norm(b), 1e-300)


def _engine(name, mode):
    """A handle of the shape with its model set.  mode: "split" (on = 2), True
    (on = 1), or False (dense route on the densified A)."""
    from diffopt_amd.conic import ConicBatch
    _, B, n, cones, _ = sc.shape(name)
    d = sc.data(name)
    e = ConicBatch(B, n, cones, sparse=mode)
    _set(e, d, mode)
    return e, d


def _set(e, d, mode):
    import scipy.sparse as sp
    if mode:
        e.set_csc([sp.csc_matrix(a) for a in d["A"]], d["b"], d["c"], d["x"], d["s"], d["y"])
    else:
        e.set(d["A"], d["b"], d["c"], d["x"], d["s"], d["y"])


def _flat(res):
    (out, fdx), (g, dA, db, dc) = res
    return [np.asarray(a) for a in (out, fdx, g, dA, db, dc)]


def _forward_reverse(name, mode):
    e, d = _engine(name, mode)
    res = e.forward_reverse(d["dx"], d["dA"], d["db"], d["dc"])
    st = {k: v.copy() for k, v in e.lsqr_stats().items()}
    e.close()
    for a in _flat(res):
        a.setflags(write=False)
    return res, st


@functools.lru_cache(maxsize=None)
def _split_run(name):
    """forward_reverse of the shape on the new route: one run per shape, shared
    (read-only) by the tests that compare it with something."""
    return _forward_reverse(name, "split")


def _same_lsqr(name, res, st, other, ost):
    """Two runs of one LSQR that differ in summation order: per problem and
    output ≤ 1e-7 where both stopped at the same iteration, else ≤ 1e-6;
    iteration counts at most 2 apart, stop codes equal."""
    B = sc.shape(name)[1]
    worst = 0.0
    for b in range(B):
        for its, codes, outs in (("fwd_iterations", "fwd_istop", (0, 1)), ("iterations", "istop", (2, 3, 4, 5))):
            da = abs(int(st[its][b]) - int(ost[its][b]))
            assert da <= 2, (name, b, its, st[its][b], ost[its][b])
            assert st[codes][b] == ost[codes][b], (name, b, codes)
            bar = 1e-7 if da == 0 else 1e-6
            for k in outs:
                err = relfro(_flat(res)[k][b], _flat(other)[k][b])
                print(f"{name} problem {b} output {k}: {err:.3e} (iterations {st[its][b]} / {ost[its][b]})")
                worst = max(worst, err)
                assert err <= bar, (name, b, k, err, bar)
    return worst


# 1 --------------------------------------------------------------------------
@pytest.mark.parametrize("name", [s[0] for s in sc.BIG])
def test_large_psd_vs_oracle(name):
    """S1 / S2 (a PSD side above 64: refused by on = 1) against the oracle:
    every output at 1e-6, the oracle's stop codes; an output above 1e-6 held to
    the exact min-norm bar, at most half of the B × 6 outputs."""
    from test_sparse_gpu import _conic_vs_oracle
    _, B, _, cones, _ = sc.shape(name)
    res, st = _split_run(name)
    worst, judged = _conic_vs_oracle(sc.data(name), cones, B, res, st, minnorm=True)
    print(f"{name}: worst {worst:.3e}, {judged} outputs on the min-norm bar")
    assert judged <= B * 6 // 2


# 2 --------------------------------------------------------------------------
@pytest.mark.parametrize("name", [s[0] for s in sc.BIG])
def test_large_psd_vs_dense_split_route(name, monkeypatch):
    monkeypatch.setenv("DOPT_CONIC_SPLIT", "1")
    res, st = _split_run(name)
    dres, dst = _forward_reverse(name, False)
    _same_lsqr(name, res, st, dres, dst)


# 3 --------------------------------------------------------------------------
@pytest.mark.parametrize("name", [s[0] for s in sc.SMALL])
def test_small_vs_oracle_and_one_workgroup_route(name):
    """Every cone code at sizes where everything stays in LDS: the oracle at
    1e-6 with nothing relaxed, and on = 1 on the same arrays."""
    from test_sparse_gpu import _conic_vs_oracle
    _, B, _, cones, _ = sc.shape(name)
    res, st = _split_run(name)
    _conic_vs_oracle(sc.data(name), cones, B, res, st)
    ores, ost = _forward_reverse(name, True)
    _same_lsqr(name, res, st, ores, ost)


@pytest.mark.parametrize("case", sc.LANES, ids=[s[0] for s in sc.LANES])
def test_lane_widths_vs_one_workgroup_route(case):
    """The pass kernel's 4- and 16-lane groups per output (15 entries per row,
    a dense A_moi) against on = 1, which picks the same width."""
    name, lanes = case[0], case[6]
    assert sc.lanes(name) == lanes
    res, st = _split_run(name)
    ores, ost = _forward_reverse(name, True)
    _same_lsqr(name, res, st, ores, ost)


# 4 --------------------------------------------------------------------------
def _assert_same_bits(got, want):
    for a, b in zip(got, want):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b))


def test_forward_reverse_is_forward_plus_reverse_bitwise():
    """S1: the pass kernel serves both sequences from one load of an entry,
    each sum in its single-sequence order."""
    res, st = _split_run("S1")
    e, d = _engine("S1", "split")
    fwd = e.forward(d["dA"], d["db"], d["dc"])
    fst = {k: v.copy() for k, v in e.lsqr_stats().items()}
    rev = e.reverse(d["dx"])
    rst = e.lsqr_stats()
    e.close()
    _assert_same_bits(fwd, res[0])
    _assert_same_bits(rev, res[1])
    for k in ("istop", "iterations"):
        np.testing.assert_array_equal(fst[k], st["fwd_" + k])
        np.testing.assert_array_equal(rst[k], st[k])


def test_reverse_k_is_k_reverse_calls_bitwise():
    e, d = _engine("m69", "split")
    rng = np.random.default_rng(7)
    seeds = np.stack([d["dx"], rng.standard_normal(d["dx"].shape), -2.0 * d["dx"][::-1]])
    gk, Ak, bk, ck = e.reverse_k(seeds)
    stk = e.lsqr_stats_k(3)
    for j in range(3):
        one = e.reverse(seeds[j])
        _assert_same_bits(one, (gk[j], Ak[j], bk[j], ck[j]))
        s1 = e.lsqr_stats()
        np.testing.assert_array_equal(stk["istop"][j], s1["istop"])
        np.testing.assert_array_equal(stk["iterations"][j], s1["iterations"])
    e.close()


# 5 --------------------------------------------------------------------------
def test_lsqr_edges():
    _, B, n, cones, _ = sc.shape("m69")
    e, d = _engine("m69", "split")
    # no tangents: the forward right-hand side is exactly zero
    out, fdx = e.forward()
    st = e.lsqr_stats()
    assert np.all(np.asarray(out) == 0) and np.all(np.asarray(fdx) == 0)
    assert np.all(st["istop"] == 0) and np.all(st["iterations"] == 0)
    # a reverse seed with ‖dz‖ ≤ 1e-4: g = 0 without iterating (ConicProgram.jl:369-370)
    tiny = 5e-5 * d["dx"] / np.linalg.norm(d["dx"], axis=1, keepdims=True)
    for b in range(B):
        assert np.hypot(np.linalg.norm(tiny[b]), d["x"][b] @ tiny[b]) <= 1e-4
    g, dA, db, dc = e.reverse(tiny)
    st = e.lsqr_stats()
    for a in (g, dA, db, dc):
        assert np.all(np.asarray(a) == 0)
    assert np.all(st["istop"] == 0) and np.all(st["iterations"] == 0)
    # the iteration cap: both directions stop at istop 7 after 5 iterations
    from test_conic_gpu import _errors
    e.set_maxiter(5)
    (out, fdx), (g, dA, db, dc) = e.forward_reverse(d["dx"], d["dA"], d["db"], d["dc"])
    st = e.lsqr_stats()
    e.close()
    for b in range(B):
        cache = ocn.Cache(d["A"][b], d["b"][b], d["c"][b], d["x"][b], d["s"][b], d["y"][b], cones)
        (odx, du, dv, dw), fi = ocn.forward_differentiate(cache, d["dA"][b], d["db"][b], d["dc"][b],
                                                         return_info=True, maxiter=5)
        (og, _), ri = ocn.reverse_differentiate(cache, d["dx"][b], return_info=True, maxiter=5)
        odA, odb, odc = ocn.reverse_outputs(cache, og)
        ref = dict(fwd=np.concatenate([du, dv, [dw]]), dx=odx, g=og, dA=odA, db=odb, dc=odc)
        got = dict(fwd=np.asarray(out)[b], dx=np.asarray(fdx)[b], g=np.asarray(g)[b], dA=np.asarray(dA)[b],
                   db=np.asarray(db)[b], dc=np.asarray(dc)[b])
        assert (st["fwd_iterations"][b], st["fwd_istop"][b]) == (fi[0], fi[1]) == (5, 7), (b, fi)
        assert (st["iterations"][b], st["istop"][b]) == (ri[0], ri[1]) == (5, 7), (b, ri)
        for key, err in _errors(got, ref, cache).items():
            assert err <= RTOL, (b, key, err)


# 6 --------------------------------------------------------------------------
def test_handle_switched_between_sparse_modes():
    """One handle 2 → 1 → 2 (dopt_set_sparse drops the model: set again each
    time): every run bit-identical to a fresh handle of its mode; the handle's
    device memory is all returned by close()."""
    from diffopt_amd import _lib
    from diffopt_amd.conic import ConicBatch
    live = _lib.load().dopt_live_device_bytes
    _, B, n, cones, _ = sc.shape("m69")
    d = sc.data("m69")
    fresh = {"split": _split_run("m69"), True: _forward_reverse("m69", True)}
    start = live()
    e = ConicBatch(B, n, cones, sparse="split")
    for mode in ("split", True, "split"):
        e.set_sparse(mode)
        with pytest.raises(_lib.EngineError):      # no model after the switch
            e.reverse(d["dx"])
        _set(e, d, mode)
        res = e.forward_reverse(d["dx"], d["dA"], d["db"], d["dc"])
        st = e.lsqr_stats()
        _assert_same_bits(_flat(res), _flat(fresh[mode][0]))
        for k in STATS:
            np.testing.assert_array_equal(st[k], fresh[mode][1][k])
    assert live() > start
    e.close()
    assert live() == start


# 7 --------------------------------------------------------------------------
def test_refusals():
    from diffopt_amd import _lib
    from diffopt_amd.conic import ConicBatch
    _, B, n, cones, _ = sc.shape("m69")
    d = sc.data("m69")
    e = ConicBatch(B, n, cones, sparse="split")
    with pytest.raises(_lib.EngineError, match="dopt_conic_set_csc"):
        e.set(d["A"], d["b"], d["c"], d["x"], d["s"], d["y"])
    e.close()
    with pytest.raises(ValueError):
        ConicBatch(B, n, cones, sparse="spilt")

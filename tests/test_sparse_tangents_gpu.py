"""Sparse matrix tangents and on-pattern gradients (the `_csc` calls): a forward
tangent dA / dG / dQ given as a sparse matrix with its own pattern, as the
reference's `sparse(I, J, V)` (ConicProgram.jl:288-305, QuadraticProgram.jl:
429-433), and the reverse matrix gradients read at the entries of a pattern
(`_get_dA`, ConicProgram.jl:430-443; QuadraticProgram.jl:461-473) — no dense
rows × n array on the way.

Exact reduction used below: a matrix tangent equals a pair of shifted vector
tangents in exact arithmetic (the right-hand side's last entry cancels),
    conic  (dA, db, dc)          ≡ (0, db − dA·x, dc + dAᵀvp)
    LP     (dG, dA, dq, dh, db)  ≡ (0, 0, dq + dGᵀλ + dAᵀν, dh − dG z, db − dA z).
Tolerances: 1e-6 against the oracle (the project's parity bar).  Against the
dense-tangent call the issue's bar is 1e-7, and the engine's claim is stronger:
the sparse right-hand-side kernels sum in the dense kernels' order, so the
right-hand side, the LSQR run and every output are bit-identical to the
dense-tangent call's on the densified tangent — asserted with
assert_array_equal beside the 1e-7 bar, so that a change of summation order
shows.  Per-entry bounds of a few ε·Σ|terms| for
the sampled gradients against the dense ones (each is a sum of two products,
every operation rounded once, fused or not, in two kernels)."""

import os

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import conic as ocn
from oracle import qp as oqp
from test_sparse_gpu import CONIC_ALL5, relfro

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
M69 = CONIC_ALL5[0]


# ---------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------
def _rand_sparse(rng, shape, density, B, empty_cols=(), empty_rows=()):
    """B random matrices with independent patterns (values N(0, 1))."""
    out = []
    for _ in range(B):
        mask = rng.random(shape) < density
        mask[:, list(empty_cols)] = False
        mask[list(empty_rows), :] = False
        out.append(sp.csc_matrix(np.where(mask, rng.standard_normal(shape), 0.0)))
    return out


def _dense(mats):
    return np.stack([M.toarray() for M in mats])


def _conic_data(shape, B=None):
    from diffopt_amd.synthetic import conic_numpy_wellcond
    _, B0, n, cones, seed = shape
    B = B or B0
    return conic_numpy_wellcond(B, n, cones, seed, pair_norm=1.0), cones, B, n


def _conic_handle(d, cones, B, n, route):
    """route: "sparse", or the dense handle with DOPT_CONIC_SPLIT = "0" / "1"."""
    from diffopt_amd.conic import ConicBatch
    old = os.environ.get("DOPT_CONIC_SPLIT")
    if route != "sparse":
        os.environ["DOPT_CONIC_SPLIT"] = route
    try:
        e = ConicBatch(B, n, cones, sparse=(route == "sparse"))
    finally:
        if route != "sparse":
            if old is None:
                del os.environ["DOPT_CONIC_SPLIT"]
            else:
                os.environ["DOPT_CONIC_SPLIT"] = old
    if route == "sparse":
        e.set_csc([sp.csc_matrix(a) for a in d["A"]], d["b"], d["c"], d["x"], d["s"], d["y"])
    else:
        e.set(d["A"], d["b"], d["c"], d["x"], d["s"], d["y"])
    return e


def _lp_handle(d, sparse=True):
    from test_sparse_gpu import _batch
    return _batch(d, sparse=sparse)


def _conic_forward_raw(e, packed, db, dc):
    """dopt_conic_forward_csc on hand-made CSC arrays (None: NULL colptr)."""
    from diffopt_amd import _lib
    from diffopt_amd._arrays import csc_args
    B, n, m = e.batch, e.n, e.m
    e._stage([db, dc])
    db = np.ascontiguousarray(db, dtype=np.float64)
    dc = np.ascontiguousarray(dc, dtype=np.float64)
    out, dx = np.empty((B, e.N)), np.empty((B, n))
    rc = e.lib.dopt_conic_forward_csc(e.h, *csc_args(packed), db.ctypes.data, dc.ctypes.data, out.ctypes.data,
                                      dx.ctypes.data)
    _lib.check(rc, e.h)
    return out, dx


def _qp_forward_raw(e, packs, dq, dh, db):
    """dopt_qp_forward_csc on hand-made CSC arrays: packs = (dQ, dG, dA), None = absent."""
    from diffopt_amd import _lib
    from diffopt_amd._arrays import csc_args
    e._stage([dq, dh, db])
    vecs = [np.ascontiguousarray(v, dtype=np.float64) for v in (dq, dh, db)]
    args = []
    for pk, v in zip(packs, vecs):
        args += csc_args(pk) + [v.ctypes.data]
    out = np.empty((e.batch, e.L))
    _lib.check(e.lib.dopt_qp_forward_csc(e.h, *args, out.ctypes.data), e.h)
    return out


# ---------------------------------------------------------------------------
# 1. conic against the oracle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", CONIC_ALL5, ids=[s[0] for s in CONIC_ALL5])
def test_conic_forward_csc_vs_oracle(shape):
    d, cones, B, n = _conic_data(shape)
    m = d["b"].shape[1]
    rng = np.random.default_rng(shape[4] + 1000)
    dA = _rand_sparse(rng, (m, n), 0.05, B)
    e = _conic_handle(d, cones, B, n, "sparse")
    out, dx = e.forward(dA=dA, db=d["db"], dc=d["dc"])
    st = e.lsqr_stats()
    e.close()
    worst = 0.0
    for b in range(B):
        cache = ocn.Cache(d["A"][b], d["b"][b], d["c"][b], d["x"][b], d["s"][b], d["y"][b], cones)
        (odx, du, dv, dw), (it, istop) = ocn.forward_differentiate(cache, dA[b].toarray(), d["db"][b], d["dc"][b],
                                                                  return_info=True)
        assert istop in (1, 2), (b, it, istop)
        assert st["istop"][b] == istop, (b, st["istop"][b], istop)
        e1, e2 = relfro(out[b], np.concatenate([du, dv, [dw]])), relfro(dx[b], odx)
        print(f"{shape[0]} b={b} it={it} istop={istop} out {e1:.2e} dx {e2:.2e}")
        worst = max(worst, e1, e2)
    assert worst <= 1e-6, worst


# ---------------------------------------------------------------------------
# 2. conic against the dense tangent, every route
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["sparse", "0", "1"], ids=["sparse", "persistent", "split"])
def test_conic_forward_csc_vs_dense_tangent(route):
    d, cones, B, n = _conic_data(M69)
    m = d["b"].shape[1]
    rng = np.random.default_rng(7)
    dA = _rand_sparse(rng, (m, n), 0.05, B)
    e = _conic_handle(d, cones, B, n, route)
    out_d, dx_d = e.forward(dA=_dense(dA), db=d["db"], dc=d["dc"])
    out_s, dx_s = e.forward(dA=dA, db=d["db"], dc=d["dc"])
    for b in range(B):
        e1, e2 = relfro(out_s[b], out_d[b]), relfro(dx_s[b], dx_d[b])
        print(f"{route} b={b} out {e1:.2e} dx {e2:.2e}")
        assert e1 <= 1e-7 and e2 <= 1e-7, (b, e1, e2)
    np.testing.assert_array_equal(out_s, out_d)      # the dense right-hand-side kernel's bits
    np.testing.assert_array_equal(dx_s, dx_d)
    g, _, rdb, rdc = e.reverse(d["dx"], want_dA=False)
    (fo, fdx), (fg, fdA, fdb, fdc) = e.forward_reverse(d["dx"], dA=dA, db=d["db"], dc=d["dc"])
    assert fdA is None
    for got, want in ((fo, out_s), (fdx, dx_s), (fg, g), (fdb, rdb), (fdc, rdc)):
        np.testing.assert_array_equal(got, want)
    e.close()


# ---------------------------------------------------------------------------
# 3. tangent densities and edges
# ---------------------------------------------------------------------------
# (density, B, one problem of the batch empty, entries per output (lo, hi]).
# The issue's three densities — ≈ 2, ≈ 20 and ≈ 60 entries per output,
# 2·nnz / (B·(m + n)), the bands in which the engine's LSQR products change
# their lane width (≤ 12, ≤ 48, above) — each with an empty first and last
# column and an empty row.  The right-hand-side kernel has one form for all
# densities; what the cases cover is short, medium and nearly full columns and
# rows of it (a column of > 64 entries takes several rounds of
# sparse_col_lane_sum, a row ≡ another mod 64 shares its lane).  An empty
# problem in the batch caps the mean at 40.8 entries per output for B = 3, so
# the densest B = 3 case has none and a B = 5 case adds one.
DENSITY_CASES = [("per2", 0.05, 3, True, (1.0, 3.0)), ("per20", 0.48, 3, True, (17.0, 23.0)),
                 ("per58", 0.95, 3, False, (48.0, 64.0)), ("per49_empty_problem", 1.0, 5, True, (48.0, 64.0))]


@pytest.mark.parametrize("case", DENSITY_CASES, ids=[c[0] for c in DENSITY_CASES])
def test_conic_tangent_densities_and_edges(case):
    from diffopt_amd._arrays import csc_pack
    _, density, B, with_empty, (lo, hi) = case
    d, cones, B, n = _conic_data(M69, B=B)
    m = d["b"].shape[1]
    assert (n, m) == (60, 69)
    rng = np.random.default_rng(11)
    dA = _rand_sparse(rng, (m, n), density, B, empty_cols=(0, n - 1), empty_rows=(17,))
    if with_empty:
        dA[1] = sp.csc_matrix((m, n))
    nnz = csc_pack(dA, B, (m, n))[3]
    per = 2.0 * nnz / (B * (m + n))
    assert lo < per <= hi, per
    e = _conic_handle(d, cones, B, n, "sparse")
    out_d, dx_d = e.forward(dA=_dense(dA), db=d["db"], dc=d["dc"])
    out_s, dx_s = e.forward(dA=dA, db=d["db"], dc=d["dc"])
    e.close()
    for b in range(B):
        e1, e2 = relfro(out_s[b], out_d[b]), relfro(dx_s[b], dx_d[b])
        print(f"{case[0]} per={per:.1f} b={b} out {e1:.2e} dx {e2:.2e}")
        assert e1 <= 1e-7 and e2 <= 1e-7, (b, e1, e2)
    np.testing.assert_array_equal(out_s, out_d)
    np.testing.assert_array_equal(dx_s, dx_d)


@pytest.mark.parametrize("route", ["sparse", "0"], ids=["sparse", "persistent"])
def test_conic_absent_and_empty_tangent_bit_identical(route):
    from diffopt_amd._arrays import csc_pack
    d, cones, B, n = _conic_data(M69, B=3)
    m = d["b"].shape[1]
    e = _conic_handle(d, cones, B, n, route)
    out0, dx0 = e.forward(dA=None, db=d["db"], dc=d["dc"])
    out_a, dx_a = _conic_forward_raw(e, None, d["db"], d["dc"])                    # NULL colptr
    out_e, dx_e = e.forward(dA=sp.csc_matrix((m, n)), db=d["db"], dc=d["dc"])      # nnz = 0
    out_r, dx_r = _conic_forward_raw(e, csc_pack(sp.csc_matrix((m, n)), B, (m, n)), d["db"], d["dc"])
    e.close()
    for got in (out_a, out_e, out_r):
        np.testing.assert_array_equal(got, out0)
    for got in (dx_a, dx_e, dx_r):
        np.testing.assert_array_equal(got, dx0)


# ---------------------------------------------------------------------------
# 4. sampled dA, conic
# ---------------------------------------------------------------------------
def test_conic_reverse_grads_at():
    """On a genuinely sparse A_moi (test_sparse_gpu's converging sparse-pattern
    family), so that a foreign pattern covers entries where A is zero."""
    from diffopt_amd import _lib
    from diffopt_amd.synthetic import conic_numpy_wellcond
    cones = [(0, 10), (3, 20)] * 20 + [(1, 200)] + [(4, 21)] * 2 + [(2, 50)]
    n, B = 900, 2
    d = conic_numpy_wellcond(B, n, cones, 77, pair_norm=1.0, sparse_k=5)
    m = d["b"].shape[1]
    A = [sp.csc_matrix(a) for a in d["A"]]
    for M in A:
        M.sort_indices()
    e = _conic_handle(d, cones, B, n, "sparse")
    g, dA, _, _ = e.reverse(d["dx"])
    rng = np.random.default_rng(5)
    foreign = _rand_sparse(rng, (m, n), 0.01, B)
    own_vals = e.reverse_grads_at(g)
    for_vals = e.reverse_grads_at(g, foreign)
    e.close()
    for b in range(B):
        assert (foreign[b].toarray() != 0)[d["A"][b] == 0].any()      # entries where A is zero
        cache = ocn.Cache(d["A"][b], d["b"][b], d["c"][b], d["x"][b], d["s"][b], d["y"][b], cones)
        odA, _, _ = ocn.reverse_outputs(cache, g[b])
        gx, gv = g[b][:n], g[b][n:n + m]
        for name, pat, vals in (("own", A[b], own_vals[b]), ("foreign", foreign[b], for_vals[b])):
            coo = pat.tocoo()     # canonical CSC order: column-major, rows ascending
            order = np.lexsort((coo.row, coo.col))
            i, j = coo.row[order], coo.col[order]
            assert vals.shape == i.shape
            bound = 4 * EPS * (np.abs(gv[i] * d["x"][b][j]) + np.abs(cache.vp[i] * gx[j]))
            diff = np.abs(vals - dA[b][i, j])
            print(f"{name} b={b} entries={len(i)} worst diff/bound {np.max(diff / np.maximum(bound, 1e-300)):.2f}")
            assert np.all(diff <= bound)
            assert relfro(vals, odA[i, j]) <= 1e-6


def test_conic_reverse_grads_at_null_pattern_needs_sparse_handle():
    from diffopt_amd import _lib
    from diffopt_amd.conic import ConicBatch
    d, cones, B, n = _conic_data(M69, B=1)
    e = ConicBatch(B, n, cones)
    e.set_csc([sp.csc_matrix(a) for a in d["A"]], d["b"], d["c"], d["x"], d["s"], d["y"])    # densified
    g = e.reverse(d["dx"], want_dA=False)[0]
    with pytest.raises(_lib.EngineError, match="sparse-route"):
        e.reverse_grads_at(g)
    # a given pattern works on every route
    pat = sp.csc_matrix(np.eye(d["b"].shape[1], n))
    vals = e.reverse_grads_at(g, pat)[0]
    dA = e.reverse(d["dx"])[1][0]
    np.testing.assert_allclose(vals, np.diag(dA)[: len(vals)], rtol=1e-12, atol=1e-15)
    e.close()


# ---------------------------------------------------------------------------
# 5. LP against the oracle and the dense tangents
# ---------------------------------------------------------------------------
def _shifted(d, b, dG, dA):
    """The vector tangents (dq', dh', db') a matrix tangent (dG, dA) reduces to."""
    return (d["dq"][b] + dG.T @ d["lam"][b] + dA.T @ d["nu"][b], d["dh"][b] - dG @ d["z"][b],
            d["db"][b] - dA @ d["z"][b])


def _qp_grad_check(d, b, rev, vals, pat, which, dense=None):
    """Sampled gradient values against the entry formulas in numpy — and against
    the dense gradient's entries when given — within 8·ε·Σ|terms|."""
    n, m = d["z"].shape[1], d["lam"].shape[1]
    z, lam, nu = d["z"][b], d["lam"][b], d["nu"][b]
    dz, dl, dn = rev[b][:n], rev[b][n:n + m], rev[b][n + m:]
    coo = pat.tocoo()
    order = np.lexsort((coo.row, coo.col))
    i, j = coo.row[order], coo.col[order]
    assert vals.shape == i.shape
    if which == "dG":
        t1, t2 = lam[i] * dl[i] * z[j], lam[i] * dz[j]
    elif which == "dA":
        t1, t2 = dn[i] * z[j], nu[i] * dz[j]
    else:
        t1, t2 = 0.5 * dz[i] * z[j], 0.5 * z[i] * dz[j]
    bound = 8 * EPS * (np.abs(t1) + np.abs(t2))
    diff = np.abs(vals - (t1 + t2))
    assert np.all(diff <= bound), (which, b, np.max(diff / np.maximum(bound, 1e-300)))
    if dense is not None:
        diff = np.abs(vals - dense[i, j])
        assert np.all(diff <= bound), (which, b, "dense", np.max(diff / np.maximum(bound, 1e-300)))


_LP5 = {}


def _lp5():
    """The LP of item 5 and every engine result its three tests read, computed once."""
    if _LP5:
        return _LP5
    from diffopt_amd.synthetic import lp_sparse_numpy
    B, n = 3, 300
    d = lp_sparse_numpy(B, n, 20, 200, 4, 101)
    m, p = d["lam"].shape[1], d["nu"].shape[1]
    rng = np.random.default_rng(9)
    dG = _rand_sparse(rng, (m, n), 0.02, B)
    dA = _rand_sparse(rng, (p, n), 0.05, B)
    patG = _rand_sparse(rng, (m, n), 0.02, B)
    patA = _rand_sparse(rng, (p, n), 0.05, B)
    e = _lp_handle(d)
    fwd_d = np.array(e.forward(dq=d["dq"], dG=_dense(dG), dh=d["dh"], dA=_dense(dA), db=d["db"]))
    it_d = e.lsqr_stats()[:, 1, :].copy()
    fwd_s = np.array(e.forward(dq=d["dq"], dG=dG, dh=d["dh"], dA=dA, db=d["db"]))
    stats = e.lsqr_stats().copy()
    rev_s, fwd_fr = e.forward_reverse(d["dl_dz"], dq=d["dq"], dG=dG, dh=d["dh"], dA=dA, db=d["db"])
    rev = np.array(rev_s)
    rev1 = np.array(e.reverse(d["dl_dz"]))
    dense = {k: np.array(v) for k, v in e.reverse_grads(rev, dQ=False).items() if k in ("dG", "dA")}
    at = {"foreign": e.reverse_grads_at(rev, G=patG, A=patA), "own": e.reverse_grads_at(rev)}
    e.close()
    _LP5.update(d=d, B=B, dG=dG, dA=dA, pats={"foreign": (patG, patA), "own": (d["G"], d["A"])}, fwd_d=fwd_d,
                it_d=it_d, fwd_s=fwd_s, stats=stats, rev=rev, rev1=rev1, fwd_fr=np.array(fwd_fr), dense=dense, at=at)
    return _LP5


def test_lp_forward_csc_vs_dense_tangents():
    """≤ 1e-7 (the issue's bar) and, as designed, bit for bit."""
    L = _lp5()
    errs = [relfro(L["fwd_s"][b], L["fwd_d"][b]) for b in range(L["B"])]
    print("lp vs dense tangents", [f"{v:.2e}" for v in errs], "iterations dense", L["it_d"][:, 1],
          "sparse", L["stats"][:, 1, 1])
    np.testing.assert_array_equal(L["fwd_fr"], L["fwd_s"])      # the fused call: the same runs, bit for bit
    np.testing.assert_array_equal(L["rev"], L["rev1"])
    assert max(errs) <= 1e-7, errs
    np.testing.assert_array_equal(L["fwd_s"], L["fwd_d"])
    np.testing.assert_array_equal(L["stats"][:, 1, :], L["it_d"])


def test_lp_forward_csc_vs_oracle():
    L = _lp5()
    d = L["d"]
    for b in range(L["B"]):
        dq2, dh2, db2 = _shifted(d, b, L["dG"][b], L["dA"][b])
        _, ofw, _, (itf, isf) = oqp.lp_sparse_differentiate(d["G"][b], d["h"][b], d["A"][b], d["z"][b], d["lam"][b],
                                                           d["nu"][b], d["dl_dz"][b], dq2, dh2, db2)
        eo = relfro(L["fwd_s"][b], ofw)
        print(f"lp b={b} vs oracle {eo:.2e} it={itf} istop={isf} engine {L['stats'][b, 1]}")
        assert isf in (1, 2) and L["stats"][b, 1, 0] == isf, (b, L["stats"][b], isf)
        assert eo <= 1e-6, (b, eo)


@pytest.mark.parametrize("which", ["foreign", "own"])
def test_lp_reverse_grads_at(which):
    """Sampled dG / dA against reverse_grads' dense entries and the entry formulas."""
    L = _lp5()
    d = L["d"]
    for b in range(L["B"]):
        for key, pat in zip(("dG", "dA"), L["pats"][which]):
            _qp_grad_check(d, b, L["rev"], L["at"][which][key][b], pat[b], key, dense=L["dense"][key][b])


@pytest.mark.parametrize("symmetric", [True, False], ids=["sym", "nonsym"])
def test_lp_sparse_dQ_vs_dense_dQ(symmetric):
    from diffopt_amd.synthetic import lp_sparse_numpy
    B, n = 3, 300
    d = lp_sparse_numpy(B, n, 20, 200, 4, 101)
    rng = np.random.default_rng(13)
    dQ = _rand_sparse(rng, (n, n), 0.02, B)
    if symmetric:
        dQ = [sp.csc_matrix(M + M.T) for M in dQ]
    e = _lp_handle(d)
    fd = e.forward(dQ=_dense(dQ), dq=d["dq"])
    fs = e.forward(dQ=dQ, dq=d["dq"])
    e.close()
    for b in range(B):
        err = relfro(fs[b], fd[b])
        print(f"dQ sym={symmetric} b={b} {err:.2e}")
        assert err <= 1e-7, (b, err)
    np.testing.assert_array_equal(fs, fd)


# ---------------------------------------------------------------------------
# 6. above the dense cap
# ---------------------------------------------------------------------------
def test_lp_above_dense_cap_matrix_tangents():
    """n + m + p = 9 100 > 8 192: dG and dA on the model's patterns; no dense
    m × n array is created anywhere in this test."""
    from diffopt_amd.qp import QPBatch
    from diffopt_amd.synthetic import lp_sparse_numpy
    n = 4000
    d = lp_sparse_numpy(1, n, 100, 1000, 5, 103)
    m, p = d["lam"].shape[1], d["nu"].shape[1]
    assert n + m + p > QPBatch.DENSE_MAX
    rng = np.random.default_rng(17)
    dG, dA = d["G"][0].copy(), d["A"][0].copy()
    dG.data = rng.standard_normal(dG.nnz)
    dA.data = rng.standard_normal(dA.nnz)
    e = _lp_handle(d, sparse=False)      # sparse by itself above the cap
    assert e.sparse
    fwd = e.forward(dq=d["dq"], dG=[dG], dh=d["dh"], dA=[dA], db=d["db"])
    stats = e.lsqr_stats()
    dq2, dh2, db2 = _shifted(d, 0, dG, dA)
    fwd_v = e.forward(dq=dq2[None], dh=dh2[None], db=db2[None])
    orv, ofw, _, (itf, isf) = oqp.lp_sparse_differentiate(d["G"][0], d["h"][0], d["A"][0], d["z"][0], d["lam"][0],
                                                         d["nu"][0], d["dl_dz"][0], dq2, dh2, db2)
    e1, e2 = relfro(fwd[0], ofw), relfro(fwd[0], fwd_v[0])
    print(f"above cap: vs oracle {e1:.2e} (it={itf} istop={isf}) vs vector tangents {e2:.2e}")
    assert isf in (1, 2) and stats[0, 1, 0] == isf
    assert e1 <= 1e-6 and e2 <= 1e-7, (e1, e2)
    rev = np.asarray(e.reverse(d["dl_dz"]))
    got = e.reverse_grads_at(rev)                     # NULL patterns: the handle's own G and A
    G0, A0 = d["G"][0].copy(), d["A"][0].copy()
    _qp_grad_check(d, 0, rev, got["dG"][0], G0, "dG")
    _qp_grad_check(d, 0, rev, got["dA"][0], A0, "dA")
    e.close()


# ---------------------------------------------------------------------------
# 7. reused handle
# ---------------------------------------------------------------------------
def test_reused_conic_handle_matches_fresh():
    d1, cones, B, n = _conic_data(M69, B=3)
    d2, _, _, _ = _conic_data(("m69b", 3, 60, M69[3], 43))
    m = d1["b"].shape[1]
    rng = np.random.default_rng(21)
    large = _rand_sparse(rng, (m, n), 0.6, B)
    small = _rand_sparse(rng, (m, n), 0.01, B)
    zero = [sp.csc_matrix((m, n))] * B
    steps = [("csc", large), ("dense", None), ("csc", small), ("set", None), ("csc", zero), ("csc", large)]
    e = _conic_handle(d1, cones, B, n, "sparse")
    d = d1
    for kind, T in steps:
        if kind == "dense":
            e.forward(dA=_dense(small), db=d["db"], dc=d["dc"])
        elif kind == "set":
            d = d2
            e.set_csc([sp.csc_matrix(a) for a in d["A"]], d["b"], d["c"], d["x"], d["s"], d["y"])
        else:
            got = e.forward(dA=T, db=d["db"], dc=d["dc"])
            f = _conic_handle(d, cones, B, n, "sparse")
            want = f.forward(dA=T, db=d["db"], dc=d["dc"])
            f.close()
            np.testing.assert_array_equal(got[0], want[0])
            np.testing.assert_array_equal(got[1], want[1])
    e.close()


def test_reused_lp_handle_matches_fresh():
    from diffopt_amd.synthetic import lp_sparse_numpy
    B, n = 2, 120
    d1 = lp_sparse_numpy(B, n, 10, 80, 3, 102)
    d2 = lp_sparse_numpy(B, n, 10, 80, 3, 202)
    m, p = d1["lam"].shape[1], d1["nu"].shape[1]
    rng = np.random.default_rng(23)

    def tangents(density):
        return (_rand_sparse(rng, (m, n), density, B), _rand_sparse(rng, (p, n), density, B))

    large, small = tangents(0.5), tangents(0.01)
    zero = ([sp.csc_matrix((m, n))] * B, [sp.csc_matrix((p, n))] * B)
    steps = [("csc", large), ("dense", None), ("csc", small), ("set", None), ("csc", zero), ("csc", large)]
    e = _lp_handle(d1)
    d = d1
    for kind, T in steps:
        if kind == "dense":
            e.forward(dq=d["dq"], dG=_dense(small[0]), dh=d["dh"], dA=_dense(small[1]), db=d["db"])
        elif kind == "set":
            d = d2
            e.set_csc([sp.csc_matrix((n, n))] * B, d["G"], d["h"], d["A"], d["z"], d["lam"], d["nu"])
        else:
            got = e.forward(dq=d["dq"], dG=T[0], dh=d["dh"], dA=T[1], db=d["db"])
            f = _lp_handle(d)
            want = f.forward(dq=d["dq"], dG=T[0], dh=d["dh"], dA=T[1], db=d["db"])
            f.close()
            np.testing.assert_array_equal(got, want)
    e.close()


# ---------------------------------------------------------------------------
# 8. refusals
# ---------------------------------------------------------------------------
def _broken(packed, ncols, rows, how):
    cp, rv, nz, nnz = (np.array(a, copy=True) if isinstance(a, np.ndarray) else a for a in packed)
    if how == "colptr":
        cp[1] = cp[-1] + 5          # column 0 ends past nnz, column 1 ends before it starts
    elif how == "rowval":
        rv[nnz // 2] = rows + 3
    else:                                                         # overlap: problem 1 reuses problem 0's entry range
        cp[ncols + 1: 2 * (ncols + 1)] = cp[: ncols + 1]
    return cp, rv, nz, nnz


@pytest.mark.parametrize("how", ["colptr", "rowval", "overlap"])
def test_conic_csc_refusals(how):
    from diffopt_amd import _lib
    from diffopt_amd._arrays import csc_pack
    d, cones, B, n = _conic_data(M69, B=2)
    m = d["b"].shape[1]
    rng = np.random.default_rng(31)
    good = _rand_sparse(rng, (m, n), 0.1, B)
    e = _conic_handle(d, cones, B, n, "sparse")
    before = e.forward(dA=good, db=d["db"], dc=d["dc"])
    bad = _broken(csc_pack(good, B, (m, n)), n, m, how)
    with pytest.raises(_lib.EngineError, match={"colptr": "colptr", "rowval": "rowval", "overlap": "disjoint"}[how]):
        _conic_forward_raw(e, bad, d["db"], d["dc"])
    after = e.forward(dA=good, db=d["db"], dc=d["dc"])
    np.testing.assert_array_equal(after[0], before[0])
    np.testing.assert_array_equal(after[1], before[1])
    e.close()


@pytest.mark.parametrize("how", ["colptr", "rowval", "overlap"])
def test_lp_csc_refusals(how):
    from diffopt_amd import _lib
    from diffopt_amd._arrays import csc_pack
    from diffopt_amd.synthetic import lp_sparse_numpy
    B, n = 2, 120
    d = lp_sparse_numpy(B, n, 10, 80, 3, 102)
    m = d["lam"].shape[1]
    rng = np.random.default_rng(33)
    good = _rand_sparse(rng, (m, n), 0.1, B)
    e = _lp_handle(d)
    before = e.forward(dq=d["dq"], dG=good, dh=d["dh"], db=d["db"])
    bad = _broken(csc_pack(good, B, (m, n)), n, m, how)
    with pytest.raises(_lib.EngineError, match={"colptr": "colptr", "rowval": "rowval", "overlap": "disjoint"}[how]):
        _qp_forward_raw(e, (None, bad, None), d["dq"], d["dh"], d["db"])
    after = e.forward(dq=d["dq"], dG=good, dh=d["dh"], db=d["db"])
    np.testing.assert_array_equal(after, before)
    e.close()


def test_qp_csc_calls_refused_on_dense_route():
    from diffopt_amd import _lib
    from diffopt_amd.synthetic import lp_sparse_numpy
    B, n = 2, 120
    d = lp_sparse_numpy(B, n, 10, 80, 3, 102)
    m, p = d["lam"].shape[1], d["nu"].shape[1]
    rng = np.random.default_rng(35)
    dG = _rand_sparse(rng, (m, n), 0.05, B)
    e = _lp_handle(d, sparse=False)
    assert not e.sparse
    before = e.forward_reverse(d["dl_dz"], dq=d["dq"], dh=d["dh"], db=d["db"])
    with pytest.raises(_lib.EngineError, match=r"takes dopt_qp_forward$"):
        e.forward(dq=d["dq"], dG=dG)
    with pytest.raises(_lib.EngineError, match=r"takes dopt_qp_forward_reverse$"):
        e.forward_reverse(d["dl_dz"], dq=d["dq"], dG=dG)
    with pytest.raises(_lib.EngineError, match=r"takes dopt_qp_reverse_grads$"):
        e.reverse_grads_at(np.asarray(before[0]), G=dG)
    after = e.forward_reverse(d["dl_dz"], dq=d["dq"], dh=d["dh"], db=d["db"])
    np.testing.assert_array_equal(after[0], before[0])
    np.testing.assert_array_equal(after[1], before[1])
    e.close()

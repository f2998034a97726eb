"""The cone edge cases (cone_edge_cases.py) are what they claim — on the
oracle alone, no GPU.  Per cone: the branch the oracle takes (the SOC case
index; every eigenvalue ≥ 0, every eigenvalue < 0, the exact ties in the
Daleckii–Krein weights), the guard band of every non-exact cone, and on exact
cones the oracle's π against the closed form bit for bit.  Per problem: the
capped runs stop as (k, 7), the π probe is one exact LSQR step with
db = −4·π(v), and the measured spreads — the oracle under 1-ulp perturbations,
and against the same oracle on a second eigensolver (jacobi_dpi) — from which
test_cone_edges_gpu.py takes its bars, never from the engine.  Every family
prints its spreads and bars (pytest -s)."""

import numpy as np
import pytest

import cone_edge_cases as ec
from oracle import cones as C


def _slices(d):
    off = C.cone_offsets(d["cones"])
    return [slice(off[i], off[i + 1]) for i in range(len(d["cones"]))]


def _check_cone(d, p, i, sl, cache):
    code, dim = d["cones"][i]
    kind, exact, branch = d["info"][p][i]
    what = ec.cone_label(d, p, i)
    v, vp = cache.v[sl], cache.vp[sl]
    if dim == 0:
        assert branch == "empty" and cache.blocks[i].shape == (0, 0)
        return
    blk = cache.blocks[i]
    if code in (C.ZEROS, C.NONNEG, C.NONPOS):
        if exact:
            assert np.any(v == 0.0) and np.all(v == np.round(2 * v) / 2), what
            closed = v if code == C.ZEROS else np.maximum(v, 0.0) if code == C.NONNEG else np.minimum(v, 0.0)
            np.testing.assert_array_equal(vp, closed, err_msg=what)
            if code != C.ZEROS:    # engine and oracle agree on 0.5 at v = 0
                np.testing.assert_array_equal(np.diag(blk)[v == 0.0], 0.5, err_msg=what)
        else:
            assert np.all(np.abs(v) >= 0.5), what
            assert dim == 1 or ((v > 0).any() and (v < 0).any()), what
        return
    if code == C.SOC:
        _, cs, closed = branch
        t, nx = v[0], float(np.linalg.norm(v[1:]))
        took = 0 if nx <= t else 1 if nx <= -t else 2
        assert took == cs, (what, took, cs)
        if cs == 0:
            np.testing.assert_array_equal(blk, np.eye(dim), err_msg=what)
        if cs == 1:
            assert not blk.any() and not vp.any(), what
        if exact:
            np.testing.assert_array_equal(vp, closed, err_msg=what)
        else:
            assert abs(nx - abs(t)) >= 0.1 * nx, (what, nx, t)
        return
    _, spec, lam0 = branch
    side = C.psd_side(dim)
    lam = np.linalg.eigvalsh(C.smat(v, side))
    ident = isinstance(blk, np.ndarray) and np.array_equal(blk, np.eye(dim)) or getattr(blk, "ident", False)
    if kind in ("pos", "diagpos", "pos1", "zero1"):
        assert np.all(lam >= 0) and ident, what
    elif kind in ("neg", "neg1"):
        assert np.all(lam < 0) and not vp.any() if exact else np.all(lam < 0), what
        zero = (blk @ np.ones(dim)) if not isinstance(blk, np.ndarray) else blk
        assert np.abs(zero).max() == 0.0, what
    else:
        assert lam.min() < 0 < lam.max() and not ident, what
    if exact:
        np.testing.assert_array_equal(lam, np.sort(lam0), err_msg=what)     # LAPACK leaves a diagonal input alone
        np.testing.assert_array_equal(vp, C.tri(np.diag(np.maximum(lam0, 0.0))), err_msg=what)
        # exact ties in B off the diagonal, as designed (the li == lj branch), zeros among them
        ties = sum(lam[a] == lam[b] for a in range(side) for b in range(side) if a != b)
        want = sum(lam0[a] == lam0[b] for a in range(side) for b in range(side) if a != b)
        assert ties == want, (what, ties, want)
        if kind == "diag" and side >= 4:
            assert ties >= 2 and np.sum(lam == 0.0) >= 2, what
    else:
        assert np.abs(lam).min() >= 1e-3 * np.abs(lam).max(), (what, lam)
        np.testing.assert_allclose(lam, np.sort(lam0), rtol=0, atol=1e-13 * side)


@pytest.mark.parametrize("family", ec.FAMILIES)
def test_cases_take_their_branches(family):
    kinds = set()
    for ti, d in enumerate(ec.batches(family)):
        sls = _slices(d)
        for p in range(d["B"]):
            cache = ec.reference(family, ti, p, 1)["cache"]
            np.testing.assert_array_equal(cache.v, d["y"][p] - d["s"][p])
            for i, sl in enumerate(sls):
                _check_cone(d, p, i, sl, cache)
                kinds.add((d["cones"][i][0], d["info"][p][i][0]))
            for k in ec.CAPS:
                for sparse in ((False,) if family in ec.SPLIT_ONLY else (False, True)):
                    info = ec.reference(family, ti, p, k, sparse)["info"]
                    assert info == ((k, 7), (k, 7)), (family, ti, p, k, sparse, info)
            g, db, info, vp = ec.probe_reference(family, ti, p)
            assert info == (1, 1), (family, ti, p, info)
            np.testing.assert_array_equal(g, np.concatenate([np.zeros(d["m"] + 1), [4.0]]))
            np.testing.assert_array_equal(db, -4.0 * vp)
            np.testing.assert_array_equal(vp, cache.vp)
    print(f"[cone-edge] {family}: kinds " + ", ".join(sorted(f"{C.NAMES[c][:3]}:{k}" for c, k in kinds)))


def test_every_listed_branch_occurs():
    """Over all families: every SOC kind, every spectrum, both elementwise
    kinds on Nonnegatives and Nonpositives."""
    seen = {(d["cones"][i][0], d["info"][p][i][0]) for f in ec.FAMILIES for d in ec.batches(f)
            for p in range(d["B"]) for i in range(len(d["cones"])) if d["cones"][i][1] > 0}
    for k in list(ec.SOC_EXACT) + list(ec.SOC_GENERIC):
        assert (C.SOC, k) in seen, k
    for k in ec.SPECTRA + ["diagpos", "pos1", "neg1", "zero1"]:
        assert (C.PSD, k) in seen, k
    for code in (C.NONNEG, C.NONPOS):
        assert (code, "rand") in seen and (code, "ints") in seen
    # the table sizes around the LDS copy of the cone table and the fused split's partial-sum stride
    assert [len(d["cones"]) for d in ec.batches("many_cones")] == [128, 129, 300]


@pytest.mark.parametrize("side", [1, 2, 7, 16, 33])
def test_jacobi_is_a_second_reference(side):
    """jacobi_dpi against LAPACK on a well-separated spectrum: eigenvalues,
    π and the dense block to rounding."""
    rng = np.random.default_rng(side)
    lam = ec.psd_spectrum(side, "mixed", rng) if side > 1 else np.array([-1.5])
    Q = np.linalg.qr(rng.standard_normal((side, side)))[0]
    v = C.tri((Q * lam) @ Q.T)
    w, U = ec.jacobi_eigh(C.smat(v, side))
    np.testing.assert_allclose(w, np.sort(lam), rtol=0, atol=1e-14 * side)
    np.testing.assert_allclose(U.T @ U, np.eye(side), rtol=0, atol=1e-14 * side)
    pi, blk = ec.jacobi_dpi(v)
    np.testing.assert_allclose(pi, C.proj(C.PSD, v), rtol=0, atol=1e-13)
    np.testing.assert_allclose(blk, C.dproj(C.PSD, v), rtol=0, atol=1e-13)


@pytest.mark.parametrize("family", ec.FAMILIES)
def test_spreads_and_bars(family):
    """Measured on the oracle alone; every spread ≤ SPREAD_LIMIT, so no bar
    exceeds 1e-9 (DESIGN.md §5c has the table)."""
    for ti, d in enumerate(ec.batches(family)):
        for p in range(d["B"]):
            sp = ec.spread(family, ti, p)
            bar = ec.bar(family, ti, p)
            print(f"[cone-edge] {family} table {ti} ({len(d['cones'])} cones, m = {d['m']}) problem {p}: "
                  f"1-ulp spread {sp['ulp']:.2e}, LAPACK − Jacobi {sp['jacobi']:.2e}, bar {bar:.2e}")
            assert max(sp.values()) <= ec.SPREAD_LIMIT, (family, ti, p, sp)
            assert ec.BAR_FLOOR <= bar <= 10 * ec.SPREAD_LIMIT

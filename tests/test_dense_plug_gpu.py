"""The engine's arbitrary-matrix entry on matrices the test chooses
(dense_plug_cases.py, pinned by test_dense_plug_cases_cpu.py): the
``LinearAlgebraSolver`` plug point (dopt_lhs_solve / dopt_lhs_resolve,
``MI355XSolver``) and KKT mode (dopt_nlp_set_kkt / _factor / _kkt_solve), and
through them the no-pivot LU and its acceptance tests (qp_nopiv.hip), the
partial-pivoting blocked LU (qp_blocked.hip), the singular-pivot verdict
(nlp.hip) and the MFMA multi-RHS sweep (qp_multi.hip: every direct solve on
this entry, k = 1 too) — at the block, panel, LDS-storage and seed-chunk
edges, with both ``trans``, under the default LU and under DOPT_LU=0.

Discrete results are exact: ``lu_kind`` is NOPIV exactly where the CPU
predicate ``nopiv_accepts`` says so (PIVOT everywhere under DOPT_LU=0),
``info`` is the zeroed column + 1, ``corrections`` is the oracle's; the spike
solutions equal the exact integer solution to 1e-13 absolute.

Every regular solve (one problem of one call, its k right-hand sides) is held
to LAPACK (``np.linalg.solve``) on the same system, with the exact x*
(b = M·x* in integers) as the forward reference.  Every side must satisfy

    η(x)   = ‖b − M x‖∞ / (‖M‖∞‖x‖∞ + ‖b‖∞)  ≤  max(C·η_lapack,   rows·ε)
    fwd(x) = ‖x − x*‖₂ / ‖x*‖₂                ≤  max(C·fwd_lapack, rows·ε)

in long double, where η_lapack / fwd_lapack is LAPACK's worst side of that
solve.  Both codes are backward-stable LUs with bounded growth; they differ
by pivot ties and summation order (the rows·ε term) and by the no-pivot
route's multipliers of up to 10 (C).  The yardstick is per solve, not side
against side: at equal η the forward error of one side is a matter of its
direction — LAPACK's own spreads over 4.6e-15 … 9.2e-14 across the 17 sides of
the 65-row ``gauss`` matrix of the KKT case, and side against side the engine
/ LAPACK ratio reaches 39.7 there (engine 1.9e-13 on a side where LAPACK
has 4.8e-15) while worst against worst it is 2.8.

Measured on the MI355X (every solve of this module, about 1550, both LU
modes; worst per family and route; "ratio" = engine / LAPACK over the solves
whose engine figure is above the rows·ε floor — below it the floor admits
them and C plays no part — and "(any)" the same ratio over all solves):

    family   route   η worst   ratio (any)     fwd worst   ratio (any)
    dom      NOPIV   13.3 ε    – (11.4)        2.4e-15     – (9.6)
    dom      PIVOT   13.8 ε    – (11.3)        2.4e-15     – (9.6)
    perm     PIVOT    3.9 ε    – (5.0)         9.4e-16     – (4.4)
    antidiag PIVOT    4.0 ε    – (4.9)         9.4e-16     – (4.3)
    gauss    PIVOT   20.6 ε    – (10.9)        5.0e-12     4.78 (4.78)
    saddle   PIVOT    0.1 ε    – (2.0)         no bar (condition ≈ 1e8)
    (perm, antidiag, gauss NOPIV: the 1 × 1 cases only, solved exactly)

No η is above its floor (the largest, 20.6 ε, is at 1536 rows).  The worst
ratio is 4.78 (``gauss`` under partial pivoting, 95 rows, forward error
4.4e-14 against 9.3e-15), so C = 32, the next power of two above 4 × 4.78."""

import ctypes

import numpy as np
import pytest

import dense_plug_cases as dc

pytestmark = pytest.mark.gpu

C = 32.0


@pytest.fixture(params=["nopiv", "pivot"])
def lu_mode(request, monkeypatch):
    if request.param == "pivot":
        monkeypatch.setenv("DOPT_LU", "0")
    else:
        monkeypatch.delenv("DOPT_LU", raising=False)
    return request.param


def _kind_name(kind):
    from diffopt_amd import _lib
    return {_lib.LU_KIND_NOPIV: "NOPIV", _lib.LU_KIND_PIVOT: "PIVOT"}.get(int(kind), str(int(kind)))


def want_kinds(lu_mode, accepted):
    """NOPIV exactly where the no-pivot rule accepts, PIVOT everywhere under DOPT_LU=0."""
    from diffopt_amd import _lib
    return [_lib.LU_KIND_NOPIV if (a and lu_mode == "nopiv") else _lib.LU_KIND_PIVOT for a in accepted]


def _ratio(got, lapack, floor):
    """engine / LAPACK where the engine's figure is above the rows·ε floor, else 0."""
    if not got > floor:
        return 0.0
    return got / lapack if lapack > 0 else float("inf")


class Judge:
    """Collects every figure of a test before anything is asserted: one
    printed line per problem and ``trans`` (pytest -s), then ``done()``."""

    def __init__(self, what):
        self.what, self.bad = what, []

    def regular(self, tag, family, kind, A, x, b, xstar, lap):
        """One solve: x (rows, k) against b = A·xstar; lap = dc.lapack_errors'
        (η, fwd) of the same solve.  Every side is held to LAPACK's worst side."""
        rows, k = b.shape
        floor = rows * dc.EPS
        assert x.shape == b.shape
        if not np.isfinite(x).all():
            self.bad.append(f"{tag}: non-finite solution")
            return
        lap_eta = float(lap[0].max())
        etas = np.array([dc.eta(A, x[:, c], b[:, c]) for c in range(k)])
        for c in np.flatnonzero(~(etas <= max(C * lap_eta, floor))):
            self.bad.append(f"{tag} side {c}: η {etas[c] / dc.EPS:.2f} ε, LAPACK {lap_eta / dc.EPS:.2f} ε")
        line = (f"η {etas.max() / dc.EPS:.2f} ε (LAPACK {lap_eta / dc.EPS:.2f} ε, "
                f"ratio above floor {_ratio(etas.max(), lap_eta, floor):.2f})")
        if xstar is not None:
            lap_fwd = float(lap[1].max())
            fwds = np.array([dc.forward_error(x[:, c], xstar[:, c]) for c in range(k)])
            for c in np.flatnonzero(~(fwds <= max(C * lap_fwd, floor))):
                self.bad.append(f"{tag} side {c}: forward error {fwds[c]:.3e}, LAPACK {lap_fwd:.3e}")
            line += (f"; fwd {fwds.max():.2e} (LAPACK {lap_fwd:.2e}, ratio above floor "
                     f"{_ratio(fwds.max(), lap_fwd, floor):.2f}, side by side "
                     f"{max(_ratio(f, l, floor) for f, l in zip(fwds, lap[1])):.2f})")
        print(f"[dense-plug] {self.what} {tag} family {family} route {_kind_name(kind)} rows {rows} k {k}: {line}")

    def done(self):
        assert not self.bad, "\n".join(self.bad)


def _sides(mats, seeds, k, trans):
    """(B, rows, k) right-hand sides b = M·x* (Mᵀ·x*), and the x*."""
    pairs = [dc.rhs(M, k, s, trans) for M, s in zip(mats, seeds)]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def run_family_batch(what, lu_mode, families, rows, seeds, k):
    """solve_system on the batch, then dopt_lhs_resolve with trans 0 and 1;
    lu_kind against the predicate; every side of every problem judged."""
    from diffopt_amd.qp import MI355XSolver
    mats = [dc.matrix(f, rows, s) for f, s in zip(families, seeds)]
    Ms = np.stack(mats)
    B0, X0 = _sides(mats, seeds, k, False)
    B1, X1 = _sides(mats, seeds, k, True)
    s = MI355XSolver()
    try:
        got = s.solve_system(Ms, B0)
        kinds = s.lu_kind()
        again = s.resolve(B0, trans=False)
        gott = s.resolve(B1, trans=True)
        kinds_after = s.lu_kind()
    finally:
        s.close()
    np.testing.assert_array_equal(kinds, want_kinds(lu_mode, [dc.accepts(f, rows, sd) for f, sd in zip(families, seeds)]))
    np.testing.assert_array_equal(kinds_after, kinds)
    np.testing.assert_array_equal(again, got)      # the same factors, sides and kernel
    j = Judge(what)
    for b, (f, sd, M) in enumerate(zip(families, seeds, mats)):
        j.regular(f"problem {b} trans 0", f, kinds[b], M, got[b], B0[b], X0[b], dc.lapack(f, rows, sd, k, False))
        j.regular(f"problem {b} trans 1", f, kinds[b], M.T, gott[b], B1[b], X1[b], dc.lapack(f, rows, sd, k, True))
    j.done()


# ---- a. block edges -----------------------------------------------------------
@pytest.mark.parametrize("family", dc.FAMILIES)
@pytest.mark.parametrize("rows", dc.BLOCK_ROWS)
def test_block_edges(rows, family, lu_mode):
    run_family_batch("block", lu_mode, [family, family], rows, [0, 1], 3)


# ---- b. storage and panel edges -----------------------------------------------
@pytest.mark.parametrize("family", dc.STORAGE_FAMILIES)
@pytest.mark.parametrize("rows", dc.STORAGE_ROWS)
def test_storage_and_panel_edges(rows, family, lu_mode):
    run_family_batch("storage", lu_mode, [family, family], rows, [0, 1], 3)


@pytest.mark.parametrize("family", dc.STORAGE_FAMILIES)
def test_two_chunks_in_global_workspace(family, lu_mode):
    run_family_batch("storage-2chunks", lu_mode, [family, family], 1153, [0, 1], dc.MKC + 1)


@pytest.mark.parametrize("family", dc.STORAGE_FAMILIES)
@pytest.mark.parametrize("rows", dc.PACK_ROWS)
def test_pinned_pack_threshold(rows, family, lu_mode):
    run_family_batch("pack", lu_mode, [family], rows, [0], 1)


def test_above_pivot_max_refused(lu_mode):
    from diffopt_amd import _lib
    from diffopt_amd.qp import MI355XSolver
    rows = dc.PIVOT_MAX + 1
    M = dc.dom(rows)
    s = MI355XSolver()
    try:
        with pytest.raises(_lib.EngineError, match=f"larger than {dc.PIVOT_MAX}") as ei:
            s.solve_system(M, dc.rhs(M, 1)[0])
        assert not isinstance(ei.value, _lib.SingularException) and ei.value.code < 0
    finally:
        s.close()


# ---- c. seed-chunk edges --------------------------------------------------------
@pytest.mark.parametrize("batch", dc.CHUNK_BATCHES)
@pytest.mark.parametrize("k", dc.CHUNK_K)
def test_seed_chunk_edges(k, batch, lu_mode):
    """perm and dom mixed in one batch (both factor kinds in one launch);
    every seed of every problem is compared."""
    families = [("perm", "dom")[b % 2] for b in range(batch)]
    run_family_batch("chunk", lu_mode, families, dc.CHUNK_ROWS, list(range(batch)), k)


# ---- d. acceptance sites ----------------------------------------------------------
@pytest.mark.parametrize("site", dc.SPIKE_SITES)
def test_acceptance_sites(site, lu_mode):
    """One batch of the four spikes ±10, ±10.5 at the site: accepted, accepted,
    refused, refused; the solution is the exact integer one either way."""
    from diffopt_amd.qp import MI355XSolver
    i, jc = site
    mats = [dc.spike(dc.SPIKE_ROWS, i, jc, c) for c in dc.SPIKE_C]
    seeds = list(range(len(mats)))
    B0, X0 = _sides(mats, seeds, 3, False)
    B1, X1 = _sides(mats, seeds, 3, True)
    s = MI355XSolver()
    try:
        got = s.solve_system(np.stack(mats), B0)
        kinds = s.lu_kind()
        gott = s.resolve(B1, trans=True)
    finally:
        s.close()
    print(f"[dense-plug] spike {site}: kinds {[_kind_name(v) for v in kinds]}, "
          f"max |x − x*| {np.abs(got - X0).max():.2e} (trans 1: {np.abs(gott - X1).max():.2e})")
    np.testing.assert_array_equal(kinds, want_kinds(lu_mode, [abs(c) <= dc.NOPIV_LMAX for c in dc.SPIKE_C]))
    np.testing.assert_allclose(got, X0, rtol=0, atol=1e-13)
    np.testing.assert_allclose(gott, X1, rtol=0, atol=1e-13)


# ---- e. singular verdicts (raw ABI: the outputs survive the non-zero return) ------
def _seed_major(Bs):
    return np.ascontiguousarray(np.transpose(Bs, (2, 0, 1)))      # (B, rows, k) → (k, B, rows)


@pytest.mark.parametrize("how", ("zero", "tiny"))
@pytest.mark.parametrize("family", ("dom", "perm"))
@pytest.mark.parametrize("rows", dc.SINGULAR_ROWS)
def test_singular_verdicts(rows, family, how, lu_mode):
    """[dom, a singular matrix, gauss] per zeroed column: info = column + 1 from
    dopt_lhs_solve and again from dopt_lhs_resolve, the singular problem's
    output all zeros, the regular problems' within the bars.  "zero": the LU
    itself meets the zero pivot; "tiny" (column scaled by 2^-80): no pivot is
    zero and the rank-revealing test alone gives the verdict — on the
    no-pivot factors for ``dom``, which the scaling leaves accepted."""
    from diffopt_amd import _lib
    from diffopt_amd.qp import MI355XSolver
    lib = _lib.load()
    k = 3
    j = Judge("singular")
    for col in dc.singular_columns(rows):
        Z = (dc.zero_col if how == "zero" else dc.tiny_col)(family, rows, 1, col)
        mats = [dc.dom(rows, 0), Z, dc.gauss(rows, 2)]
        fams, seeds = ["dom", None, "gauss"], [0, 1, 2]
        B0, X0 = _sides(mats, seeds, k, False)
        B1, X1 = _sides(mats, seeds, k, True)
        Mc = np.ascontiguousarray(np.swapaxes(np.stack(mats), 1, 2))   # column-major per problem
        h = ctypes.c_void_p()
        assert lib.dopt_create(ctypes.byref(h), 0, 3, rows, 0, 0, _lib.DOPT_KIND_NLP) == 0
        try:
            outs = []
            r0 = _seed_major(B0)
            x0 = np.full_like(r0, np.nan)
            rc = lib.dopt_lhs_solve(h, rows, Mc.ctypes.data, k, r0.ctypes.data, x0.ctypes.data, 0)
            assert rc == col + 1, (rows, family, col, rc)
            kinds = np.zeros(3, dtype=np.int8)
            assert lib.dopt_qp_get_lu_kind(h, kinds.ctypes.data) == 0
            outs.append((0, x0, B0, X0))
            for trans, Bs, Xs in ((0, B0, X0), (1, B1, X1)):
                r = _seed_major(Bs)
                x = np.full_like(r, np.nan)
                rc = lib.dopt_lhs_resolve(h, k, r.ctypes.data, x.ctypes.data, trans)
                assert rc == col + 1, (rows, family, col, trans, rc)   # the same info again
                outs.append((trans, x, Bs, Xs))
        finally:
            lib.dopt_destroy(h)
        np.testing.assert_array_equal(kinds, want_kinds(lu_mode, [True, dc.nopiv_accepts(Z), False]))
        for n, (trans, x, Bs, Xs) in enumerate(outs):
            X = np.transpose(x, (1, 2, 0))                                 # (B, rows, k)
            np.testing.assert_array_equal(X[1], 0.0)                       # the singular problem: zeros
            for b in (0, 2):
                A = mats[b].T if trans else mats[b]
                j.regular(f"column {col} call {n} problem {b} trans {trans}", fams[b], kinds[b], A, X[b], Bs[b],
                          Xs[b], dc.lapack(fams[b], rows, seeds[b], k, bool(trans)))
        # through the wrapper: SingularException carries the same info
        s = MI355XSolver()
        try:
            with pytest.raises(_lib.SingularException) as ei:
                s.solve_system(np.stack(mats), B0)
            assert ei.value.info == col + 1
            with pytest.raises(_lib.SingularException) as ei:
                s.resolve(B1, trans=True)
            assert ei.value.info == col + 1
        finally:
            s.close()
    j.done()


# ---- f. KKT mode with inertia correction ---------------------------------------------
@pytest.mark.parametrize("rows", dc.SADDLE_ROWS)
def test_kkt_mode_saddles(rows, lu_mode):
    """[saddle (zero row first), gauss, saddle (zero row last)]: corrections
    [1, 0, 1] as the oracle (pinned on the CPU); the saddles' solves are judged
    by η on the corrected matrix M + 1e-6·D — its condition is ≈ 1e8, so no
    forward-error bar — and the regular middle problem by both bars.  KKT
    mode with the inertia correction goes to partial pivoting directly."""
    from diffopt_amd.nlp import NLPBatch
    nw, nc = dc.saddle_split(rows)
    mats = [dc.saddle(nw, nc, 0), dc.gauss(rows, 3), dc.saddle(nw, nc, nc - 1)]
    e = NLPBatch(3, rows, 0, 0)
    j = Judge("kkt")
    try:
        e.set_kkt(np.stack(mats), nw, nc)
        e.factor()
        np.testing.assert_array_equal(e.corrections(), [1, 0, 1])
        kinds = e.lu_kind()
        np.testing.assert_array_equal(kinds, want_kinds(lu_mode, [False, False, False]))
        for k in (1, dc.MKC + 1):
            Bg, Xg = dc.rhs(mats[1], k, 3)
            Bs = np.stack([dc.solution(rows, k, 10), Bg, dc.solution(rows, k, 12)])   # saddles: integer sides
            x = np.transpose(e.kkt_solve(_seed_major(Bs)), (1, 2, 0))
            for b in (0, 2):
                Cm = dc.saddle_corrected(mats[b], nw, nc, 1)
                j.regular(f"k {k} problem {b}", "saddle", kinds[b], Cm, x[b], Bs[b], None,
                          dc.lapack_errors(Cm, Bs[b], None))
            j.regular(f"k {k} problem 1", "gauss", kinds[1], mats[1], x[1], Bg, Xg, dc.lapack("gauss", rows, 3, k))
        np.testing.assert_array_equal(e.corrections(), [1, 0, 1])
    finally:
        e.close()
    j.done()

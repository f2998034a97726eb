"""Model sequences for one long-lived handle (test_reuse_cases_cpu.py proves
their properties on the oracle, test_handle_reuse_gpu.py runs them).

The shipped callers keep one handle per shape and set model after model on it
(the Julia QPModel / ConicModel, bench.py, the sharded driver), so every
sequence here crosses some state the handle carries from the previous model:
sizes (the padded batch size, the multi-RHS buffers), factorisation kinds
(no-pivot / partial pivoting / generic / LSQR / the one-workgroup small
path), the P-symmetric route, staging and memory mode, the sparse route, and
for conic handles the cone table, the packed Dπ length and the large-PSD
scratch; for NLP handles the structure (num_w, the bound blocks, the rows of
M), the route of single problems (reduced, inertia-corrected on the full M,
asymmetric), the speculative launch's switch and a deferred factorisation.

A step is a dict: ``name``, ``data`` (the generator's arrays, batch-stacked;
never modified by a test), and the properties it is built to have —

* QP: ``nsys`` (N' = n + kept rows + p per problem; every row is kept on the
  LSQR branch), ``lu_kind`` (the kind
  ``dopt_qp_get_lu_kind`` reports under the default LU mode after the
  step's last factorisation), ``iterative`` (the reference's norm(Q) ≈ 0
  branch), ``sym`` (the P-symmetric route, default mode), ``how`` (the
  setter: "set", "csc" or "device");
* conic: ``cones`` and ``comparable`` (the oracle's LSQR converges, istop
  1–2, forward and reverse, on every problem: the step is held to the oracle
  at 1e-6 with no relaxed output);
* NLP: ``st`` (the structure), ``restructure`` (the step calls set_structure
  first), ``nsys`` (n + c on the reduced route, the rows of M for a corrected
  problem), ``corrected`` and ``asym`` (the problems concerned), ``saddle``
  (equalities only, no bounds: M itself is the saddle-point matrix).

Sequences are built once per process (lru_cache) and shared."""

import functools

import numpy as np

from diffopt_amd.synthetic import conic_numpy, conic_numpy_wellcond, lp_sparse_numpy, nlp_numpy, qp_numpy
from oracle import conic as ocn
from oracle import nlp as onlp
from oracle import qp as oqp

LSQR, NOPIV, PIVOT, SMALL = 0, 1, 2, 3   # _lib.LU_KIND_*
SM_MAX, PIVOT_MAX = 128, 1536            # dopt_internal.h

QP_KEYS = ("Q", "G", "h", "A", "z", "lam", "nu")


# ---------------------------------------------------------------------------
# QP
# ---------------------------------------------------------------------------
def indefinite(d, idx, seed=5):
    """Q of the problems `idx` replaced by a symmetric indefinite matrix with
    a 1e-4 diagonal: the no-pivot LU's first multipliers are ~1e4, the
    threshold test rejects the problem (test_qp_gpu._indefinite).  The engine
    never reads q, so (z, λ, ν) stays a KKT point."""
    rng = np.random.default_rng(seed)
    n = d["Q"].shape[1]
    for b in idx:
        S = rng.standard_normal((n, n))
        Q = (S + S.T) / 2
        Q[np.diag_indices(n)] = 1e-4
        d["Q"][b] = Q
    return d


def stacked(parts):
    """One batch from single-problem generator results (problems of
    different φ in one batch)."""
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def qp_kept(B, n, m, p, phi, seed, extra=0):
    """qp_numpy(φ) with `extra` of each problem's inactive rows given the
    interior-point-like dual λ = 1e-9 (s ≠ 0 as before), so that they are kept
    too: N' = n + ⌊φ·m⌋ + extra + p.  A sequence reaches a large reduced size
    this way because active rows alone cannot take it there: the rows with
    s = 0 and the equality rows form the block [G_a; A] of LHS with zeros on
    the diagonal below it, so more than n of them make LHS singular whatever Q
    is — the reference's `LHS \\ RHS` has no answer there and no parity bar
    can be held.  Kept inactive rows carry s_i ≠ 0 on the diagonal and do not
    count against n."""
    d = qp_numpy(B, n, m, p, phi, seed)
    for b in range(B):
        ina = np.flatnonzero(d["lam"][b] == 0)
        assert len(ina) >= extra
        d["lam"][b, ina[:extra]] = 1e-9
    return d


def _qp_step(name, d, n, m, p, n_active, kinds, iterative=None, sym=None, how="set"):
    B = d["z"].shape[0]
    act = [n_active] * B if np.isscalar(n_active) else list(n_active)
    kinds = [kinds] * B if np.isscalar(kinds) else list(kinds)
    iterative = [False] * B if iterative is None else list(iterative)
    sym = [int(k == NOPIV) for k in kinds] if sym is None else list(sym)
    # (the LSQR branch runs on the full LHS: nothing is eliminated)
    return dict(name=name, data=d, nsys=[n + (m if it else a) + p for a, it in zip(act, iterative)], lu_kind=kinds, iterative=iterative, sym=sym,
                how=how)


SIZES_SHAPE = (4, 150, 200, 10)


@functools.lru_cache(maxsize=None)
def qp_sizes():
    """a. batched route: the padded size grows, shrinks below the first, is
    mixed within one batch, reaches n + m + p, and returns to the first
    model (same seed: the same arrays)."""
    B, n, m, p = SIZES_SHAPE
    first = qp_numpy(B, n, m, p, 0.3, 8100)
    # 180 kept rows (N' = 340): 120 active (φ = 0.6; 120 + p ≤ n) and 60 kept inactive ones — see qp_kept
    mixed = stacked([qp_kept(1, n, m, p, phi, 8110 + i, extra) for i, (phi, extra) in
                     enumerate(((0.05, 0), (0.6, 60), (0.3, 0), (0.6, 0)))])
    return [
        _qp_step("phi 0.3", first, n, m, p, 60, NOPIV),
        _qp_step("180 rows kept (grown)", qp_kept(B, n, m, p, 0.6, 8101, 60), n, m, p, 180, NOPIV),
        _qp_step("phi 0.05 (shrunk)", qp_numpy(B, n, m, p, 0.05, 8102), n, m, p, 10, NOPIV),
        _qp_step("mixed sizes", mixed, n, m, p, [10, 180, 60, 120], NOPIV),
        _qp_step("lam_eps (nothing eliminated)", qp_numpy(B, n, m, p, 0.3, 8104, lam_eps=1e-9), n, m, p, 200, NOPIV),
        _qp_step("phi 0.3 again", first, n, m, p, 60, NOPIV),
    ]


KINDS_SHAPE = (6, 60, 80, 5)


@functools.lru_cache(maxsize=None)
def qp_kinds():
    """b. batched route at one size (N' = 129 > SM_MAX), the factorisation
    kind of single problems changing from model to model."""
    B, n, m, p = KINDS_SHAPE

    def gen(i):   # 64 kept rows: 40 active (40 + p ≤ n) and 24 kept inactive ones — see qp_kept
        return qp_kept(B, n, m, p, 0.5, 8200 + i, 24)

    lp = gen(3)
    lp["Q"][2] = 0.0
    asym = gen(5)
    asym["Q"][3] = asym["Q"][3] + 1e-3 * np.triu(np.random.default_rng(3).standard_normal((n, n)), 1)
    it2 = [b == 2 for b in range(B)]
    return [
        _qp_step("all accepted", gen(0), n, m, p, 64, NOPIV),
        _qp_step("1 and 4 rejected", indefinite(gen(1), [1, 4]), n, m, p, 64,
                 [NOPIV, PIVOT, NOPIV, NOPIV, PIVOT, NOPIV]),
        _qp_step("all accepted again", gen(2), n, m, p, 64, NOPIV),
        _qp_step("problem 2 on the LSQR branch", lp, n, m, p, 64, [NOPIV, NOPIV, LSQR, NOPIV, NOPIV, NOPIV],
                 iterative=it2, sym=[1, 1, 0, 1, 1, 1]),
        _qp_step("none iterative", gen(4), n, m, p, 64, NOPIV),
        # the assembly's symmetry check takes an asymmetric Q off the
        # P-symmetric route: re-assembled in full, partial pivoting
        _qp_step("problem 3 asymmetric", asym, n, m, p, 64, [NOPIV, NOPIV, NOPIV, PIVOT, NOPIV, NOPIV]),
        _qp_step("all symmetric", gen(6), n, m, p, 64, NOPIV),
        _qp_step("every problem rejected", indefinite(gen(7), range(B)), n, m, p, 64, PIVOT),
        _qp_step("all accepted at last", gen(8), n, m, p, 64, NOPIV),
    ]


TALL_SHAPE = (2, 1200, 700, 0)


@functools.lru_cache(maxsize=None)
def qp_tall():
    """c. reduced sizes on both sides of PIVOT_MAX: entry-chunked solves, a
    rejected tall problem (generic LU), a rejected one below the panel's limit
    (partial-pivoting panel), and back to a clean batch."""
    B, n, m, p = TALL_SHAPE
    return [
        _qp_step("phi 0.6 (N' 1620)", qp_numpy(B, n, m, p, 0.6, 8300), n, m, p, 420, NOPIV),
        _qp_step("phi 0.1 (N' 1270)", qp_numpy(B, n, m, p, 0.1, 8301), n, m, p, 70, NOPIV),
        _qp_step("phi 0.6, problem 1 rejected (generic LU)", indefinite(qp_numpy(B, n, m, p, 0.6, 8302), [1]),
                 n, m, p, 420, [NOPIV, PIVOT]),
        _qp_step("phi 0.1, problem 1 rejected (pivoting panel)", indefinite(qp_numpy(B, n, m, p, 0.1, 8303), [1]),
                 n, m, p, 70, [NOPIV, PIVOT]),
        _qp_step("phi 0.6 clean", qp_numpy(B, n, m, p, 0.6, 8304), n, m, p, 420, NOPIV),
    ]


SMALL_SHAPE = (50, 80, 30)


@functools.lru_cache(maxsize=None)
def qp_small_batched(B):
    """d. the one-workgroup small path (N' = 96 ≤ SM_MAX) and the batched
    route (N' = 152) by turns; the last three small steps are the handle's
    third and later small calls (pinned I/O)."""
    n, m, p = SMALL_SHAPE
    out = []
    for i, small in enumerate((True, True, False, False, True, True, True)):
        # 72 kept rows (N' = 152): the 16 active ones (16 + p ≤ n) and 56 kept inactive ones — see qp_kept
        d = qp_kept(B, n, m, p, 0.2, 8400 + i, 0 if small else 56)
        out.append(_qp_step(f"step {i} N' {96 if small else 152}", d, n, m, p, 16 if small else 72,
                            SMALL if small else NOPIV, sym=[0 if small else 1] * B))
    return out


STAGING_SHAPE = (3, 150, 120, 10)


@functools.lru_cache(maxsize=None)
def qp_staging():
    """e. the setter and the memory mode change from model to model; the CSC
    steps carry a 30 %-dense G (h moved so that s = Gz − h keeps its zeros
    and signs)."""
    B, n, m, p = STAGING_SHAPE
    out = []
    for i, how in enumerate(("set", "csc", "device", "set", "csc")):
        d = qp_numpy(B, n, m, p, 0.4, 8500 + i)
        if how == "csc":
            s = np.einsum("bmn,bn->bm", d["G"], d["z"]) - d["h"]
            d["G"] = d["G"] * (np.random.default_rng(8550 + i).random(d["G"].shape) < 0.3)
            d["h"] = np.einsum("bmn,bn->bm", d["G"], d["z"]) - np.where(d["lam"] == 0, s, 0.0)
        out.append(_qp_step(f"step {i} {how}", d, n, m, p, 48, NOPIV, how=how))
    return out


TOGGLE_SHAPE = (2, 40, 60, 10)


@functools.lru_cache(maxsize=None)
def qp_sparse_toggle():
    """f. (dense QP, sparse-route LP with scipy G / A, a QP the sparse route
    refuses) at one shape."""
    B, n, m, p = TOGGLE_SHAPE
    qp = _qp_step("dense QP", qp_numpy(B, n, m, p, 0.5, 8600), n, m, p, 30, NOPIV)
    lp = lp_sparse_numpy(B, n, p, m - (n - p), 3, 8601)
    assert lp["lam"].shape == (B, m)
    refused = qp_numpy(B, n, m, p, 0.5, 8602)
    return qp, lp, refused


def oracle_kept(d, b):
    """The reference's elimination set (λ == 0 and (Gz − h) != 0, Gz − h in
    Julia's sparse mul! order): the rows kept are the complement.  On the
    `iterative` branch (norm(Q) ≈ 0) LSQR runs on the full LHS: every row."""
    if oqp.is_iterative(d["Q"][b]):
        return np.ones(d["lam"].shape[1], dtype=bool)
    s = oqp.gz_minus_h(d["G"][b], d["z"][b], d["h"][b])
    return ~((d["lam"][b] == 0) & (s != 0))


_QP_REF = {}


def qp_oracle(step, b):
    """(reverse, forward) of problem b — [dz | dλ | dν] each — computed once
    per step; forward is None on the LSQR branch (held on reverse only, as
    test_small_path_fallbacks does)."""
    key = (id(step["data"]), b)
    if key not in _QP_REF:
        d = step["data"]
        args = [d[k][b] for k in QP_KEYS]
        rev = np.concatenate(oqp.reverse_differentiate(*args, d["dl_dz"][b]))
        fwd = None
        if not step["iterative"][b]:
            fwd = np.concatenate(oqp.forward_differentiate(*args, dq=d["dq"][b], dh=d["dh"][b], db=d["db"][b]))
        _QP_REF[key] = (rev, fwd, d)   # (d held: its id stays unique)
    return _QP_REF[key][:2]


# ---------------------------------------------------------------------------
# conic
# ---------------------------------------------------------------------------
M69 = [(0, 2), (1, 30), (2, 20), (3, 8), (4, 6), (4, 3)]   # test_conic_gpu.ALL5_SHAPES, m = 69
CONIC_B, CONIC_N = 4, 60


def _conic_step(name, cones, d, comparable):
    return dict(name=name, cones=list(cones), data=d, comparable=comparable)


def _wellcond(cones, seed, B=CONIC_B, n=CONIC_N):
    return conic_numpy_wellcond(B, n, cones, seed, pair_norm=1.0)


@functools.lru_cache(maxsize=None)
def conic_second_model():
    """g. three models under one cone table: the SOC pairs' cases (interior /
    dual-interior / boundary) and the PSD ranks differ from model to model;
    the middle one is the non-converging family (conic_numpy: a PSD rank of
    side // 2, boundary SOC pairs only)."""
    return [
        _conic_step("wellcond seed 42", M69, _wellcond(M69, 42), True),
        _conic_step("conic_numpy seed 43", M69, conic_numpy(CONIC_B, CONIC_N, M69, 43), False),
        _conic_step("wellcond seed 45", M69, _wellcond(M69, 45), True),
    ]


TABLES = [M69,
          [(4, 55), (3, 8), (1, 6)],                                   # one side-10 PSD block: a longer packed Dπ
          [(0, 2), (1, 20), (2, 30), (3, 5), (3, 3), (4, 6), (4, 3)],
          M69]


@functools.lru_cache(maxsize=None)
def conic_tables():
    """h. the cone table changes under a fixed (n, m) = (60, 69); the last
    model is the first again."""
    first = _conic_step("M69", M69, _wellcond(M69, 42), True)
    return [first,
            _conic_step("PSD(55) + SOC(8) + Nonneg(6)", TABLES[1], _wellcond(TABLES[1], 54), True),
            _conic_step("two SOCs, two PSDs", TABLES[2], _wellcond(TABLES[2], 47), True),
            _conic_step("M69 again", M69, first["data"], True)]


BIG_PSD_TABLES = [[(4, 2211), (4, 15), (1, 5)],            # side 66 > 64: global scratch
                  [(3, 50)] * 44 + [(1, 31)],               # no PSD cone at all
                  [(4, 2211), (4, 15), (1, 5)]]
BIG_PSD_N, BIG_PSD_M = 60, 2231


@functools.lru_cache(maxsize=None)
def conic_big_psd():
    """i. the large-PSD global scratch is needed, not needed, needed again
    (fresh-handle comparison only)."""
    first = _conic_step("side 66", BIG_PSD_TABLES[0], conic_numpy(1, BIG_PSD_N, BIG_PSD_TABLES[0], 8700), False)
    return [first,
            _conic_step("44 SOCs", BIG_PSD_TABLES[1], conic_numpy(1, BIG_PSD_N, BIG_PSD_TABLES[1], 8701), False),
            _conic_step("side 66 again", BIG_PSD_TABLES[0], first["data"], False)]


_CONIC_REF = {}


def conic_oracle(step, b):
    """The oracle's outputs of problem b (test_conic_gpu._oracle_outputs'
    layout, plus the cache), computed once per step."""
    key = (id(step["data"]), b)
    if key not in _CONIC_REF:
        d = step["data"]
        cache = ocn.Cache(d["A"][b], d["b"][b], d["c"][b], d["x"][b], d["s"][b], d["y"][b], step["cones"])
        (odx, du, dv, dw), fi = ocn.forward_differentiate(cache, d["dA"][b], d["db"][b], d["dc"][b],
                                                          return_info=True)
        (og, _), ri = ocn.reverse_differentiate(cache, d["dx"][b], return_info=True)
        odA, odb, odc = ocn.reverse_outputs(cache, og)
        _CONIC_REF[key] = dict(fwd=np.concatenate([du, dv, [dw]]), dx=odx, g=og, dA=odA, db=odb, dc=odc,
                               info=(fi, ri), cache=cache, data=d)   # (d held: its id stays unique)
    return _CONIC_REF[key]


# ---------------------------------------------------------------------------
# NLP
# ---------------------------------------------------------------------------
NLP_SHAPE = (4, 20, 12, 4)
NLP_KEYS = ("Hxx", "Hxp", "Jx", "Jp", "x", "cval", "crhs", "y", "xl", "xu", "yl", "yu")


def _nlp_points(seed, count, **kw):
    """`count` batches of one structure: nlp_numpy draws the structure first,
    then problem after problem, so one draw of count·B problems is cut up."""
    B, n, c, P = NLP_SHAPE
    st, pt, dp, dx, dd = nlp_numpy(count * B, n, c, P, seed, **kw)
    cut = lambda a, i: a[i * B:(i + 1) * B].copy()
    return st, [dict(pt={k: cut(v, i) for k, v in pt.items()}, dp=cut(dp, i), dx=cut(dx, i), dd=cut(dd, i))
                for i in range(count)]


def _nlp_step(name, st, d, restructure, corrected=(), asym=()):
    B, n, c, P = NLP_SHAPE
    L = onlp.Layout(st["con_kind"], st["has_low"], st["has_up"])
    return dict(name=name, st=st, data=d, restructure=restructure, corrected=list(corrected), asym=list(asym),
                nsys=[L.rows if b in corrected else n + c for b in range(B)], saddle=L.rows == n + c)


@functools.lru_cache(maxsize=None)
def nlp_structures():
    """k. one NLP handle: a generic structure (bounds, all three row kinds);
    equalities only without bounds (num_w and the rows shrink to n + c, the
    saddle-only route); all inequalities (num_w grows); the first structure
    with problem 1 singular (two identical equality rows: inertia-corrected,
    on the full M); the same structure with a regular point (no shift or
    correction may survive, every problem reduced again); problem 2 with an
    asymmetric Hxx (the speculative launch misses and is switched off); the
    first structure set again with the first point (the launch is tried
    again), whose outputs equal the first step's bit for bit."""
    # (seed 8806: the oracle's SuperLU cancels the dependent pivot to exactly
    # zero and corrects, as the reference's UMFPACK does — on other draws it is
    # left at rounding level, test_nlp_gpu.test_saddle_only_dependent_equality;
    # test_reuse_cases_cpu.py holds the step to it)
    first, (a, sing, regular, asym) = _nlp_points(8806, 4)
    eq, (e0,) = _nlp_points(8801, 1, frac_geq=0, frac_leq=0, frac_low=0, frac_up=0)
    ineq, (i0,) = _nlp_points(8802, 1, frac_geq=0.5, frac_leq=0.5)
    i, j = np.flatnonzero(first["con_kind"] == 0)[:2]
    sing["pt"]["Jx"][1, j] = sing["pt"]["Jx"][1, i]
    sing["pt"]["Jp"][1, j] = sing["pt"]["Jp"][1, i]
    n = NLP_SHAPE[1]
    asym["pt"]["Hxx"][2] = asym["pt"]["Hxx"][2] + 0.05 * np.triu(np.random.default_rng(3).standard_normal((n, n)), 1)
    return [
        _nlp_step("generic structure", first, a, True),
        _nlp_step("equalities only, no bounds", eq, e0, True),
        _nlp_step("all inequalities", ineq, i0, True),
        _nlp_step("first structure, problem 1 singular", first, sing, True, corrected=[1]),
        _nlp_step("regular point", first, regular, False),
        _nlp_step("problem 2 asymmetric", first, asym, False, asym=[2]),
        _nlp_step("first structure and point again", first, a, True),
    ]


_NLP_REF = {}


def nlp_oracle(step, b):
    """(∂s, Layout, corrections) of problem b, computed once per step."""
    key = (id(step["data"]), b)
    if key not in _NLP_REF:
        st, pt = step["st"], step["data"]["pt"]
        ds, L, _, _, corr = onlp.compute_sensitivity(st["con_kind"], st["has_low"], st["has_up"], st["sense"],
                                                     *[pt[k][b] for k in NLP_KEYS], return_info=True)
        _NLP_REF[key] = (ds, L, corr, step["data"])   # (data held: its id stays unique)
    return _NLP_REF[key][:3]

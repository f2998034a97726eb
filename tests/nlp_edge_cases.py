"""NLP points for the reduced KKT route of csrc/nlp.hip at every elimination
state and at the LU's block edges.  test_nlp_edge_cases_cpu.py pins on the CPU
what each case is (the census below, the oracle's verdict, the conditioning of
M), test_nlp_edges_gpu.py runs them through nlp_red_prep_kernel,
nlp_red_rhs_kernel<1|2>, nlp_red_recover_kernel<1|2>, the left-looking LU's
reads of R (nlp_R_codes / nlp_R_ref_lower), the assembled R (nlp_R) and the
speculative launch.

``synthetic.nlp_numpy`` only draws strictly complementary points with an
exactly symmetric Hxx: an inactive row or bound has dual 0, an active one
slack 0.  Every case here is such a draw (fixed seed) plus explicit edits that
put the point into a state the generator never reaches:

* ``rho_rows``            every inactive GreaterThan / LessThan row gets a dual
                          of its set's sign (±U(0.5, 1.5)): slack ≠ 0 and dual
                          ≠ 0, the regularised row ``yst == 2``, ρ = 1/δ_t —
                          what an interior-point solution has on every
                          inactive row;
* ``delta_primal``        every inactive primal bound gets a dual (yl > 0,
                          yu < 0): δ = V/d is O(1) beside H; variables 0, 1, 2
                          carry both bounds, both inactive, both duals
                          non-zero (two contributions to one δ);
* ``rho_delta_asym_all``  both, and Hxx += 0.05·triu(N(0,1), 1) in every
                          problem (``meta.sym == 0`` on the reduced route);
* ``asym_one``            the asymmetry in problem 1 only: the batch leaves the
                          left-looking route, the speculative launch misses
                          (``pt_sym`` is the same batch before the edit);
  (each of these for MIN and MAX: ``rho_rows_min``, ``rho_rows_max``, …)
* ``x_all_fixed_c0``      (70, 0, 1): every variable on an active lower bound,
                          R = I, 70 known x (two ballots of wave_compact), no
                          constraint at all (the ``d.c ? … : kx`` alias of
                          nlp_code, the null Jx);
* ``y_all_known``         (20, 70, 1): every row an inactive inequality with
                          dual 0 — 70 known y;
* ``slacks_all_fixed``    (80, 30, 1): every row an active inequality, no
                          variable bounds;
* ``edge_31`` … ``edge_65``  n + c on both sides of the LU's 32-row blocks,
                          P = 1, with a fixed unknown (an identity row and
                          column of R) at each of the R-indices 31, 32, 63, 64
                          that exists: an index below n is a primal variable
                          given an active lower bound (x₃₁, x₃₂ of the n = 40
                          shapes), one past it a constraint row made an
                          inactive GreaterThan row with dual 0 (y known);
* ``lds_optin``           (1400, 8, 2), batch 2, equalities and lower bounds
                          only: 2·num_w + c + n > 4096, so the pair kernels
                          need more than 64 KB of dynamic LDS and the single-
                          vector ones do not (``red_lds_bytes``);
* ``corrected``           (20, 12, 4): test_structured_dependent_constraint's
                          duplicated equality row in problem 1 of 3 — M exactly
                          singular, inertia-corrected, on the full M.

``census`` restates nlp_red_prep_kernel's classification, ``reduced_solve``
the whole elimination (the specification of the kernels; it moved here from
test_nlp_reduce_cpu.py, which imports it).  A case's ``expect`` is counted
from the edits themselves, not through ``census``.

Everything is built once per process (lru_cache); tests never modify it."""

import functools

import numpy as np

from diffopt_amd.synthetic import nlp_numpy
from oracle import nlp

KEYS = ("Hxx", "Hxp", "Jx", "Jp", "x", "cval", "crhs", "y", "xl", "xu", "yl", "yu")
SHAPE = (21, 13, 3)          # the state cases' (n, c, P)
EDGE_SHAPES = {31: (19, 12), 32: (20, 12), 33: (21, 12), 63: (40, 23), 64: (40, 24), 65: (40, 25)}
EDGE_INDICES = (31, 32, 63, 64)
LDS_SHAPE = (1400, 8, 2)
PIVOT_MAX = 1536             # dopt_internal.h
LDS_DEFAULT = 64 * 1024      # dynamic LDS a kernel gets without the opt-in
STATE_FAMILIES = ("rho_rows", "delta_primal", "rho_delta_asym_all", "asym_one")
DEGENERATE = ("x_all_fixed_c0", "y_all_known", "slacks_all_fixed")


# ---------------------------------------------------------------------------
# the specification: the elimination in numpy
# ---------------------------------------------------------------------------
def layout(st):
    return nlp.Layout(st["con_kind"], st["has_low"], st["has_up"])


def problem(pt, b):
    return {k: pt[k][b] for k in KEYS}


def matrices(st, pt, b):
    """(L, M, N, bounds) of problem b: the reference's full system."""
    L = layout(st)
    p = problem(pt, b)
    X, V_L, X_L, V_U, X_U = nlp.solution_and_bounds(L, st["sense"], p["x"], p["cval"], p["crhs"], p["y"], p["xl"],
                                                    p["xu"], p["yl"], p["yu"])
    M, N = nlp.build_sensitivity_matrices(L, p["Hxx"], p["Hxp"], p["Jx"], p["Jp"], X, V_L, X_L, V_U, X_U)
    return L, M, N, bounds(L, X, V_L, X_L, V_U, X_U)


def bounds(L, X, V_L, X_L, V_U, X_U):
    w, c = L.num_w, L.c
    lo0, up0 = w + c, w + c + L.nlo
    out = []   # (row of M, w index j, V, coefficient of ν in row j, d)
    for i, j in enumerate(L.has_low):
        out.append((lo0 + i, j, V_L[j], -1.0, X[j] - X_L[j]))
    for i, j in enumerate(L.has_up):
        out.append((up0 + i, j, V_U[j], 1.0, X_U[j] - X[j]))
    return out


def census(L, bnd):
    """nlp_red_prep_kernel's classification of one problem from its bound
    rows: δ_j += V/d (lower) / −= V/d (upper) for d ≠ 0; d = 0 fixes w_j (V = 0
    or a second active bound: the problem keeps the full M); an inequality
    row whose slack is not fixed has y known (δ_t = 0) or is regularised."""
    n, c, w = L.n, L.c, L.num_w
    delta = np.zeros(w)
    terms = np.zeros(w, dtype=int)
    kx = -np.ones(w, dtype=int)
    ok = True
    for q, (row, j, V, cf, d) in enumerate(bnd):
        if not (np.isfinite(d) and np.isfinite(V)):
            ok = False
        elif d != 0.0:
            delta[j] += -V * cf / d
            terms[j] += V != 0.0
        elif V == 0.0 or kx[j] >= 0:
            ok = False
        else:
            kx[j] = q
    yst = np.zeros(c, dtype=int)
    for t, k in enumerate(list(L.geq) + list(L.leq)):
        if kx[n + t] < 0:
            yst[k] = 1 if delta[n + t] == 0.0 else 2
    return dict(reduced=ok, known_x=int((kx[:n] >= 0).sum()), known_y=int((yst == 1).sum()),
                rho_rows=int((yst == 2).sum()), delta_x=int((delta[:n] != 0.0).sum()),
                delta_two=int((terms[:n] == 2).sum()), yst=yst, kx=kx, delta=delta)


def reduced_solve(L, Hxx, Jx, bounds, r, trans):
    """z = M⁻¹ r (trans False) or M⁻ᵀ r (trans True) through R.  Returns None
    when the problem takes the full route."""
    n, c, w = L.n, L.c, L.num_w
    H = Hxx.T if trans else Hxx
    rr = np.array(r, dtype=float)
    delta = np.zeros(w)
    known = {}
    act = {}
    for row, j, V, cf, d in bounds:
        a, b = (cf, V) if trans else (V, cf)
        if d != 0.0:
            delta[j] += -a * b / d
            rr[j] -= b * r[row] / d
    for row, j, V, cf, d in bounds:
        a, b = (cf, V) if trans else (V, cf)
        if d == 0.0:
            if a == 0.0 or j in known:
                return None
            known[j] = r[row] / a
            act[j] = (row, b)
    slack_of = {}
    for t, k in enumerate(list(L.geq) + list(L.leq)):
        slack_of[k] = n + t
    # constraint-row states: 0 kept (equality or active slack), 1 y known,
    # 2 regularized; rhs of the reduced rows
    N = n + c
    Rm = np.zeros((N, N))
    rhs = np.zeros(N)
    xknown = {j: v for j, v in known.items() if j < n}
    ystate = np.zeros(c, dtype=int)
    yval = np.zeros(c)
    rho = np.zeros(c)
    for k in range(c):
        rhs[n + k] = r[w + k]
        if k in slack_of:
            t = slack_of[k]
            if t in known:
                rhs[n + k] += known[t]
            elif delta[t] == 0.0:
                ystate[k], yval[k] = 1, -rr[t]
            else:
                ystate[k], rho[k] = 2, 1.0 / delta[t]
                rhs[n + k] += rr[t] / delta[t]
    for j in range(n):
        rhs[j] = rr[j]
    # reduced matrix, identity rows / columns for the known unknowns
    for j in range(n):
        for jj in range(n):
            Rm[j, jj] = H[j, jj] + (delta[j] if j == jj else 0.0)
        for k in range(c):
            Rm[j, n + k] = Jx[k, j]
            Rm[n + k, j] = Jx[k, j]
    for k in range(c):
        Rm[n + k, n + k] = -rho[k] if ystate[k] == 2 else 0.0
    for j, v in xknown.items():
        rhs[:n] -= Rm[:n, j] * v
        rhs[n:] -= Rm[n:, j] * v
    for k in range(c):
        if ystate[k] == 1:
            rhs[:n] -= Rm[:n, n + k] * yval[k]
    for j, v in xknown.items():
        Rm[j, :] = 0.0
        Rm[:, j] = 0.0
        Rm[j, j] = 1.0
        rhs[j] = v
    for k in range(c):
        if ystate[k] == 1:
            Rm[n + k, :] = 0.0
            Rm[:, n + k] = 0.0
            Rm[n + k, n + k] = 1.0
            rhs[n + k] = yval[k]
    sol = np.linalg.solve(Rm, rhs)
    x, y = sol[:n], sol[n:]
    z = np.zeros(len(r))
    z[:n] = x
    z[w:w + c] = y
    for k in range(c):
        if k in slack_of:
            t = slack_of[k]
            if t in known:
                z[t] = known[t]
            elif ystate[k] == 1:
                z[t] = Jx[k] @ x - r[w + k]
            else:
                z[t] = (rr[t] + y[k]) / delta[t]
    for row, j, V, cf, d in bounds:
        a, b = (cf, V) if trans else (V, cf)
        if d != 0.0:
            z[row] = (r[row] - a * z[j]) / d
    for j, (row, b) in act.items():
        if j < n:   # row j of the system: (H x)_j + δ_j x_j + (Jᵀ y)_j + b ν = r̃_j
            z[row] = (rr[j] - H[j] @ x - delta[j] * x[j] - Jx[:, j] @ y) / b
        else:       # slack row: −y_k + b ν = r̃_t
            k = [kk for kk, t in slack_of.items() if t == j][0]
            z[row] = (rr[j] + y[k]) / b
    return z


def red_lds_bytes(n, c, num_w):
    """Dynamic LDS the host asks for (nlp.hip: red_rhs, red_recover), per
    kernel and number of vectors: {(kernel, NV): bytes}."""
    out = {}
    for nv in (1, 2):
        out["rhs", nv] = nv * (2 * num_w + c + n) * 8 + (num_w + c + n + c + 2) * 4
        out["recover", nv] = nv * (3 * num_w + c) * 8 + (num_w + c + n + 1) * 4
    return out


# ---------------------------------------------------------------------------
# the edits
# ---------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng([20261021, *[int(k) for k in key]])


def _u(rng, size=None):
    return rng.uniform(0.5, 1.5, size)


def _inactive_rows(st, pt, b):
    k = st["con_kind"]
    return np.flatnonzero((k != 0) & (pt["cval"][b] != pt["crhs"][b]))


def force_rho(st, pt, rng):
    """Every inactive inequality row gets a dual of its set's sign.  Returns
    the number of such rows per problem."""
    out = []
    for b in range(pt["y"].shape[0]):
        rows = _inactive_rows(st, pt, b)
        for k in rows:
            pt["y"][b, k] = _u(rng) if st["con_kind"][k] == 1 else -_u(rng)
        out.append(len(rows))
    return out


def force_delta(st, pt, rng, both=(0, 1, 2)):
    """Variables `both` get both bounds (a structure edit), inactive; then every
    inactive primal bound gets a dual.  Returns (variables with δ ≠ 0,
    variables with two contributions) per problem."""
    B, n = pt["x"].shape
    for j in both:
        st["has_low"][j] = st["has_up"][j] = 1
        pt["xl"][:, j] = pt["x"][:, j] - _u(rng, B)
        pt["xu"][:, j] = pt["x"][:, j] + _u(rng, B)
        pt["yl"][:, j] = pt["yu"][:, j] = 0.0
    nd, two = [], []
    for b in range(B):
        lo = st["has_low"].astype(bool) & (pt["xl"][b] != pt["x"][b])
        up = st["has_up"].astype(bool) & (pt["xu"][b] != pt["x"][b])
        pt["yl"][b, lo] = _u(rng, int(lo.sum()))
        pt["yu"][b, up] = -_u(rng, int(up.sum()))
        nd.append(int((lo | up).sum()))
        two.append(int((lo & up).sum()))
    return nd, two


def force_asym(pt, problems, rng):
    n = pt["Hxx"].shape[1]
    for b in problems:
        pt["Hxx"][b] = pt["Hxx"][b] + 0.05 * np.triu(rng.standard_normal((n, n)), 1)


def _seeds(st, pt, P, rng):
    B, n = pt["x"].shape
    nd = len(st["con_kind"]) + int(st["has_low"].sum()) + int(st["has_up"].sum())
    return rng.standard_normal((B, P)), rng.standard_normal((B, n)), rng.standard_normal((B, nd))


def _counts(st, pt, b):
    """(primal variables on an active bound, inactive inequality rows with
    dual 0) read off the point itself."""
    kx = int(((st["has_low"] != 0) & (pt["xl"][b] == pt["x"][b])).sum() +
             ((st["has_up"] != 0) & (pt["xu"][b] == pt["x"][b])).sum())
    rows = _inactive_rows(st, pt, b)
    return kx, int((pt["y"][b, rows] == 0.0).sum())


def _case(name, st, pt, P, rng, expect, problems=None, reduced=None, **extra):
    B = pt["x"].shape[0]
    dp, dx, dd = _seeds(st, pt, P, rng)
    for a in list(pt.values()) + [dp, dx, dd, st["con_kind"], st["has_low"], st["has_up"]]:
        a.setflags(write=False)
    n, c = pt["x"].shape[1], len(st["con_kind"])
    return dict(name=name, st=st, pt=pt, dp=dp, dx=dx, dd=dd, B=B, n=n, c=c, P=P, expect=expect,
                problems=list(range(B)) if problems is None else list(problems),
                reduced=[True] * B if reduced is None else list(reduced), **extra)


# seeds: chosen once so that every checked problem has 0 corrections on the
# oracle and cond(M) ≤ 1e5 (test_nlp_edge_cases_cpu.py holds them to it)
STATE_SEED = {"rho_rows": 11, "delta_primal": 12, "rho_delta_asym_all": 13, "asym_one": 14}


def _state_case(family, sense):
    n, c, P = SHAPE
    B = 3
    seed = STATE_SEED[family] + (0 if sense == 1 else 100)
    st, pt, *_ = nlp_numpy(B, n, c, P, seed, sense=sense)
    rng = _rng(seed)
    expect = dict(rho_rows=[0] * B, delta_x=[0] * B, delta_two=[0] * B)
    extra = {}
    if family in ("rho_rows", "rho_delta_asym_all"):
        expect["rho_rows"] = force_rho(st, pt, rng)
    if family in ("delta_primal", "rho_delta_asym_all"):
        expect["delta_x"], expect["delta_two"] = force_delta(st, pt, rng)
    kx0 = [_counts(st, pt, b) for b in range(B)]
    expect.update(known_x=[k for k, _ in kx0], known_y=[y for _, y in kx0])
    if family == "rho_delta_asym_all":
        force_asym(pt, range(B), rng)
    if family == "asym_one":
        extra["pt_sym"] = {k: v.copy() for k, v in pt.items()}
        force_asym(pt, [1], rng)
        for a in extra["pt_sym"].values():
            a.setflags(write=False)
    return _case(f"{family}_{'min' if sense == 1 else 'max'}", st, pt, P, rng, expect, sense=sense, family=family,
                 **extra)


def _degenerate_case(name):
    B = 2
    rng = _rng(len(name))
    if name == "x_all_fixed_c0":
        n, c, P = 70, 0, 1
        st, pt, *_ = nlp_numpy(B, n, c, P, 21, frac_low=1.0, frac_up=0.0, active=1.0)
        expect = dict(known_x=[70] * B, known_y=[0] * B)
    elif name == "y_all_known":
        n, c, P = 20, 70, 1
        st, pt, *_ = nlp_numpy(B, n, c, P, 22, frac_geq=0.6, frac_leq=0.4, active=0.0)
        expect = dict(known_x=[0] * B, known_y=[70] * B)
    else:
        n, c, P = 80, 30, 1
        st, pt, *_ = nlp_numpy(B, n, c, P, 23, frac_geq=0.5, frac_leq=0.5, frac_low=0.0, frac_up=0.0, active=1.0)
        expect = dict(known_x=[0] * B, known_y=[0] * B)
    expect.update(rho_rows=[0] * B, delta_x=[0] * B, delta_two=[0] * B)
    return _case(name, st, pt, P, rng, expect, family=name)


def _edge_case(N):
    n, c = EDGE_SHAPES[N]
    B, P = 2, 1
    st, pt, *_ = nlp_numpy(B, n, c, P, 300 + N)
    rng = _rng(300 + N)
    fixed = [i for i in EDGE_INDICES if i < N]
    for i in fixed:
        if i < n:     # x_i on an active lower bound
            st["has_low"][i] = 1
            pt["xl"][:, i] = pt["x"][:, i]
            pt["yl"][:, i] = _u(rng, B)
            if st["has_up"][i]:   # (the upper bound, where the draw gave one, inactive with dual 0)
                pt["xu"][:, i] = pt["x"][:, i] + _u(rng, B)
                pt["yu"][:, i] = 0.0
        else:         # row i − n an inactive GreaterThan row with dual 0: y known
            k = i - n
            st["con_kind"][k] = 1
            pt["crhs"][:, k] = pt["cval"][:, k] - _u(rng, B)
            pt["y"][:, k] = 0.0
    # a re-typed row can hold what the draw gave an equality: every other
    # inequality row keeps the generator's strict complementarity
    kx0 = [_counts(st, pt, b) for b in range(B)]
    expect = dict(known_x=[k for k, _ in kx0], known_y=[y for _, y in kx0], rho_rows=[0] * B, delta_x=[0] * B,
                  delta_two=[0] * B)
    return _case(f"edge_{N}", st, pt, P, rng, expect, family="edge", fixed=fixed)


def _lds_case():
    n, c, P = LDS_SHAPE
    B = 2
    st, pt, *_ = nlp_numpy(B, n, c, P, 41, frac_geq=0.0, frac_leq=0.0, frac_low=0.08, frac_up=0.0, active=0.5)
    kx0 = [_counts(st, pt, b) for b in range(B)]
    expect = dict(known_x=[k for k, _ in kx0], known_y=[0] * B, rho_rows=[0] * B, delta_x=[0] * B, delta_two=[0] * B)
    return _case("lds_optin", st, pt, P, _rng(41), expect, problems=[0], family="lds_optin")


def _corrected_case():
    n, c, P = 20, 12, 4
    st, pt, *_ = nlp_numpy(3, n, c, P, 77)
    i, j = np.flatnonzero(st["con_kind"] == 0)[:2]
    pt["Jx"][1, j] = pt["Jx"][1, i]
    pt["Jp"][1, j] = pt["Jp"][1, i]
    kx0 = [_counts(st, pt, b) for b in range(3)]
    expect = dict(known_x=[k for k, _ in kx0], known_y=[y for _, y in kx0], rho_rows=[0] * 3, delta_x=[0] * 3,
                  delta_two=[0] * 3)
    # (the elimination applies to problem 1 too: it is the singular R that
    # sends it to the inertia correction, on the full M)
    return _case("corrected", st, pt, P, _rng(77), expect, family="corrected", corrected=[1])


NAMES = tuple([f"{f}_{s}" for f in STATE_FAMILIES for s in ("min", "max")] + list(DEGENERATE) +
              [f"edge_{N}" for N in EDGE_SHAPES] + ["lds_optin", "corrected"])


@functools.lru_cache(maxsize=None)
def case(name):
    if name in DEGENERATE:
        return _degenerate_case(name)
    if name.startswith("edge_"):
        return _edge_case(int(name[5:]))
    if name == "lds_optin":
        return _lds_case()
    if name == "corrected":
        return _corrected_case()
    family, sense = name.rsplit("_", 1)
    return _state_case(family, 1 if sense == "min" else -1)


# ---------------------------------------------------------------------------
# the reference, once per (case, problem)
# ---------------------------------------------------------------------------
_ORACLE = {}


def oracle(cs, b, pt=None):
    """(∂s, Layout, M, N, corrections) of problem b of the case (of `pt`, a
    named alternative point of the case, e.g. "pt_sym")."""
    key = (cs["name"], b, pt)
    if key not in _ORACLE:
        st, p = cs["st"], cs[pt or "pt"]
        _ORACLE[key] = nlp.compute_sensitivity(st["con_kind"], st["has_low"], st["has_up"], st["sense"],
                                               *[p[k][b] for k in KEYS], return_info=True)
    return _ORACLE[key]


def corrected_matrix(cs, b):
    """The matrix the reference factorised: M, or M + k·1e-6·D after k
    corrections (NonLinearProgram.jl:356-381)."""
    _, L, M, _, corr = oracle(cs, b)
    d = np.ones(M.shape[0])
    d[L.num_w:L.num_w + L.c] = -1.0
    return M + corr * 1e-6 * np.diag(d)


def lapack_jacobian(cs, b):
    """∂s from a LAPACK solve of the same (corrected) matrix."""
    _, L, M, N, _ = oracle(cs, b)
    ds = -np.linalg.solve(corrected_matrix(cs, b), N)
    w, c, s = L.num_w, L.c, cs["st"]["sense"]
    ds[w:w + c] *= -s
    ds[w + c:w + c + L.nlo] *= s
    ds[w + c + L.nlo:] *= -s
    return ds


def reference_discrepancy(cs, b):
    """Relative Frobenius distance of the oracle's ∂s (SuperLU) from LAPACK's:
    the reference's own error on this matrix."""
    ds = oracle(cs, b)[0]
    ref = lapack_jacobian(cs, b)
    return float(np.linalg.norm(ds - ref) / np.linalg.norm(ref))

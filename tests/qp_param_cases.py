"""Parametric QP cases for the `_k` parameter calls (dopt_qp_params_forward_k /
dopt_qp_params_reverse_k): a numpy restatement of the reference's POI glue
extended by the constraints' parameter×variable terms, the golden fixtures,
and a synthetic case builder.  Test infrastructure only.

A term is (param, kind, index, coef) for kinds 0-3 (oracle/poi.py) or
(param, kind, row, coef, var) for
  kind 4  parameter×variable term c·p·x_var of LessThan row `row`
  kind 5  the same of EqualTo row `row`
(ParametricQuadraticFunction constraints: reference src/parameters.jl:147-203
forward, :390-441 reverse).
"""

import json
import math
import os

import numpy as np

from oracle import qp as oqp

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(3, 20, 30, 4), (2, 12, 0, 5), (2, 9, 7, 0), (2, 200, 300, 0)]   # (B, n, m, p)
NPARAMS = [1, 16, 17, 33]


def fixtures():
    with open(os.path.join(HERE, "golden", "qp_param_fixtures.json")) as f:
        return json.load(f)


def fixture_arrays(fx):
    """The fixture's problem as (Q, G, h, A, z, lam, nu) numpy arrays of one problem."""
    n, m, p = fx["n"], fx["m"], fx["p"]
    f = lambda k, shape: np.array(fx[k], dtype=float).reshape(shape)
    return (f("Q", (n, n)), f("G", (m, n)), f("h", (m,)), f("A", (p, n)), f("z", (n,)), f("lam", (m,)),
            f("nu", (p,)))


def isapprox(a, b, rtol, atol):
    """Julia's isapprox(a, b; rtol, atol) on scalars."""
    return abs(a - b) <= max(atol, rtol * max(abs(a), abs(b)))


def term5(t):
    """(param, kind, index, coef, var) with var = 0 where the term has none."""
    return (int(t[0]), int(t[1]), int(t[2]), float(t[3]), int(t[4]) if len(t) > 4 else 0)


def poi_forward_full(terms, dp, n, m, p):
    """parameter_input_forward → ForwardConstraintFunction / ForwardObjectiveFunction
    (parameters.jl:91-300, the ParametricQuadraticFunction constraints
    :147-203): cte(row) += dp·coef, the coefficient of v in row i += dp·coef
    for a parameter×variable term, the objective's coefficient of v likewise.
    Returned as the dense QP forward tangents of one problem under the `_fill`
    rules (diff_opt.jl:616-622): dq, dh = −cte (LessThan), db = −cte (EqualTo),
    dG (m×n), dA (p×n)."""
    cte_le, cte_eq, dq = np.zeros(m), np.zeros(p), np.zeros(n)
    dG, dA = np.zeros((m, n)), np.zeros((p, n))
    for t in terms:
        par, kind, idx, coef, var = term5(t)
        if kind == 0:
            cte_le[idx] += dp[par] * coef
        elif kind == 1:
            cte_eq[idx] += dp[par] * coef
        elif kind == 3:
            dq[idx] += dp[par] * coef
        elif kind == 4:
            dG[idx, var] += dp[par] * coef
        elif kind == 5:
            dA[idx, var] += dp[par] * coef
        elif kind != 2:
            raise ValueError(kind)
    return dq, -cte_le, -cte_eq, dG, dA


def poi_reverse_full(terms, nparam, z, lam, nu, rev):
    """parameter_output_backward (parameters.jl:341-534; the
    ParametricQuadraticFunction constraints :390-441): value(p) += coef · s
    with s the getter the reference reads off `rev` = [dz | dλ | dν] of one
    problem — the constant of ReverseConstraintFunction(ci) (kinds 0, 1), the
    objective's constant 0.0 (kind 2) and coefficient of v (kind 3), and for a
    parameter×variable constraint term JuMP.coefficient(
    ReverseConstraintFunction(ci), v): λ_i dλ_i z_v + λ_i dz_v (LessThan),
    dν_i z_v + ν_i dz_v (EqualTo) (QuadraticProgram.jl:461-473)."""
    n, m = z.shape[0], lam.shape[0]
    dz, dl, dn = rev[:n], rev[n:n + m], rev[n + m:]
    out = np.zeros(nparam)
    for t in terms:
        par, kind, i, coef, v = term5(t)
        if kind == 0:
            s = lam[i] * dl[i]
        elif kind == 1:
            s = dn[i]
        elif kind == 2:
            s = 0.0
        elif kind == 3:
            s = dz[i]
        elif kind == 4:
            s = lam[i] * dl[i] * z[v] + lam[i] * dz[v]
        elif kind == 5:
            s = dn[i] * z[v] + nu[i] * dz[v]
        else:
            raise ValueError(kind)
        out[par] += coef * s
    return out


def kept_rows(d, b):
    """Mask of problem b's LessThan rows the reference keeps (False: λ_i = 0 and s_i ≠ 0, eliminated)."""
    s = oqp.gz_minus_h(d["G"][b], d["z"][b], d["h"][b])
    return ~((d["lam"][b] == 0.0) & (s != 0.0))


def synthetic_case(B, n, m, p, nparam, seed, phi=0.4):
    """diffopt_amd.synthetic.qp_numpy plus a random term table of every kind the
    shape allows (kinds 0 / 4 need m > 0, 1 / 5 need p > 0).  With nparam ≥ 3
    the last parameter has no terms and the one before it kind-2 terms only;
    the others ("active") carry the rest.  For every problem of the batch one
    eliminated and one kept LessThan row get a kind-0 and a kind-4 term each
    (the term table is shared by the batch, so that is up to 2·B rows), and
    two terms repeat one (parameter, row, variable).  Returns dict(d, terms,
    nparam, active, structured) — `structured` lists (problem, eliminated row,
    kept row)."""
    from diffopt_amd.synthetic import qp_numpy
    d = qp_numpy(B, n, m, p, phi, seed)
    rng = np.random.default_rng(seed + 977)
    na = nparam - 2 if nparam >= 3 else nparam
    kinds = [2, 3] + ([0, 4] if m else []) + ([1, 5] if p else [])
    terms = []

    def add(par, kind):
        c = float(np.round(rng.uniform(-2.0, 2.0), 3)) or 0.5
        if kind in (0, 4):
            row = int(rng.integers(m))
        elif kind in (1, 5):
            row = int(rng.integers(p))
        elif kind == 3:
            row = int(rng.integers(n))
        else:
            row = 0
        terms.append((par, kind, row, c, int(rng.integers(n))) if kind in (4, 5) else (par, kind, row, c))

    for par in range(na):
        for _ in range(int(rng.integers(3, 7))):
            add(par, int(rng.choice(kinds)))
    structured = []
    for b in range(B if m else 0):
        keep = kept_rows(d, b)
        ie, ik = int(np.flatnonzero(~keep)[0]), int(np.flatnonzero(keep)[0])
        structured.append((b, ie, ik))
        for row in (ie, ik):
            par = int(rng.integers(na))
            terms.append((par, 0, row, float(np.round(rng.uniform(0.5, 2.0), 3))))
            terms.append((par, 4, row, float(np.round(rng.uniform(0.5, 2.0), 3)), int(rng.integers(n))))
    # two terms on the same (parameter, row, variable), not adjacent in the caller's order
    dup = (0, 4, int(rng.integers(m)), 0.75, int(rng.integers(n))) if m else (0, 5, int(rng.integers(p)), 0.75,
                                                                             int(rng.integers(n)))
    terms.insert(0, dup)
    terms.append(dup[:3] + (-1.25,) + dup[4:])
    if nparam >= 3:
        terms.insert(len(terms) // 2, (nparam - 2, 2, 0, 1.5))
        terms.append((nparam - 2, 2, 0, -0.5))
    return dict(d=d, terms=terms, nparam=nparam, active=na, structured=structured, shape=(B, n, m, p))


def relfro(a, b):
    nb = np.linalg.norm(b)
    return np.linalg.norm(np.asarray(a) - b) / (nb if nb > 0 else 1.0)


def unit(nparam, j):
    e = np.zeros(nparam)
    e[j] = 1.0
    return e


def oracle_forward_jacobian(case, b):
    """(n+m+p, nparam): column j = the oracle's forward_differentiate on poi_forward_full(e_j), problem b."""
    d, (B, n, m, p) = case["d"], case["shape"]
    cols = []
    for j in range(case["nparam"]):
        dq, dh, db, dG, dA = poi_forward_full(case["terms"], unit(case["nparam"], j), n, m, p)
        cols.append(np.concatenate(oqp.forward_differentiate(
            d["Q"][b], d["G"][b], d["h"][b], d["A"][b], d["z"][b], d["lam"][b], d["nu"][b], dq=dq, dG=dG, dh=dh,
            dA=dA, db=db)))
    return np.stack(cols, axis=1)


def oracle_reverse_outputs(d, b):
    """(n, n+m+p): row i = the oracle's reverse_differentiate(e_i) of problem b (no terms involved)."""
    n = d["z"].shape[1]
    return np.stack([np.concatenate(oqp.reverse_differentiate(
        d["Q"][b], d["G"][b], d["h"][b], d["A"][b], d["z"][b], d["lam"][b], d["nu"][b], unit(n, i)))
        for i in range(n)])


def dense_tangents(case, dp):
    """poi_forward_full per problem for dp (B, nparam) → dict of batched dense tangents for QPBatch.forward."""
    B, n, m, p = case["shape"]
    parts = [poi_forward_full(case["terms"], dp[b], n, m, p) for b in range(B)]
    dq, dh, db, dG, dA = (np.stack(x) for x in zip(*parts))
    return dict(dq=dq, dh=dh, db=db, dG=dG, dA=dA)

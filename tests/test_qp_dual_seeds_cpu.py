"""The numpy restatement of the QP reverse mode with seeds on the duals
(tests/qp_dual_seed_cases.py), pinned on the CPU: by finite differences of a
re-solved QP, by the eliminated rows' closed form, by the adjoint identity
with the oracle's forward mode and by its reduction to the oracle's reverse
mode (QuadraticProgram.jl:316-351, :357-446) at zero dual seeds."""

import numpy as np
import pytest

import qp_dual_seed_cases as dc
from oracle import qp as oqp

KEYS = ("Q", "G", "h", "A", "z", "lam", "nu")


def _seeds(c, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(c["z"].shape[0]), rng.standard_normal(c["lam"].shape[0]),
            rng.standard_normal(c["nu"].shape[0]))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_finite_differences_of_the_resolved_qp(seed):
    """l = ⟨gz, z⟩ + ⟨gl, λ⟩ + ⟨gn, ν⟩ of the optimum re-solved on its active
    set: central differences at ε = 1e-6 in q, h and b against the getters
    dl/dq = dz, dl/dh = −λ∘dλ, dl/db = −dν (each side's norm-relative error
    ≤ 1e-6; the differences' own error is ε² times a third derivative, which
    is zero here — the solution is linear in (q, h, b) on a fixed active set —
    plus rounding/ε ≈ 1e-10)."""
    c = dc.tiny_case(seed)
    z, lam, nu = dc.active_set_solve(c, c["q"], c["h"], c["b"])
    np.testing.assert_allclose(z, c["z"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(lam, c["lam"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(nu, c["nu"], rtol=0, atol=1e-12)
    gz, gl, gn = _seeds(c, 100 + seed)
    dz, dlam, dnu = dc.reverse_duals(*[c[k] for k in KEYS], gz, gl, gn)

    def loss(q, h, b):
        zz, ll, vv = dc.active_set_solve(c, q, h, b)
        return gz @ zz + gl @ ll + gn @ vv

    eps = 1e-6

    def fd(key):
        out = np.zeros_like(c[key])
        for i in range(out.size):
            hi = {k: c[k].copy() for k in ("q", "h", "b")}
            lo = {k: c[k].copy() for k in ("q", "h", "b")}
            hi[key][i] += eps
            lo[key][i] -= eps
            out[i] = (loss(hi["q"], hi["h"], hi["b"]) - loss(lo["q"], lo["h"], lo["b"])) / (2 * eps)
        return out

    assert dc.relfro(fd("q"), dz) <= 1e-6
    assert dc.relfro(fd("h"), -c["lam"] * dlam) <= 1e-6
    assert dc.relfro(fd("b"), -dnu) <= 1e-6
    # the dual seeds matter: without them the gradient is another one
    dz0 = oqp.reverse_differentiate(*[c[k] for k in KEYS], gz)[0]
    assert dc.relfro(dz0, dz) > 1e-2


def test_eliminated_rows_closed_form():
    """An eliminated row (λ_i == 0, s_i ≠ 0): row n+i of LHS reads
    G_i·x_z + s_i·x_λi = g_λi, and column n+i is zero in the z rows, so the
    row's seed reaches nothing else."""
    c = dc.tiny_case(3)
    args = [c[k] for k in KEYS]
    n, m = 6, 5
    s = oqp.gz_minus_h(c["G"], c["z"], c["h"])
    el = (c["lam"] == 0.0) & (s != 0.0)
    assert el.sum() == 2
    gz, gl, gn = _seeds(c, 7)
    dz, dlam, dnu = dc.reverse_duals(*args, gz, gl, gn)
    want = -(gl[el] - c["G"][el] @ (-dz)) / s[el]      # x = −[dz; dλ; dν]
    np.testing.assert_allclose(dlam[el], want, rtol=1e-13, atol=1e-14)
    # a seed on the eliminated rows alone
    only = np.where(el, gl, 0.0)
    dz, dlam, dnu = dc.reverse_duals(*args, np.zeros(n), only, np.zeros(2))
    # (the dense solve pivots across the whole LHS: zero to its rounding, not bit for bit)
    tol = 1e-14 * np.linalg.norm(only)
    assert max(np.abs(dz).max(), np.abs(dnu).max(), np.abs(dlam[~el]).max()) <= tol
    np.testing.assert_allclose(dlam[el], -only[el] / s[el], rtol=1e-13, atol=0)


@pytest.mark.parametrize("seed", [4, 5])
def test_adjoint_identity_with_the_oracle_forward(seed):
    """⟨g, forward(t)⟩ = ⟨reverse(g), forward_rhs(t)⟩: forward(t) =
    −LHS⁻ᵀ·rhs(t), reverse(g) = −LHS⁻¹·g."""
    c = dc.tiny_case(seed)
    args = [c[k] for k in KEYS]
    rng = np.random.default_rng(seed)
    t = dict(dQ=None, dq=rng.standard_normal(6), dG=rng.standard_normal((5, 6)), dh=rng.standard_normal(5),
             dA=rng.standard_normal((2, 6)), db=rng.standard_normal(2))
    S = rng.standard_normal((6, 6))
    t["dQ"] = (S + S.T) / 2
    g = np.concatenate(_seeds(c, 50 + seed))
    fwd = np.concatenate(oqp.forward_differentiate(*args, **t))
    rev = np.concatenate(dc.reverse_duals(*args, g[:6], g[6:11], g[11:]))
    lhs, rhs = g @ fwd, rev @ oqp.forward_rhs(*args, **t)
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs)), (lhs, rhs)


def test_zero_dual_seeds_are_the_oracle_reverse():
    from diffopt_amd.synthetic import qp_numpy
    for d, b in ((qp_numpy(2, 12, 9, 3, 0.4, 8), 1), (qp_numpy(1, 7, 0, 2, 0.4, 9), 0), (qp_numpy(1, 7, 4, 0, 0.5, 10), 0)):
        args = [d[k][b] for k in KEYS]
        m, p = d["lam"].shape[1], d["nu"].shape[1]
        got = dc.reverse_duals(*args, d["dl_dz"][b], np.zeros(m), np.zeros(p))
        want = oqp.reverse_differentiate(*args, d["dl_dz"][b])
        for a, w in zip(got, want):
            assert np.array_equal(a, w)

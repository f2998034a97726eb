"""QP reverse mode with a loss gradient on the duals (dopt_qp_reverse_duals_k):
a numpy restatement and the small case its CPU checks run on.  Test
infrastructure only.

For a loss l(z, λ, ν) and the KKT residual F = [Qz + q + Gᵀλ + Aᵀν;
λ∘(Gz − h); Az − b], the reference's LHS (QuadraticProgram.jl:256-282) is
J_Fᵀ, so
    [dz; dλ; dν] = −LHS⁻¹·[dl/dz; dl/dλ; dl/dν]        (λ, ν in OptNet sign)
and the reference's getters read it unchanged: dl/dq = dz, dl/dh = −λ∘dλ,
dl/db = −dν.  With zero dual seeds this is oracle/qp.py's
reverse_differentiate (QuadraticProgram.jl:316-351).
"""

import numpy as np

from oracle import qp as oqp


def reverse_duals(Q, G, h, A, z, lam, nu, gz, gl, gn):
    """(dz, dλ, dν) = split(−LHS \\ [gz; gl; gn]) of one problem; solve_system
    picks LSQR when Q == 0, as the reference does (:333-337)."""
    n = Q.shape[0]
    m = 0 if G is None else G.shape[0]
    LHS = oqp.create_LHS_matrix(z, lam, Q, G, h, A)
    RHS = np.concatenate([np.asarray(gz, float), np.asarray(gl, float), np.asarray(gn, float)])
    it = oqp.is_iterative(Q)
    if it and not np.any(RHS):
        x = np.zeros_like(RHS)   # as oqp.reverse_differentiate: the reference's lsqr gives NaN
    else:
        x = oqp.solve_system(LHS, RHS, it)
    g = -x
    return g[:n], g[n:n + m], g[n + m:]


def reverse_duals_flat(d, b, gz, gl, gn):
    """The restatement on problem b of a batch dict, as one [dz | dλ | dν] vector."""
    args = [d[k][b] for k in ("Q", "G", "h", "A", "z", "lam", "nu")]
    return np.concatenate(reverse_duals(*args, gz, gl, gn))


def tiny_case(seed=0, n=6, m=5, active=3, p=2):
    """A strictly complementary QP at its optimum: `active` rows with s = 0 and
    λ ~ U(0.5, 1.5), the others with λ = 0 and s ~ −U(0.5, 1.5)."""
    rng = np.random.default_rng(seed)
    L = rng.standard_normal((n, n))
    Q = L @ L.T / n + 0.5 * np.eye(n)
    Q = 0.5 * (Q + Q.T)
    G = rng.standard_normal((m, n))
    A = rng.standard_normal((p, n))
    z = rng.standard_normal(n)
    act = np.zeros(m, dtype=bool)
    act[rng.permutation(m)[:active]] = True
    lam = np.where(act, rng.uniform(0.5, 1.5, m), 0.0)
    s = np.where(act, 0.0, -rng.uniform(0.5, 1.5, m))
    nu = rng.standard_normal(p)
    # (h from oqp.gz_minus_h's sum, so that the active rows' s is exactly 0 there too)
    h = oqp.gz_minus_h(G, z, np.zeros(m)) - s
    b = A @ z
    q = -(Q @ z + G.T @ lam + A.T @ nu)
    return dict(Q=Q, q=q, G=G, h=h, A=A, b=b, z=z, lam=lam, nu=nu, act=act)


def active_set_solve(c, q, h, b):
    """The optimum of the case for nearby data (q, h, b): its active set does
    not change under a small perturbation (strict complementarity), so (z, λ_act,
    ν) solve the equality-constrained KKT system and the other λ stay 0."""
    Q, G, A, act = c["Q"], c["G"], c["A"], c["act"]
    n, m, p = Q.shape[0], G.shape[0], A.shape[0]
    Ga = G[act]
    na = Ga.shape[0]
    K = np.zeros((n + na + p, n + na + p))
    K[:n, :n] = Q
    K[:n, n:n + na] = Ga.T
    K[n:n + na, :n] = Ga
    K[:n, n + na:] = A.T
    K[n + na:, :n] = A
    x = np.linalg.solve(K, np.concatenate([-q, h[act], b]))
    lam = np.zeros(m)
    lam[act] = x[n:n + na]
    return x[:n], lam, x[n + na:]


def relfro(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    nb = np.linalg.norm(b)
    return np.linalg.norm(a - b) / (nb if nb > 0 else 1.0)

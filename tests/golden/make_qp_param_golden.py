"""Transcribe the reference's parametric QP known-answer tests into a JSON
golden fixture (tests/golden/qp_param_fixtures.json).

    python tests/golden/make_qp_param_golden.py

No solver (HiGHS) is available, so every primal-dual point is written out
exactly.  Each constraint is written as G z ≤ h with its parametric part on the
left: `x ≥ 3p` is `−x + 3p ≤ 0`, i.e. G = [−1], h = [−3p] at the parameter's
value and the term (p, kind 0, row 0, +3).  λ is in the engine's (OptNet) sign,
λ ≥ 0 for G z ≤ h: stationarity is Q z + q + Gᵀλ = 0.

test/parameters.jl:32-101 (test_diff_rhs): x ≥ 3p, Min 2x, so x(p) = 3p and
x'(p) = 3.  z = 3p, λ = 2 (2 − λ = 0), Q = 0: the LSQR branch.  Forward
directions 1 and 2 at p = 3 and at p = 2; the reverse checks (ReverseVariablePrimal
1 and 2) run at p = 2 only, so the p = 3 case carries none.

test/parameters.jl:259-315 (test_affine_changes_compact): pc·x ≥ 3p, Min 2x,
for p, pc ∈ 1:3: −pc·x + 3p ≤ 0, G = [−pc], h = [−3p], z = 3p/pc, λ = 2/pc
(2 − pc·λ = 0); terms (p, 0, row 0, 3) and (pc, 4, row 0, −1, var 0).
x(p, pc) = 3p/pc: dx/dp = 3/pc, dx/dpc = −3p/pc².  Forward directions
(direction_pc, direction_p) ∈ (0:2)², reverse direction_x ∈ 0:2.

test/parameters.jl:570-610 (test_quadratic_objective_qp): Min 3px + x² + 5p +
7p², x ≥ −10, p = 3: Q = [2], q = [3p], G = [−1], h = [10], z = −3p/2 = −4.5,
λ = 0 with s = G z − h = −5.5 (an eliminated row); terms (p, 3, var 0, 3) and
(p, 2, 0, 5) — the parameter×parameter term 7p² is outside the term table (its
tangent multiplies the objective's constant, which never enters the KKT system).
dx/dp = −3/2; directions 0:2 in both modes, atol = 1e-4.

Tolerances: the one the reference's test states (`atol = 1e-4`, which makes
Julia's rtol default 0), else Julia's `≈` default rtol = √eps(Float64), atol = 0:
|a − b| ≤ max(atol, rtol·max(|a|, |b|)).
"""

import json
import os

OUT = os.path.dirname(os.path.abspath(__file__))
SQRT_EPS = 2.0 ** -26   # √eps(Float64)


def case(name, source, Q, q, G, h, z, lam, nparam, terms, fwd, rev, rtol=SQRT_EPS, atol=0.0):
    return dict(name=name, source=source, n=1, m=1, p=0, Q=Q, q=q, G=G, h=h, A=[], b=[], z=z, lam=lam, nu=[],
                nparam=nparam, terms=terms, rtol=rtol, atol=atol, fwd=fwd, rev=rev)


def main():
    cases = []
    for p in (3.0, 2.0):
        fwd = [dict(dp=[d], dx=[3.0 * d]) for d in (1.0, 2.0)]
        rev = [dict(dx=[d], dp=[3.0 * d]) for d in (1.0, 2.0)] if p == 2.0 else []
        cases.append(case(f"diff_rhs_p{int(p)}", "test/parameters.jl:32-101", [[0.0]], [2.0], [[-1.0]], [-3.0 * p],
                          [3.0 * p], [2.0], 1, [[0, 0, 0, 3.0]], fwd, rev))
    for p in (1.0, 2.0, 3.0):
        for pc in (1.0, 2.0, 3.0):
            fwd = [dict(dp=[dp, dpc], dx=[-dpc * 3 * p / pc ** 2 + dp * 3 / pc])
                   for dpc in (0.0, 1.0, 2.0) for dp in (0.0, 1.0, 2.0)]
            rev = [dict(dx=[float(dx)], dp=[dx * 3 / pc, -dx * 3 * p / pc ** 2]) for dx in (0, 1, 2)]
            cases.append(case(f"affine_changes_compact_p{int(p)}_pc{int(pc)}", "test/parameters.jl:259-315",
                              [[0.0]], [2.0], [[-pc]], [-3.0 * p], [3.0 * p / pc], [2.0 / pc], 2,
                              [[0, 0, 0, 3.0], [1, 4, 0, -1.0, 0]], fwd, rev))
    p = 3.0
    sweep = (0.0, 1.0, 2.0)
    cases.append(case("quadratic_objective_qp_p3", "test/parameters.jl:570-610", [[2.0]], [3.0 * p], [[-1.0]], [10.0],
                      [-3.0 * p / 2], [0.0], 1, [[0, 3, 0, 3.0], [0, 2, 0, 5.0]],
                      [dict(dp=[d], dx=[d * (-3 / 2)]) for d in sweep],
                      [dict(dx=[d], dp=[d * (-3 / 2)]) for d in sweep], rtol=0.0, atol=1e-4))
    with open(os.path.join(OUT, "qp_param_fixtures.json"), "w") as f:
        json.dump(cases, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

"""Transcribe the reference's parametric cone-program known-answer test into
a JSON golden fixture (tests/golden/conic_param_fixtures.json).

    python tests/golden/make_conic_param_golden.py

test/parameters.jl:103-152 (test_diff_vector_rhs): one variable x, one
parameter p, the constraint [x − 3p] ∈ Zeros(1), a placeholder
[0, 0, 0] ∈ SecondOrderCone, objective Min 2x.  So x(p) = 3p and x'(p) = 3.
For p ∈ 0:3 and direction ∈ 0:3 the test sets ForwardConstraintSet of the
parameter to `direction` and expects ForwardVariablePrimal(x) = 3·direction,
then sets ReverseVariablePrimal(x) = direction and expects
ReverseConstraintSet of the parameter = 3·direction, both at atol = 1e-3.

The solver (SCS) is not available, so the primal-dual point is written out
exactly: x = 3p; the Zeros row's slack is 0 and its dual is 2 (stationarity
c − A_moiᵀy = 0 with c = 2, A_moi = [1]); the placeholder cone's rows are
all zero.  In the geometric form A_moi x + b ∈ K the parametric row is
x + (−3p), i.e. one term (parameter 0, kind 0, row 0, coefficient −3).
"""

import json
import os

OUT = os.path.dirname(os.path.abspath(__file__))


def main():
    cases = []
    for p in range(4):
        sweeps = [dict(direction=float(d), dx=3.0 * d, dp=3.0 * d) for d in range(4)]
        cases.append(dict(name=f"diff_vector_rhs_p{p}", source="test/parameters.jl:103-152", p=float(p), n=1,
                          cones=[[0, 1], [3, 3]], A=[[1.0], [0.0], [0.0], [0.0]],
                          b=[-3.0 * p, 0.0, 0.0, 0.0], c=[2.0], max_sense=False, x=[3.0 * p],
                          s=[0.0, 0.0, 0.0, 0.0], y=[2.0, 0.0, 0.0, 0.0], nparam=1,
                          terms=[[0, 0, 0, -3.0]], atol=1e-3, sweeps=sweeps))
    with open(os.path.join(OUT, "conic_param_fixtures.json"), "w") as f:
        json.dump(cases, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

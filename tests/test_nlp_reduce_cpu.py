"""The NLP engine's exact elimination of the bound and slack rows (the reduced
KKT route of csrc/nlp.hip), restated in numpy and checked against the oracle's
full solve with M (oracle/nlp.py, the reference's sIpopt system,
nlp_utilities.jl:358-394) — the specification the HIP kernels follow.

M over [w; y; ν_L; ν_U] (w = [x; s_geq; s_leq]):  bound row i on w_j reads
``a_i·z_j + d_i·z_νi = r_i`` and row j carries ``b_i·z_νi``; for M,
(a, b) = (V, ∓1), for Mᵀ (a, b) = (∓1, V) — the same elimination serves both
directions:

* d_i ≠ 0 (an inactive bound):  z_νi = (r_i − a_i z_j)/d_i, so row j gains
  δ_j = −a_i b_i / d_i on its diagonal and r_j −= b_i r_i / d_i;
* d_i = 0 (active):  z_j = r_i / a_i is known (a_i = 0 or two active bounds
  on one variable: no reduction, the full route);
* slack t of constraint k (W is zero on slacks): known (active bound) →
  constraint row k reads J_k x = r_k + z_t; else row t reads
  δ_t z_t − y_k = r̃_t: δ_t = 0 → y_k = −r̃_t is known (row / column k drop
  out, z_t = J_k x − r_k afterwards); δ_t ≠ 0 → z_t = (r̃_t + y_k)/δ_t and row
  k reads J_k x − y_k/δ_t = r_k + r̃_t/δ_t.

What is left is R = [H + diag(δ_x), Jᵀ; J, −diag(ρ)] over [x; y] with the known
unknowns as identity rows / columns — symmetric when H is, the same matrix for
both directions.
"""

import numpy as np
import pytest

from diffopt_amd.synthetic import nlp_numpy
from nlp_edge_cases import bounds as _bounds, reduced_solve   # the numpy elimination (shared with the edge cases)
from oracle import nlp


@pytest.mark.parametrize("sense", [1, -1])
@pytest.mark.parametrize("trans", [False, True])
def test_reduced_elimination_matches_full_solve(sense, trans):
    st, pt, _, _, _ = nlp_numpy(3, 12, 7, 3, 4321 + sense, sense=sense)
    for b in range(3):
        L = nlp.Layout(st["con_kind"], st["has_low"], st["has_up"])
        p = {k: v[b] for k, v in pt.items()}
        X, V_L, X_L, V_U, X_U = nlp.solution_and_bounds(L, sense, p["x"], p["cval"], p["crhs"], p["y"], p["xl"],
                                                        p["xu"], p["yl"], p["yu"])
        M, _ = nlp.build_sensitivity_matrices(L, p["Hxx"], p["Hxp"], p["Jx"], p["Jp"], X, V_L, X_L, V_U, X_U)
        bnd = _bounds(L, X, V_L, X_L, V_U, X_U)
        r = np.random.default_rng(b).standard_normal(M.shape[0])
        z = reduced_solve(L, p["Hxx"], p["Jx"], bnd, r, trans)
        assert z is not None
        ref = np.linalg.solve(M.T if trans else M, r)
        assert np.linalg.norm(z - ref) <= 1e-9 * np.linalg.norm(ref)

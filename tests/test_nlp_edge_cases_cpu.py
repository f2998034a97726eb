"""The NLP edge cases (nlp_edge_cases.py) are what they are named for — on the
CPU alone, no GPU:

* the census of every problem (the numpy restatement of nlp_red_prep_kernel)
  equals the counts the case states, and the table's own figures hold (70
  known x, 70 known y, ρ on every inactive inequality row and at least 3 of
  them, 3 variables with two δ terms, fixed unknowns at the R-indices 31 / 32 /
  63 / 64, more than 64 KB of LDS for the pair kernels only);
* the oracle applies no inertia correction, except on problem 1 of
  ``corrected``;
* the reference alone is far inside the GPU tests' 1e-6: cond(M) ≤ 1e5 on
  every checked problem (the corrected matrix's is printed), and the oracle's
  ∂s (SuperLU) agrees with a LAPACK solve of the same matrix to 1e-9;
* the numpy elimination — the specification the kernels follow — agrees with
  the full solves of M and Mᵀ to 1e-9 on the states it had not seen before
  (ρ rows, O(1) δ, an asymmetric H) and on the block-edge shapes.

A generator or seed change that lets a case degenerate fails here, not
silently in test_nlp_edges_gpu.py."""

import numpy as np
import pytest

import nlp_edge_cases as ec

CENSUS_KEYS = ("known_x", "known_y", "rho_rows", "delta_x", "delta_two")
STATE = [n for n in ec.NAMES if n.rsplit("_", 1)[0] in ec.STATE_FAMILIES]
EDGES = [n for n in ec.NAMES if n.startswith("edge_")]


def _census(cs, b, pt="pt"):
    L, _, _, bnd = ec.matrices(cs["st"], cs[pt], b)
    return L, ec.census(L, bnd)


@pytest.mark.parametrize("name", ec.NAMES)
def test_census(name):
    cs = ec.case(name)
    assert (cs["n"], cs["c"], cs["P"]) == {**{f"edge_{N}": s + (1,) for N, s in ec.EDGE_SHAPES.items()},
                                           "x_all_fixed_c0": (70, 0, 1), "y_all_known": (20, 70, 1),
                                           "slacks_all_fixed": (80, 30, 1), "lds_optin": ec.LDS_SHAPE,
                                           "corrected": (20, 12, 4)}.get(name, ec.SHAPE)
    assert 2 <= cs["B"] <= 4
    for b in range(cs["B"]):
        L, got = _census(cs, b)
        assert got["reduced"] == cs["reduced"][b], (name, b)
        for k in CENSUS_KEYS:
            assert got[k] == cs["expect"][k][b], (name, b, k, got[k], cs["expect"][k][b])
        assert L.rows <= ec.PIVOT_MAX


@pytest.mark.parametrize("name", STATE)
def test_state_cases_hold_their_state(name):
    cs = ec.case(name)
    st, pt = cs["st"], cs["pt"]
    kinds = st["con_kind"]
    assert st["sense"] == cs["sense"] == (1 if name.endswith("_min") else -1)
    for b in range(cs["B"]):
        _, got = _census(cs, b)
        inactive = (kinds != 0) & (pt["cval"][b] != pt["crhs"][b])
        sym = np.array_equal(pt["Hxx"][b], pt["Hxx"][b].T)
        if cs["family"] in ("rho_rows", "rho_delta_asym_all"):
            # yst == 2 on exactly the inactive inequality rows, duals of the set's sign
            np.testing.assert_array_equal(got["yst"] == 2, inactive)
            assert inactive.sum() >= 3 and got["known_y"] == 0
            y = pt["y"][b]
            assert (y[inactive & (kinds == 1)] >= 0.5).all() and (y[inactive & (kinds == 2)] <= -0.5).all()
        else:
            assert got["rho_rows"] == 0
        if cs["family"] in ("delta_primal", "rho_delta_asym_all"):
            lo = (st["has_low"] != 0) & (pt["xl"][b] != pt["x"][b])
            up = (st["has_up"] != 0) & (pt["xu"][b] != pt["x"][b])
            assert (pt["yl"][b][lo] >= 0.5).all() and (pt["yu"][b][up] <= -0.5).all()
            assert got["delta_two"] >= 3 and got["delta_x"] > got["delta_two"]
            # O(1) beside H (a single term is U(0.5, 1.5) / U(0.5, 1.5); two
            # terms have opposite signs and may nearly cancel): nothing swamps H
            dl = np.abs(got["delta"][:cs["n"]])
            one = dl[lo ^ up]
            assert dl.max() <= 2 * 3.0 and len(one) >= 3 and one.min() >= 1 / 3 and one.max() <= 3.0
        else:
            assert got["delta_x"] == 0
        assert sym == (cs["family"] not in ("rho_delta_asym_all", "asym_one") or
                       (cs["family"] == "asym_one" and b != 1)), (name, b)
    if cs["family"] == "asym_one":   # the batch before the edit: symmetric everywhere, otherwise the same point
        for k in ec.KEYS:
            same = np.array_equal(cs["pt_sym"][k], pt[k])
            assert same == (k != "Hxx")
        assert all(np.array_equal(h, h.T) for h in cs["pt_sym"]["Hxx"])
        np.testing.assert_array_equal(cs["pt_sym"]["Hxx"][[0, 2]], pt["Hxx"][[0, 2]])


def test_degenerate_counts():
    x = ec.case("x_all_fixed_c0")
    assert x["expect"]["known_x"] == [70, 70] and x["c"] == 0 and x["pt"]["Jx"].shape == (2, 0, 70)
    assert x["st"]["has_low"].all() and not x["st"]["has_up"].any()
    y = ec.case("y_all_known")
    assert y["expect"]["known_y"] == [70, 70] and (y["st"]["con_kind"] != 0).all() and not y["pt"]["y"].any()
    s = ec.case("slacks_all_fixed")
    assert (s["st"]["con_kind"] != 0).all() and not s["st"]["has_low"].any() and not s["st"]["has_up"].any()
    for b in range(2):
        _, got = _census(s, b)
        assert (got["kx"][80:] >= 0).all() and len(got["kx"]) == 110 and (got["yst"] == 0).all()
    # more than one ballot of wave_compact (64 lanes) in both lists
    assert min(x["expect"]["known_x"]) > 64 and min(y["expect"]["known_y"]) > 64
    assert {c["P"] for c in (x, y, s)} == {1}


@pytest.mark.parametrize("name", EDGES)
def test_edges_fix_the_block_boundary_unknowns(name):
    cs = ec.case(name)
    N, n = cs["n"] + cs["c"], cs["n"]
    assert N == int(name[5:]) and cs["fixed"] == [i for i in (31, 32, 63, 64) if i < N]
    if n == 40:
        assert cs["fixed"][:2] == [31, 32]   # x₃₁ and x₃₂
    for b in range(cs["B"]):
        _, got = _census(cs, b)
        for i in cs["fixed"]:   # an identity row / column of R at index i
            assert (got["kx"][i] >= 0) if i < n else (got["yst"][i - n] == 1), (name, b, i)


def test_lds_optin_sizes():
    cs = ec.case("lds_optin")
    L = ec.layout(cs["st"])
    assert (cs["st"]["con_kind"] == 0).all() and not cs["st"]["has_up"].any()
    assert 2 * L.num_w + L.c + L.n > 4096 and L.rows <= ec.PIVOT_MAX
    frac = cs["st"]["has_low"].mean()
    assert 0.06 < frac < 0.10
    for b in range(cs["B"]):
        assert 0.3 < cs["expect"]["known_x"][b] / cs["st"]["has_low"].sum() < 0.7
    lds = ec.red_lds_bytes(L.n, L.c, L.num_w)
    for kern in ("rhs", "recover"):
        assert lds[kern, 1] < ec.LDS_DEFAULT < lds[kern, 2] <= 160 * 1024


@pytest.mark.parametrize("name", ec.NAMES)
def test_oracle_verdict_and_reference_accuracy(name):
    cs = ec.case(name)
    for b in range(cs["B"]):
        if name == "lds_optin" and b not in cs["problems"]:
            continue   # (0.4 s a problem in the oracle: only the checked one)
        _, L, M, N, corr = ec.oracle(cs, b)
        if b in cs.get("corrected", ()):
            assert corr >= 1, (name, b)
        else:
            assert corr == 0, (name, b, corr)
        if b not in cs["problems"]:
            continue
        cond = np.linalg.cond(ec.corrected_matrix(cs, b))
        disc = ec.reference_discrepancy(cs, b)
        print(f"{name}[{b}]: rows {L.rows} corrections {corr} cond {cond:.3g} SuperLU-vs-LAPACK {disc:.3g}")
        if corr == 0:
            assert cond <= 1e5, (name, b, cond)
        assert disc <= 1e-9, (name, b, disc)
    if name == "corrected":
        assert cs["corrected"] == [1] and cs["B"] == 3


@pytest.mark.parametrize("trans", [False, True], ids=["M", "Mt"])
@pytest.mark.parametrize("name", [n for n in STATE if not n.startswith("asym_one")] + EDGES)
def test_elimination_on_the_new_states(name, trans):
    cs = ec.case(name)
    for b in range(cs["B"]):
        L, M, _, bnd = ec.matrices(cs["st"], cs["pt"], b)
        r = np.random.default_rng(b).standard_normal(M.shape[0])
        z = ec.reduced_solve(L, cs["pt"]["Hxx"][b], cs["pt"]["Jx"][b], bnd, r, trans)
        assert z is not None
        ref = np.linalg.solve(M.T if trans else M, r)
        assert np.linalg.norm(z - ref) <= 1e-9 * np.linalg.norm(ref), (name, b)

"""The reused-handle sequences (reuse_cases.py) have the properties their
steps state — on the oracle alone, no GPU: the reduced size N' of every
problem (the reference's exact elimination set), the `iterative` branch, the
sizes' place relative to the engine's route thresholds, and for the conic
steps flagged oracle-comparable that the oracle's LSQR converges (istop 1–2)
in both directions on every problem, and for the NLP steps the structure's
sizes, the oracle's corrections and the problems' symmetry.  A generator change that lets a sequence
degenerate (a step no longer growing, a model no longer converging) fails
here, not silently in test_handle_reuse_gpu.py."""

import numpy as np
import pytest

import reuse_cases as rc
from oracle import qp as oqp

QP_SEQUENCES = {
    "sizes": (rc.qp_sizes, rc.SIZES_SHAPE),
    "kinds": (rc.qp_kinds, rc.KINDS_SHAPE),
    "tall": (rc.qp_tall, rc.TALL_SHAPE),
    "small_batched_B2": (lambda: rc.qp_small_batched(2), (2,) + rc.SMALL_SHAPE),
    "small_batched_B1": (lambda: rc.qp_small_batched(1), (1,) + rc.SMALL_SHAPE),
    "staging": (rc.qp_staging, rc.STAGING_SHAPE),
    "sparse_toggle": (lambda: [rc.qp_sparse_toggle()[0]], rc.TOGGLE_SHAPE),
}


@pytest.mark.parametrize("name", list(QP_SEQUENCES))
def test_qp_steps_have_their_stated_properties(name):
    steps, (B, n, m, p) = QP_SEQUENCES[name]
    for st in steps():
        d = st["data"]
        assert d["z"].shape == (B, n) and d["lam"].shape == (B, m) and d["nu"].shape == (B, p), st["name"]
        for b in range(B):
            kept = rc.oracle_kept(d, b)
            assert n + kept.sum() + p == st["nsys"][b], (st["name"], b)
            assert oqp.is_iterative(d["Q"][b]) == st["iterative"][b], (st["name"], b)
            assert (st["lu_kind"][b] == rc.LSQR) == st["iterative"][b], (st["name"], b)
            # the small path takes exactly the reduced systems up to SM_MAX
            assert (st["lu_kind"][b] == rc.SMALL) == (name.startswith("small") and st["nsys"][b] <= rc.SM_MAX)
            if not st["iterative"][b]:
                # LHS can be non-singular: the rows with s = 0 (λ ~ U(0.5, 1.5))
                # and the equality rows number at most n (reuse_cases.qp_kept)
                assert (d["lam"][b] >= 0.5).sum() + p <= n, (st["name"], b)
            if st["sym"][b]:   # the P-symmetric route needs an exactly symmetric Q
                assert np.array_equal(d["Q"][b], d["Q"][b].T), (st["name"], b)


def test_qp_sequences_cross_the_sizes_they_claim():
    a = [max(s["nsys"]) for s in rc.qp_sizes()]
    assert a == [220, 340, 170, 340, 360, 220]                        # grown, shrunk below the first, ...
    assert rc.qp_sizes()[3]["nsys"] == [170, 340, 220, 280]           # mixed padded sizes in one batch
    assert min(min(s["nsys"]) for s in rc.qp_sizes()) > rc.SM_MAX
    assert rc.qp_sizes()[5]["data"] is rc.qp_sizes()[0]["data"]       # the first model again
    for s in rc.qp_kinds():   # the whole batch on the batched route; the LSQR problem on its full LHS
        assert s["nsys"] == [145 if it else 129 for it in s["iterative"]] and sum(s["iterative"]) <= 1
    assert [s["nsys"][0] for s in rc.qp_tall()] == [1620, 1270, 1620, 1270, 1620]
    assert 1270 <= rc.PIVOT_MAX < 1620
    for B in (1, 2):
        assert [s["nsys"][0] for s in rc.qp_small_batched(B)] == [96, 96, 152, 152, 96, 96, 96]
    assert [s["how"] for s in rc.qp_staging()] == ["set", "csc", "device", "set", "csc"]
    for s in rc.qp_staging():
        if s["how"] == "csc":
            dens = (s["data"]["G"] != 0).mean()
            assert 0.25 < dens < 0.35, dens
    # the asymmetric Q of sequence b is asymmetric, its neighbours are not
    asym = rc.qp_kinds()[5]["data"]["Q"]
    assert not np.array_equal(asym[3], asym[3].T) and np.array_equal(asym[2], asym[2].T)


def test_sparse_toggle_lp_is_an_lp_the_oracle_solves():
    _, lp, refused = rc.qp_sparse_toggle()
    B, n, m, p = rc.TOGGLE_SHAPE
    assert lp["z"].shape == (B, n) and lp["lam"].shape == (B, m) and lp["nu"].shape == (B, p)
    for b in range(B):
        _, _, (_, isr), (_, isf) = oqp.lp_sparse_differentiate(
            lp["G"][b], lp["h"][b], lp["A"][b], lp["z"][b], lp["lam"][b], lp["nu"][b], lp["dl_dz"][b],
            lp["dq"][b], lp["dh"][b], lp["db"][b])
        assert isr in (1, 2) and isf in (1, 2)
        assert not oqp.is_iterative(refused["Q"][b])


CONIC_SEQUENCES = {"second_model": rc.conic_second_model, "tables": rc.conic_tables}


@pytest.mark.parametrize("name", list(CONIC_SEQUENCES))
def test_conic_comparable_steps_converge_on_the_oracle(name):
    steps = CONIC_SEQUENCES[name]()
    assert sum(s["comparable"] for s in steps) >= 2
    for st in steps:
        assert sum(d for _, d in st["cones"]) == 69
        if not st["comparable"]:
            continue
        for b in range(rc.CONIC_B):
            fi, ri = rc.conic_oracle(st, b)["info"]
            assert fi[1] in (1, 2) and ri[1] in (1, 2), (st["name"], b, fi, ri)


def test_conic_sequences_change_what_they_claim():
    g = rc.conic_second_model()
    # SOC(8) of M69, rows 52..59: the pair's case (s interior, y = 0 / s = 0,
    # y interior / boundary pair) differs between the models of some problem
    def soc_case(d, b):
        s, y = d["s"][b, 52:60], d["y"][b, 52:60]
        return (bool(np.any(s)), bool(np.any(y)))
    cases = {tuple(soc_case(st["data"], b) for st in g) for b in range(rc.CONIC_B)}
    assert any(len(set(c)) > 1 for c in cases), cases
    t = rc.conic_tables()
    assert [st["cones"] for st in t] == rc.TABLES and t[3]["data"] is t[0]["data"]
    big = rc.conic_big_psd()
    assert all(sum(d for _, d in st["cones"]) == rc.BIG_PSD_M for st in big)
    assert big[0]["cones"][0] == (4, 66 * 67 // 2) and all(c != 4 for c, _ in big[1]["cones"])
    assert big[2]["data"] is big[0]["data"]


def test_nlp_steps_have_their_stated_properties():
    from oracle import nlp as onlp
    steps = rc.nlp_structures()
    B, n, c, P = rc.NLP_SHAPE
    lay = [onlp.Layout(s["st"]["con_kind"], s["st"]["has_low"], s["st"]["has_up"]) for s in steps]
    # num_w / nlo / nup change on the live handle: shrink to the saddle-only shape, grow past the first
    assert lay[1].num_w == n and lay[1].nlo == lay[1].nup == 0 and lay[1].rows == n + c and steps[1]["saddle"]
    assert lay[2].num_w == n + c > lay[0].num_w > n and lay[2].rows > lay[0].rows > n + c
    assert (steps[2]["st"]["con_kind"] != 0).all() and lay[0].nlo > 0 and lay[0].nup > 0
    assert [s["restructure"] for s in steps] == [True, True, True, True, False, False, True]
    assert all(s["st"] is steps[0]["st"] for s in steps[3:]) and steps[6]["data"] is steps[0]["data"]
    assert [s["corrected"] for s in steps] == [[], [], [], [1], [], [], []]
    assert [s["asym"] for s in steps] == [[], [], [], [], [], [2], []]
    for s, L in zip(steps, lay):
        pt = s["data"]["pt"]
        assert pt["x"].shape == (B, n) and pt["Jx"].shape == (B, c, n) and pt["Hxp"].shape == (B, n, P)
        assert s["data"]["dd"].shape == (B, c + len(L.low_p) + len(L.up_p))
        for b in range(B):
            _, _, corr = rc.nlp_oracle(s, b)
            assert (corr >= 1) == (b in s["corrected"]) and corr >= 0, (s["name"], b, corr)
            assert s["nsys"][b] == (L.rows if b in s["corrected"] else n + c)
            assert np.array_equal(pt["Hxx"][b], pt["Hxx"][b].T) == (b not in s["asym"]), (s["name"], b)
    # the regular point after the corrected one is another point of the same structure
    assert not np.array_equal(steps[4]["data"]["pt"]["Jx"], steps[3]["data"]["pt"]["Jx"])

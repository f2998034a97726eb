"""The NLP reduced route on the GPU at every elimination state and block edge:
the cases of nlp_edge_cases.py (pinned on the CPU by
test_nlp_edge_cases_cpu.py) through csrc/nlp.hip — nlp_red_prep_kernel,
nlp_red_rhs_kernel<1|2>, nlp_red_recover_kernel<1|2>, R as the left-looking LU
reads it from the inputs and as nlp_assemble_kernel writes it, the speculative
launch, the > 64 KB dynamic-LDS opt-in and the inertia-corrected `redo` path.

Every case: the factorised sizes and the corrections the oracle's; forward,
reverse and the Jacobian at north_star's 1e-6 relative Frobenius against the
oracle's full solve with M; forward_reverse (the NV = 2 kernels) bit-equal to
the separate calls (NV = 1) — on an asymmetric H the only check that tells the
two direction-specific reads of H apart; the adjoint identity at 1e-10; and
the full route (DOPT_NLP_REDUCE=0) within 1e-9 of the reduced one."""

import numpy as np
import pytest

import nlp_edge_cases as ec
from oracle import nlp as onlp

pytestmark = pytest.mark.gpu
RTOL = 1e-6
KEYS = list(ec.KEYS)
ROUTED = [n for n in ec.NAMES if n not in ("lds_optin", "corrected")]   # the state, degenerate and edge cases


def relfro(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    nb = np.linalg.norm(b)
    return np.linalg.norm(a - b) / (nb if nb > 0 else 1.0)


@pytest.fixture(params=["nopiv", "pivot"])
def lu_mode(request, monkeypatch):
    if request.param == "pivot":
        monkeypatch.setenv("DOPT_LU", "0")
    else:
        monkeypatch.delenv("DOPT_LU", raising=False)
    return request.param


def engine(cs, pt="pt", deferred=False):
    from diffopt_amd.nlp import NLPBatch
    st = cs["st"]
    e = NLPBatch(cs["B"], cs["n"], cs["c"], cs["P"], deferred=deferred)
    e.set_structure(st["con_kind"], st["has_low"], st["has_up"], st["sense"])
    e.set(*[cs[pt][k] for k in KEYS])
    e.factor()
    return e


def oracle_outputs(cs, b):
    ds, L, _, _, corr = ec.oracle(cs, b)
    ox, od = onlp.forward(ds, L, cs["dp"][b])
    return np.concatenate([ox, od]), onlp.reverse(ds, L, cs["dx"][b], cs["dd"][b]), ds, corr


def check_sizes(e, cs):
    rows = e.layout()["rows"]
    assert rows == ec.layout(cs["st"]).rows
    want = [rows if (not r or b in cs.get("corrected", ())) else cs["n"] + cs["c"] for b, r in enumerate(cs["reduced"])]
    np.testing.assert_array_equal(e.system_size(), want)
    # (lds_optin: the oracle's verdict on the unchecked problem is pinned 0 by construction, not recomputed)
    corr = [ec.oracle(cs, b)[4] if (b in cs["problems"] or cs["name"] != "lds_optin") else 0 for b in range(cs["B"])]
    np.testing.assert_array_equal(e.corrections(), corr)


def check_outputs(cs, fx, fd, rp, J, bar=RTOL, where=""):
    for b in cs["problems"]:
        of, orv, ds, _ = oracle_outputs(cs, b)
        errs = dict(forward=relfro(np.concatenate([fx[b], fd[b]]), of), reverse=relfro(rp[b], orv))
        if J is not None:
            errs["jacobian"] = relfro(J[b], ds)
        print(f"{cs['name']}{where}[{b}]: " + " ".join(f"{k} {v:.3g}" for k, v in errs.items()))
        for k, v in errs.items():
            assert v <= bar, (cs["name"], where, b, k, v)


def check_case(cs):
    """The per-case checks on a fresh handle.  Returns its outputs."""
    e = engine(cs)
    check_sizes(e, cs)
    dp, dx, dd = cs["dp"], cs["dx"], cs["dd"]
    fx, fd = e.forward(dp)
    rp = e.reverse(dx, dd)
    J = e.jacobian()
    check_outputs(cs, fx, fd, rp, J)
    gx, gd, gp = e.forward_reverse(dp, dx, dd)   # one call against two: NV = 2 against NV = 1
    np.testing.assert_array_equal(gx, fx)
    np.testing.assert_array_equal(gd, fd)
    np.testing.assert_array_equal(gp, rp)
    lhs = np.einsum("bi,bi->b", dx, fx) + np.einsum("bi,bi->b", dd, fd)   # ⟨Δw, ∂s·Δp⟩ = ⟨∂sᵀΔw, Δp⟩
    np.testing.assert_allclose(lhs, np.einsum("bi,bi->b", rp, dp), rtol=1e-10, atol=1e-12)
    # the Jacobian's columns are the forward call's: ∂s·Δp from both
    Jf = np.einsum("brp,bp->br", J, dp)
    assert relfro(Jf[:, :cs["n"]], fx) <= 1e-10
    e.close()
    return fx, fd, rp, J


@pytest.mark.parametrize("name", ROUTED)
def test_case(name, lu_mode, monkeypatch):
    cs = ec.case(name)
    monkeypatch.delenv("DOPT_NLP_REDUCE", raising=False)
    fx, fd, rp, J = check_case(cs)
    # reduced against full route (test_reduced_route_sizes_and_parity's bar)
    monkeypatch.setenv("DOPT_NLP_REDUCE", "0")
    f = engine(cs)
    assert (f.system_size() == f.layout()["rows"]).all()
    np.testing.assert_array_equal(f.corrections(), 0)
    gx, gd = f.forward(cs["dp"])
    assert relfro(np.concatenate([gx, gd], axis=1), np.concatenate([fx, fd], axis=1)) <= 1e-9
    assert relfro(f.reverse(cs["dx"], cs["dd"]), rp) <= 1e-9
    assert relfro(f.jacobian(), J) <= 1e-9
    f.close()


def _calls(e, cs, factor_each=False):
    """forward, reverse, jacobian, forward_reverse — with `factor_each` every
    one on a factorisation of its own (in the deferred form: each call
    finishes a pending one after its right-hand sides are queued)."""
    out = {}
    for call in ("forward", "reverse", "jacobian", "forward_reverse"):
        if factor_each:
            e.factor()
        if call == "forward":
            out["fx"], out["fd"] = e.forward(cs["dp"])
        elif call == "reverse":
            out["rp"] = e.reverse(cs["dx"], cs["dd"])
        elif call == "jacobian":
            out["J"] = e.jacobian()
        else:
            out["gx"], out["gd"], out["gp"] = e.forward_reverse(cs["dp"], cs["dx"], cs["dd"])
    return out


@pytest.mark.parametrize("deferred", [False, True], ids=["sync", "deferred"])
@pytest.mark.parametrize("sense", ["min", "max"])
def test_asym_one_after_a_correct_guess(sense, deferred, lu_mode):
    """The speculative launch missing because of asymmetry alone: the handle's
    first batch is symmetric everywhere (the guess was right), then problem 1's
    H is asymmetric — it stays on the reduced route (n + c), the batch leaves
    the left-looking LU.  Kinds and sizes straight after factor() and every
    call equal a fresh handle's; all at the oracle bar."""
    cs = ec.case(f"asym_one_{sense}")
    e = engine(cs, "pt_sym", deferred=deferred)
    fx, fd = e.forward(cs["dp"])   # the symmetric batch, against its own oracle
    for b in range(cs["B"]):
        ds, L, *_ = ec.oracle(cs, b, "pt_sym")
        ox, od = onlp.forward(ds, L, cs["dp"][b])
        assert relfro(np.concatenate([fx[b], fd[b]]), np.concatenate([ox, od])) <= RTOL
    ref = engine(cs)
    want = _calls(ref, cs, factor_each=True)
    for _ in range(2):   # the miss, and the same handle again (guessing now off)
        e.set(*[cs["pt"][k] for k in KEYS])
        e.factor()
        kinds, sizes = e.lu_kind(), e.system_size()
        np.testing.assert_array_equal(kinds, ref.lu_kind())
        np.testing.assert_array_equal(sizes, ref.system_size())
        np.testing.assert_array_equal(sizes, cs["n"] + cs["c"])
        got = _calls(e, cs, factor_each=True)
        np.testing.assert_array_equal(e.corrections(), 0)
        for k in want:
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)
        check_outputs(cs, got["fx"], got["fd"], got["rp"], got["J"], where=" (reused)")
        check_outputs(cs, got["gx"], got["gd"], got["gp"], None, where=" (reused, pair)")
    ref.close()
    e.close()


@pytest.mark.parametrize("deferred", [False, True], ids=["sync", "deferred"])
def test_corrected(deferred):
    """An inertia-corrected problem (problem 1: M exactly singular, k·1e-6·D
    added, the full M) beside reduced neighbours, through every call — in the
    deferred form each call finishes the factorisation after its right-hand
    sides were queued and forms the reduction's sides again (`redo` of
    nlp_finish_after_rhs).  Bar: 1e-6, as everywhere — the reference's own
    error on the corrected matrix (SuperLU against LAPACK, cond 3.6e6) is
    1e-11, so 1e3 × that stays below the floor."""
    cs = ec.case("corrected")
    bar = max(RTOL, 1e3 * ec.reference_discrepancy(cs, 1))
    assert bar == RTOL
    e = engine(cs, deferred=deferred)
    got = _calls(e, cs, factor_each=True)
    check_sizes(e, cs)
    assert e.corrections()[1] >= 1
    check_outputs(cs, got["fx"], got["fd"], got["rp"], got["J"], bar=bar)
    check_outputs(cs, got["gx"], got["gd"], got["gp"], None, bar=bar, where=" (pair)")
    for a, b in (("gx", "fx"), ("gd", "fd"), ("gp", "rp")):
        np.testing.assert_array_equal(got[a], got[b])
    e.close()


def test_lds_optin():
    """2·num_w + c + n > 4096: the pair kernels ask for more than the default
    64 KB of dynamic LDS (hipFuncSetAttribute), the single-vector ones do not.
    The two formulas are red_rhs's and red_recover's (nlp.hip)."""
    cs = ec.case("lds_optin")
    L = ec.layout(cs["st"])
    n, c, w = L.n, L.c, L.num_w
    for nv, more in ((1, False), (2, True)):
        rhs = nv * (2 * w + c + n) * 8 + (w + c + n + c + 2) * 4
        rec = nv * (3 * w + c) * 8 + (w + c + n + 1) * 4
        assert (rhs > 64 * 1024) == more and (rec > 64 * 1024) == more and max(rhs, rec) <= 160 * 1024
    check_case(cs)

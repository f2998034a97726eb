"""The prepare kernel's batch summary (QPSummary: the last workgroup to finish
reduces every problem's metadata to the four numbers the host sizes the
factorisation from and writes them to pinned memory) against the copy of
every QPMeta it replaces (DOPT_QP_SUMMARY=0).

One handle is taken through five models whose sizes and routes differ —
padded N'max 96, grown to 160, shrunk to one 64-block (one diagonal launch,
no column launch), a batch with a Q = 0 problem (LSQR branch: the assembly
tiles are launched) and an asymmetric Q (rejected at the first diagonal
launch), no active row at all — so every call sizes its launches from its own
summary, never from the call before.  After each model the fused call's
outputs, info, system_size, lu_kind and sym_route are bit-equal to a fresh
handle's and to the copy path's, and meet the oracle at test_qp_gpu's bar.
Batch 12: above the small path's limit."""
import os

import numpy as np
import pytest

from reuse_cases import LSQR, NOPIV, PIVOT, indefinite, qp_kept
from oracle import qp as oqp

pytestmark = pytest.mark.gpu

RTOL = 1e-6   # relative Frobenius (test_qp_gpu.RTOL)
B, N, M, P = 12, 50, 110, 0
KEYS = ("Q", "G", "h", "A", "z", "lam", "nu")


def relfro(a, b):
    nb = np.linalg.norm(b)
    return np.linalg.norm(np.asarray(a) - b) / (nb if nb > 0 else 1.0)


def _model(active, extra, seed):
    return qp_kept(B, N, M, P, (active + 0.5) / M, seed, extra)


def _sets():
    mixed = _model(20, 20, 9104)
    mixed["Q"][3] = 0.0
    mixed["Q"][7] = mixed["Q"][7] + 1e-3 * np.triu(np.random.default_rng(3).standard_normal((N, N)), 1)
    kinds4 = [NOPIV] * B
    kinds4[3], kinds4[7] = LSQR, PIVOT
    # (name, data, N' of the LU problems, lu_kind)
    return [
        ("npmax 96", _model(20, 20, 9101), 90, [NOPIV] * B),
        ("grown to 160", indefinite(_model(20, 80, 9102), [5]), 150, [NOPIV] * 5 + [PIVOT] + [NOPIV] * 6),
        ("one 64-block", _model(10, 0, 9103), 60, [NOPIV] * B),
        ("Q = 0 and asymmetric Q", mixed, 90, kinds4),
        ("no active row", _model(0, 0, 9105), 50, [NOPIV] * B),
    ]


def _run(e, d):
    e.set(*(d[k] for k in KEYS))
    rev, fwd = e.forward_reverse(d["dl_dz"], dq=d["dq"], dh=d["dh"], db=d["db"])
    out = dict(rev=np.array(rev), fwd=np.array(fwd), info=e.info(), size=e.system_size(), kind=e.lu_kind(),
               sym=e.sym_route())
    # the split API: qp_factor sizes its launches the same way
    e.factor()
    out["rev_split"] = np.array(e.reverse(d["dl_dz"]))
    return out


@pytest.fixture(scope="module")
def runs():
    """Per set: the reused handle's results under the summary and under the
    copy path, and a fresh handle's (summary)."""
    from diffopt_amd.qp import QPBatch
    sets = _sets()
    res = {"sets": sets}
    old = os.environ.get("DOPT_QP_SUMMARY")
    try:
        for mode in ("1", "0"):
            os.environ["DOPT_QP_SUMMARY"] = mode   # read by dopt_create
            e = QPBatch(B, N, M, P)
            res[mode] = [_run(e, d) for _, d, _, _ in sets]
            e.close()
        os.environ["DOPT_QP_SUMMARY"] = "1"
        res["fresh"] = []
        for _, d, _, _ in sets:
            e = QPBatch(B, N, M, P)
            res["fresh"].append(_run(e, d))
            e.close()
    finally:
        if old is None:
            os.environ.pop("DOPT_QP_SUMMARY", None)
        else:
            os.environ["DOPT_QP_SUMMARY"] = old
    return res


@pytest.mark.parametrize("i", range(5), ids=["npmax96", "grown160", "shrunk64", "lsqr_asym", "no_active"])
def test_reused_handle_matches_fresh_handle_and_copy_path(runs, i):
    got = runs["1"][i]
    for other in ("fresh", "0"):
        for k, v in runs[other][i].items():
            np.testing.assert_array_equal(got[k], v, err_msg=f"{k} vs {other}")


@pytest.mark.parametrize("i", range(5), ids=["npmax96", "grown160", "shrunk64", "lsqr_asym", "no_active"])
def test_every_set_meets_the_oracle(runs, i):
    _, d, nsys, kinds = runs["sets"][i]
    got = runs["1"][i]
    np.testing.assert_array_equal(got["kind"], kinds)
    np.testing.assert_array_equal(got["info"], 0)
    for b in range(B):
        it = kinds[b] == LSQR
        assert got["size"][b] == (N + M + P if it else nsys)
        assert got["sym"][b] == (kinds[b] == NOPIV)
        args = [d[k][b] for k in KEYS]
        ref = np.concatenate(oqp.reverse_differentiate(*args, d["dl_dz"][b]))
        err = relfro(got["rev"][b], ref)
        print(f"set {i} problem {b} reverse relfro {err:.3e}")
        assert err <= RTOL
        assert relfro(got["rev_split"][b], ref) <= RTOL
        if it:   # the LSQR branch is held on reverse (reuse_cases.qp_oracle)
            continue
        ref = np.concatenate(oqp.forward_differentiate(*args, dq=d["dq"][b], dh=d["dh"][b], db=d["db"][b]))
        err = relfro(got["fwd"][b], ref)
        print(f"set {i} problem {b} forward relfro {err:.3e}")
        assert err <= RTOL

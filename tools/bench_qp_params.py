#!/usr/bin/env python3
"""Forward-mode parameter Jacobian of a batch of QPs on the config-2 shape
(n = 200, m = 300, 1024 problems, host arrays, one factorisation kept):

  loop      what a caller can do with the entry points that predate
            dopt_qp_params_forward_k: per parameter a unit dp through
            dopt_qp_params_forward, the resulting dq / dh packed seed-major in
            numpy, then ONE dopt_qp_forward_k on the nparam seeds (which
            launches its right-hand-side kernel once per seed on the dense
            vector tangents)
  jacobian  one dopt_qp_params_forward_k call with dp = NULL

Two term tables, per parameter: `obj` eight LessThan-row terms and two
objective parameter×variable terms (kinds 0 and 3), and `con` those plus two
constraint parameter×variable terms (kind 4).  Only `obj` has a loop side: a
kind-4 term has no route through the older entry points short of a dense dG
(m·n·B·k doubles).

Both sides are warmed, then timed alternately `--reps` times with an untimed
`--settle` wait before every timed call (the loop hands freshly allocated
numpy arrays to the engine, after which the HIP runtime stays busy for a while:
DESIGN.md §6); host clock around calls that return with their outputs copied
back.  The medians are compared and every repeat is reported.  A second,
untimed pass with per-phase HIP events gives the right-hand-side phase of each
side on its own (qp_rhs as [ms, phase brackets]: one bracket holds all of a
call's right-hand-side launches; events slow the host, so that pass is not the
timed one).  The Jacobian is checked against the loop's blocks at the engine-vs-
engine bar 1e-10 (relative Frobenius, worst problem and seed).  One JSON line
per variant and nparam.

  python tools/bench_qp_params.py [--batch 1024] [--nparam 4 16 64] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffopt.jl_amd"))


def make_terms(nparam, n, m, seed, constraint_pv):
    import numpy as np
    rng = np.random.default_rng(seed)
    terms = []
    for p in range(nparam):
        terms += [(p, 0, int(rng.integers(m)), float(rng.standard_normal())) for _ in range(8)]
        terms += [(p, 3, int(rng.integers(n)), float(rng.standard_normal())) for _ in range(2)]
        if constraint_pv:
            terms += [(p, 4, int(rng.integers(m)), float(rng.standard_normal()), int(rng.integers(n)))
                      for _ in range(2)]
    return terms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--nparam", type=int, nargs="+", default=[4, 16, 64])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--settle", type=float, default=0.05, help="untimed wait before every timed call, seconds")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    import numpy as np
    from diffopt_amd.qp import QPBatch
    from diffopt_amd.synthetic import QP_CONFIGS, qp_config_numpy
    c = QP_CONFIGS[2]
    B, n, m, p = a.batch, c["n"], c["m"], c["p"]
    d = qp_config_numpy(2, batch=B)
    e = QPBatch(B, n, m, p)
    e.set(d["Q"], d["G"], d["h"], d["A"], d["z"], d["lam"], d["nu"])
    e.factor()

    def timed(fn):
        time.sleep(a.settle)
        t0 = time.perf_counter()
        r = fn()   # host arrays: every call returns with its outputs copied back
        return time.perf_counter() - t0, r

    def rhs_phase(fn):
        e.set_profiling(True, phases=["qp_rhs"])
        e.phase_times()
        fn()
        ms, launches = e.phase_times().get("qp_rhs", (0.0, 0))
        e.set_profiling(False)
        return round(ms, 4), launches

    for nparam in a.nparam:
        for variant in ("obj", "con"):
            terms = make_terms(nparam, n, m, 11, variant == "con")

            def loop():
                dq, dh = np.empty((nparam, B, n)), np.empty((nparam, B, m))
                for j in range(nparam):
                    dp = np.zeros((B, nparam))
                    dp[:, j] = 1.0
                    q, h_, _ = e.params_forward(dp, terms)
                    dq[j], dh[j] = q, h_
                return e.forward_k(dq=dq, dh=dh)

            def jac():
                return e.params_jacobian(terms, nparam, 0)   # a (B, n+m+p, nparam) view of the seed-major buffer

            has_loop = variant == "obj"
            for _ in range(a.warmup):
                ref = loop() if has_loop else None
                J = jac()
            tl, tj = [], []
            for _ in range(a.reps):
                if has_loop:
                    tl.append(timed(loop)[0])
                tj.append(timed(jac)[0])
            ms = lambda ts: [round(1e3 * t, 3) for t in ts]
            mj = statistics.median(tj)
            rec = {"config": f"config 2 (n={n}, m={m}, p={p}), factor kept, host arrays", "batch": B,
                   "variant": variant, "nparam": nparam, "nterms": len(terms), "settle_s": a.settle,
                   "jacobian_ms": round(1e3 * mj, 3), "jacobian_ms_reps": ms(tj),
                   "jacobian_rhs_ms_launches": rhs_phase(jac)}
            if has_loop:
                ml = statistics.median(tl)
                Jk = np.transpose(np.asarray(J), (2, 0, 1))   # (nparam, B, L) as forward_k's
                num = np.linalg.norm(Jk - ref, axis=2)
                den = np.linalg.norm(ref, axis=2)
                worst = float(np.max(num / np.where(den > 0, den, 1.0)))
                rec.update({"loop_ms": round(1e3 * ml, 3), "loop_ms_reps": ms(tl), "speedup": round(ml / mj, 3),
                            "loop_rhs_ms_launches": rhs_phase(loop), "worst_relfro_vs_loop": worst,
                            "within_1e-10": bool(worst <= 1e-10)})
            else:
                rec.update({"loop_ms": None, "note": "no loop side: kind 4 has no route through the older entries"})
            line = json.dumps(rec)
            print(line, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(line + "\n")
    e.close()


if __name__ == "__main__":
    main()

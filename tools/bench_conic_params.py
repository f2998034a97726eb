#!/usr/bin/env python3
"""Parameter Jacobian of a batch of cone programs, forward mode, on the
config-4 shape (n = 500, 20 × SOC(25), 512 problems, host arrays, one
factorisation, LSQR capped at 50 iterations as the multi-seed line):

  loop      what a caller could do before dopt_conic_params_jacobian: per
            parameter, db / dc built in numpy from the term table, one
            dopt_conic_forward call, its dx kept (nparam calls)
  jacobian  one dopt_conic_params_jacobian call (mode 0)

The loop uses only entry points that predate the Jacobian call, whose kernels
this call leaves untouched.  Both sides are warmed twice, then timed
alternately `--reps` times; the medians are compared and every repeat is
reported.  Before each timed call the host waits `--settle` seconds (default
0.05; untimed, both sides alike): the loop hands freshly allocated numpy
arrays to the engine, and for 10–25 ms after it returns the HIP runtime is
still busy with them, which stalls whichever engine call comes next, however
small.  `--settle 0` shows that stall on the Jacobian side.
The Jacobian is checked bitwise against the loop's columns.  One JSON line
per route and nparam.

  python tools/bench_conic_params.py [--batch 512] [--nparam 4 16] [--routes persistent split] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffopt.jl_amd"))


def make_terms(nparam, n, m, seed):
    """Per parameter eight constraint-row terms and two objective parameter×variable terms."""
    import numpy as np
    rng = np.random.default_rng(seed)
    terms = []
    for p in range(nparam):
        terms += [(p, 0, int(rng.integers(m)), float(rng.standard_normal())) for _ in range(8)]
        terms += [(p, 3, int(rng.integers(n)), float(rng.standard_normal())) for _ in range(2)]
    return terms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--nparam", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--settle", type=float, default=0.05, help="untimed wait before every timed call, seconds")
    ap.add_argument("--cap", type=int, default=50, help="LSQR iteration cap (0: the default maxiter)")
    ap.add_argument("--routes", nargs="+", default=["persistent", "split"], choices=["persistent", "split"])
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    import numpy as np
    from diffopt_amd.conic import ConicBatch
    from diffopt_amd.synthetic import CONIC_CONFIGS, SEED0, conic_numpy
    c = CONIC_CONFIGS[4]
    B, n, cones = a.batch, c["n"], c["cones"]
    m = sum(dim for _, dim in cones)
    d = conic_numpy(B, n, cones, SEED0 + 4)

    def timed(fn):
        time.sleep(a.settle)
        t0 = time.perf_counter()
        r = fn()   # host arrays: every call returns with its outputs copied back
        return time.perf_counter() - t0, r

    for route in a.routes:
        os.environ["DOPT_CONIC_SPLIT"] = "1" if route == "split" else "0"   # read when the handle is created
        e = ConicBatch(B, n, cones)
        e.set(d["A"], d["b"], d["c"], d["x"], d["s"], d["y"])
        e.factor()
        e.set_maxiter(a.cap)
        for nparam in a.nparam:
            terms = make_terms(nparam, n, m, 11)

            def loop():
                cols = []
                for j in range(nparam):
                    db, dc = np.zeros((B, m)), np.zeros((B, n))
                    for (p, kind, idx, coef) in terms:
                        if p == j and kind == 0:
                            db[:, idx] += coef
                        elif p == j and kind == 3:
                            dc[:, idx] += coef
                    cols.append(np.array(e.forward(None, db, dc)[1]))
                return np.stack(cols, axis=2)

            def jac():
                return e.params_jacobian(terms, nparam, 0)

            for _ in range(a.warmup):
                ref = loop()
                J, st = jac()
            tl, tj = [], []
            for _ in range(a.reps):
                tl.append(timed(loop)[0])
                tj.append(timed(jac)[0])
            ml, mj = statistics.median(tl), statistics.median(tj)
            ms = lambda ts: [round(1e3 * t, 3) for t in ts]
            line = json.dumps({"config": f"config 4 (n={n}, m={m}, 20 x SOC(25)), factor kept, host arrays",
                               "batch": B, "route": route, "settle_s": a.settle, "maxiter": a.cap or n + m + 1, "nparam": nparam,
                               "iterations_mean": round(float(st["iterations"].mean()), 1),
                               "loop_ms": round(1e3 * ml, 3), "jacobian_ms": round(1e3 * mj, 3),
                               "loop_ms_reps": ms(tl), "jacobian_ms_reps": ms(tj),
                               "speedup": round(ml / mj, 3), "bitwise": bool(np.array_equal(ref, J))})
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")
        e.close()


if __name__ == "__main__":
    main()

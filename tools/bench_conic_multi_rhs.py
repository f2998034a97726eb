#!/usr/bin/env python3
"""Conic multi-seed timing on the config-4 shape (n = 500, 20 × SOC(25),
device-resident inputs, one factorisation): k single-seed dopt_conic_reverse /
_forward calls against one dopt_conic_reverse_k / _forward_k call
(conic_lsqrk_kernel: groups of seeds share each sweep over A).  Two regimes:
LSQR capped at 50 iterations (dopt_conic_set_maxiter) and the default maxiter.
The loop and the k-call are timed alternately, `--reps` times each after one
warm-up of both; every repeat is reported (the run-to-run spread), the best
one is compared.  The k-call's outputs are checked bitwise against the loop's.
Prints one JSON line per regime and k.

  python tools/bench_conic_multi_rhs.py [--batch 512] [--k 1 4 8 16] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffopt.jl_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--k", type=int, nargs="+", default=[1, 4, 8, 16])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cap", type=int, default=50, help="iteration cap of the capped regime")
    ap.add_argument("--regimes", nargs="+", default=["capped", "default"], choices=["capped", "default"])
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    import torch
    from diffopt_amd.conic import ConicBatch
    from diffopt_amd.synthetic import CONIC_CONFIGS, SEED0, conic_numpy
    c = CONIC_CONFIGS[4]
    B, n, cones = a.batch, c["n"], c["cones"]
    m = sum(dim for _, dim in cones)
    d = conic_numpy(B, n, cones, SEED0 + 4)
    dev = {k: torch.from_numpy(d[k]).cuda() for k in ["A", "b", "c", "x", "s", "y"]}
    del d
    e = ConicBatch(B, n, cones)
    e.set(dev["A"], dev["b"], dev["c"], dev["x"], dev["s"], dev["y"])
    e.factor()
    g = torch.Generator(device="cuda")
    g.manual_seed(7)

    def once(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    def pair(loop, multi, same):
        """Both forms warmed once, then timed alternately; (loop times, k-call
        times, outputs bitwise equal)."""
        _, rl = once(loop)
        _, rk = once(multi)
        ok = same(rl, rk)
        del rl, rk
        tl, tk = [], []
        for _ in range(a.reps):
            tl.append(once(loop)[0])
            tk.append(once(multi)[0])
        return tl, tk, ok

    def side(tl, tk, k, ok):
        ms = lambda ts: [round(1e3 * t, 3) for t in ts]
        return {"loop_ms": round(1e3 * min(tl), 3), "k_ms": round(1e3 * min(tk), 3), "loop_ms_reps": ms(tl),
                "k_ms_reps": ms(tk), "seed_solves_per_s": round(k * B / min(tk), 1),
                "speedup": round(min(tl) / min(tk), 3), "bitwise": bool(ok)}

    for regime in a.regimes:
        e.set_maxiter(a.cap if regime == "capped" else 0)
        for k in a.k:
            dx = torch.randn(k, B, n, generator=g, device="cuda", dtype=torch.float64)
            db = torch.randn(k, B, m, generator=g, device="cuda", dtype=torch.float64)
            dc = torch.randn(k, B, n, generator=g, device="cuda", dtype=torch.float64)
            rl, rk, rok = pair(lambda: [e.reverse(dx[j], want_dA=False) for j in range(k)],
                               lambda: e.reverse_k(dx, want_dA=False),
                               lambda lo, mu: all(torch.equal(lo[j][i], mu[i][j]) for j in range(k) for i in (0, 2, 3)))
            it = e.lsqr_stats_k(k)["iterations"]
            fl, fk, fok = pair(lambda: [e.forward(db=db[j], dc=dc[j]) for j in range(k)],
                               lambda: e.forward_k(db=db, dc=dc),
                               lambda lo, mu: all(torch.equal(lo[j][i], mu[i][j]) for j in range(k) for i in (0, 1)))
            loop, multi = min(rl) + min(fl), min(rk) + min(fk)
            line = json.dumps({"config": f"config 4 (n={n}, m={m}, 20 x SOC(25)), factor kept", "batch": B,
                               "regime": regime, "maxiter": a.cap if regime == "capped" else n + m + 1, "k": k,
                               "reverse_iterations_mean": round(float(it.mean()), 1),
                               "reverse": side(rl, rk, k, rok), "forward": side(fl, fk, k, fok),
                               "loop_ms": round(1e3 * loop, 3), "k_ms": round(1e3 * multi, 3),
                               "seed_solves_per_s": round(2 * k * B / multi, 1), "speedup": round(loop / multi, 3)})
            print(line, flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Timing of the QP reverse mode with seeds on the duals at the config-2 shape
(device-resident inputs, factors kept), ms per call:
  (a) dopt_qp_reverse_k — on another build of the library with --base-lib
      (the commit before the dual seeds), else on the in-tree one,
  (b) dopt_qp_reverse_duals_k with the dual seeds NULL,
  (c) dopt_qp_reverse_duals_k with all three seed blocks dense.
The sides alternate call by call; warm-up calls first, then the median of
--reps timed calls each, then one profiled call each for the qp_rhs /
qp_solve / qp_output phase times.  One JSON line per k.

  python tools/bench_qp_dual_seeds.py [--batch 1024] [--k 16 32] [--base-lib PATH]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "diffopt.jl_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--k", type=int, nargs="+", default=[16, 32])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--base-lib", default=None)
    a = ap.parse_args()
    import torch
    from diffopt_amd import _lib
    from diffopt_amd.qp import QPBatch
    from diffopt_amd.synthetic import QP_CONFIGS, SEED0, qp_torch
    c = QP_CONFIGS[2]
    B, n, m, p = a.batch, c["n"], c["m"], c["p"]
    d = qp_torch(B, n, m, p, c["phi"], SEED0 + 2)

    def engine(lib=None):
        e = QPBatch(B, n, m, p)
        if lib is not None:   # the same wrapper on the other build's handle
            e.close()
            e.lib = lib
            h = ctypes.c_void_p()
            assert lib.dopt_create(ctypes.byref(h), 0, B, n, m, p, _lib.DOPT_KIND_QP) == 0
            e.h = h
        e.set(d["Q"], d["G"], d["h"], d["A"], d["z"], d["lam"], d["nu"])
        e.factor()
        return e

    new = engine()
    base = new
    if a.base_lib:
        lib = ctypes.CDLL(a.base_lib)
        for name, (res, args) in _lib.SIGNATURES.items():
            if hasattr(lib, name):
                getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
        base = engine(lib)
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    for k in a.k:
        gz = torch.randn(k, B, n, generator=g, device="cuda", dtype=torch.float64)
        gl = torch.randn(k, B, m, generator=g, device="cuda", dtype=torch.float64)
        sides = {"a_reverse_k": lambda: base.reverse_k(gz),
                 "b_duals_null": lambda: new.reverse_duals_k(gz),
                 "c_duals_dense": lambda: new.reverse_duals_k(gz, gl, None)}   # (p = 0: no ν block)
        for _ in range(a.warmup):
            for fn in sides.values():
                fn()
        torch.cuda.synchronize()
        times = {s: [] for s in sides}
        for _ in range(a.reps):
            for s, fn in sides.items():
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[s].append(1e3 * (time.perf_counter() - t0))
        phases = {}
        for s, fn in sides.items():
            e = base if s == "a_reverse_k" else new
            e.set_profiling(True)
            e.phase_times()
            fn()
            pt = _lib.phase_times(e.lib, e.h)
            e.set_profiling(False)
            phases[s] = {ph: round(pt[ph][0], 3) for ph in ("qp_rhs", "qp_solve", "qp_output") if ph in pt}
        print(json.dumps({"config": f"config 2 (n={n}, m={m}), factors kept, device memory", "batch": B, "k": k,
                          "base_lib": "other build" if a.base_lib else "in-tree", "reps": a.reps,
                          "ms_median": {s: round(statistics.median(v), 3) for s, v in times.items()},
                          "ms_min": {s: round(min(v), 3) for s, v in times.items()},
                          "ms_max": {s: round(max(v), 3) for s, v in times.items()},
                          "phase_ms": phases}), flush=True)


if __name__ == "__main__":
    main()

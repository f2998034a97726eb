#!/usr/bin/env python
"""The sparse split route (dopt_set_sparse(h, 2)) against what it replaces.

One "call" is ConicBatch.forward_reverse with vector tangents (db, dc, dx; no
matrix tangent, no matrix gradient) on host arrays: two LSQR runs per problem.

  --case config8   bench.py's config-8 shape (sparse conic programs, every PSD
                   side ≤ 64) at --batch problems:
                     --mode 1      the one-workgroup sparse route (reference:
                                   run it on a build of the parent commit)
                     --mode split  the sparse split route (this build)
  --case psd100    a sparse program with --psd-blocks PSD(100) cones, --nonneg
                   non-negative rows and --n variables, ≈ --k entries per row
                   (conic_numpy_wellcond, sparse_k):
                     --mode dense  the dense split route on the densified
                                   problem (set_csc on a dense-route handle
                                   densifies on the device; reference: parent
                                   build).  on = 1 refuses this cone list.
                     --mode split  the sparse split route (this build)

--tree names the built checkout to import diffopt_amd and bench.py from (the
reference sides: a checkout of the parent commit); --lib an engine build to
load instead of the tree's own (DOPT_LIB: kernel variants of this tree).

Per side it prints one JSON line: per-call time (median over --runs runs of
--reps calls each, with min and max; host clock around calls that return
after a stream synchronise), the LSQR iteration counts of the last call, and
dopt_live_device_bytes with the handle alive after its calls.  Append the
lines of both sides to one file under profiles/sparse_split/ and alternate
the sides in one job, so that both see the same machine."""

import argparse
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--case", choices=["config8", "psd100"], required=True)
    ap.add_argument("--mode", choices=["1", "split", "dense"], required=True)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--lib", default=None, help="engine build to load instead of the tree's (sets DOPT_LIB)")
    ap.add_argument("--build", default=None, help="label of the build in the output line (default: the tree's path)")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--n", type=int, default=10000, help="psd100: variables")
    ap.add_argument("--psd-blocks", type=int, default=2, help="psd100: PSD(100) cones")
    ap.add_argument("--nonneg", type=int, default=400, help="psd100: rows of the non-negative cone")
    ap.add_argument("--k", type=int, default=5, help="psd100: entries per row of A_moi")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="append the JSON line to this file as well")
    args = ap.parse_args()
    if args.mode not in {"config8": ("1", "split"), "psd100": ("dense", "split")}[args.case]:
        ap.error("config8 takes --mode 1 or split; psd100 takes --mode dense or split (on = 1 refuses its PSD sides)")
    tree = os.path.abspath(args.tree)
    sys.path[:0] = [tree, os.path.join(tree, "diffopt.jl_amd")]
    if args.lib:
        os.environ["DOPT_LIB"] = os.path.abspath(args.lib)
    if args.mode == "dense":
        os.environ["DOPT_CONIC_SPLIT"] = "1"

    import numpy as np
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    import bench
    from diffopt_amd import _lib
    from diffopt_amd import synthetic as syn
    from diffopt_amd.conic import ConicBatch
    B = args.batch
    if args.case == "config8":
        c = bench.SPARSE_CFG[8]
        n, cones, k = c["n"], c["cones"], c["k"]
        seed = bench.SEED0_SPARSE + 8
    else:
        n, k = args.n, args.k
        cones = [(4, 100 * 101 // 2)] * args.psd_blocks + [(1, args.nonneg)]
        seed = bench.SEED0_SPARSE + 100
    m = sum(dim for _, dim in cones)
    d = syn.conic_numpy_wellcond(B, n, cones, seed, pair_norm=1.0, sparse_k=k, sparse_out=True)
    nnz = sum(M.nnz for M in d["A"])
    live = _lib.load().dopt_live_device_bytes
    live0 = int(live())
    sparse = {"1": True, "split": "split", "dense": False}[args.mode]
    eng = ConicBatch(B, n, cones, sparse=sparse)
    eng.set_csc(d["A"], d["b"], d["c"], d["x"], d["s"], d["y"])

    def call():
        return eng.forward_reverse(d["dx"], db=d["db"], dc=d["dc"], want_dA=False)

    def timed(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            last = call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3, last

    for _ in range(args.warmup):
        call()
    runs = []
    for _ in range(args.runs):
        ms, last = timed(args.reps)
        runs.append(ms)
    st = eng.lsqr_stats()
    held = int(live()) - live0
    line = {
        "tool": "bench_sparse_split", "case": args.case, "mode": args.mode, "build": args.build or args.lib or tree,
        "shape": dict(n=n, m=m, cones=len(cones), max_psd_side=max([0] + [int((8 * dim + 1) ** 0.5 - 1) // 2
                                                                         for code, dim in cones if code == 4])),
        "batch": B, "nnz_per_problem": nnz / B, "dense_matrix_bytes_per_batch": 8 * B * m * n,
        "call": "forward_reverse(db, dc, dx), host arrays, no matrix tangent or gradient",
        "ms_per_call_median": round(statistics.median(runs), 4), "ms_per_call_min": round(min(runs), 4),
        "ms_per_call_max": round(max(runs), 4), "ms_per_call_runs": [round(v, 4) for v in runs],
        "runs": args.runs, "reps_per_run": args.reps, "warmup_calls": args.warmup,
        "lsqr_iterations": {key: [int(st[key].min()), int(st[key].max())] for key in ("iterations", "fwd_iterations")},
        "lsqr_istop": sorted(set(int(v) for key in ("istop", "fwd_istop") for v in st[key])),
        "live_device_bytes": held,
    }
    del last
    eng.close()
    s = json.dumps(line)
    print(s, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()

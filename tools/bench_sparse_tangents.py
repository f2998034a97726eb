#!/usr/bin/env python
"""Matrix tangents and matrix gradients on the sparse route, dense against sparse.

At bench.py's config-7 shape (sparse LPs above the dense cap) and config-8
shape (sparse conic programs) — both read from bench.py's SPARSE_CFG — with a
small batch and a tangent on the model's own pattern, one "call" is a forward
+ reverse solve with a matrix tangent in and the matrix gradient out:

  --side dense   the dense-tangent call plus the dense gradient
                 (ConicBatch.forward_reverse(dA=dense, want_dA=True);
                 QPBatch.forward_reverse(dG=dense, dA=dense) + reverse_grads),
                 device tensors.  This side uses only calls that predate the
                 `_csc` entries, so it runs on a build of the parent commit:
                 --tree names that checkout (built).
  --side csc     the `_csc` call plus reverse_grads_at (scipy-sparse tangents,
                 host arrays), on this tree.

Per side it prints one JSON line: the per-call time (median over --runs runs of
--reps calls each, with min and max; host clock around calls that end in a
device synchronise), the right-hand-side and output phase times per call
(dopt_get_phase_times, from a separate profiled pass), and the device memory
the side holds after its calls (torch.cuda.mem_get_info before the handle
exists minus after the last call, results alive).  Append the lines of both
sides to one file under profiles/sparse_tangents/ and alternate the sides in
one job, so that both see the same machine."""

import argparse
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--side", choices=["dense", "csc"], required=True)
    ap.add_argument("--config", type=int, choices=[7, 8], required=True)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="repository root to import diffopt_amd and bench.py from (dense side: a built checkout of "
                         "the parent commit)")
    ap.add_argument("--build", default=None, help="label of the build in the output line (default: the tree's path)")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="append the JSON line to this file as well")
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path[:0] = [tree, os.path.join(tree, "diffopt.jl_amd")]

    import numpy as np
    import scipy.sparse as sp
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    import bench
    from diffopt_amd import synthetic as syn
    c = bench.SPARSE_CFG[args.config]
    B = args.batch
    seed = bench.SEED0_SPARSE + args.config
    rng = np.random.default_rng(seed + 1)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")

    def on_pattern(mats):      # a tangent on the model's own pattern, random values
        out = []
        for M in mats:
            M = sp.csc_matrix(M, copy=True)
            M.data = rng.standard_normal(M.nnz)
            out.append(M)
        return out

    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    if args.config == 7:
        from diffopt_amd.qp import QPBatch
        n, p = c["n"], c["p"]
        d = syn.lp_sparse_numpy(B, n, p, c["m_extra"], c["k"], seed)
        m = d["lam"].shape[1]
        dG, dA = on_pattern(d["G"]), on_pattern(d["A"])
        nnz = sum(M.nnz for M in dG) + sum(M.nnz for M in dA)
        eng = QPBatch(B, n, m, p)
        eng.set_csc([sp.csc_matrix((n, n))] * B, d["G"], d["h"], d["A"], d["z"], d["lam"], d["nu"])
        phases = ["qp_rhs", "qp_output"]
        shape = dict(n=n, m=m, p=p)
        dense_bytes = 8 * B * (m + p) * n
        if args.side == "dense":
            dl, dq, dh, db = t(d["dl_dz"]), t(d["dq"]), t(d["dh"]), t(d["db"])
            tG = torch.stack([t(M.toarray()) for M in dG])
            tA = torch.stack([t(M.toarray()) for M in dA])

            def call():
                rev, fwd = eng.forward_reverse(dl, dq=dq, dG=tG, dh=dh, dA=tA, db=db)
                return rev, fwd, eng.reverse_grads(rev, dQ=False)
        else:
            def call():
                rev, fwd = eng.forward_reverse(d["dl_dz"], dq=d["dq"], dG=dG, dh=d["dh"], dA=dA, db=d["db"])
                return rev, fwd, eng.reverse_grads_at(rev)
    else:
        from diffopt_amd.conic import ConicBatch
        n, cones = c["n"], c["cones"]
        d = syn.conic_numpy_wellcond(B, n, cones, seed, pair_norm=1.0, sparse_k=c["k"], sparse_out=True)
        m = sum(dim for _, dim in cones)
        dA = on_pattern(d["A"])
        nnz = sum(M.nnz for M in dA)
        eng = ConicBatch(B, n, cones, sparse=True)
        eng.set_csc(d["A"], d["b"], d["c"], d["x"], d["s"], d["y"])
        phases = ["conic_rhs", "conic_output"]
        shape = dict(n=n, m=m)
        dense_bytes = 8 * B * m * n
        if args.side == "dense":
            dx, db, dc = t(d["dx"]), t(d["db"]), t(d["dc"])
            tA = torch.stack([t(M.toarray()) for M in dA])

            def call():
                return eng.forward_reverse(dx, dA=tA, db=db, dc=dc, want_dA=True)
        else:
            def call():
                f, r = eng.forward_reverse(d["dx"], dA=dA, db=d["db"], dc=d["dc"])
                return f, r, eng.reverse_grads_at(r[0])

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
    torch.cuda.synchronize()
    used = free0 - torch.cuda.mem_get_info()[0]
    # the phase breakdown from a pass of its own (the events cost queue time)
    eng.phase_times()
    eng.set_profiling(True, phases=phases)
    for _ in range(args.reps):
        call()
    torch.cuda.synchronize()
    pt = eng.phase_times()
    eng.set_profiling(False)
    line = {
        "tool": "bench_sparse_tangents", "side": args.side, "build": args.build or tree, "config": args.config,
        "shape": shape, "batch": B, "tangent_nnz_per_problem": nnz / B, "dense_matrix_bytes_per_batch": dense_bytes,
        "call": ("forward_reverse(dense matrix tangents) + dense matrix gradient, device tensors"
                 if args.side == "dense" else "forward_reverse(_csc tangents) + reverse_grads_at, host arrays"),
        "ms_per_call_median": round(statistics.median(runs), 4), "ms_per_call_min": round(min(runs), 4),
        "ms_per_call_max": round(max(runs), 4), "ms_per_call_runs": [round(v, 4) for v in runs],
        "runs": args.runs, "reps_per_run": args.reps, "warmup_calls": args.warmup,
        "phase_ms_per_call": {k: round(pt[k][0] / args.reps, 4) for k in phases if k in pt},
        "device_memory_held_bytes": int(used),
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

"""Diffusion gates for many queries on config 3 (N = 100 000, D = 768, k = 32) and on 20 000 x 128:
microseconds per query of `diffusion_gates_many` for Q in {1, 32, 256} and both methods, against the per-query loop
`compute_diffusion_gates(Y, psis[q], lattice=lat)` timed in the same process, with the iterations per query.

    python scripts/bench_gates_many.py [--reps 5 --loop-queries 16 --out profiles/gates_many.json]
    python scripts/bench_gates_many.py --shapes 20000x128x32    # one shape (N x D x k)
    python scripts/bench_gates_many.py --shapes 100000x768x32 --profile-q 256 --profile-method cg   # the run to put under
                                                                # rocprofv3 --kernel-trace --stats: the batch alone

One JSON line per shape."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run_shape(N, D, k, reps, loop_queries, gamma, profile_q=0, profile_method="cg"):
    from oscillink_amd import Oscillink, compute_diffusion_gates

    rng = np.random.default_rng(0)
    Y = rng.standard_normal((N, D)).astype(np.float32)
    t0 = time.perf_counter()
    lat = Oscillink(Y, kneighbors=k, deterministic_k=True)
    create_ms = 1e3 * (time.perf_counter() - t0)
    P = rng.standard_normal((256, D)).astype(np.float32)
    P[::4] = Y[rng.integers(0, N, 64)] + 0.1 * rng.standard_normal((64, D)).astype(np.float32)  # some queries near anchors
    rec = {"N": N, "D": D, "k": k, "gamma": gamma, "create_ms": create_ms, "reordered": lat.build_info()["reordered"],
           "nnz": int(lat.graph_stats()[0])}
    for method in ((profile_method,) if profile_q else ("direct", "cg")):
        kw = dict(gamma=gamma, method=method, tol=1e-4, max_iters=256)
        out = {}
        for Q in ((profile_q,) if profile_q else (1, 32, 256)):
            res = lat.diffusion_gates_many(P[:Q], **kw)  # warm-up: scratch, the normalised anchors
            ts = []
            for _ in range(reps):
                t = time.perf_counter()
                res = lat.diffusion_gates_many(P[:Q], **kw)
                ts.append(time.perf_counter() - t)
            med = float(np.median(ts))
            it = res["iters"]
            out[str(Q)] = {"batch_ms": 1e3 * med, "min_ms": 1e3 * min(ts), "per_query_us": 1e6 * med / Q,
                           "iters_mean": float(it.mean()), "iters_min": int(it.min()), "iters_max": int(it.max())}
        if profile_q:
            rec[method] = out
            continue
        nl = min(loop_queries, 256)
        compute_diffusion_gates(Y, P[0], lattice=lat, **kw)  # warm-up
        ts, worst = [], 0.0
        for q in range(nl):
            t = time.perf_counter()
            g = compute_diffusion_gates(Y, P[q], lattice=lat, **kw)
            ts.append(time.perf_counter() - t)
            worst = max(worst, float(np.abs(g - res["gates"][q]).max()))
        per = float(np.median(ts))
        out["loop"] = {"queries": nl, "per_query_us": 1e6 * per, "mean_us": 1e6 * float(np.mean(ts)),
                       "max_abs_diff_to_batch": worst}
        out["loop_over_batch_q256"] = 1e6 * per / out["256"]["per_query_us"]
        out["loop_over_batch_q1"] = 1e6 * per / out["1"]["per_query_us"]
        rec[method] = out
    lat.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="100000x768x32,20000x128x32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-queries", type=int, default=16)
    ap.add_argument("--gamma", type=float, default=0.1)
    ap.add_argument("--profile-q", type=int, default=0, help="only time the batch at this Q (for a profiler run)")
    ap.add_argument("--profile-method", default="cg")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for shape in a.shapes.split(","):
        N, D, k = (int(x) for x in shape.split("x"))
        lines.append(json.dumps(run_shape(N, D, k, a.reps, a.loop_queries, a.gamma, a.profile_q, a.profile_method)))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

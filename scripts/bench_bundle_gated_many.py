"""Bundles under per-query gates: `bundle_gated_many(psis, gates)` for Q in {64, 256}, with given
gates and with gates="diffusion", against the per-query loop `set_query(psi, gates=g); bundle()` on the same build, timed
in the same process.  Shapes: config 2 (1200 x 128, k 16), 5000 x 768 (k 16), 20 000 x 128 (k 16) and config 3
(100 000 x 768, k 32).  Median and p10-p90 over the repeats; the loop is timed per query over its first `--loop-queries`
queries and scaled to Q.

    python scripts/bench_bundle_gated_many.py [--reps 5 --loop-queries 16 --out profiles/bundle_gated_many.json]
    python scripts/bench_bundle_gated_many.py --shapes 20000x128x16 --qs 64      # one shape (N x D x k), one Q

One JSON line per shape, each with the hash of the library's sources."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(ts):
    a = 1e3 * np.asarray(ts, dtype=np.float64)
    return {"median_ms": float(np.median(a)), "p10_ms": float(np.percentile(a, 10)), "p90_ms": float(np.percentile(a, 90))}


def run_shape(N, D, k, qs, reps, loop_queries, source_hash):
    from oscillink_amd import Oscillink

    rng = np.random.default_rng(0)
    Y = rng.standard_normal((N, D)).astype(np.float32)
    lat = Oscillink(Y, kneighbors=k, deterministic_k=True)
    Qmax = max(qs)
    P = rng.standard_normal((Qmax, D)).astype(np.float32)
    P[::4] = Y[rng.integers(0, N, (Qmax + 3) // 4)] + 0.1 * rng.standard_normal(((Qmax + 3) // 4, D)).astype(np.float32)
    G = lat.diffusion_gates_many(P)["gates"]
    rec = {"N": N, "D": D, "k": k, "reps": reps, "library": source_hash, "reordered": lat.build_info()["reordered"]}
    # the loop: per query, its first loop_queries queries, `reps` passes
    nl = min(loop_queries, Qmax)
    lat.set_query(P[0], gates=G[0])
    lat.bundle(k=8)  # warm-up
    per = []
    for _ in range(reps):
        t = time.perf_counter()
        for q in range(nl):
            lat.set_query(P[q], gates=G[q])
            lat.bundle(k=8)
        per.append((time.perf_counter() - t) / nl)
    loop = _stats(per)
    rec["loop_per_query"] = {"queries": nl, **loop, "iters_last": int(lat.last_ustar["iters"])}
    lat.set_query(P[0], gates=np.ones(N, np.float32))
    for Q in qs:
        for mode in ("given", "diffusion"):
            g = G[:Q] if mode == "given" else "diffusion"
            lat.bundle_gated_many(P[:Q], k=8, gates=g, as_arrays=True)  # warm-up: scratch, the normalised anchors
            ts = []
            for _ in range(reps):
                t = time.perf_counter()
                lat.bundle_gated_many(P[:Q], k=8, gates=g, as_arrays=True)
                ts.append(time.perf_counter() - t)
            st = _stats(ts)
            it = lat.last_bundle_gated["iters"]
            # the A/B rule of DESIGN.md section 10: a gain counts from 3 x the wider p10-p90 band on (both per query)
            band = max(st["p90_ms"] - st["p10_ms"], Q * (loop["p90_ms"] - loop["p10_ms"]))
            gain = Q * loop["median_ms"] - st["median_ms"]
            rec[f"q{Q}_{mode}"] = {**st, "per_query_us": 1e3 * st["median_ms"] / Q, "loop_ms": Q * loop["median_ms"],
                                   "loop_over_batch": Q * loop["median_ms"] / st["median_ms"],
                                   "gain_over_band": gain / band if band > 0 else float("inf"),
                                   "iters_mean": float(it.mean()), "iters_max": int(it.max()),
                                   "converged": int(lat.last_bundle_gated["converged"].sum())}
    lat.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1200x128x16,5000x768x16,20000x128x16,100000x768x32")
    ap.add_argument("--qs", default="64,256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-queries", type=int, default=16)
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="add the lines to --out instead of replacing it")
    a = ap.parse_args()
    from oscillink_amd import _build

    _build.build()
    source_hash = _build._source_hash()
    qs = [int(x) for x in a.qs.split(",")]
    lines = []
    for shape in a.shapes.split(","):
        N, D, k = (int(x) for x in shape.split("x"))
        lines.append(json.dumps(run_shape(N, D, k, qs, a.reps, a.loop_queries, source_hash)))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if a.append else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

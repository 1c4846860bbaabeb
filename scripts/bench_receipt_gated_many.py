"""Receipts under per-query gates: `receipt_gated_many(psis, gates, bundle_k=8)` for Q in
{64, 256}, light and full detail, with and without `settle`, against the per-query loop `set_query(psi, gates=g);
[settle();] receipt(); bundle(8)` on the same build, timed in the same process.  Shapes: config 2 (1200 x 128, k 16) and
20 000 x 128 (k 16).  Median and p10-p90 over the repeats; the loop is timed per query over its first `--loop-queries`
queries (every one started from U = Y) and scaled to Q.

    python scripts/bench_receipt_gated_many.py [--reps 5 --loop-queries 16 --out profiles/receipt_gated_many.json]
    python scripts/bench_receipt_gated_many.py --shapes 20000x128x16 --qs 64      # one shape (N x D x k), one Q

One JSON line per (shape, detail), each with the hash of the library's sources."""
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


def _loop(lat, P, G, nl, settle, reps):
    """per-query time of the four-call flow over the first nl queries"""
    def one(q):
        lat.reset_U(wait=False)
        lat.set_query(P[q], gates=G[q])
        if settle:
            lat.settle()
        lat.receipt()
        lat.bundle(k=8)

    one(0)  # warm-up
    per = []
    for _ in range(reps):
        t = time.perf_counter()
        for q in range(nl):
            one(q)
        per.append((time.perf_counter() - t) / nl)
    return _stats(per)


def run_shape(N, D, k, qs, reps, loop_queries, detail, source_hash):
    from oscillink_amd import Oscillink

    rng = np.random.default_rng(0)
    Y = rng.standard_normal((N, D)).astype(np.float32)
    lat = Oscillink(Y, kneighbors=k, deterministic_k=True)
    lat.set_receipt_detail(detail)
    Qmax = max(qs)
    P = rng.standard_normal((Qmax, D)).astype(np.float32)
    P[::4] = Y[rng.integers(0, N, (Qmax + 3) // 4)] + 0.1 * rng.standard_normal(((Qmax + 3) // 4, D)).astype(np.float32)
    G = lat.diffusion_gates_many(P)["gates"]
    rec = {"N": N, "D": D, "k": k, "detail": detail, "reps": reps, "library": source_hash,
           "reordered": lat.build_info()["reordered"]}
    nl = min(loop_queries, Qmax)
    for settle in (False, True):
        tag = "settle" if settle else "plain"
        loop = _loop(lat, P, G, nl, settle, reps)
        rec[f"loop_per_query_{tag}"] = {"queries": nl, **loop}
        lat.reset_U()
        lat.set_query(P[0], gates=np.ones(N, np.float32))
        for Q in qs:
            kw = dict(settle=True if settle else None, bundle_k=8, as_arrays=True)
            lat.receipt_gated_many(P[:Q], G[:Q], **kw)  # warm-up: scratch, the normalised anchors
            ts = []
            for _ in range(reps):
                t = time.perf_counter()
                lat.receipt_gated_many(P[:Q], G[:Q], **kw)
                ts.append(time.perf_counter() - t)
            st = _stats(ts)
            rep = lat.last_receipt_gated
            # the A/B rule of DESIGN.md section 10: a gain counts from 3 x the wider p10-p90 band on (both per call)
            band = max(st["p90_ms"] - st["p10_ms"], Q * (loop["p90_ms"] - loop["p10_ms"]))
            gain = Q * loop["median_ms"] - st["median_ms"]
            rec[f"q{Q}_{tag}"] = {**st, "per_query_us": 1e3 * st["median_ms"] / Q, "loop_ms": Q * loop["median_ms"],
                                  "loop_over_batch": Q * loop["median_ms"] / st["median_ms"],
                                  "gain_over_band": gain / band if band > 0 else float("inf"),
                                  "ustar_iters_mean": float(rep["iters"].mean()), "ustar_iters_max": int(rep["iters"].max()),
                                  "converged": int(rep["converged"].sum()),
                                  "settle_iters_mean": float(rep["settle_iters"].mean()) if settle else None}
    lat.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1200x128x16,20000x128x16")
    ap.add_argument("--qs", default="64,256")
    ap.add_argument("--details", default="light,full")
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
        for detail in a.details.split(","):
            lines.append(json.dumps(run_shape(N, D, k, qs, a.reps, a.loop_queries, detail, source_hash)))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if a.append else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

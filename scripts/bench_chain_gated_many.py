"""Per-query gates with per-query chain priors: `chain_gated_many(psis, gates, chains, lamP,
settle=True, bundle_k=8)` for Q = 256, light and full detail, against
  (a) the six-call loop `add_chain(chain, lamP); set_query(psi, gates=g); settle(); receipt(); chain_receipt(chain);
      bundle(8)` on the same lattice, timed per query over its first `--loop-queries` queries (every one started from U = Y)
      and scaled to Q;
  (b) `receipt_gated_many` with the same settings (what the chain adds: one small launch per PCG iteration and the edge stage);
  (c) `receipt_gated_many` and `bundle_gated_many` themselves, to be compared between two commits: `--tree PATH` imports the
      package from another checkout (one without `chain_gated_many` reports (c) alone).
Shapes: config 2 (1200 x 128, k 16), 20 000 x 128 and 5 000 x 768.  Median and p10-p90 over the repeats.

    python scripts/bench_chain_gated_many.py [--reps 5 --loop-queries 8 --out profiles/chain_gated_many.json]
    python scripts/bench_chain_gated_many.py --shapes 20000x128x16 --details light --tree ../parent

One JSON line per (shape, detail), each with the hash of the library's sources."""
import argparse
import json
import os
import sys
import time

import numpy as np

CHAIN_NODES, LAMP = 8, 0.2


def _stats(ts):
    a = 1e3 * np.asarray(ts, dtype=np.float64)
    return {"median_ms": float(np.median(a)), "p10_ms": float(np.percentile(a, 10)), "p90_ms": float(np.percentile(a, 90))}


def _timed(fn, reps):
    fn()  # warm-up: scratch, the normalised anchors
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return _stats(ts)


def _loop(lat, P, G, chains, nl, reps):
    """per-query time of the six-call flow over the first nl queries"""
    def one(q):
        lat.clear_chain()
        lat.reset_U(wait=False)
        lat.add_chain(chains[q], LAMP)
        lat.set_query(P[q], gates=G[q])
        lat.settle()
        lat.receipt()
        lat.chain_receipt(chains[q])
        lat.bundle(k=8)

    one(0)  # warm-up
    per = []
    for _ in range(reps):
        t = time.perf_counter()
        for q in range(nl):
            one(q)
        per.append((time.perf_counter() - t) / nl)
    lat.clear_chain()
    return _stats(per)


def run_shape(N, D, k, Q, reps, loop_queries, detail, source_hash):
    from oscillink_amd import Oscillink

    rng = np.random.default_rng(0)
    Y = rng.standard_normal((N, D)).astype(np.float32)
    lat = Oscillink(Y, kneighbors=k, deterministic_k=True)
    lat.set_receipt_detail(detail)
    P = rng.standard_normal((Q, D)).astype(np.float32)
    P[::4] = Y[rng.integers(0, N, (Q + 3) // 4)] + 0.1 * rng.standard_normal(((Q + 3) // 4, D)).astype(np.float32)
    G = lat.diffusion_gates_many(P)["gates"]
    chains = [[int(v) for v in rng.choice(N, CHAIN_NODES, replace=False)] for _ in range(Q)]
    rec = {"N": N, "D": D, "k": k, "Q": Q, "detail": detail, "reps": reps, "library": source_hash,
           "chain_nodes": CHAIN_NODES, "lamP": LAMP, "reordered": lat.build_info()["reordered"]}
    kw = dict(settle=True, bundle_k=8, as_arrays=True)
    rec["receipt_gated_many"] = _timed(lambda: lat.receipt_gated_many(P, G, **kw), reps)
    rec["bundle_gated_many"] = _timed(lambda: lat.bundle_gated_many(P, G, k=8, as_arrays=True), reps)
    if hasattr(lat, "chain_gated_many"):
        st = _timed(lambda: lat.chain_gated_many(P, G, chains, LAMP, **kw), reps)
        rep = lat.last_chain_gated
        nl = min(loop_queries, Q)
        loop = _loop(lat, P, G, chains, nl, reps)
        lat.reset_U()
        # the A/B rule of DESIGN.md section 10: a gain counts from 3 x the wider p10-p90 band on (both per call)
        band = max(st["p90_ms"] - st["p10_ms"], Q * (loop["p90_ms"] - loop["p10_ms"]))
        gain = Q * loop["median_ms"] - st["median_ms"]
        rec["chain_gated_many"] = {**st, "per_query_us": 1e3 * st["median_ms"] / Q,
                                   "ustar_iters_mean": float(rep["iters"].mean()), "ustar_iters_max": int(rep["iters"].max()),
                                   "settle_iters_mean": float(rep["settle_iters"].mean()),
                                   "converged": int(rep["converged"].sum())}
        rec["loop_per_query"] = {"queries": nl, **loop}
        rec["loop_over_batch"] = Q * loop["median_ms"] / st["median_ms"]
        rec["gain_over_band"] = gain / band if band > 0 else float("inf")
        rec["chain_over_receipt_gated"] = st["median_ms"] / rec["receipt_gated_many"]["median_ms"]
    lat.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1200x128x16,20000x128x16,5000x768x16")
    ap.add_argument("--q", type=int, default=256)
    ap.add_argument("--details", default="light,full")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-queries", type=int, default=8)
    ap.add_argument("--tree", default=None, help="import oscillink_amd from this checkout instead of the script's own")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="add the lines to --out instead of replacing it")
    a = ap.parse_args()
    root = os.path.abspath(a.tree) if a.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    from oscillink_amd import _build

    _build.build()
    source_hash = _build._source_hash()
    lines = []
    for shape in a.shapes.split(","):
        N, D, k = (int(x) for x in shape.split("x"))
        for detail in a.details.split(","):
            lines.append(json.dumps({"tree": a.tree or ".",
                                     **run_shape(N, D, k, a.q, a.reps, a.loop_queries, detail, source_hash)}))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if a.append else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

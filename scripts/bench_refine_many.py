"""Corpus refine at config 3's corpus (N = 100 000, D = 768): per-query time of `Corpus.refine_many` at Q in {1, 64, 256}
against the reference's retrieval loop (device search, then per query `Oscillink(Y[cand])` + `set_query` + `bundle`) over
32 queries, for (top_k 100, k 8) and (top_k 1000, k 1000) as scripts/bench_beir.py runs them.  Writes
profiles/refine_many_bench.json.

    python scripts/bench_refine_many.py [--N 100000 --D 768 --reps 5 --loop 32]
    python scripts/bench_refine_many.py --profile --reps 3   # the run to put under rocprofv3 --kernel-trace --stats"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETTINGS = [(100, 8), (1000, 1000)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=100_000)
    ap.add_argument("--D", type=int, default=768)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop", type=int, default=32)
    ap.add_argument("--profile", action="store_true", help="only refine_many at Q = 256, top_k 100 (profiler run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_many_bench.json"))
    a = ap.parse_args()
    from oscillink_amd import Corpus, Oscillink

    rng = np.random.default_rng(0)
    Y = rng.standard_normal((a.N, a.D)).astype(np.float32)
    P = (Y[rng.integers(0, a.N, 256)] + 0.5 * rng.standard_normal((256, a.D))).astype(np.float32)
    t0 = time.perf_counter()
    c = Corpus(Y)
    rec = {"N": a.N, "D": a.D, "kneighbors": 6, "create_ms": 1e3 * (time.perf_counter() - t0)}
    settings = SETTINGS[:1] if a.profile else SETTINGS
    for top_k, k in settings:
        key = f"top{top_k}_k{k}"
        out = {"chunk": c.info(top_k, 6, k)}
        for Q in ([256] if a.profile else [1, 64, 256]):
            c.refine_many(P[:Q], top_k, k, as_arrays=True)
            ts = []
            for _ in range(a.reps):
                t = time.perf_counter()
                r = c.refine_many(P[:Q], top_k, k, as_arrays=True)
                ts.append(time.perf_counter() - t)
            med = float(np.median(ts))
            out[f"Q{Q}"] = {"batch_ms": 1e3 * med, "min_ms": 1e3 * min(ts), "per_query_us": 1e6 * med / Q,
                            "ustar_iters_mean": float(np.mean(r["ustar_iters"]))}
        if not a.profile:
            ids, _ = c.search(P[: a.loop], top_k)
            loop = []
            for q in range(a.loop):
                t = time.perf_counter()
                cand, _ = c.search(P[q:q + 1], top_k)
                lat = Oscillink(Y[cand[0]], kneighbors=6)
                lat.set_query(P[q])
                lat.bundle(k, 0.5)
                lat.close()
                loop.append(time.perf_counter() - t)
            per = float(np.median(loop))
            out["loop"] = {"per_query_ms": 1e3 * per, "mean_ms": 1e3 * float(np.mean(loop)), "queries": a.loop}
            out["ratio_q256"] = out["Q256"]["per_query_us"] / (1e6 * per)
        rec[key] = out
    c.close()
    line = json.dumps(rec)
    print(line)
    if not a.profile:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

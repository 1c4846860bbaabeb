"""Ragged corpus refine at config 3's corpus (N = 100 000, D = 768), Q = 256, top_k 100, k 8,
kneighbors 6: the median and the p10-p90 band of device-synchronised `Corpus.refine_many` calls (the call returns once its
results are on the host) for

    plain       a per-query (Q, N) `allow` under which every query has at least K eligible rows (the uniform call)
    ragged      `ragged=True`, eligible rows spread evenly over 1 .. 100 (skipped on a tree without the keyword)
    workaround  what a tree without the keyword has to do for those queries: one call per distinct size, top_k = size

Results are merged into profiles/refine_ragged_bench.json under --label, so that a parent checkout and this tree can be
measured by the same script on the same machine:

    python scripts/bench_refine_ragged.py --label this --modes plain,ragged
    python scripts/bench_refine_ragged.py --label parent --modes plain,workaround --tree /path/to/parent/checkout
    python scripts/bench_refine_ragged.py --profile      # ragged calls only: the run to put under rocprofv3 --kernel-trace --stats"""
import argparse
import inspect
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOP_K, K_PICK, KNEIGHBORS = 100, 8, 6


def _stats(ts):
    ms = 1e3 * np.asarray(ts)
    return {"median_ms": float(np.median(ms)), "p10_ms": float(np.percentile(ms, 10)), "p90_ms": float(np.percentile(ms, 90)),
            "min_ms": float(ms.min()), "calls": len(ts)}


def _timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return _stats(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=100_000)
    ap.add_argument("--D", type=int, default=768)
    ap.add_argument("--Q", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--modes", default="plain,ragged,workaround")
    ap.add_argument("--label", default="this", help="key of this run in the output file")
    ap.add_argument("--tree", default=ROOT, help="the checkout to import oscillink_amd from (built already)")
    ap.add_argument("--profile", action="store_true", help="ragged calls only, nothing written (profiler run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_ragged_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    from oscillink_amd import Corpus

    has_ragged = "ragged" in inspect.signature(Corpus.refine_many).parameters
    rng = np.random.default_rng(0)
    Y = rng.standard_normal((a.N, a.D)).astype(np.float32)
    P = (Y[rng.integers(0, a.N, a.Q)] + 0.5 * rng.standard_normal((a.Q, a.D))).astype(np.float32)
    wide = rng.random((a.Q, a.N)) < 0.5  # every query keeps about N / 2 rows: far more than K
    sizes = 1 + (np.arange(a.Q) * TOP_K) // a.Q  # 1 .. 100, evenly
    short = np.zeros((a.Q, a.N), dtype=bool)
    for q, n in enumerate(sizes):
        short[q, rng.choice(a.N, size=int(n), replace=False)] = True
    kw = dict(as_arrays=True, kneighbors=KNEIGHBORS)
    c = Corpus(Y)
    modes = ["ragged"] if a.profile else a.modes.split(",")
    rec = {"N": a.N, "D": a.D, "Q": a.Q, "top_k": TOP_K, "k": K_PICK, "kneighbors": KNEIGHBORS, "has_ragged": has_ragged,
           "sizes": [int(sizes.min()), int(sizes.max()), int(np.unique(sizes).size)]}
    for mode in modes:
        if mode == "plain":
            rec[mode] = _timed(lambda: c.refine_many(P, TOP_K, K_PICK, allow=wide, **kw), a.reps, a.warmup)
        elif mode == "ragged" and has_ragged:
            rec[mode] = _timed(lambda: c.refine_many(P, TOP_K, K_PICK, allow=short, ragged=True, **kw), a.reps, a.warmup)
        elif mode == "workaround":
            groups = [np.flatnonzero(sizes == n) for n in np.unique(sizes)]

            def per_size():
                for g in groups:
                    c.refine_many(P[g], int(sizes[g[0]]), K_PICK, allow=short[g], **kw)

            rec[mode] = dict(_timed(per_size, a.reps, a.warmup), calls_per_batch=len(groups))
    c.close()
    print(json.dumps({a.label: rec}))
    if a.profile:
        return
    merged = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            merged = json.load(f)
    merged[a.label] = rec
    with open(a.out, "w") as f:
        f.write(json.dumps(merged, indent=1) + "\n")


if __name__ == "__main__":
    main()

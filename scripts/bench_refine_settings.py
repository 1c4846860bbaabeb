"""Per-query settings of Corpus.refine_many at config 3's corpus (N = 100 000, D = 768), Q = 256,
top_k 100, k 8, as scripts/bench_refine_many.py: the median and the p10-p90 band of device-synchronised calls (the call
returns once its results are on the host) for

    scalar_plain  the all-scalar call, defaults                       (what the feature costs those who do not use it:
    scalar_full   the same with receipts="full"                        measure on the parent checkout and on this tree)
    grouped       256 queries under 16 distinct settings tuples, 16 queries each, interleaved -- kneighbors 4 .. 8, the
                  lambdas within the +-15 % of the reference's exploring profiles (cloud/app/learners.py:148-192) -- as the 16
                  scalar calls a tree without the feature has to make, one per tuple
    armed         the same 256 queries and tuples as ONE call with length-Q arrays (skipped on a tree without the feature)

Results are merged into --out under --label, so that a parent checkout and this tree can be measured alternately by the
same script in one session:

    python scripts/bench_refine_settings.py --label this_1 --modes scalar_plain,scalar_full,grouped,armed
    python scripts/bench_refine_settings.py --label parent_1 --modes scalar_plain,scalar_full,grouped --tree /path/to/parent"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOP_K, K_PICK, TUPLES = 100, 8, 16


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
    ap.add_argument("--modes", default="scalar_plain,scalar_full,grouped,armed")
    ap.add_argument("--label", default="this", help="key of this run in the output file")
    ap.add_argument("--tree", default=ROOT, help="the checkout to import oscillink_amd from (built already)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_settings_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    from oscillink_amd import Corpus

    rng = np.random.default_rng(0)
    Y = rng.standard_normal((a.N, a.D)).astype(np.float32)
    P = (Y[rng.integers(0, a.N, a.Q)] + 0.5 * rng.standard_normal((a.Q, a.D))).astype(np.float32)
    jitter = lambda base: base * (1.0 + rng.uniform(-0.15, 0.15, TUPLES))  # noqa: E731
    tuples = {"lamG": jitter(1.0), "lamC": jitter(0.5), "lamQ": jitter(4.0), "kneighbors": 4 + np.arange(TUPLES) % 5}
    of_query = np.arange(a.Q) % TUPLES  # interleaved: neighbours in the batch never share a tuple
    per_query = {n: v[of_query] for n, v in tuples.items()}
    groups = [np.flatnonzero(of_query == t) for t in range(TUPLES)]
    c = Corpus(Y)
    has = True
    try:
        c.refine_many(P[:2], TOP_K, K_PICK, lamG=np.ones(2))
    except (TypeError, ValueError):
        has = False
    rec = {"N": a.N, "D": a.D, "Q": a.Q, "top_k": TOP_K, "k": K_PICK, "tuples": TUPLES, "has_per_query_settings": has}

    def grouped():
        for t, g in enumerate(groups):
            c.refine_many(P[g], TOP_K, K_PICK, as_arrays=True, lamG=float(tuples["lamG"][t]), lamC=float(tuples["lamC"][t]),
                          lamQ=float(tuples["lamQ"][t]), kneighbors=int(tuples["kneighbors"][t]))

    for mode in a.modes.split(","):
        if mode == "scalar_plain":
            rec[mode] = _timed(lambda: c.refine_many(P, TOP_K, K_PICK, as_arrays=True), a.reps, a.warmup)
        elif mode == "scalar_full":
            rec[mode] = _timed(lambda: c.refine_many(P, TOP_K, K_PICK, as_arrays=True, receipts="full"), a.reps, a.warmup)
        elif mode == "grouped":
            rec[mode] = dict(_timed(grouped, a.reps, a.warmup), calls_per_batch=TUPLES)
        elif mode == "armed" and has:
            rec[mode] = _timed(lambda: c.refine_many(P, TOP_K, K_PICK, as_arrays=True, **per_query), a.reps, a.warmup)
    c.close()
    print(json.dumps({a.label: rec}))
    merged = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            merged = json.load(f)
    merged[a.label] = rec
    with open(a.out, "w") as f:
        f.write(json.dumps(merged, indent=1) + "\n")


if __name__ == "__main__":
    main()

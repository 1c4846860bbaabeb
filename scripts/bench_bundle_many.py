"""Multi-query bundles at config 3's shape (N = 100 000, D = 768, k = 32): the query basis solve, batch time and
queries/s of `bundle_many` for Q in {1, 8, 64, 256}, and the per-query `set_query` + `bundle` loop on 8 queries.

    python scripts/bench_bundle_many.py [--N 100000 --D 768 --k 32 --reps 5]
    python scripts/bench_bundle_many.py --kernel-stats kernel_stats.csv   # k_query_gemm TF/s from a rocprofv3 --stats run
    python scripts/bench_bundle_many.py --profile-q 256 --reps 3          # the run to put under rocprofv3

The TF/s of the query dots (k_query_gemm<0>) come from a rocprofv3 --kernel-trace --stats table of a --profile-q run:
2 N D Q flops per launch against the fp32 matrix peak of 155 TF (MI355X_MICROARCH.md)."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TF = 155.0


def kernel_tf(path, N, D, Q):
    rows = list(csv.DictReader(open(path)))
    out = {}
    for r in rows:
        name = r.get("Name") or r.get("KernelName") or ""
        if "k_query_gemm" not in name:
            continue
        avg_ns = float(r.get("AverageNs") or r.get("Average(ns)") or 0.0)
        calls = int(float(r.get("Calls") or 0))
        mode = 0 if "<0>" in name else 1
        flops = 2.0 * N * D * Q
        out[f"k_query_gemm<{mode}>"] = {"calls": calls, "avg_us": avg_ns / 1e3, "tf_s": flops / avg_ns / 1e3,
                                        "fraction_of_peak": flops / avg_ns / 1e3 / PEAK_TF}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=100_000)
    ap.add_argument("--D", type=int, default=768)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--profile-q", type=int, default=0, help="only time bundle_many at this Q (for a profiler run)")
    ap.add_argument("--kernel-stats", default=None)
    a = ap.parse_args()
    if a.kernel_stats:
        print(json.dumps({"N": a.N, "D": a.D, "Q": 256, "kernels": kernel_tf(a.kernel_stats, a.N, a.D, 256)}))
        return
    from oscillink_amd import Oscillink, _native

    rng = np.random.default_rng(0)
    Y = rng.standard_normal((a.N, a.D)).astype(np.float32)
    t0 = time.perf_counter()
    lat = Oscillink(Y, kneighbors=a.k, deterministic_k=True)
    create_ms = 1e3 * (time.perf_counter() - t0)
    P = rng.standard_normal((256, a.D)).astype(np.float32)
    P /= np.linalg.norm(P, axis=1, keepdims=True)
    P[0] = Y[:32].mean(axis=0) / np.linalg.norm(Y[:32].mean(axis=0))
    # the basis solve, for the largest |psi|_inf of the set (later batches then reuse it as it is)
    lat.bundle_many(P[:1] * (np.max(np.abs(P)) / np.max(np.abs(P[0]))), k=8)
    rec = {"N": a.N, "D": a.D, "k": a.k, "create_ms": create_ms, "basis": dict(lat.last_query_basis),
           "query_chunk": _native.OSC_QUERY_CHUNK}
    qs = [a.profile_q] if a.profile_q else [1, 8, 64, 256]
    batches = {}
    for Q in qs:
        lat.bundle_many(P[:Q], k=8)
        ts = []
        for _ in range(a.reps):
            t = time.perf_counter()
            lat.bundle_many(P[:Q], k=8)
            ts.append(time.perf_counter() - t)
        med = float(np.median(ts))
        batches[str(Q)] = {"batch_ms": 1e3 * med, "min_ms": 1e3 * min(ts), "queries_per_s": Q / med,
                           "per_query_us": 1e6 * med / Q}
    rec["bundle_many"] = batches
    rec["query_basis_solves"] = lat.stats["query_basis_solves"]
    if not a.profile_q:
        loop = []
        for q in range(8):
            t = time.perf_counter()
            lat.set_query(P[q])
            lat.bundle(k=8)
            loop.append(time.perf_counter() - t)
        per = float(np.median(loop))
        rec["per_query_loop"] = {"per_query_ms": 1e3 * per, "queries_per_s": 1.0 / per, "all_ms": [1e3 * x for x in loop]}
        if "256" in batches:
            rec["amortised_ratio_q256"] = batches["256"]["per_query_us"] / (1e6 * per)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

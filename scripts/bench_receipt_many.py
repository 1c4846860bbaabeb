"""Multi-query receipts at config 3's shape (N = 100 000, D = 768, k = 32): the query basis solve, then the batch time of
`receipt_many` for Q in {1, 8, 64, 256} in three modes -- light, full + OSCILLINK_RECEIPT_NULL_CAP=16 as arrays and full + cap
16 as dicts -- and the per-query `set_query` + `receipt` loop on 8 queries in the same modes.

    python scripts/bench_receipt_many.py [--N 100000 --D 768 --k 32 --reps 5]
    python scripts/bench_receipt_many.py --profile-q 256 --reps 3   # the run to put under rocprofv3 --kernel-trace --stats"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = {"light": ("light", False), "full_cap16_arrays": ("full", True), "full_cap16_dicts": ("full", False)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=100_000)
    ap.add_argument("--D", type=int, default=768)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--profile-q", type=int, default=0, help="only time full + cap 16 as arrays at this Q (profiler run)")
    a = ap.parse_args()
    from oscillink_amd import Oscillink, _native

    os.environ["OSCILLINK_RECEIPT_NULL_CAP"] = "16"
    rng = np.random.default_rng(0)
    Y = rng.standard_normal((a.N, a.D)).astype(np.float32)
    t0 = time.perf_counter()
    lat = Oscillink(Y, kneighbors=a.k, deterministic_k=True)
    create_ms = 1e3 * (time.perf_counter() - t0)
    P = rng.standard_normal((256, a.D)).astype(np.float32)
    P /= np.linalg.norm(P, axis=1, keepdims=True)
    P[0] = Y[:32].mean(axis=0) / np.linalg.norm(Y[:32].mean(axis=0))
    lat.set_query(P[0])
    lat.settle(max_iters=12, tol=1e-3)
    # the basis solve, for the largest |psi|_inf of the set (later batches reuse it as it is)
    t = time.perf_counter()
    lat.receipt_many(P[:1] * (np.max(np.abs(P)) / np.max(np.abs(P[0]))), as_arrays=True)
    first_ms = 1e3 * (time.perf_counter() - t)
    rec = {"N": a.N, "D": a.D, "k": a.k, "create_ms": create_ms, "basis": dict(lat.last_query_basis),
           "first_call_ms": first_ms, "query_chunk": _native.OSC_QUERY_CHUNK, "null_cap": 16}
    modes = {"full_cap16_arrays": MODES["full_cap16_arrays"]} if a.profile_q else MODES
    qs = [a.profile_q] if a.profile_q else [1, 8, 64, 256]
    for name, (detail, arrays) in modes.items():
        lat.set_receipt_detail(detail)
        batches = {}
        for Q in qs:
            lat.receipt_many(P[:Q], as_arrays=arrays)
            ts = []
            for _ in range(a.reps):
                t = time.perf_counter()
                lat.receipt_many(P[:Q], as_arrays=arrays)
                ts.append(time.perf_counter() - t)
            med = float(np.median(ts))
            batches[str(Q)] = {"batch_ms": 1e3 * med, "min_ms": 1e3 * min(ts), "per_query_us": 1e6 * med / Q}
        rec[name] = batches
        if not a.profile_q:
            loop = []
            for q in range(8):
                t = time.perf_counter()
                lat.set_query(P[q])
                lat.receipt()
                loop.append(time.perf_counter() - t)
            lat.set_query(P[0])
            per = float(np.median(loop))
            rec[name + "_loop"] = {"per_query_ms": 1e3 * per, "all_ms": [1e3 * x for x in loop]}
            rec[name + "_ratio_q256"] = batches["256"]["per_query_us"] / (1e6 * per)
    rec["query_basis_solves"] = lat.stats["query_basis_solves"]
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

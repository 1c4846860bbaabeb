"""Chain priors in receipt_many at config 3's shape (N = 100 000, D = 768, k = 32): `receipt_many(P, chains=..., lamP=...)` for
Q = 1 / 32 / 256 queries with an 8-node chain that walks graph edges -- one chain shared by every query, and a chain per
query -- in light detail (dicts) and in full detail (null cap 16, `as_arrays=True`), against the loop it replaces,
`add_chain(chain_q, lamP); set_query(psi_q); receipt()`, measured in the same process on the same build (the loop on a second
lattice of the same anchors, 4 queries: each is a full U* solve), and against the plain `receipt_many` call.

    python scripts/bench_receipt_prior_many.py [--N 100000 --D 768 --k 32 --lamP 0.2 --reps 5 --out profiles/receipt_prior_many.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.bench_chain_receipt_many import walk  # noqa: E402


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)), float(min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=100_000)
    ap.add_argument("--D", type=int, default=768)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--Qs", type=int, nargs="+", default=[1, 32, 256])
    ap.add_argument("--nodes", type=int, default=8)
    ap.add_argument("--lamP", type=float, default=0.2)
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--null_cap", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop_queries", type=int, default=4)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    os.environ["OSCILLINK_RECEIPT_NULL_CAP"] = str(a.null_cap)
    from oscillink_amd import Oscillink

    rng = np.random.default_rng(0)
    Y = rng.standard_normal((a.N, a.D)).astype(np.float32)
    lat = Oscillink(Y, kneighbors=a.k, deterministic_k=True)
    Qmax = max(a.Qs)
    P = rng.standard_normal((Qmax, a.D)).astype(np.float32)
    P /= np.linalg.norm(P, axis=1, keepdims=True)
    lat.set_query(P[0])
    rowptr, col = lat.graph_csr()[:2]
    deg = np.diff(rowptr)
    per_query = []
    for s in (int(s) for s in rng.permutation(a.N) if deg[s] > 0):
        w = walk(rowptr, col, s, a.nodes)
        if len(w) == a.nodes:
            per_query.append(w)
        if len(per_query) == Qmax:
            break
    assert len(per_query) == Qmax
    modes = (("light", False), ("full", True))  # light: dicts; full: null cap and arrays
    t = time.perf_counter()
    lat.receipt_many(P, chains=per_query[0], lamP=a.lamP, tol=a.tol, as_arrays=True)  # the shifted basis and its terms
    first_ms = 1e3 * (time.perf_counter() - t)
    rec = {"N": a.N, "D": a.D, "k": a.k, "chain_nodes": a.nodes, "lamP": a.lamP, "tol": a.tol, "null_cap": a.null_cap,
           "first_call_ms": first_ms, "shifted_basis": dict(lat.last_shifted_basis), "batch": {}}
    for detail, arrays in modes:
        lat.set_receipt_detail(detail)
        for Q in a.Qs:
            for name, chains in (("shared", per_query[0]), ("per_query", per_query[:Q])):
                med, lo = timed(lambda: lat.receipt_many(P[:Q], chains=chains, lamP=a.lamP, tol=a.tol, as_arrays=arrays), a.reps)
                pr = lat.last_receipt_prior
                rec["batch"][f"{detail}_Q{Q}_{name}"] = {
                    "batch_ms": 1e3 * med, "min_ms": 1e3 * lo, "per_query_us": 1e6 * med / Q,
                    "prior_res_max": float(pr["res"].max()), "prior_iters_max": int(pr["iters"].max())}
            med, _ = timed(lambda: lat.receipt_many(P[:Q], tol=a.tol, as_arrays=arrays), a.reps)
            rec["batch"][f"{detail}_Q{Q}_plain"] = {"batch_ms": 1e3 * med, "per_query_us": 1e6 * med / Q}
    rec["shifted_basis_solves"] = lat.shifted_basis_solves  # 1: the timed calls solved no basis
    rec["shifted_basis_bytes"] = lat.build_info()["shifted_basis_bytes"]
    # the loop, same process, same build, a lattice of its own
    lat2 = Oscillink(Y, kneighbors=a.k, deterministic_k=True)
    lat2.set_query(P[0])
    rec["loop"] = {}
    for detail, _ in modes:
        lat2.set_receipt_detail(detail)
        lat2.add_chain(per_query[Qmax - 1], lamP=a.lamP)
        lat2.receipt()  # warm
        loop = []
        for q in range(a.loop_queries):
            t = time.perf_counter()
            lat2.add_chain(per_query[q], lamP=a.lamP)
            lat2.set_query(P[q])
            lat2.receipt()
            loop.append(time.perf_counter() - t)
        rec["loop"][detail] = {"per_query_us": 1e6 * float(np.median(loop)), "all_ms": [1e3 * x for x in loop],
                               "ustar_iters": int(lat2.last_ustar["iters"])}
    for key, b in rec["batch"].items():
        b["ratio_to_loop"] = b["per_query_us"] / rec["loop"][key.split("_")[0]]["per_query_us"]
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()

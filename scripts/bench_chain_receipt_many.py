"""Multi-query chain receipts at config 3's shape (N = 100 000, D = 768, k = 32): the batch time of `chain_receipt_many` for
Q = 256 queries with an 8-node chain that walks graph edges -- one chain shared by every query, and a chain per query -- as
arrays and as dicts, against the per-query `set_query` + `chain_receipt` loop on 8 queries, and the bytes the gather asks for
(Q E (deg + 3) D 4: per chain edge row i, row j and the rows of i's graph and path neighbours).

    python scripts/bench_chain_receipt_many.py [--N 100000 --D 768 --k 32 --Q 256 --reps 5]
    python scripts/bench_chain_receipt_many.py --profile --reps 3   # the run to put under rocprofv3 --kernel-trace --stats"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def walk(rowptr, col, start, n):
    """From `start`, step to the first unvisited neighbour, for n nodes."""
    out, seen = [int(start)], {int(start)}
    while len(out) < n:
        nxt = [int(c) for c in col[rowptr[out[-1]]: rowptr[out[-1] + 1]] if int(c) not in seen]
        if not nxt:
            break
        out.append(nxt[0])
        seen.add(nxt[0])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=100_000)
    ap.add_argument("--D", type=int, default=768)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--Q", type=int, default=256)
    ap.add_argument("--nodes", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--profile", action="store_true", help="only the two array forms (profiler run)")
    a = ap.parse_args()
    from oscillink_amd import Oscillink, _native

    rng = np.random.default_rng(0)
    Y = rng.standard_normal((a.N, a.D)).astype(np.float32)
    t0 = time.perf_counter()
    lat = Oscillink(Y, kneighbors=a.k, deterministic_k=True)
    create_ms = 1e3 * (time.perf_counter() - t0)
    P = rng.standard_normal((a.Q, a.D)).astype(np.float32)
    P /= np.linalg.norm(P, axis=1, keepdims=True)
    lat.set_query(P[0])
    rowptr, col = lat.graph_csr()[:2]
    deg = np.diff(rowptr)
    starts = [int(s) for s in rng.permutation(a.N) if deg[s] > 0]
    per_query = []
    for s in starts:
        w = walk(rowptr, col, s, a.nodes)
        if len(w) == a.nodes:
            per_query.append(w)
        if len(per_query) == a.Q:
            break
    assert len(per_query) == a.Q
    forms = {"shared": per_query[0], "per_query": per_query}
    t = time.perf_counter()
    lat.chain_receipt_many(P, per_query[0], as_arrays=True)  # the basis solve
    first_ms = 1e3 * (time.perf_counter() - t)
    rec = {"N": a.N, "D": a.D, "k": a.k, "Q": a.Q, "chain_nodes": a.nodes, "create_ms": create_ms,
           "basis": dict(lat.last_query_basis), "first_call_ms": first_ms, "query_chunk": _native.OSC_QUERY_CHUNK}
    for name, chains in forms.items():
        lists = [chains] * a.Q if name == "shared" else chains
        rows = sum(int(deg[c]) + 3 for ch in lists for c in ch[:-1])  # per edge: i, j, deg graph and <= 2 path neighbours
        rec[name + "_gather_bytes"] = rows * a.D * 4
        rec[name + "_mean_degree"] = float(np.mean([deg[c] for ch in lists for c in ch[:-1]]))
        for arrays in (True,) if a.profile else (True, False):
            lat.chain_receipt_many(P, chains, as_arrays=arrays)
            ts = []
            for _ in range(a.reps):
                t = time.perf_counter()
                lat.chain_receipt_many(P, chains, as_arrays=arrays)
                ts.append(time.perf_counter() - t)
            med = float(np.median(ts))
            rec[f"{name}_{'arrays' if arrays else 'dicts'}"] = {"batch_ms": 1e3 * med, "min_ms": 1e3 * min(ts),
                                                              "per_query_us": 1e6 * med / a.Q}
    if not a.profile:
        loop = []
        for q in range(8):
            t = time.perf_counter()
            lat.set_query(P[q])
            lat.chain_receipt(per_query[q])
            loop.append(time.perf_counter() - t)
        lat.set_query(P[0])
        per = float(np.median(loop))
        rec["loop"] = {"per_query_ms": 1e3 * per, "all_ms": [1e3 * x for x in loop]}
        for name in forms:
            rec[name + "_ratio"] = rec[name + "_arrays"]["per_query_us"] / (1e6 * per)
    rec["query_basis_solves"] = lat.stats["query_basis_solves"]
    print(json.dumps(rec))


if __name__ == "__main__":
    main()

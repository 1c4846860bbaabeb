"""Corpus refine with chain priors at config 3's corpus (N = 100 000, D = 768), Q = 256, top_k 100, k 8, kneighbors 6, chain
range(8), lamP 0.2 (scripts/benchmark.py's chain): per-query time of `Corpus.refine_many(chains=..., as_arrays=True)` with
`receipts=None` and `"full"`, against the same calls without chains in the same process and against the loop the reference
ships (device search, then per query `Oscillink(Y[cand])` + `add_chain` + `set_query` + `settle` + `bundle` + `receipt` +
`chain_receipt`) over 32 queries.  Every timed call ends with the library's own stream synchronisation before it returns,
so each clock read follows a synchronisation; every shape is warmed up once; the figures are the median of --reps calls with
min and max.  Writes profiles/refine_chains_bench.json.

    python scripts/bench_refine_chains.py [--N 100000 --D 768 --reps 5 --loop 32]
    python scripts/bench_refine_chains.py --parent-lib PATH   # also: the calls without chains (osc_corpus_refine and
                                                              # osc_corpus_refine_receipts), this build against the library
                                                              # built from the parent commit, alternating in one process
    python scripts/bench_refine_chains.py --profile --reps 3  # the run to put under rocprofv3 --kernel-trace --stats"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_refine_gated import K_PICK, TOP_K, parent_ab, stats, timed  # noqa: E402

CHAIN = list(range(8))
LAM_P = 0.2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=100_000)
    ap.add_argument("--D", type=int, default=768)
    ap.add_argument("--Q", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop", type=int, default=32)
    ap.add_argument("--parent-lib", default=None, help="liboscillink_hip.so built from the parent commit (the calls without chains, A/B)")
    ap.add_argument("--profile", action="store_true", help="only the batches (profiler run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_chains_bench.json"))
    a = ap.parse_args()
    from oscillink_amd import Corpus, Oscillink

    rng = np.random.default_rng(2024)  # config 3's corpus (scripts/bench_refine_receipts.py)
    Y = rng.standard_normal((a.N, a.D)).astype(np.float32)
    P = (Y[rng.integers(0, a.N, a.Q)] + 0.5 * rng.standard_normal((a.Q, a.D))).astype(np.float32)
    c = Corpus(Y)
    ck = dict(chains=[CHAIN] * a.Q, lamP=LAM_P)
    rec = {"N": a.N, "D": a.D, "Q": a.Q, "top_k": TOP_K, "k": K_PICK, "kneighbors": 6, "chain_len": len(CHAIN), "lamP": LAM_P,
           "chunk": c.info(TOP_K, 6, K_PICK)}
    r = c.refine_many(P, TOP_K, K_PICK, as_arrays=True, receipts="full", **ck)
    rec["settle_iters_mean"] = float(r["settle_iters"].mean())
    rec["ustar_iters_mean"] = float(r["ustar_iters"].mean())
    rec["verdict_true"] = int(r["chain_verdict"].sum())

    def batch(receipts, **kw):
        return stats(timed(lambda: c.refine_many(P, TOP_K, K_PICK, as_arrays=True, receipts=receipts, **kw), a.reps), a.Q)

    rec["plain"] = batch(None)
    rec["plain_chains"] = batch(None, **ck)
    rec["full"] = batch("full")
    rec["full_chains"] = batch("full", **ck)
    rec["added_ms"] = {"plain": rec["plain_chains"]["batch_ms"] - rec["plain"]["batch_ms"],
                       "full": rec["full_chains"]["batch_ms"] - rec["full"]["batch_ms"]}
    if not a.profile:

        def one(q):
            cand, _ = c.search(P[q:q + 1], TOP_K)
            lat = Oscillink(Y[cand[0]], kneighbors=6)
            lat.add_chain(CHAIN, lamP=LAM_P)
            lat.set_query(P[q])
            lat.settle()
            lat.bundle(K_PICK, 0.5)
            lat.receipt()
            lat.chain_receipt(CHAIN)
            lat.close()

        one(0)
        loop = []
        for q in range(a.loop):
            t = time.perf_counter()
            one(q)
            loop.append(time.perf_counter() - t)
        per = float(np.median(loop))
        rec["loop"] = {"per_query_ms": 1e3 * per, "min_ms": 1e3 * min(loop), "max_ms": 1e3 * max(loop), "queries": a.loop}
        rec["ratio_full_chains_to_loop"] = rec["full_chains"]["per_query_us"] / (1e6 * per)
    c.close()
    if a.parent_lib and not a.profile:
        rec["plain_ab"] = parent_ab(a.parent_lib, Y, P, max(5, a.reps))
        rec["full_ab"] = parent_ab(a.parent_lib, Y, P, max(5, a.reps), "receipts")
    line = json.dumps(rec)
    print(line)
    if not a.profile:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

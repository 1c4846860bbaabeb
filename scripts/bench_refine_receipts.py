"""Corpus refine with receipts at config 3's corpus (N = 100 000, D = 768), Q = 256, top_k 100, k 8, kneighbors 6: per-query
time of `Corpus.refine_many(receipts="full" / "light", as_arrays=True)`, ungated and with diffusion gates (gamma 0.15),
against `refine_many(receipts=None)` in the same process and against the loop the reference ships (device search, then per
query `Oscillink(Y[cand])` + `set_query` + `settle` + `bundle` + `receipt`) over 32 queries.  Every timed call ends with the
library's own stream synchronisation before it returns, so each clock read follows a synchronisation; every shape is
warmed up once; the figures are the median of --reps calls with min and max.  Writes profiles/refine_receipts_bench.json.

    python scripts/bench_refine_receipts.py [--N 100000 --D 768 --reps 5 --loop 32]
    python scripts/bench_refine_receipts.py --parent-lib PATH   # also: receipts=None and "full", this build against the library
                                                                # built from the parent commit, alternating in one process
    python scripts/bench_refine_receipts.py --profile --reps 3  # the run to put under rocprofv3 --kernel-trace --stats"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_refine_gated import BETA, GAMMA, K_PICK, TOP_K, parent_ab, stats, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=100_000)
    ap.add_argument("--D", type=int, default=768)
    ap.add_argument("--Q", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop", type=int, default=32)
    ap.add_argument("--parent-lib", default=None, help="liboscillink_hip.so built from the parent commit (receipts=None and \"full\" A/B)")
    ap.add_argument("--profile", action="store_true", help="only the batches (profiler run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_receipts_bench.json"))
    a = ap.parse_args()
    from oscillink_amd import Corpus, Oscillink

    rng = np.random.default_rng(2024)  # config 3's corpus (tests/test_gpu_refine_receipts_fullsize.py)
    Y = rng.standard_normal((a.N, a.D)).astype(np.float32)
    P = (Y[rng.integers(0, a.N, a.Q)] + 0.5 * rng.standard_normal((a.Q, a.D))).astype(np.float32)
    c = Corpus(Y)
    gk = dict(gates="diffusion", gate_beta=BETA, gate_gamma=GAMMA)
    rec = {"N": a.N, "D": a.D, "Q": a.Q, "top_k": TOP_K, "k": K_PICK, "kneighbors": 6, "beta": BETA, "gamma": GAMMA,
           "chunk": c.info(TOP_K, 6, K_PICK)}
    r = c.refine_many(P, TOP_K, K_PICK, as_arrays=True, receipts="full")
    rec["settle_iters"] = {"min": int(r["settle_iters"].min()), "mean": float(r["settle_iters"].mean()),
                           "max": int(r["settle_iters"].max())}
    rec["ustar_iters_mean"] = float(r["ustar_iters"].mean())
    rec["null_points_mean"] = float(r["null_total"].mean())

    def batch(receipts, **kw):
        return stats(timed(lambda: c.refine_many(P, TOP_K, K_PICK, as_arrays=True, receipts=receipts, **kw), a.reps), a.Q)

    rec["plain"] = batch(None)
    rec["full"] = batch("full")
    rec["light"] = batch("light")
    rec["plain_gated"] = batch(None, **gk)
    rec["full_gated"] = batch("full", **gk)
    rec["added_ms"] = {"full": rec["full"]["batch_ms"] - rec["plain"]["batch_ms"],
                       "light": rec["light"]["batch_ms"] - rec["plain"]["batch_ms"],
                       "full_gated": rec["full_gated"]["batch_ms"] - rec["plain_gated"]["batch_ms"]}
    if not a.profile:
        rec["full_dicts"] = stats(timed(lambda: c.refine_many(P, TOP_K, K_PICK, receipts="full"), a.reps), a.Q)

        def one(q, detail):
            cand, _ = c.search(P[q:q + 1], TOP_K)
            lat = Oscillink(Y[cand[0]], kneighbors=6)
            lat.set_receipt_detail(detail)
            lat.set_query(P[q])
            lat.settle()
            lat.bundle(K_PICK, 0.5)
            lat.receipt()
            lat.close()

        for detail in ("full", "light"):
            one(0, detail)
            loop = []
            for q in range(a.loop):
                t = time.perf_counter()
                one(q, detail)
                loop.append(time.perf_counter() - t)
            per = float(np.median(loop))
            rec["loop_" + detail] = {"per_query_ms": 1e3 * per, "min_ms": 1e3 * min(loop), "max_ms": 1e3 * max(loop),
                                     "queries": a.loop}
            rec["ratio_%s_to_loop" % detail] = rec[detail]["per_query_us"] / (1e6 * per)
        rec["target_ratio"] = 1.0 / 20.0
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

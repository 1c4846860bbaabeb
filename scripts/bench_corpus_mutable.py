"""The mutable Corpus at config 3's corpus (N = 100 000, D = 768), Q = 256, top_k 100: medians of
`--reps` timed calls after a warm-up, host clock around calls that end in a device synchronise.

  (a) search on a plain corpus (k_cq_select), with 10 % tombstones and with a per-query filter (k_cq_select_masked) --
      end to end here, filter packing and upload included; the kernels' own times come from the --profile run
  (b) refine_many on a corpus built by an append against a fresh one, alternating
  (c) append of 1 000 rows with and without growth of the device buffers
  (d) compact at 10 % tombstones
with the byte floors of (c) and (d) beside them.  Writes profiles/corpus_mutable_bench.json.

    python scripts/bench_corpus_mutable.py [--N 100000 --D 768 --reps 20]
    python scripts/bench_corpus_mutable.py --profile   # the run to put under rocprofv3 --kernel-trace --stats: part (a)
                                                       # only, its three phases in order, `reps` searches each"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.3e12   # achievable copy rate of the MI355X's HBM3E
PCIE_BYTES_PER_S = 63e9    # PCIe Gen5 x16, spec


def median_ms(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return {"median_ms": 1e3 * float(np.median(ts)), "min_ms": 1e3 * min(ts), "max_ms": 1e3 * max(ts), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=100_000)
    ap.add_argument("--D", type=int, default=768)
    ap.add_argument("--Q", type=int, default=256)
    ap.add_argument("--top_k", type=int, default=100)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--profile", action="store_true", help="part (a) only (profiler run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corpus_mutable_bench.json"))
    a = ap.parse_args()
    from oscillink_amd import Corpus

    N, D, Q, top_k = a.N, a.D, a.Q, a.top_k
    ldn = (D + 31) // 32 * 32
    rng = np.random.default_rng(0)
    Y = rng.standard_normal((N, D)).astype(np.float32)
    P = (Y[rng.integers(0, N, Q)] + 0.5 * rng.standard_normal((Q, D))).astype(np.float32)
    dead = rng.choice(N, N // 10, replace=False)
    allow = rng.random((Q, N)) < 0.9
    rec = {"N": N, "D": D, "Q": Q, "top_k": top_k}

    # (a) the three searches; the tombstoned corpus is a second handle so that the phases can alternate
    plain, tomb = Corpus(Y), Corpus(Y)
    tomb.remove(dead)
    rec["search"] = {
        "plain": median_ms(lambda: plain.search(P, top_k), a.reps),
        "tombstones_10pct": median_ms(lambda: tomb.search(P, top_k), a.reps),
        "per_query_filter": median_ms(lambda: plain.search(P, top_k, allow=allow), a.reps),
        "shared_filter": median_ms(lambda: plain.search(P, top_k, allow=allow[0]), a.reps),
    }
    tomb.close()
    if a.profile:
        plain.close()
        print(json.dumps(rec))
        return

    # (b) refine_many: appended against fresh, alternating
    grown = Corpus(Y[: N * 6 // 10])
    grown.append(Y[N * 6 // 10:])
    assert grown.n_live == grown.N == N
    for c in (plain, grown):
        c.refine_many(P, top_k, 8, as_arrays=True)
    ts = {"fresh": [], "appended": []}
    for _ in range(a.reps):
        for name, c in (("fresh", plain), ("appended", grown)):
            t = time.perf_counter()
            c.refine_many(P, top_k, 8, as_arrays=True)
            ts[name].append(time.perf_counter() - t)
    rec["refine_many"] = {k: {"median_ms": 1e3 * float(np.median(v)), "min_ms": 1e3 * min(v), "max_ms": 1e3 * max(v),
                              "per_query_us": 1e6 * float(np.median(v)) / Q, "reps": a.reps} for k, v in ts.items()}
    grown.close()
    plain.close()

    # (c) append of 1 000 rows: a fresh corpus is full, so its first append moves the buffers; the following ones fit
    M = 1000
    new = rng.standard_normal((M, D)).astype(np.float32)
    grow_ts, fit_ts = [], []
    base = Y[: N - M]
    for rep in range(a.reps + 1):
        c = Corpus(base)
        t = time.perf_counter()
        c.append(new)
        grow_ts.append(time.perf_counter() - t)
        if rep == 0:
            cap = c.capacity
            for _ in range(a.reps + 2):
                assert c.N + M <= cap
                t = time.perf_counter()
                c.append(new)
                fit_ts.append(time.perf_counter() - t)
        c.close()
    grow_ts, fit_ts = grow_ts[1:], fit_ts[2:]
    rec["append_1000"] = {
        "with_growth": {"median_ms": 1e3 * float(np.median(grow_ts)), "min_ms": 1e3 * min(grow_ts), "reps": len(grow_ts),
                        "capacity_after": cap,
                        "floor_ms": 1e3 * (2 * 2 * (N - M) * ldn * 4 / HBM_BYTES_PER_S + M * D * 4 / PCIE_BYTES_PER_S),
                        "floor": "device copy of Y and Yn (read + write) at 6.3 TB/s, plus the upload"},
        "without_growth": {"median_ms": 1e3 * float(np.median(fit_ts)), "min_ms": 1e3 * min(fit_ts), "reps": len(fit_ts),
                           "floor_ms": 1e3 * M * D * 4 / PCIE_BYTES_PER_S, "floor": "upload of M D floats at 63 GB/s"},
    }

    # (d) compact at 10 % tombstones; the rows go back by an append, which the clock does not see
    c = Corpus(Y)
    comp = []
    for _ in range(a.reps + 2):
        gone = rng.choice(c.N, N // 10, replace=False)
        c.remove(gone)
        t = time.perf_counter()
        c.compact()
        comp.append(time.perf_counter() - t)
        c.append(Y[: N // 10])
    c.close()
    comp = comp[2:]
    rec["compact_10pct"] = {"median_ms": 1e3 * float(np.median(comp)), "min_ms": 1e3 * min(comp), "reps": len(comp),
                            "floor_ms": 1e3 * 2 * 2 * (N - N // 10) * ldn * 4 / HBM_BYTES_PER_S,
                            "floor": "gather of the kept rows of Y and Yn (read + write) at 6.3 TB/s"}
    line = json.dumps(rec)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()

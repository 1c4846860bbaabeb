"""Gated corpus refine at config 3's corpus (N = 100 000, D = 768), top_k 100, k 8, gamma 0.15: per-query time of
`Corpus.refine_many(gates="diffusion")` and of `Corpus.diffusion_gates_many` at Q = 256 against the gated loop of the
reference's retrieval examples (device search, then per query `Oscillink(Y[cand])` + `compute_diffusion_gates(...,
lattice=lat)` + `set_query(psi, gates=g)` + `bundle`) over 32 queries.  Every timed call ends with the library's own
stream synchronisation before it returns, so each clock read follows a synchronisation; every shape is warmed up once;
the figures are the median of --reps calls with min and max.  Writes profiles/refine_gated_bench.json.

    python scripts/bench_refine_gated.py [--N 100000 --D 768 --reps 5 --loop 32]
    python scripts/bench_refine_gated.py --parent-lib PATH   # also: the ungated and the gated refine, this build against the
                                                             # library built from the parent commit, alternating in one process
    python scripts/bench_refine_gated.py --profile --reps 3  # the run to put under rocprofv3 --kernel-trace --stats"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TOP_K, K_PICK, GAMMA, BETA = 100, 8, 0.15, 1.0


def stats(ts, Q):
    med = float(np.median(ts))
    return {"batch_ms": 1e3 * med, "min_ms": 1e3 * min(ts), "max_ms": 1e3 * max(ts), "per_query_us": 1e6 * med / Q}


def timed(fn, reps):
    fn()  # warm-up of this shape
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return ts


AB_ENTRY = {"ungated": "osc_corpus_refine", "gated": "osc_corpus_refine_gated", "receipts": "osc_corpus_refine_receipts"}


def raw_refine(lib, Y, P, kind="ungated"):
    """One refine entry point of a library through ctypes alone (the signatures are the same in both builds): "ungated" is
    osc_corpus_refine, "gated" osc_corpus_refine_gated with diffusion gates, "receipts" osc_corpus_refine_receipts without
    gates in full detail -- each with refine_many's arguments.  call() returns copies of every array the call fills."""
    from oscillink_amd import _native as nat

    for name in ("osc_corpus_create", "osc_corpus_destroy", AB_ENTRY[kind]):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = nat.SIGNATURES[name]
    h = nat.Handle()
    assert lib.osc_corpus_create(nat.f32(Y), Y.shape[0], Y.shape[1], 0, C.byref(h)) == 0
    Q = P.shape[0]
    cand, g = np.zeros((Q, TOP_K), np.int32), np.zeros((Q, TOP_K), np.float32)
    local, score, align = np.zeros((Q, K_PICK), np.int32), np.zeros((Q, K_PICK), np.float32), np.zeros((Q, K_PICK), np.float32)
    iters, g_iters, s_iters, total = (np.zeros(Q, np.int32) for _ in range(4))
    rs, g_res, s_res = (np.zeros(Q, np.float32) for _ in range(3))
    sums, offsets = np.zeros((4, Q), np.float64), np.zeros(Q + 1, np.int64)
    ni, nj = np.zeros(Q * TOP_K, np.int32), np.zeros(Q * TOP_K, np.int32)
    nz, nr = np.zeros(Q * TOP_K, np.float32), np.zeros(Q * TOP_K, np.float32)
    ptr = {np.dtype(np.int32): nat.i32, np.dtype(np.float32): nat.f32, np.dtype(np.int64): nat.i64,
           np.dtype(np.float64): lambda v: v.ctypes.data_as(nat.c_f64p)}
    solve = (6, 1.0, 1.0, 0.5, 4.0, 1e-4, 64, K_PICK, 0.5)  # kneighbors, row cap, lambdas, U* settings, k, alpha
    gate = (BETA, GAMMA, 0, 1e-4, 256)  # method "direct"
    gated_outs = [cand, g, local, score, align, iters, rs, g_iters, g_res]
    if kind == "ungated":
        outs = [cand, local, score, align, iters, rs]
        args = [nat.f32(P), Q, TOP_K, None, *solve, *outs]
    elif kind == "gated":
        outs = gated_outs
        args = [nat.f32(P), Q, TOP_K, None, None, *gate, *solve, *outs]
    else:  # gate_mode 0; settle(1.0, 12, 1e-3), full detail, z_th 3, no cap; no graph fields
        outs = gated_outs + [s_iters, s_res, *sums, total, offsets, ni, nj, nz, nr]
        args = [nat.f32(P), Q, TOP_K, None, 0, None, *gate, *solve, 1.0, 12, 1e-3, 1, 3.0, 0, *outs, Q * TOP_K, None, None,
                None, 2048]
    args = [ptr[a.dtype](a) if isinstance(a, np.ndarray) else a for a in args]
    fn = getattr(lib, AB_ENTRY[kind])

    def call():
        assert fn(h, *args) == 0
        return [o.copy() for o in outs]

    return call, lambda: lib.osc_corpus_destroy(h)


def parent_ab(parent_path, Y, P, reps, kind="ungated"):
    """Parent build and this build, the same call (raw_refine's kind), alternating (so drift hits both alike)."""
    from oscillink_amd import _native as nat

    mine, close_mine = raw_refine(C.CDLL(nat.LIB_PATH), Y, P, kind)
    theirs, close_theirs = raw_refine(C.CDLL(parent_path), Y, P, kind)
    a, b = mine(), theirs()  # warm-up, and the answers are the same bytes
    same = all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    tm, tp = [], []
    for _ in range(reps):
        t = time.perf_counter()
        theirs()
        tp.append(time.perf_counter() - t)
        t = time.perf_counter()
        mine()
        tm.append(time.perf_counter() - t)
    close_mine()
    close_theirs()
    Q = P.shape[0]
    out = {"entry": AB_ENTRY[kind], "parent": stats(tp, Q), "this": stats(tm, Q), "same_bytes": same, "reps": reps}
    spread = out["parent"]["max_ms"] - out["parent"]["min_ms"]
    out["parent_spread_ms"] = spread
    out["not_slower"] = bool(out["this"]["batch_ms"] <= out["parent"]["batch_ms"] + spread)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=100_000)
    ap.add_argument("--D", type=int, default=768)
    ap.add_argument("--Q", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop", type=int, default=32)
    ap.add_argument("--parent-lib", default=None, help="liboscillink_hip.so built from the parent commit (ungated and gated A/B)")
    ap.add_argument("--profile", action="store_true", help="only the gated and the ungated batch (profiler run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_gated_bench.json"))
    a = ap.parse_args()
    from oscillink_amd import Corpus, Oscillink, compute_diffusion_gates

    rng = np.random.default_rng(0)
    Y = rng.standard_normal((a.N, a.D)).astype(np.float32)
    P = (Y[rng.integers(0, a.N, a.Q)] + 0.5 * rng.standard_normal((a.Q, a.D))).astype(np.float32)
    c = Corpus(Y)
    gk = dict(gates="diffusion", gate_beta=BETA, gate_gamma=GAMMA)
    rec = {"N": a.N, "D": a.D, "Q": a.Q, "top_k": TOP_K, "k": K_PICK, "kneighbors": 6, "beta": BETA, "gamma": GAMMA,
           "chunk": c.info(TOP_K, 6, K_PICK)}
    r = c.refine_many(P, TOP_K, K_PICK, as_arrays=True, **gk)
    rec["gate_iters"] = {"min": int(r["gate_iters"].min()), "mean": float(r["gate_iters"].mean()),
                         "max": int(r["gate_iters"].max())}
    rec["ustar_iters_mean"] = float(r["ustar_iters"].mean())
    rec["gated"] = stats(timed(lambda: c.refine_many(P, TOP_K, K_PICK, as_arrays=True, **gk), a.reps), a.Q)
    rec["ungated"] = stats(timed(lambda: c.refine_many(P, TOP_K, K_PICK, as_arrays=True), a.reps), a.Q)
    if not a.profile:
        rec["gates_only"] = stats(timed(lambda: c.diffusion_gates_many(P, TOP_K, beta=BETA, gamma=GAMMA), a.reps), a.Q)
        rec["gates_only_cg"] = stats(timed(lambda: c.diffusion_gates_many(P, TOP_K, beta=BETA, gamma=GAMMA, method="cg"),
                                           a.reps), a.Q)
        rec["search_only"] = stats(timed(lambda: c.search(P, TOP_K), a.reps), a.Q)

        def one(q):
            cand, _ = c.search(P[q:q + 1], TOP_K)
            lat = Oscillink(Y[cand[0]], kneighbors=6)
            g = compute_diffusion_gates(Y[cand[0]], P[q], kneighbors=6, beta=BETA, gamma=GAMMA, lattice=lat)
            lat.set_query(P[q], gates=g)
            lat.bundle(K_PICK, 0.5)
            lat.close()

        one(0)
        loop = []
        for q in range(a.loop):
            t = time.perf_counter()
            one(q)
            loop.append(time.perf_counter() - t)
        per = float(np.median(loop))
        rec["loop"] = {"per_query_ms": 1e3 * per, "min_ms": 1e3 * min(loop), "max_ms": 1e3 * max(loop), "queries": a.loop}
        rec["ratio_gated_to_loop"] = rec["gated"]["per_query_us"] / (1e6 * per)
        rec["target_ratio"] = 1.0 / 20.0
    c.close()
    if a.parent_lib and not a.profile:
        rec["ungated_ab"] = parent_ab(a.parent_lib, Y, P, max(5, a.reps))
        rec["gated_ab"] = parent_ab(a.parent_lib, Y, P, max(5, a.reps), "gated")
    line = json.dumps(rec)
    print(line)
    if not a.profile:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

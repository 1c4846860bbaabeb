"""OscillinkLattice.append against a fresh create: where the planner's thresholds come from.

For a base lattice and M new rows: the appended handle's creation (osc_create_appended, what `append` spends its time in) in
auto, forced-incremental and rebuild mode, against `OscillinkLattice(np.concatenate([Y, Ynew]))` from host anchors -- medians
of `--reps` timed calls after a warm-up, alternating, host clock around calls that end in a device synchronise -- with the
incremental route's own split (scores + selection / merge scan / graph assembly) and the bytes the merge scan has to read
against the time it took.

    python scripts/bench_append.py [--quick]        # every step in a child process under its own time limit; the first
                                                    # failure ends the run with a non-zero status and writes nothing;
                                                    # a complete run writes profiles/append_bench.json
    python scripts/bench_append.py --step N D k M   # one step, one JSON line on stdout
    rocprofv3 --kernel-trace --stats -d out -- python scripts/bench_append.py --step 100000 768 32 1024 --reps 3
                                                    # kernel times, in a run of its own
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 6.3e12  # achievable copy rate of the MI355X's HBM3E

# config 3 and 1M x 384 (panel route: butterfly-scored lists), and a dense-route lattice (MFMA-scored lists)
MFMA = [(8000, 64, 16, m) for m in (1, 256, 2048)]
FULL = [(100_000, 768, 32, m) for m in (1, 32, 256, 1024, 4096, 16384)] + [(1_000_000, 384, 16, m) for m in (1, 1024)] + MFMA
QUICK = [(100_000, 768, 32, m) for m in (1, 256, 4096)] + MFMA


def stats(ts):
    ts = np.asarray(ts) * 1e3
    return {"median_ms": float(np.median(ts)), "min_ms": float(ts.min()), "max_ms": float(ts.max()), "reps": int(ts.size)}


def step(N, D, k, M, reps):
    from oscillink_amd import OscillinkLattice
    from oscillink_amd import _native as nat

    rng = np.random.default_rng(N + D + k)
    Y = rng.standard_normal((N + M, D)).astype(np.float32)
    Ynew = np.ascontiguousarray(Y[N:])
    base = OscillinkLattice(Y[:N], kneighbors=k)
    L = nat.lib()

    def appended(mode):
        h = nat.Handle()
        t = time.perf_counter()
        rc = L.osc_create_appended(base._h, nat.f32(Ynew), M, mode, C.byref(h))
        dt = time.perf_counter() - t
        if rc != 0:
            return None, None
        info = [C.c_int32(0), C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int32(0), C.c_double(0), C.c_double(0), C.c_double(0),
                C.c_int64(0), C.c_int64(0), C.c_int32(0)]
        nat.check(L.osc_append_info(h, *[C.byref(x) for x in info]), h, "osc_append_info")
        L.osc_destroy(h)
        names = ("route", "new_rows", "merged_rows", "redo_rows", "family", "score_ms", "merge_ms", "back_half_ms", "merge_hits",
                 "merge_scan_bytes", "denied")
        return dt, {n: x.value for n, x in zip(names, info)}

    def fresh():
        t = time.perf_counter()
        lat = OscillinkLattice(Y, kneighbors=k)
        dt = time.perf_counter() - t
        lat.close()
        return dt

    times = {"fresh_create": [], "auto": [], "incremental": [], "rebuild": []}
    infos = {}
    for r in range(reps + 2):  # two warm-up rounds; the four forms alternate
        t = {"fresh_create": fresh()}
        for name, mode in (("auto", 0), ("incremental", 1), ("rebuild", 2)):
            t[name], infos[name] = appended(mode)
        if r >= 2:
            for n, v in t.items():
                if v is not None:
                    times[n].append(v)
    rec = {"N": N, "D": D, "k": k, "M": M, **{n: stats(v) for n, v in times.items() if v}}
    for n in ("auto", "incremental"):
        if infos.get(n):
            rec[n]["info"] = infos[n]
    inc = infos.get("incremental")
    if inc and inc["merge_scan_bytes"] > 0:
        rec["merge_scan"] = {"bytes": inc["merge_scan_bytes"], "floor_ms": 1e3 * inc["merge_scan_bytes"] / HBM_BYTES_PER_S,
                             "measured_ms": inc["merge_ms"]}
    base.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=0)
    ap.add_argument("--step", nargs=4, type=int, metavar=("N", "D", "k", "M"))
    ap.add_argument("--limit", type=int, default=240, help="seconds per step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "append_bench.json"))
    a = ap.parse_args()
    if a.step:
        print("APPEND_BENCH " + json.dumps(step(*a.step, a.reps or 20)), flush=True)
        return 0
    reps = a.reps or (5 if a.quick else 20)
    rows, complete = [], True
    for N, D, k, M in (QUICK if a.quick else FULL):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", str(N), str(D), str(k), str(M), "--reps", str(reps)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"step {(N, D, k, M)} passed its time limit of {a.limit} s: stopping", flush=True)
            complete = False
            break
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("APPEND_BENCH ")]
        if r.returncode != 0 or not line:
            print(f"step {(N, D, k, M)} failed ({r.returncode}): stopping\n{r.stdout[-2000:]}", flush=True)
            complete = False
            break
        rec = json.loads(line[0][len("APPEND_BENCH "):])
        rows.append(rec)
        inc = rec.get("incremental", {})
        print(f"N {N} D {D} k {k} M {M}: fresh {rec['fresh_create']['median_ms']:.2f} ms, auto {rec['auto']['median_ms']:.2f} "
              f"(route {rec['auto']['info']['route']}), incremental {inc.get('median_ms', float('nan')):.2f}, "
              f"rebuild {rec['rebuild']['median_ms']:.2f}; split {inc.get('info', {}).get('score_ms', 0):.2f} / "
              f"{inc.get('info', {}).get('merge_ms', 0):.2f} / {inc.get('info', {}).get('back_half_ms', 0):.2f}", flush=True)
    if not complete:  # a partial run replaces no earlier result
        print(f"incomplete run: {a.out} is left as it was", flush=True)
        return 1
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"quick": bool(a.quick), "reps": reps, "rows": rows}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""OscillinkLattice.update against a fresh create and against remove + append: where the planner's
threshold comes from.

For a base lattice, M random ids and M new rows: the updated handle's creation (osc_create_updated, what `update` spends
its time in) in rebuild, forced-incremental and auto mode, against `OscillinkLattice(Y2)` from host anchors (Y2 = Y with the
rows replaced) and against what an edit costs without `update`, osc_create_removed followed by osc_create_appended (both in
auto mode) -- medians of `--reps` timed calls after two warm-up rounds, the five forms alternating in one process, host
clock around calls that end in a device synchronise -- with the incremental route's redo count, merge hits and phase split
(scores + selection / merge scans / graph assembly) and what auto mode chose.

    python scripts/bench_update.py [--quick]        # every step in a child process under its own time limit; the first
                                                    # failure ends the run with a non-zero status and writes nothing;
                                                    # a complete run writes profiles/update_bench.json
    python scripts/bench_update.py --step N D k M   # one step, one JSON line on stdout
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

MS = (1, 8, 32, 128, 1024)
# config 3 and 1M x 384 (panel route: butterfly-scored lists), and a dense-route lattice (MFMA-scored lists)
FULL = [(100_000, 768, 32, m) for m in MS] + [(1_000_000, 384, 16, m) for m in MS] + [(8000, 64, 16, m) for m in MS]
QUICK = [(100_000, 768, 32, m) for m in (1, 128)] + [(8000, 64, 16, 1)]


def stats(ts):
    ts = np.asarray(ts) * 1e3
    return {"median_ms": float(np.median(ts)), "min_ms": float(ts.min()), "max_ms": float(ts.max()), "reps": int(ts.size)}


def step(N, D, k, M, reps):
    from oscillink_amd import OscillinkLattice
    from oscillink_amd import _native as nat

    rng = np.random.default_rng(N + D + k)
    Y = rng.standard_normal((N, D)).astype(np.float32)
    ids = np.sort(rng.choice(N, size=M, replace=False)).astype(np.int32)
    Ynew = rng.standard_normal((M, D)).astype(np.float32)
    Y2 = Y.copy()
    Y2[ids] = Ynew
    base = OscillinkLattice(Y, kneighbors=k)
    L = nat.lib()
    names = ("route", "replaced_rows", "merged_rows", "redo_rows", "family", "score_ms", "merge_ms", "back_half_ms", "merge_hits",
             "denied")

    def updated(mode):
        h = nat.Handle()
        t = time.perf_counter()
        rc = L.osc_create_updated(base._h, nat.i32(ids), nat.f32(Ynew), M, mode, C.byref(h))
        dt = time.perf_counter() - t
        if rc != 0:
            return None, None
        info = [C.c_int32(0), C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int32(0), C.c_double(0), C.c_double(0), C.c_double(0),
                C.c_int64(0), C.c_int32(0)]
        nat.check(L.osc_update_info(h, *[C.byref(x) for x in info]), h, "osc_update_info")
        L.osc_destroy(h)
        return dt, {n: x.value for n, x in zip(names, info)}

    def remove_then_append():
        h1, h2 = nat.Handle(), nat.Handle()
        t = time.perf_counter()
        rc = L.osc_create_removed(base._h, nat.i32(ids), M, 0, C.byref(h1))
        if rc != 0:
            return None
        rc = L.osc_create_appended(h1, nat.f32(Ynew), M, 0, C.byref(h2))
        dt = time.perf_counter() - t
        L.osc_destroy(h1)
        if rc != 0:
            return None
        L.osc_destroy(h2)
        return dt

    def fresh():
        t = time.perf_counter()
        lat = OscillinkLattice(Y2, kneighbors=k)
        dt = time.perf_counter() - t
        lat.close()
        return dt

    times = {"fresh_create": [], "rebuild": [], "incremental": [], "auto": [], "remove_then_append": []}
    infos = {}
    for r in range(reps + 2):  # two warm-up rounds; the five forms alternate
        t = {"fresh_create": fresh()}
        for name, mode in (("rebuild", 2), ("incremental", 1), ("auto", 0)):
            t[name], infos[name] = updated(mode)
        t["remove_then_append"] = remove_then_append()
        if r >= 2:
            for n, v in t.items():
                if v is not None:
                    times[n].append(v)
    rec = {"N": N, "D": D, "k": k, "M": M, **{n: stats(v) for n, v in times.items() if v}}
    if infos.get("incremental"):
        rec["incremental"]["info"] = infos["incremental"]
    rec["auto_route"] = None if infos.get("auto") is None else infos["auto"]["route"]
    base.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=0)
    ap.add_argument("--step", nargs=4, type=int, metavar=("N", "D", "k", "M"))
    ap.add_argument("--limit", type=int, default=240, help="seconds per step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update_bench.json"))
    a = ap.parse_args()
    if a.step:
        print("UPDATE_BENCH " + json.dumps(step(*a.step, a.reps or 20)), flush=True)
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
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("UPDATE_BENCH ")]
        if r.returncode != 0 or not line:
            print(f"step {(N, D, k, M)} failed ({r.returncode}): stopping\n{r.stdout[-2000:]}", flush=True)
            complete = False
            break
        rec = json.loads(line[0][len("UPDATE_BENCH "):])
        rows.append(rec)
        inc = rec.get("incremental", {})
        info = inc.get("info", {})

        def cell(name):
            c = rec.get(name)
            return "-" if not c else f"{c['median_ms']:.2f} [{c['min_ms']:.2f}, {c['max_ms']:.2f}]"

        print(f"N {N} D {D} k {k} M {M}: fresh {cell('fresh_create')}, rebuild {cell('rebuild')}, incremental {cell('incremental')}, "
              f"auto {cell('auto')} (route {rec['auto_route']}), remove+append {cell('remove_then_append')}; redo {info.get('redo_rows')}, "
              f"hits {info.get('merge_hits')}, split {info.get('score_ms', 0):.2f} / {info.get('merge_ms', 0):.2f} / "
              f"{info.get('back_half_ms', 0):.2f}", flush=True)
    if not complete:  # a partial run replaces no earlier result
        print(f"incomplete run: {a.out} is left as it was", flush=True)
        return 1
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"quick": bool(a.quick), "reps": reps, "rows": rows}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

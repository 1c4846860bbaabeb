"""`keep_state=True` of OscillinkLattice.append / remove / update: what carrying U on the device costs
and what it buys.

Per lattice shape: three `settle()` calls, then `update` of 1 row, of 100 rows and of 1 % of the rows, `append` of 1 row and
`remove` of 1 row.  Every call is timed in three forms --
    plain       the call as it was: U = Y afterwards
    keep        the call with keep_state=True
    round_trip  the same U by way of the host: `U = lat.U`, the call, the rule applied to U with NumPy, `lat.U = U2`
                (its four parts are reported as well)
-- medians of `--reps` device-synchronised repeats after one warm-up round, the three forms alternating in one process,
host clock around work that ends in a device synchronise.  Every repeat starts from a lattice built anew from the anchors
whose state is the saved result of the three settles, uploaded, with the host mirror of U dropped, so that `lat.U` reads the
device as it does after a settle.  Then the effect, once per call: `receipt()["deltaH_total"]` right after the plain and
the keep form, and the next settle's iteration count and time.

    python scripts/bench_keep_state.py [--quick]    # every shape in a child process under its own time limit; the first
                                                    # failure ends the run with a non-zero status and writes nothing;
                                                    # a complete run writes profiles/keep_state.json
    python scripts/bench_keep_state.py --step N D k # one shape, one JSON line on stdout
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FULL = [(100_000, 768, 32), (20_000, 128, 32)]  # config 3 and a lattice a twentieth of its bytes
QUICK = [(20_000, 128, 32)]


def med(ts):
    ts = np.asarray(ts) * 1e3
    return {"median_ms": float(np.median(ts)), "min_ms": float(ts.min()), "max_ms": float(ts.max()), "reps": int(ts.size)}


def step(N, D, k, reps):
    from oscillink_amd import OscillinkLattice
    from oscillink_amd import _native as nat

    rng = np.random.default_rng(N + D + k)
    Y = rng.standard_normal((N, D)).astype(np.float32)
    psi = Y[:32].mean(axis=0)
    psi = (psi / (np.linalg.norm(psi) + 1e-12)).astype(np.float32)
    L = nat.lib()

    def wait():
        nat.check(L.osc_device_synchronize(0), None, "osc_device_synchronize")

    base = OscillinkLattice(Y, kneighbors=k)
    base.set_query(psi)
    settles = [base.settle() for _ in range(3)]
    U3 = base.U.copy()
    base.close()

    def settled_lattice():
        lat = OscillinkLattice(Y, kneighbors=k)
        lat.set_query(psi)
        lat.U = U3
        lat._U_host = None  # (as after a settle: the next `lat.U` reads the device)
        wait()
        return lat

    pct = max(1, N // 100)
    calls = [("update_1", "update", 1), ("update_100", "update", 100), (f"update_{pct}", "update", pct), ("append_1", "append", 1),
             ("remove_1", "remove", 1)]
    rows = []
    for name, op, M in calls:
        ids = np.sort(rng.choice(N, size=M, replace=False))
        Ynew = rng.standard_normal((M, D)).astype(np.float32)

        def call(lat, **kw):
            if op == "append":
                lat.append(Ynew, **kw)
            elif op == "remove":
                lat.remove(ids, **kw)
            else:
                lat.update(ids, Ynew, **kw)

        def rule(U):
            if op == "append":
                return np.concatenate([U, Ynew])
            if op == "remove":
                return np.delete(U, ids, axis=0)
            U[ids] = Ynew  # (in place: the cheapest honest form of the workaround)
            return U

        times = {"plain": [], "keep": [], "round_trip": []}
        parts = {"read_back": [], "call": [], "host_rule": [], "assign": []}
        effect = {}
        for r in range(reps + 1):  # one warm-up round; the three forms alternate
            for form in ("plain", "keep", "round_trip"):
                lat = settled_lattice()
                t0 = time.perf_counter()
                if form == "plain":
                    call(lat)
                elif form == "keep":
                    call(lat, keep_state=True)
                else:
                    U = lat.U
                    t1 = time.perf_counter()
                    call(lat)
                    wait()
                    t2 = time.perf_counter()
                    U2 = rule(U)
                    t3 = time.perf_counter()
                    lat.U = U2
                wait()
                t4 = time.perf_counter()
                if r >= 1:
                    times[form].append(t4 - t0)
                    if form == "round_trip":
                        for pname, v in zip(("read_back", "call", "host_rule", "assign"), (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                            parts[pname].append(v)
                if r == reps and form in ("plain", "keep"):
                    dH = float(lat.receipt()["deltaH_total"])
                    st = lat.settle()
                    effect[form] = {"deltaH_total": dH, "next_settle_iters": int(st["iters"]), "next_settle_ms": float(st["t_ms"]),
                                    "next_settle_res": float(st["res"])}
                lat.close()
        rows.append({"call": name, "op": op, "rows": M, **{f: med(v) for f, v in times.items()},
                     "round_trip_parts": {p: med(v) for p, v in parts.items()},
                     "carry_adds_ms": med(times["keep"])["median_ms"] - med(times["plain"])["median_ms"],
                     "cold": effect["plain"], "carried": effect["keep"]})
    return {"N": N, "D": D, "k": k, "settles_before": [{"iters": int(s["iters"]), "t_ms": float(s["t_ms"])} for s in settles],
            "calls": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--step", nargs=3, type=int, metavar=("N", "D", "k"))
    ap.add_argument("--limit", type=int, default=300, help="seconds per shape")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keep_state.json"))
    a = ap.parse_args()
    if a.step:
        print("KEEP_STATE_BENCH " + json.dumps(step(*a.step, a.reps)), flush=True)
        return 0
    shapes = []
    for N, D, k in (QUICK if a.quick else FULL):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", str(N), str(D), str(k), "--reps", str(a.reps)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"shape {(N, D, k)} passed its time limit of {a.limit} s: stopping", flush=True)
            return 1
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("KEEP_STATE_BENCH ")]
        if r.returncode != 0 or not line:
            print(f"shape {(N, D, k)} failed ({r.returncode}): stopping\n{r.stdout[-2000:]}", flush=True)
            return 1
        rec = json.loads(line[0][len("KEEP_STATE_BENCH "):])
        shapes.append(rec)
        print(f"{N} x {D}, k {k}   (ms, medians of {a.reps})")
        print(f"  {'call':<13}{'plain':>8}{'keep':>8}{'adds':>7}{'round trip':>12}  (read {'':>1}call  rule  assign)   dH cold -> carried"
              f"        next settle cold -> carried")
        for c in rec["calls"]:
            p = c["round_trip_parts"]
            print(f"  {c['call']:<13}{c['plain']['median_ms']:8.2f}{c['keep']['median_ms']:8.2f}{c['carry_adds_ms']:7.2f}"
                  f"{c['round_trip']['median_ms']:12.2f}  ({p['read_back']['median_ms']:.1f} {p['call']['median_ms']:.1f} "
                  f"{p['host_rule']['median_ms']:.1f} {p['assign']['median_ms']:.1f})   {c['cold']['deltaH_total']:.4g} -> "
                  f"{c['carried']['deltaH_total']:.4g}   {c['cold']['next_settle_iters']} it {c['cold']['next_settle_ms']:.2f} ms -> "
                  f"{c['carried']['next_settle_iters']} it {c['carried']['next_settle_ms']:.2f} ms", flush=True)
    if not a.quick:
        with open(a.out, "w") as f:
            json.dump({"what": "scripts/bench_keep_state.py on one MI355X", "reps": a.reps, "shapes": shapes}, f, indent=1)
            f.write("\n")
        print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Host overhead of the CG driver, this build against the library built from the parent commit, in alternating FRESH child
processes (one library per process, chosen by OSC_LIB_PATH): per round and build, (1) `reset_U()` + `settle(max_iters=4)` at
20 000 x 128, k = 8 -- the launch-bound regime, 50 warm-up and 400 timed steps, each device-synchronised -- and (2)
`bench.py --gpus 1 --steps 20 --warmup 3`.  Reports per build the median and the p10-p90 band over the rounds of the child
medians (settle, us) and of bench.py's value (settles/s); stops at the first child that fails.

    python scripts/bench_cg_loop_ab.py --parent-lib PATH [--rounds 5] [--out FILE.json]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def settle_child():
    import oscillink_amd as amd
    from oscillink_amd import _native as nat

    rng = np.random.default_rng(0)
    N, D, k = 20000, 128, 8
    Y = rng.standard_normal((N, D), dtype=np.float32)
    psi = Y[:32].mean(axis=0)
    lat = amd.Oscillink(Y, kneighbors=k)
    lat.set_query((psi / np.linalg.norm(psi)).astype(np.float32))
    ts, iters = [], 0
    for i in range(450):
        nat.lib().osc_device_synchronize(0)
        t = time.perf_counter()
        lat.reset_U(wait=False)
        iters = lat.settle(max_iters=4, tol=1e-3)["iters"]
        nat.lib().osc_device_synchronize(0)
        if i >= 50:
            ts.append(1e6 * (time.perf_counter() - t))
    a, info = np.asarray(ts), lat.build_info()
    print(json.dumps({"median_us": float(np.median(a)), "p10_us": float(np.percentile(a, 10)), "p90_us": float(np.percentile(a, 90)),
                      "iters": int(iters), "x_ring_slots": info["x_ring_slots"], "src_blocks": info["apply_src_blocks"]}))


def band(vals):
    a = np.asarray(vals, dtype=np.float64)
    return {"median": float(np.median(a)), "p10": float(np.percentile(a, 10)), "p90": float(np.percentile(a, 90)), "n": int(a.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="liboscillink_hip.so built from the parent commit")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--settle-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.settle_child:
        return settle_child()
    libs = {"parent": os.path.abspath(a.parent_lib), "this": os.path.join(ROOT, "oscillink_amd", "liboscillink_hip.so")}
    rec = {"settle_small": {"parent": [], "this": []}, "bench": {"parent": [], "this": []}}

    def child(cmd, lib, limit):
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable] + cmd, cwd=ROOT, env=dict(os.environ, OSC_LIB_PATH=lib),
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:
            sys.exit(f"child {cmd} failed with status {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])

    for rnd in range(a.rounds):
        for name in ("parent", "this"):
            rec["settle_small"][name].append(child([os.path.abspath(__file__), "--settle-child"], libs[name], 120))
            print(rnd, name, "settle", rec["settle_small"][name][-1], flush=True)
        for name in ("parent", "this"):
            b = child(["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "3"], libs[name], 240)
            rec["bench"][name].append({k: b[k] for k in ("value", "ms_per_step", "ms_per_step_p10", "ms_per_step_p90")})
            print(rnd, name, "bench", rec["bench"][name][-1], flush=True)
    rec["summary"] = {"settle_small_median_us": {n: band([c["median_us"] for c in rec["settle_small"][n]]) for n in libs},
                      "bench_value": {n: band([c["value"] for c in rec["bench"][n]]) for n in libs}}
    print(json.dumps(rec["summary"]))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

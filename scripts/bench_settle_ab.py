"""The headline step (bench.py: `reset_U` + `settle`, config 3: N = 100 000, D = 768, k = 32, dt 1, 12 iterations at most,
tol 1e-3) of this build against the library built from the parent commit, alternating in ONE process on the same lattice
inputs, so that clock and thermal drift hit both alike.  Both libraries are driven through the C ABI alone (the calls a
step makes have the same signatures in both builds).  Per seed: both lattices are created, warmed up, then `--rounds`
alternations of `--steps` steps each (parent, this, parent, this, ...); every step is device-synchronised before and
after and timed on its own.  Reports median and p10 / p90 of the per-step times per build, the same for the U* solve, the
create times, and whether the settled states are the same bytes.  Writes one JSON line (and --out).

    python scripts/bench_settle_ab.py --parent-lib PATH [--seeds 0,1,2 --rounds 5 --steps 20 --warmup 5]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CALLS = ("osc_create", "osc_destroy", "osc_set_query", "osc_set_lams", "osc_set_U", "osc_get_U", "osc_settle", "osc_solve_ustar",
         "osc_device_synchronize", "osc_last_error")


class Raw:
    """One lattice of one build of the library."""

    def __init__(self, path, Y, psi, k):
        from oscillink_amd import _native as nat

        self.nat, self.lib = nat, C.CDLL(path)
        for name in CALLS:
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = nat.SIGNATURES[name]
        self.h = nat.Handle()
        self.N, self.D = Y.shape
        self.sync()
        t = time.perf_counter()
        self.ok(self.lib.osc_create(nat.f32(Y), self.N, self.D, k, 1.0, 0, -1, 0, 1, C.byref(self.h)), "osc_create")
        self.sync()
        self.create_ms = 1e3 * (time.perf_counter() - t)
        self.ok(self.lib.osc_set_query(self.h, nat.f32(psi), None), "osc_set_query")
        self.ok(self.lib.osc_set_lams(self.h, 1.0, 0.5, 4.0), "osc_set_lams")

    def ok(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what}: status {rc}: {self.lib.osc_last_error(self.h)}")

    def sync(self):
        self.lib.osc_device_synchronize(0)

    def step(self, max_iters, tol):
        """reset_U(wait=False) + settle, as bench.py's step; (ms, iters, res)"""
        it, rs, ms = C.c_int32(0), C.c_float(0.0), C.c_double(0.0)
        self.sync()
        t = time.perf_counter()
        self.ok(self.lib.osc_set_U(self.h, None), "osc_set_U")
        self.ok(self.lib.osc_settle(self.h, 1.0, max_iters, tol, 1, 1, 0.0, C.byref(it), C.byref(rs), C.byref(ms)), "osc_settle")
        self.sync()
        return 1e3 * (time.perf_counter() - t), int(it.value), float(rs.value)

    def ustar(self):
        it, rs, ms = C.c_int32(0), C.c_float(0.0), C.c_double(0.0)
        self.sync()
        t = time.perf_counter()
        self.ok(self.lib.osc_solve_ustar(self.h, 1e-4, 64, None, C.byref(it), C.byref(rs), C.byref(ms)), "osc_solve_ustar")
        self.sync()
        return 1e3 * (time.perf_counter() - t), int(it.value), float(rs.value)

    def U(self):
        out = np.empty((self.N, self.D), np.float32)
        self.ok(self.lib.osc_get_U(self.h, self.nat.f32(out)), "osc_get_U")
        return out

    def close(self):
        self.lib.osc_destroy(self.h)


def summary(ts):
    a = np.asarray(ts, dtype=np.float64)
    p10, med, p90 = (float(np.percentile(a, q)) for q in (10, 50, 90))
    return {"median_ms": med, "p10_ms": p10, "p90_ms": p90, "spread_ms": p90 - p10, "n": int(a.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="liboscillink_hip.so built from the parent commit")
    ap.add_argument("--N", type=int, default=100_000)
    ap.add_argument("--D", type=int, default=768)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--tol", type=float, default=1e-3)
    ap.add_argument("--max-iters", type=int, default=12)
    ap.add_argument("--seeds", default="0,1,2")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from oscillink_amd import _native as nat

    rec = {"N": a.N, "D": a.D, "k": a.k, "tol": a.tol, "max_iters": a.max_iters, "rounds": a.rounds, "steps": a.steps,
           "warmup": a.warmup, "seeds": []}
    all_t = {"parent": [], "this": []}
    all_u = {"parent": [], "this": []}
    for seed in (int(s) for s in a.seeds.split(",")):
        rng = np.random.default_rng(seed)
        Y = rng.standard_normal((a.N, a.D)).astype(np.float32)
        psi = Y[:32].mean(axis=0)
        psi = (psi / (np.linalg.norm(psi) + 1e-12)).astype(np.float32)
        lats = {"parent": Raw(a.parent_lib, Y, psi, a.k), "this": Raw(nat.LIB_PATH, Y, psi, a.k)}
        last = {}
        for name, lt in lats.items():
            for _ in range(a.warmup):
                last[name] = lt.step(a.max_iters, a.tol)
        same = bool(last["parent"][1:] == last["this"][1:] and np.array_equal(lats["parent"].U(), lats["this"].U()))
        ts = {"parent": [], "this": []}
        for _ in range(a.rounds):
            for name in ("parent", "this"):
                for _ in range(a.steps):
                    ts[name].append(lats[name].step(a.max_iters, a.tol)[0])
        us = {"parent": [], "this": []}
        for name, lt in lats.items():
            lt.ustar()  # (first use of this kind of solve)
        for _ in range(a.rounds):
            for name in ("parent", "this"):
                us[name].append(lats[name].ustar()[0])
        rec["seeds"].append({"seed": seed, "iters": last["this"][1], "same_bytes": same,
                             "create_ms": {n: lats[n].create_ms for n in lats},
                             "step": {n: summary(ts[n]) for n in ts}, "ustar": {n: summary(us[n]) for n in us}})
        for n in ts:
            all_t[n] += ts[n]
            all_u[n] += us[n]
        for lt in lats.values():
            lt.close()
    rec["step"] = {n: summary(all_t[n]) for n in all_t}
    rec["ustar"] = {n: summary(all_u[n]) for n in all_u}
    gain = rec["step"]["parent"]["median_ms"] - rec["step"]["this"]["median_ms"]
    noise = max(rec["step"]["parent"]["spread_ms"], rec["step"]["this"]["spread_ms"])
    rec["gain_ms"] = gain
    rec["noise_ms"] = noise
    rec["faster_beyond_noise"] = bool(gain > noise)
    rec["same_bytes"] = all(s["same_bytes"] for s in rec["seeds"])
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

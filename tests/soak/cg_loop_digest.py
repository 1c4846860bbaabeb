#!/usr/bin/env python3
"""Digest of what the general CG driver (csrc/osc_solve.hip: run_cg) computes, for comparing two builds of the library bit
for bit: run it once per build (OSC_LIB_PATH selects the library; this tree's build when unset), each in a fresh process,
and compare the two files byte for byte -- a refactor of the driver must leave them equal.

One process, seed 7, k = 8.  Per case the per-handle switches go into os.environ before Oscillink(...), then
    settle(12, 1e-3) . reset_U . settle(12, 1e-3) (the right guess) . settle(40, 1e-6) (the guess too low: the solve goes
    on) . settle(2, 1e-6) (stops at max_iters) . solve_Ustar(1e-4, 64, use_cache=False)
and per step the iteration count, the residual history as float32 bit patterns and sha256 of the state; at the end the
build_info() counters of the driver, and sha256 of the graph (two files that differ there differ before any solve).
Shapes: the smallest that reach each path -- the one-launch solve, the plain apply with a padded pitch, the slab apply, two
2048-column windows, and the blocked apply with each ring / x-update / INIT / anchor-image switch, gates, a chain prior and
a column window; then a one-rank RCCL communicator with the stop test beside the solve and inside it.
usage: cg_loop_digest.py OUT.json"""
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import oscillink_amd as amd  # noqa: E402
from oscillink_amd.sharding import rccl_unique_id  # noqa: E402

SWITCHES = ["OSC_SMALL_PATH", "OSC_SPMM_XS", "OSC_SPMM_BLOCKED", "OSC_LD", "OSC_X_RING", "OSC_X_DEFER", "OSC_BLK_INIT",
            "OSC_ANCHOR_SLAB", "OSC_ANCHOR_WY", "OSC_FAKE_COL_SHARD", "OSC_COMM_OVERLAP", "OSC_SHARD"]
COUNTERS = ["blocked_applies", "x_ring_slots", "x_ring_flushes", "x_ring_passes", "cached_inits", "rows_to_slab_launches",
            "y_to_u_copies", "apply_src_blocks", "small_solves"]
BLOCKED = {"OSC_SPMM_XS": "1", "OSC_SPMM_BLOCKED": "3", "OSC_LD": "128"}


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def step(lat, iters, state):
    hist = np.asarray(lat.residual_history(), dtype=np.float32).view(np.uint32)
    return {"iters": int(iters), "history": [int(v) for v in hist], "state": sha(state)}


def run_case(name, N, D, env, gates=False, chain=False, comm=False):
    for s in SWITCHES:
        os.environ.pop(s, None)
    os.environ.update(env)
    rng = np.random.default_rng(7)
    Y = rng.standard_normal((N, D), dtype=np.float32)
    psi = rng.standard_normal(D).astype(np.float32)
    psi /= np.linalg.norm(psi)
    g = rng.random(N).astype(np.float32) if gates else None
    lat = amd.Oscillink(Y, kneighbors=8, **({"comm": (rccl_unique_id(), 0, 1)} if comm else {}))
    lat.set_query(psi, gates=g)
    if chain:
        lat.add_chain([int(c) for c in rng.choice(N, size=9, replace=False)], lamP=0.25)
    steps = []
    for reset, max_iters, tol in [(False, 12, 1e-3), (True, 12, 1e-3), (False, 40, 1e-6), (False, 2, 1e-6)]:
        if reset:
            lat.reset_U()
        st = lat.settle(max_iters=max_iters, tol=tol)
        steps.append(step(lat, st["iters"], lat.U))
    us = lat.solve_Ustar(tol=1e-4, max_iters=64, use_cache=False)
    steps.append(step(lat, lat.last_ustar["iters"], us))
    info = lat.build_info()
    out = {"case": name, "N": N, "D": D, "env": env, "graph": sha(*lat.graph_csr()), "steps": steps,
           "counters": {c: int(info[c]) for c in COUNTERS}}
    lat.close()
    print(name, [s["iters"] for s in steps], out["counters"], flush=True)
    return out


def main():
    cases = [run_case("one_launch", 700, 32, {}),
             run_case("plain_padded", 2500, 100, {"OSC_SMALL_PATH": "0", "OSC_SPMM_XS": "0"}),
             run_case("slab", 6500, 96, {"OSC_SPMM_XS": "1", "OSC_SPMM_BLOCKED": "0", "OSC_LD": "128"}),
             run_case("two_windows", 6500, 2100, {"OSC_SPMM_XS": "0"})]
    variants = [("default", {}), ("ring0", {"OSC_X_RING": "0"}), ("ring2", {"OSC_X_RING": "2"}), ("ring4", {"OSC_X_RING": "4"}),
                ("defer0", {"OSC_X_DEFER": "0"}), ("defer2", {"OSC_X_DEFER": "2"}), ("init0", {"OSC_BLK_INIT": "0"}),
                ("init2", {"OSC_BLK_INIT": "2"}), ("no_anchor_slab", {"OSC_ANCHOR_SLAB": "0"}), ("no_anchor_wy", {"OSC_ANCHOR_WY": "0"}),
                ("window_1_of_2", {"OSC_FAKE_COL_SHARD": "1/2"})]
    for name, env in variants:
        cases.append(run_case("blocked_" + name, 20011, 96, {**BLOCKED, **env}))
    cases.append(run_case("blocked_gates", 20011, 96, dict(BLOCKED), gates=True))
    cases.append(run_case("blocked_chain", 20011, 96, dict(BLOCKED), chain=True))
    for overlap in ("1", "0"):  # the two sharded stop tests, as tests/test_gpu_multirank.py sets them up
        cases.append(run_case("one_rank_overlap" + overlap, 3000, 96, {"OSC_SMALL_PATH": "0", "OSC_COMM_OVERLAP": overlap}, comm=True))
    with open(sys.argv[1], "w") as f:
        json.dump(cases, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()

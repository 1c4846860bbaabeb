#!/usr/bin/env python3
"""Benchmark of the lattice settle hot path on MI355X (BASELINE.json metric: settles/sec + ms/settle at N x D).

    python bench.py --gpus 1 --steps 20 --warmup 3
    python bench.py --gpus 8 --steps 20 --warmup 3          # starts its own 8 ranks (one process per GPU)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W              # ... or runs as one rank of a launcher's job

Workload: BASELINE.json configs[2] -- N=100000, D=768, k=32, fp32, synthetic Gaussian anchors
(default_rng(seed).standard_normal), psi = normalise(mean of the first 32 rows), lams (1.0, 0.5, 4.0), row cap 1.0.
One *step* = `reset_U` (U <- Y on the device, a 307 MB device-to-device copy that is INSIDE the timed step) + one
`settle(dt=1, max_iters=12, tol=1e-3)` from that state, so every step does identical work: 4-5 CG iterations.  The
graph build (kNN + mutual + cap + Laplacian weights) is timed separately, as the reference's own harness does
(scripts/scale_benchmark.py:44-46).

Protocol (the reference's scale benchmark seeds its runs): one seed (0) unless --seeds says
otherwise, W warm-up steps and then EXACTLY K timed steps between barrier + device drain on both sides; every step is
also timed by itself (the host returns from a settle when it has read the last residual).  `ms_per_step` = median
over all timed steps (max over the ranks of the per-rank medians), p10 / p90 beside it, `value` = 1000 / median; the
bracketed regions' mean is reported as `ms_per_step_mean` (max over ranks).  --full times seeds {0, 1, 2} on one GPU
(K steps each) and adds the measurements listed below.

--dump-outputs DIR: after the timed steps, what the last timed step of the first seed computed is written as float32 /
float64 .npy files (rank 0 writes; under a communicator every rank takes part in the read-back):
  U.npy           : rows of the settled state U (N x D, float32) -- all of them when U fits in 48 MiB, else a fixed
                    sample of 48 MiB worth of rows (default_rng(DUMP_SAMPLE_SEED), sorted)
  U_rows.npy      : the row ids of U.npy (float64)
  settle_iters.npy, settle_res.npy : what that settle() returned (CG iterations, final residual; float64, shape (1,))
The inputs depend on the seeds and the size arguments only, so two builds run with the same arguments can be compared
output for output.

N > 1: strong scaling of the same settle -- the CG is column-sharded (per-column alpha/beta), each rank owns a
D/N column slab and the only per-iteration exchange is one RCCL all-reduce(max) of the residual.  This script uses no
PyTorch: a launcher only provides RANK / LOCAL_RANK / WORLD_SIZE / MASTER_PORT; the ncclUniqueId travels through a
rendezvous directory on the node, the timing barrier and the max over ranks go through the library's own communicator
(osc_comm_allreduce_f64).  Started WITHOUT a launcher (`python bench.py --gpus N`, no RANK / WORLD_SIZE in the
environment) the script is its own launcher: the parent never loads the library or touches a GPU, checks that N
devices are visible (else exit 3 before any build), builds the library, starts N fresh child processes of itself with
the launcher environment set, waits with a time limit, kills stragglers, forwards rank 0's ONE JSON line and exits
with the worst child's code.  If the communicator cannot be set up on every rank the run FAILS (exit code 3, no JSON
line): N independent replicas are not a measurement of this job.  The JSON line carries `comm` = what the library's
communicator reports (kind "rccl", world N, RCCL's version) so that a reader can see RCCL really spanned N ranks.

Prints ONE JSON line on rank 0 (metric, value, unit, higher_is_better, dtype, ms_per_step, ...) with this extra
object, taken from the timed steps themselves:
  roofline        : the operator apply (SpMM, the CG matvec): algorithmic bytes per launch / mean launch time (HIP
                    events on the library's own stream) against the 8 TB/s HBM3E peak; `settle` = the whole settle's
                    algorithmic bytes / ms_per_step; `traffic` only from a committed PMC profile taken with THIS build;
                    `per_rank` = every rank's window apply against its own algorithmic bytes.
and, with --full only (each takes runs of its own after the timed region; --no-extras / --no-cpu-baseline drop them again):
  knn             : the lattice build: route, device time, GEMM+top-k kernel time, 2 N^2 D flops against the MFMA peak.
  ustar_solve_ms, receipt_ms : medians of the stationary solve and of light / full receipts (U* resident).
  first_settle_ms, mispredict_settle_ms : what a fresh handle's first settle and a settle whose iteration count the
                    handle guessed wrong cost (the loop predicts its last iteration from the previous solve).
  cpu_baseline    : the CPU oracle (NumPy/SciPy CSR restatement, oracle/) on the same settle: warm-up + >= 3
                    repetitions, median and p10/p90, column-parallel on the host cores.
"""
import argparse
import copy
import ctypes as C
import glob
import json
import math
import os
import shutil
import signal
import socket
import subprocess
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

DUMP_SAMPLE_SEED = 20240917  # --dump-outputs: the fixed row sample of U when U is larger than DUMP_U_BYTES
DUMP_U_BYTES = 48 << 20
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
MFMA_F16_DENSE_TFLOPS = 2500.0  # dense f16/bf16 matrix peak (the prefilter route's GEMM)
MFMA_F32_TFLOPS = 157.3  # fp32 matrix peak (the exact route's GEMM)


# ---- rendezvous without a distributed runtime: a directory on the node -------------------------------------------
class FileRendezvous:
    """Single-node exchange of small blobs between the ranks one launcher started (same parent process, same
    MASTER_PORT): rank 0 publishes, everyone polls.  Used for the 128-byte communicator id and for agreeing on whether
    every rank joined the communicator."""

    def __init__(self, rank, world):
        self.rank, self.world = rank, world
        tag = f"{os.environ.get('MASTER_PORT', '0')}_{os.getppid()}_{os.environ.get('TORCHELASTIC_RESTART_COUNT', '0')}"
        self.dir = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"osc_rdzv_{tag}")
        os.makedirs(self.dir, exist_ok=True)

    def put(self, name, blob: bytes):
        tmp = os.path.join(self.dir, f".{name}.{self.rank}.tmp")
        with open(tmp, "wb") as f:
            f.write(blob)
        os.replace(tmp, os.path.join(self.dir, name))

    def get(self, name, timeout_s=300.0) -> bytes:
        path = os.path.join(self.dir, name)
        t0 = time.time()
        while not os.path.exists(path):
            if time.time() - t0 > timeout_s:
                raise TimeoutError(f"rendezvous: {name} never appeared in {self.dir}")
            time.sleep(0.002)
        with open(path, "rb") as f:
            return f.read()

    def gather(self, name, blob: bytes, timeout_s=300.0):
        """Every rank contributes a blob; returns all of them (also serves as a barrier)."""
        self.put(f"{name}.{self.rank}", blob)
        return [self.get(f"{name}.{r}", timeout_s) for r in range(self.world)]

    def close(self, timeout_s=60.0):
        """Leave the rendezvous.  Rank 0 removes the directory, but only after every other rank has said it will not
        read from it again (a rank still polling a file would otherwise wait for its timeout)."""
        if self.rank != 0:
            self.put(f"bye.{self.rank}", b"1")
            return
        t0 = time.time()
        while time.time() - t0 < timeout_s and not all(
                os.path.exists(os.path.join(self.dir, f"bye.{r}")) for r in range(1, self.world)):
            time.sleep(0.002)
        shutil.rmtree(self.dir, ignore_errors=True)


class StdoutToStderr:
    """Route the PROCESS's stdout (fd 1) to stderr for a while: RCCL prints its version banner to stdout when a communicator
    is created, and this script's stdout is one JSON line."""

    def __enter__(self):
        sys.stdout.flush()
        self.saved = os.dup(1)
        os.dup2(2, 1)
        return self

    def __exit__(self, *exc):
        sys.stdout.flush()
        os.dup2(self.saved, 1)
        os.close(self.saved)
        return False


# ---- self-launcher: `python bench.py --gpus N` without torch.distributed.run ----------------------------------------
EXIT_REFUSED = 3  # the job this command line asks for cannot be measured here (too few devices / no communicator)


def visible_device_count() -> int:
    """HIP devices this process tree would see, counted by a short-lived CHILD (the launcher parent must never
    initialise a GPU itself: its children are fresh processes, and a parent holding a context would also occupy one of
    the box's few process slots on the card).  0 when the runtime is missing or reports an error."""
    code = ("import ctypes\n"
            "n = ctypes.c_int(0)\n"
            "try:\n"
            "    lib = None\n"
            "    for name in ('libamdhip64.so', '/opt/rocm/lib/libamdhip64.so'):\n"
            "        try:\n"
            "            lib = ctypes.CDLL(name)\n"
            "            break\n"
            "        except OSError:\n"
            "            pass\n"
            "    ok = lib is not None and lib.hipGetDeviceCount(ctypes.byref(n)) == 0\n"
            "    print(n.value if ok else 0)\n"
            "except Exception:\n"
            "    print(0)\n")
    try:
        r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True,
                           timeout=180)
        return int(r.stdout.strip().splitlines()[-1])
    except Exception:  # noqa: BLE001
        return 0


def free_port() -> int:
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def launch_ranks(world: int, child_argv: list, timeout_s: float = 1500.0, grace_s: float = 20.0, env_extra=None,
                 out=None, err=None) -> int:
    """Start `world` fresh processes running `child_argv` with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT
    set (what torch.distributed.run would provide), wait for them with a time limit, and return the job's exit code:
    0 only if EVERY rank exited 0 and rank 0 printed a JSON line, which is then forwarded to `out` as the job's only
    stdout line.  When a rank fails the others get `grace_s` to fail on their own (they usually notice through the
    rendezvous) and are then killed by process group; the same at the time limit.  Never execs: children are new
    processes, each in its own session, so a kill reaches exactly the processes started here."""
    out = out or sys.stdout
    err = err or sys.stderr
    port = free_port()
    procs = []
    r0_lines = []
    for rank in range(world):
        env = dict(os.environ)
        env.update({"RANK": str(rank), "LOCAL_RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_WORLD_SIZE": str(world),
                    "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "OSC_BENCH_LAUNCHED_BY": str(os.getpid())})
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: RCCL across processes needs it on this stack
        env.update(env_extra or {})
        procs.append(subprocess.Popen(child_argv, env=env, stdout=subprocess.PIPE, stderr=None, text=True,
                                      start_new_session=True))

    def pump(rank, p):  # rank 0's stdout is the job's stdout (collected); the other ranks' stdout goes to stderr
        for line in p.stdout:
            if rank == 0:
                r0_lines.append(line)
            else:
                err.write(f"[rank {rank}] {line}")
                err.flush()

    threads = [threading.Thread(target=pump, args=(r, p), daemon=True) for r, p in enumerate(procs)]
    for t in threads:
        t.start()

    killed = set()  # ranks this launcher ended itself: their signal codes say nothing about the job

    def kill_all(sig):
        for r, p in enumerate(procs):
            if p.poll() is None:
                killed.add(r)
                try:
                    os.killpg(p.pid, sig)  # (own session: pgid == pid)
                except (ProcessLookupError, PermissionError):
                    pass

    t0 = time.time()
    first_fail = None
    reason = None
    while any(p.poll() is None for p in procs):
        now = time.time()
        if first_fail is None and any(p.poll() not in (None, 0) for p in procs):
            first_fail = now
        if first_fail is not None and now - first_fail > grace_s:
            reason = "a rank failed and the others did not exit by themselves"
            break
        if now - t0 > timeout_s:
            reason = f"time limit of {timeout_s:.0f} s reached"
            break
        time.sleep(0.05)
    if reason:
        err.write(f"bench.py launcher: {reason}; killing the remaining ranks\n")
        kill_all(signal.SIGTERM)
        t1 = time.time()
        while any(p.poll() is None for p in procs) and time.time() - t1 < 10.0:
            time.sleep(0.05)
        kill_all(signal.SIGKILL)
    for p in procs:
        p.wait()
    for t in threads:
        t.join(5.0)
    codes = [p.returncode if p.returncode >= 0 else 128 - p.returncode for p in procs]  # (killed by signal s: 128 + s)
    worst = max([c for r, c in enumerate(codes) if r not in killed] or [0])  # the worst of the ranks that ended by themselves
    if reason and worst == 0:
        worst = 124  # nobody failed, somebody never finished
    if worst != 0:
        err.write(f"bench.py launcher: rank exit codes {codes} -> exit {worst}; no result line\n")
        err.flush()
        return worst
    lines = [ln for ln in r0_lines if ln.lstrip().startswith("{")]
    try:
        json.loads(lines[-1])
    except (IndexError, ValueError):
        err.write("bench.py launcher: every rank exited 0 but rank 0 printed no JSON line\n")
        return 4
    for ln in r0_lines:  # anything else rank 0 printed is not part of the one-line contract
        if ln is not lines[-1] and ln.strip():
            err.write(f"[rank 0] {ln}")
    out.write(lines[-1] if lines[-1].endswith("\n") else lines[-1] + "\n")
    out.flush()
    return 0


def self_launch(args) -> int:
    """`python bench.py --gpus N` (N > 1) with no launcher around it."""
    n = args.gpus
    have = visible_device_count()
    one_device = bool(os.environ.get("OSC_BENCH_ONE_DEVICE"))
    if have < n and not (one_device and have >= 1):
        print(f"bench.py: --gpus {n} but {have} HIP device(s) visible here; refusing to report replicas or oversubscribed "
              f"devices as a {n}-GPU run (nothing was built or started)", file=sys.stderr, flush=True)
        return EXIT_REFUSED
    from oscillink_amd import _build  # hipcc only: compiles, does not load the library

    _build.build()  # before the ranks start, so that N children never race one stale library
    child = [sys.executable, os.path.abspath(__file__), *sys.argv[1:]]
    return launch_ranks(n, child, timeout_s=args.launch_timeout)


def pctl(xs, q):
    return float(np.percentile(np.asarray(xs, dtype=np.float64), q))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--N", type=int, default=100_000)
    ap.add_argument("--D", type=int, default=768)
    ap.add_argument("--k", type=int, default=32)
    ap.add_argument("--tol", type=float, default=1e-3)
    ap.add_argument("--max-iters", type=int, default=12)
    ap.add_argument("--seeds", type=str, default=None,
                    help="comma-separated anchor seeds, each timed for --steps steps (default: 0; with --full 0,1,2 on one "
                         "GPU -- BASELINE.md section 2 --, 0 under a communicator)")
    ap.add_argument("--launch-timeout", type=float, default=1500.0,
                    help="self-launcher: seconds the ranks get before they are killed")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline: seeds 0,1,2 on one GPU, first / mispredicted settle, the build / U* / "
                         "receipt timings and the CPU oracle baseline (off by default: a plain run only times the steps)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU oracle baseline")
    ap.add_argument("--no-extras", action="store_true",
                    help="with --full: skip the first-settle / build / U* / receipt timings after the timed region")
    ap.add_argument("--extras", action="store_true",
                    help="with --full: run those timings in a multi-GPU run as well (default there: skipped -- they are "
                         "collective calls outside the timed region, and the one JSON line should not depend on them)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed (sampled rows of U, the settle's "
                         "iterations and residual) as DIR/<name>.npy")
    ap.add_argument("--shard", choices=["column", "row"], default="column",
                    help="multi-GPU CG partitioning: column slabs (one all-reduce(max) per iteration, default) or "
                         "row blocks (halo exchange of p + all-reduces of D-vectors, the north-star wording)")
    args = ap.parse_args()
    if args.gpus < 1 or args.steps < 1 or args.warmup < 0:
        raise SystemExit("bench.py: need --gpus >= 1, --steps >= 1, --warmup >= 0")

    under_launcher = "RANK" in os.environ and "WORLD_SIZE" in os.environ
    if args.gpus > 1 and not under_launcher:
        raise SystemExit(self_launch(args))

    os.environ["OSC_SHARD"] = args.shard
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if os.environ.get("OSC_BENCH_ONE_DEVICE"):  # rehearsal on a one-GPU box: every rank on device 0 (RCCL then refuses
        local_rank = 0                          # the communicator and the run must fail, see below)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}")
    # (rehearsal on a one-GPU box: OSC_BENCH_FORCE_COMM=1 takes the multi-GPU code path -- rendezvous, the library's RCCL
    # communicator, the sharded solve with its second stream, barriers -- with the one rank RCCL allows there)
    launched = world > 1 or bool(os.environ.get("OSC_BENCH_FORCE_COMM"))
    seeds = [int(x) for x in (args.seeds or ("0,1,2" if args.full and not launched else "0")).split(",") if x.strip() != ""]
    if not seeds:
        raise SystemExit("bench.py: --seeds is empty")

    from oscillink_amd import Oscillink
    from oscillink_amd import _native as nat
    from oscillink_amd.sharding import rccl_unique_id

    if nat.device_count() <= local_rank:  # fail before any work: this rank has no device of its own
        print(f"bench.py: rank {rank}: device {local_rank} does not exist ({nat.device_count()} visible); refusing to "
              "report replicas or shared devices as a sharded run", file=sys.stderr, flush=True)
        raise SystemExit(EXIT_REFUSED)
    N, D, k = args.N, args.D, args.k
    rdzv = FileRendezvous(rank, world) if launched else None

    def make_inputs(seed):
        rng = np.random.default_rng(seed)
        Y = rng.standard_normal((N, D)).astype(np.float32)
        psi = Y[:32].mean(axis=0)
        return Y, (psi / (np.linalg.norm(psi) + 1e-12)).astype(np.float32)

    def make_lattice(Y, tag):
        """One lattice, under the job's communicator when there is one.  Every rank learns whether ALL ranks joined; if
        not, the job fails as a whole."""
        comm = None
        comm_error = None
        if launched:  # bootstrap the library's own RCCL communicator: rank 0 makes the id, the directory carries it
            try:
                if rank == 0:
                    rdzv.put(f"uid.{tag}", rccl_unique_id())
                comm = (rdzv.get(f"uid.{tag}"), rank, world)
            except Exception as e:  # noqa: BLE001
                comm_error = f"{type(e).__name__}: {e}"
        lat = None
        if comm is not None:
            try:
                with StdoutToStderr():
                    lat = Oscillink(Y, kneighbors=k, deterministic_k=False, device=local_rank, comm=comm)
            except Exception as e:  # noqa: BLE001 -- reported by every rank below
                comm_error = f"{type(e).__name__}: {e}"
                lat = None
        if launched:
            flags = rdzv.gather(f"comm_ok.{tag}", (comm_error or "").encode())
            bad = [f.decode() for f in flags if f]
            if bad:
                if lat is not None:
                    lat.close()
                rdzv.close()
                print(f"bench.py: rank {rank}: the {world}-rank communicator could not be set up ({comm_error or bad[0]}); "
                      "refusing to report independent replicas as a sharded run", file=sys.stderr, flush=True)
                raise SystemExit(EXIT_REFUSED)
        if lat is None:
            lat = Oscillink(Y, kneighbors=k, deterministic_k=False, device=local_rank)
        return lat

    def comm_info_of(lat):
        """what the library's communicator itself says (kind "rccl" / "loopback" / "none", ranks it spans)"""
        c_rank, c_world, c_mode, c_kind = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.create_string_buffer(32)
        lat._call("osc_comm_info", C.byref(c_rank), C.byref(c_world), C.byref(c_mode), c_kind, 32)
        info = {"kind": c_kind.value.decode(), "world": int(c_world.value), "rank": int(c_rank.value),
                "shard": "row" if c_mode.value == 1 else "column"}
        ov = os.environ.get("OSC_COMM_OVERLAP")  # where the stop test's all-reduce runs (default: by world size)
        info["stop_test"] = ("none" if info["kind"] == "none" else
                             "second stream" if (ov not in (None, "0") or (ov is None and info["world"] >= 4)) else "solve's stream")
        ver = C.c_int32(0)
        nat.lib().osc_comm_backend_version(C.byref(ver))
        info["rccl_version"] = int(ver.value)
        if launched and (info["kind"] != "rccl" or info["world"] != world):
            print(f"bench.py: rank {rank}: communicator reports {info}, expected rccl over {world} ranks", file=sys.stderr,
                  flush=True)
            raise SystemExit(EXIT_REFUSED)
        return info

    def sync_all(lat):
        """barrier + device drain on every rank"""
        nat.lib().osc_device_synchronize(local_rank)
        if launched:
            lat._call("osc_comm_allreduce_f64", None, 0, 0)  # drains the stream, then a barrier over the communicator
        nat.lib().osc_device_synchronize(local_rank)

    def over_ranks(lat, x: float, op: str = "max") -> float:
        if not launched:
            return x
        v = (C.c_double * 1)(-x if op == "min" else x)
        lat._call("osc_comm_allreduce_f64", v, 1, 1)
        return float(-v[0] if op == "min" else v[0])

    def time_seed(seed, first):
        """W warm-up steps, then EXACTLY K timed steps between barrier + drain; each step also timed by itself."""
        t_in = time.time()
        Y, psi = make_inputs(seed)
        t_c = time.time()
        lat = make_lattice(Y, f"s{seed}")
        create_ms = 1000.0 * (time.time() - t_c)
        info = comm_info_of(lat)
        nnz, max_deg, dev_build_ms = lat.graph_stats()
        create_pieces = int(lat.build_info().get("create_pieces", 0))
        lat.set_query(psi)

        def step():
            lat.reset_U(wait=False)  # (ordered by the handle's stream; the settle below starts behind it)
            return lat.settle(dt=1.0, max_iters=args.max_iters, tol=args.tol)

        for _ in range(args.warmup):
            last = step()
        lat._call("osc_profile_enable", 1)
        lat._call("osc_profile_reset")
        sync_all(lat)
        per_step = []
        iters_total = 0
        t0 = time.perf_counter()
        ta = t0
        for _ in range(args.steps):
            last = step()
            tb = time.perf_counter()
            per_step.append(1000.0 * (tb - ta))
            ta = tb
            iters_total += last["iters"]
        sync_all(lat)
        elapsed = time.perf_counter() - t0
        launches, total_ms = C.c_int64(0), C.c_double(0.0)
        lat._call("osc_profile_get", 0, C.byref(launches), C.byref(total_ms))
        lat._call("osc_profile_enable", 0)
        return {"seed": seed, "lat": lat, "Y": Y, "psi": psi, "comm": info, "create_ms": create_ms, "create_pieces": create_pieces,
                "inputs_ms": 1000.0 * (t_c - t_in), "nnz": nnz, "max_deg": max_deg, "dev_build_ms": dev_build_ms,
                "per_step_ms": per_step, "elapsed_s": elapsed, "iters_total": iters_total, "last": last,
                "apply_launches": int(launches.value), "apply_total_ms": float(total_ms.value), "first": first, "step": step}

    runs = []
    for i, seed in enumerate(seeds):
        r = time_seed(seed, i == 0)
        if i > 0:  # only the first seed's lattice is kept for the numbers beside the timed region
            sync_all(r["lat"])
            r["lat"].close()
            r["lat"] = r["Y"] = r["step"] = None
        runs.append(r)
    main_run = runs[0]
    lat, Y, psi = main_run["lat"], main_run["Y"], main_run["psi"]
    if args.dump_outputs:  # before anything else touches the first seed's lattice (the later seeds had their own)
        dump_outputs(args.dump_outputs, lat, main_run["last"], rank)
    comm_info = main_run["comm"]
    nnz, max_deg = main_run["nnz"], main_run["max_deg"]

    all_steps = [t for r in runs for t in r["per_step_ms"]]
    med_local = pctl(all_steps, 50)
    ms_median = over_ranks(lat, med_local)                     # max over the ranks of the per-rank medians
    ms_p10, ms_p90 = over_ranks(lat, pctl(all_steps, 10)), over_ranks(lat, pctl(all_steps, 90))
    mean_local = 1000.0 * sum(r["elapsed_s"] for r in runs) / (args.steps * len(runs))
    ms_mean = over_ranks(lat, mean_local)                      # bracketed regions: barrier + drain on both sides
    ms_mean_min = over_ranks(lat, mean_local, "min")
    ms_median_min = over_ranks(lat, med_local, "min")
    iters_mean = sum(r["iters_total"] for r in runs) / (args.steps * len(runs))

    c0, c1 = C.c_int32(0), C.c_int32(0)
    lat._call("osc_comm_shard", C.byref(c0), C.byref(c1))
    d_local = int(c1.value - c0.value)
    n_local = N // world if (args.shard == "row" and launched) else N  # rows this rank's operator covers
    # The dominant kernel is the operator apply inside the CG loop (the CG matvec).  The library times each apply (all
    # its launches: one at config 3, column slabs elsewhere) with one HIP-event pair on its own stream; the
    # initial-residual apply of a settle (extra rhs / r / p streams) is kept in a separate slot.  Algorithmic bytes of
    # ONE apply on this rank: read X once, write the result once, ELL col + val, rowptr/B/diag per
    # row; per launch = per apply / launches.
    plan = lat.build_info()
    slabs = max(1, plan["apply_launches"])
    spmm_kernel = ("k_apply_blocked<" if plan.get("apply_src_blocks") else  # (template arguments: matched by prefix)
                   "k_spmm<8, 1, 0>" if plan["apply_xs_workgroups"] else None)
    bytes_apply = 8.0 * n_local * d_local + (8.0 * nnz + 12.0 * N) * (n_local / N)
    apply_ms = sum(r["apply_total_ms"] for r in runs) / max(1, sum(r["apply_launches"] for r in runs))
    bytes_mv = bytes_apply / slabs
    mv_ms = apply_ms / slabs
    achieved = bytes_mv / (mv_ms * 1e-3) / 1e9 if mv_ms > 0 else 0.0
    traffic, traffic_src = pmc_traffic(N, D, k, world, spmm_kernel)
    # whole settle, algorithmic: (20 + 44 I) N D + 8 nnz (I + 1) bytes, all ranks together
    bytes_settle = (20.0 + 44.0 * iters_mean) * N * D + 8.0 * nnz * (iters_mean + 1.0)
    settle_gbs = bytes_settle / (ms_median * 1e-3) / 1e9  # all GPUs together (they settle ONE lattice)

    # every rank's window apply against its own algorithmic bytes (the shapes a scaling run really times)
    mine = {"rank": rank, "columns": d_local, "rows": n_local, "apply_ms": apply_ms, "launches_per_apply": slabs,
            "algorithmic_bytes_per_apply": bytes_apply,
            "achieved_GBs": bytes_apply / (apply_ms * 1e-3) / 1e9 if apply_ms > 0 else 0.0,
            "ms_per_step_median": med_local, "ms_per_step_mean": mean_local,
            "kernel": "k_apply_blocked" if plan.get("apply_src_blocks") else "k_spmm",
            "src_blocks": plan.get("apply_src_blocks", 0)}
    mine["frac"] = mine["achieved_GBs"] / HBM_PEAK_GBS
    per_rank = [mine] if not launched else [json.loads(b.decode()) for b in rdzv.gather("rank_stats", json.dumps(mine).encode())]

    # The same launch against the bound that applies to a gather (profiles/r02_gather_bench.txt, r05_inflight_bench.txt):
    # a CU retires one random 128-byte row per N clocks depending on the footprint an XCD gathers from -- measured with
    # scripts/exp/gather_bench.hip on this part, no index loads; 256 CUs at 2.4 GHz.  Two yardsticks: the whole 32-column
    # slab (N x 128 B: what the plain apply gathers from) and an L2-resident source (what source blocking aims at).
    request_rate = None
    if spmm_kernel and world == 1 and mv_ms > 0:
        rows = float(nnz) * ((d_local + 31) // 32)                       # gathered neighbour rows per launch
        mb = N * 128.0 / 2 ** 20
        pts = [(3.6, 2.4), (6.4, 4.0), (12.8, 7.0), (32.0, 9.3), (200.0, 10.9)]  # MB per XCD -> clk per row per CU
        slab_clk = pts[0][1] if mb <= pts[0][0] else pts[-1][1]
        for (m0, c0_), (m1, c1_) in zip(pts, pts[1:]):
            if m0 < mb <= m1:
                slab_clk = c0_ + (c1_ - c0_) * (math.log(mb / m0) / math.log(m1 / m0))
        clk = mv_ms * 1e-3 * 2.4e9 * 256 / rows
        request_rate = {"gathered_rows_per_launch": rows, "achieved_clk_per_row_per_cu": clk,
                        "slab_footprint_MB_per_xcd": mb, "slab_footprint_clk_per_row_per_cu": slab_clk,
                        "l2_resident_clk_per_row_per_cu": pts[0][1], "frac_of_l2_resident_rate": pts[0][1] / clk,
                        "source": "profiles/r02_gather_bench.txt (gathers only; the apply also issues edge-list, own-row "
                                  "and output requests)"}

    out = {
        "metric": "settles/sec",
        "value": 1000.0 / ms_median,  # all ranks settle ONE lattice together
        "unit": "settles/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": ms_median,
        "ms_per_step_p10": ms_p10,
        "ms_per_step_p90": ms_p90,
        "ms_per_step_mean": ms_mean,
        "ms_per_step_over_ranks": {"median_min": ms_median_min, "median_max": ms_median, "mean_min": ms_mean_min,
                                   "mean_max": ms_mean},
        "steps_timed_total": args.steps * len(runs),
        "higher_is_better": True,
        "scaling": "strong",
        "vs_baseline": None,
        "dtype": "f32",
        "data": "synthetic",
        "config": {"workload": f"config3: N={N} D={D} k={k} fp32; one step = reset_U (U <- Y, device copy, inside the "
                               f"timed step) + settle(dt=1,max_iters={args.max_iters},tol={args.tol})",
                   "N": N, "D": D, "k": k, "nnz": nnz, "max_degree": max_deg,
                   "parallelism": "single" if not launched else f"{args.shard}-sharded CG x{world}",
                   "cg_iters_per_settle": iters_mean, "residual": main_run["last"]["res"],
                   "seeds": seeds,
                   "per_seed": [{"seed": r["seed"], "ms_per_step_median": pctl(r["per_step_ms"], 50),
                                 "ms_per_step_mean": 1000.0 * r["elapsed_s"] / args.steps, "nnz": r["nnz"],
                                 "cg_iters_per_settle": r["iters_total"] / args.steps,
                                 "graph_build_device_ms": r["dev_build_ms"]} for r in runs],
                   "statistic": "value = 1000 / median over all timed steps (max over ranks of the per-rank medians); "
                                "ms_per_step_mean = the barrier-bracketed regions / steps (max over ranks)"},
        "comm": comm_info,
        "lattice_create_ms": main_run["create_ms"],  # first call in the process: HIP context + code objects + upload + build
        # ... and the later seeds' creates (steady state): anchors from pageable host memory -> lattice; create_pieces > 0: the
        # transfer ran beside the build in that many pieces (OSC_CREATE_STREAM); never part of `value`
        "host_handover": {"create_ms_later_seeds": [r["create_ms"] for r in runs[1:]],  # (the second seed's lattice is created beside
                          # the first one's and allocates its arrays anew; from the third on the device blocks are reused)
                          "create_pieces": main_run["create_pieces"],
                          "anchors_MB": N * D * 4 / 1e6},
        "graph_build_device_ms": main_run["dev_build_ms"],
        "roofline": {"bound": "hbm",
                     "kernel": (f"k_apply_blocked (operator apply / CG matvec; one launch, XCD-affine 32-column slabs, "
                                f"source rows walked in {plan['apply_src_blocks']} blocks)" if plan.get("apply_src_blocks") else
                                "k_spmm<8,1,AP> (operator apply / CG matvec; one launch, XCD-affine 32-column slabs)"
                                if spmm_kernel else "k_spmm (operator apply / CG matvec; one column-slab launch)"),
                     "achieved": achieved,
                     "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "traffic": traffic,
                     "traffic_source": traffic_src,
                     "algorithmic_bytes_per_launch": bytes_mv, "mean_launch_ms": mv_ms,
                     "launches_per_apply": slabs, "apply_ms": apply_ms,
                     "applies_timed": sum(r["apply_launches"] for r in runs),
                     "achieved_traffic_GBs": (traffic / (mv_ms * 1e-3) / 1e9) if (traffic and mv_ms > 0) else None,
                     "request_rate": request_rate,
                     "per_rank": per_rank,
                     "settle": {"algorithmic_bytes": bytes_settle, "achieved": settle_gbs,
                                "peak": HBM_PEAK_GBS * world, "unit": "GB/s",
                                "frac": settle_gbs / (HBM_PEAK_GBS * world)}},
    }

    out["full"] = bool(args.full)
    run_extras = args.full and not args.no_extras
    run_cpu_baseline = args.full and not args.no_cpu_baseline
    if not launched and run_extras:
        out.update(cold_and_mispredicted(lat, Y, psi, args, k, local_rank, main_run["step"]))
    if run_extras and (not launched or args.extras):
        out.update(extras(lat, N, D, args, launched))
    elif launched and run_extras:
        out["extras"] = "skipped in a multi-GPU run (--extras runs them: sharded rebuilds, U* solves, receipts)"
    # The CPU oracle leg is CPU-only: rank 0 takes the device-built graph while the lattice is alive, every rank then
    # leaves the communicator (the other ranks are done), and rank 0 times the oracle -- at every world size, so that a
    # multi-GPU line carries the field too.
    csr = None
    if rank == 0 and run_cpu_baseline:
        csr = lat.graph_csr()[:3]
    if launched:
        sync_all(lat)
        lat.close()
        rdzv.close()
    if rank == 0 and run_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(csr, Y, psi, args)
    if rank == 0:
        print(json.dumps(out), flush=True)


def dump_outputs(path, lat, last, rank):
    """--dump-outputs: what the caller of the timed path receives after its last step -- the settled state U (all rows,
    or a fixed sample of them when U is larger than DUMP_U_BYTES) and the settle's own result.  Every rank reads U back
    (collective in a sharded run); rank 0 writes."""
    N, D = lat.N, lat.D
    n_rows = min(N, max(1, DUMP_U_BYTES // (4 * D)))
    if n_rows == N:
        rows = np.arange(N, dtype=np.int64)
    else:
        rows = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(N, size=n_rows, replace=False))
    U = np.ascontiguousarray(lat.U[rows], dtype=np.float32)
    if rank != 0:
        return
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "U.npy"), U)
    np.save(os.path.join(path, "U_rows.npy"), rows.astype(np.float64))
    np.save(os.path.join(path, "settle_iters.npy"), np.array([last["iters"]], dtype=np.float64))
    np.save(os.path.join(path, "settle_res.npy"), np.array([last["res"]], dtype=np.float64))


def cold_and_mispredicted(lat, Y, psi, args, k, device, step):
    """Two numbers the steady-state loop hides (run_cg predicts its last iteration from the handle's previous solve of
    the same kind, osc_api.hip: predicted_iters): (1) the first settle of a FRESH handle -- no prediction, first-use
    scratch and block-major graph copy; (2) a settle whose iteration count the handle guesses wrong, both ways: guessed
    one short (the host reads a residual it expected to be the last, re-enqueues: one round trip + the r update
    redone) and one long (a needless speculative iteration's gated-off launches).  Device-synchronised wall times of
    reset_U + settle, like a timed step; medians of 7."""
    from oscillink_amd import Oscillink
    from oscillink_amd import _native as nat

    def timed(fn):
        nat.lib().osc_device_synchronize(device)
        t0 = time.perf_counter()
        r = fn()
        nat.lib().osc_device_synchronize(device)
        return 1000.0 * (time.perf_counter() - t0), r

    fresh = Oscillink(Y, kneighbors=k, deterministic_k=False, device=device)
    fresh.set_query(psi)

    def fstep():
        fresh.reset_U(wait=False)
        return fresh.settle(dt=1.0, max_iters=args.max_iters, tol=args.tol)

    first_ms, st = timed(fstep)
    second_ms, _ = timed(fstep)
    fresh.close()
    hist = lat.residual_history()
    iters = st["iters"]
    res = {"first_settle_ms": first_ms, "second_settle_ms": second_ms}
    steady, low, high = [], [], []
    tol_short = None  # a tolerance the solve meets one iteration earlier: between the residuals of iterations iters-1 and iters-2
    if iters >= 3 and len(hist) >= iters and hist[iters - 2] > args.tol and hist[iters - 3] > hist[iters - 2]:
        tol_short = float(math.sqrt(hist[iters - 2] * hist[iters - 3]))
    for _ in range(7):
        steady.append(timed(step)[0])
        if tol_short is not None:
            lat.reset_U(wait=False)
            s0 = lat.settle(dt=1.0, max_iters=args.max_iters, tol=tol_short)   # leaves the handle guessing iters - 1
            if s0["iters"] == iters - 1:
                t, s1 = timed(step)
                if s1["iters"] == iters:
                    low.append(t)
        if iters + 1 <= args.max_iters:
            lat.reset_U(wait=False)
            lat.settle(dt=1.0, max_iters=iters + 1, tol=0.0)                   # leaves it guessing iters + 1
            t, s1 = timed(step)
            if s1["iters"] == iters:
                high.append(t)
        step()  # back to the right guess
    res["mispredict_settle_ms"] = {"steady": float(np.median(steady)),
                                   "guessed_one_short": float(np.median(low)) if low else None,
                                   "guessed_one_long": float(np.median(high)) if high else None,
                                   "note": "device-synchronised reset_U + settle, median of 7; steady = the same call with "
                                           "the right guess"}
    return res


def extras(lat, N, D, args, sharded):
    """The other timers BASELINE.md section 2 lists, outside the timed region: steady-state lattice build (second build
    in the process, kNN kernel timed by HIP events), the stationary solve, light and full receipts.  Every call here is
    collective under a communicator and all ranks make the same calls."""
    launches, total_ms = C.c_int64(0), C.c_double(0.0)
    lat._call("osc_profile_enable", 1)
    lat._call("osc_profile_reset")
    builds = []
    for _ in range(3):
        lat.rebuild_graph()
        builds.append(lat.graph_stats()[2])
    lat._call("osc_profile_get", 3, C.byref(launches), C.byref(total_ms))
    lat._call("osc_profile_enable", 0)
    info = lat.build_info()
    gemm_ms = total_ms.value / 3.0  # per build: the GEMM + selection kernels (panel route: sample sweep + thresholds + main sweep)
    route = ("panel prefilter: fp16 MFMA GEMM (query panel in registers; tile core beyond 768 columns), sampled thresholds, "
             "symmetric half sweep (row block I visits column tiles J >= I; 2 N^2 D flops are credited in full, as SURVEY 8d "
             "counts them), exact fp32 re-scoring" if info["prefilter"] == 2 else
             "tile prefilter: fp16 MFMA top-(k+16) lists + exact fp32 re-scoring" if info["prefilter"] else
             "dense fp32 MFMA + argmax select" if N <= 8192 else "exact fp32 MFMA + running top-k")
    peak = MFMA_F16_DENSE_TFLOPS if info["prefilter"] else MFMA_F32_TFLOPS
    flops = 2.0 * N * N * D
    tf = flops / (gemm_ms * 1e-3) / 1e12 if gemm_ms > 0 else 0.0
    world = int(os.environ.get("WORLD_SIZE", "1")) if sharded else 1
    # flops the matrix pipe really issues: the panel route's main sweep plus the threshold sample, a
    # strided 1 / rho of the columns, rho = (k + 16) / 4.  The main sweep's share comes from the library's own record of the
    # last build (build_info()["knn_sweep"]: 2 = the half sweep, ONE per build at every world size since the ranks of a
    # sharded build split its work items; 1 = a full sweep), not from WORLD_SIZE
    rho = (args.k + 16) / 4.0
    sweep_share = {2: 0.5, 1: 1.0}.get(info["knn_sweep"], 1.0)
    executed = flops * (sweep_share + 1.0 / rho) if info["prefilter"] == 2 else flops
    tf_exec = executed / (gemm_ms * 1e-3) / 1e12 if gemm_ms > 0 else 0.0
    knn = {"route": route, "build_device_ms": float(np.median(builds)), "gemm_topk_ms": gemm_ms,
           "flops": flops / world, "achieved": tf / world, "peak": peak, "unit": "TFLOP/s", "frac": tf / world / peak,
           "executed_flops": executed / world, "executed_achieved": tf_exec / world, "executed_frac": tf_exec / world / peak,
           "bound": "mfma", "fallback_rows": info["fallback_rows"],
           "main_sweep": {2: "half", 1: "full"}.get(info["knn_sweep"], "none"), "main_sweep_share_of_tiles": sweep_share}
    ustar = []
    for _ in range(5):
        lat._solve_ustar_device(lat._signature(), 1e-4, 64, True)
        ustar.append(lat.last_ustar["solve_ms"])
    rec = {}
    for mode in ("light", "full"):
        lat.set_receipt_detail(mode)
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            lat.receipt()
            ts.append(1000.0 * (time.perf_counter() - t0))
        rec[mode] = float(np.median(ts))
    return {"knn": knn, "ustar_solve_ms": float(np.median(ustar)), "ustar_iters": lat.last_ustar["iters"],
            "receipt_ms": rec}


def lib_hash():
    try:
        return open(os.path.join(ROOT, "oscillink_amd", "liboscillink_hip.so.stamp")).read().strip()
    except OSError:
        return None


def pmc_traffic(N, D, k, world, kernel):
    """HBM/fabric bytes per LAUNCH of the operator-apply kernel from a committed rocprofv3 PMC profile (FETCH_SIZE,
    WRITE_SIZE; gfx950 read-side x2 correction applied by scripts/summarize_profile.py) -- but only from a profile that
    was taken with THIS build (its `_meta.lib_hash` equals the source hash the running library was built from) on this
    workload and that holds this kernel; anything else would silently go stale, so it yields null."""
    h = lib_hash()
    if (N, D, k, world) != (100_000, 768, 32, 1) or kernel is None or h is None:
        return None, None
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc.json")), reverse=True):
        try:
            prof = json.load(open(path))
        except (OSError, ValueError):
            continue
        if prof.get("_meta", {}).get("lib_hash") != h:
            continue
        e = prof.get(kernel)
        if e is None and kernel.endswith("<"):  # template arguments: by prefix; of the blocked matvec's two instantiations
            names = [k_ for k_ in prof if k_.startswith(kernel)]  # the CG matvec is <..., false> (true: the INIT pass)
            names.sort(key=lambda k_: (not k_.endswith("false>"), k_))
            e = prof[names[0]] if names else None
        if e and "hbm_read_bytes_per_launch" in e and "hbm_write_bytes_per_launch" in e:
            return e["hbm_read_bytes_per_launch"] + e["hbm_write_bytes_per_launch"], os.path.relpath(path, ROOT)
    return None, None


def cpu_baseline(csr, Y, psi, args):
    """The CPU oracle (sparse flavour: SciPy CSR SpMM + NumPy, oracle/oscillink_oracle.py) on the same workload, with
    the device-built graph injected so the CPU leg times exactly the settle the GPU leg times.

    The CG's columns are independent recurrences (per-column alpha/beta), so the port runs column-parallel on the
    host cores: T threads each settle a D/T column slab for the iteration count of the full solve (tol=0 keeps every
    slab at the same number of iterations, i.e. the same arithmetic as one full-width solve; SciPy/NumPy release the
    GIL inside their kernels).  Protocol: one warm-up, then REPS timed repetitions from the
    same start state; the value is the median, p10/p90 are reported.  T is picked by one calibration repetition among
    {64, all cores} (more threads than memory channels can lose).  The single-thread full-width time (one run) and a
    sampled kNN build are reported beside it."""
    import concurrent.futures as cf

    import scipy.sparse as sp

    from oracle import oscillink_oracle as orc

    rowptr, col, a = csr  # (rowptr, col, A_ij) of the device-built lattice graph
    N, D = Y.shape
    A = sp.csr_matrix((a, col, rowptr), shape=(N, N), dtype=np.float32)
    ref = orc.OracleLattice(Y, kneighbors=args.k, dense=False, graph=A)
    ref.set_query(psi)
    t0 = time.perf_counter()
    st = ref.settle(dt=1.0, max_iters=args.max_iters, tol=args.tol)
    t_single = time.perf_counter() - t0
    try:
        cores = len(os.sched_getaffinity(0))
    except AttributeError:
        cores = os.cpu_count() or 1

    def make_slabs(threads):
        bounds = np.linspace(0, D, threads + 1).astype(int)
        slabs = []
        for t in range(threads):
            c0, c1 = int(bounds[t]), int(bounds[t + 1])
            sub = copy.copy(ref)  # shares the graph (A, W, sqrt_deg); own column slab of the state
            sub.Y = np.ascontiguousarray(Y[:, c0:c1])
            sub.U = sub.Y.copy()
            sub.D = c1 - c0
            sub.psi = np.ascontiguousarray(psi[c0:c1])
            slabs.append(sub)
        return bounds, slabs

    def run(sub):
        sub.U = sub.Y.copy()
        return sub.settle(dt=1.0, max_iters=st["iters"], tol=0.0)

    def rep(ex, slabs):
        t0 = time.perf_counter()
        list(ex.map(run, slabs))
        return time.perf_counter() - t0

    cands = sorted({max(1, min(64, cores, D // 4)), max(1, min(cores, D // 4))})
    best = None
    for threads in cands:  # calibration = warm-up
        bounds, slabs = make_slabs(threads)
        with cf.ThreadPoolExecutor(max_workers=threads) as ex:
            t = rep(ex, slabs)
        if best is None or t < best[0]:
            best = (t, threads)
    threads = best[1]
    bounds, slabs = make_slabs(threads)
    REPS = 9
    with cf.ThreadPoolExecutor(max_workers=threads) as ex:
        rep(ex, slabs)  # warm-up
        times = sorted(rep(ex, slabs) for _ in range(REPS))
    err = max(float(np.abs(s.U - ref.U[:, int(bounds[i]):int(bounds[i + 1])]).max()) for i, s in enumerate(slabs))
    t_med = float(np.median(times))
    p10, p90 = float(np.percentile(times, 10)), float(np.percentile(times, 90))

    rows = min(256, N)
    t0 = time.perf_counter()
    _knn_sample(orc, Y, args.k, rows)
    t_knn = time.perf_counter() - t0
    try:
        import threadpoolctl

        blas_threads = max([p.get("num_threads", 1) for p in threadpoolctl.threadpool_info()] or [1])
    except Exception:
        blas_threads = os.cpu_count() or 1
    return {"value": 1.0 / t_med, "unit": "settles/s", "cores": threads, "kind": "port",
            "sample": f"{REPS} timed full-size settles after a warm-up (N={N}, D={D}, {st['iters']} CG iterations each) of "
                      f"the SciPy-CSR/NumPy oracle on the device-built graph, column-parallel on {threads} threads of "
                      f"{cores} usable cores (thread count calibrated among {cands}); median; kNN build sampled on {rows} "
                      f"rows x {N} columns ({blas_threads} BLAS threads)",
            "ms_per_settle": 1000.0 * t_med, "ms_per_settle_p10": 1000.0 * p10, "ms_per_settle_p90": 1000.0 * p90,
            "reps": REPS, "ms_per_settle_single_thread": 1000.0 * t_single,
            "column_parallel_max_abs_diff": err,
            "cg_iters": st["iters"], "residual": st["res"], "knn_rows_sampled": rows, "knn_sample_ms": 1000.0 * t_knn,
            "knn_build_extrapolated_ms": 1000.0 * t_knn * N / rows, "host_cores": os.cpu_count(),
            "usable_cores": cores}


def _knn_sample(orc, Y, k, rows):
    Yn = orc.normalize_rows(Y)
    S = Yn[:rows] @ Yn.T
    S[np.arange(rows), np.arange(rows)] = -np.inf
    return np.argpartition(-S, kth=k, axis=1)[:, :k]


if __name__ == "__main__":
    main()

"""The one-launch LDS solve (csrc/small_kernels.hip: k_settle_small<4>, <2>, <1>) at every column width and at the seams
of its planner (csrc/small_plan.hpp), against the CPU oracle on the graph the device built.

Every shape states the plan it must get (asserted through `small_plan`, so the table cannot go stale) and proves by
`build_info()["small_solves"]` which path produced the answer: the one-launch kernel for cols > 0, the general path for
cols == 0.  Gates are those of test_gpu_parity._check_solves: equal iteration counts, residual histories within
rtol 2e-2 / atol 1e-7, relerr(U) and relerr(U*) below 2e-5, deltaH_total to 1e-4.

MEASURED_RATIOS below holds what test_ustar_against_fp64_solution printed on an MI355X."""
import numpy as np
import pytest

from tests import _small_reference as sr
from tests._cases import relerr

pytestmark = pytest.mark.gpu

TOL = 1e-4  # deltaH_total, as in test_gpu_parity
K = 8

# (N, D, cols): what each reaches is in DESIGN.md section 5.1
SHAPES = [
    (2395, 64, 4),    # last C = 4 size; five row sweeps, the last one ragged
    (2396, 61, 2),    # first C = 2 size; dcols 64 > D: pad columns
    (4794, 96, 2),    # LDS exactly at the 150 KiB limit: red / s_res / s_fail sit at the very end
    (4795, 96, 1),    # first C = 1 size
    (6000, 256, 1),   # 256 workgroups x 12 sweeps: the heaviest legal launch
    (5000, 3, 1),     # four workgroups, one of them a single pad column
    (2395, 1024, 4),  # 256 workgroups of 150 KiB: one on every CU
    (1259, 1024, 4),  # 256 workgroups of 79 KiB
    # 257 and 512 workgroups: planned with C = 4 and two workgroups per CU until these tests ran -- `small_solves` stayed 0,
    # every launch gave up at its barrier (k_settle_small<4> holds 161 VGPRs: three waves per SIMD, two workgroups need four)
    (1259, 1028, 0),
    (1259, 2048, 0),
    (6001, 64, 0),    # just outside: one row past C = 1
    (1260, 1028, 0),
    (4794, 516, 0),
]
VARIANT_SHAPES = [(2396, 61, 2), (4795, 96, 1), (1259, 1028, 0), (1259, 1024, 4)]
VARIANTS = ["gates", "chain", "gates_chain", "precond_none", "inertia", "cold_start", "k12", "general_path"]

# the plain operator at the variant shapes and the heaviest launch; gates and a chain at the variant shapes
FP64_CASES = [(*s, "plain") for s in VARIANT_SHAPES + [(6000, 256, 1)]] + [(*s, "gates_chain") for s in VARIANT_SHAPES]

# kernel distance / oracle distance to the float64 U* (test_ustar_against_fp64_solution), as measured on an MI355X
# (a record, not an input of any assertion; oracle distance 1.8e-7 .. 2.9e-7, iteration counts equal in every case)
MEASURED_RATIOS = {
    (2396, 61, "plain"): 0.773, (4795, 96, "plain"): 0.775, (1259, 1028, "plain"): 0.767, (1259, 1024, "plain"): 0.767,
    (6000, 256, "plain"): 0.771, (2396, 61, "gates_chain"): 0.728, (4795, 96, "gates_chain"): 0.724,
    (1259, 1028, "gates_chain"): 0.703, (1259, 1024, "gates_chain"): 0.707,
}


@pytest.fixture(scope="module")
def amd():
    import oscillink_amd
    from oscillink_amd import _native

    assert _native.device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return oscillink_amd


@pytest.fixture(scope="module")
def orc():
    from oracle import oscillink_oracle

    return oscillink_oracle


def _pair(amd, orc, N, D, cols, k=K, gates=None, chain=None):
    """(device lattice, oracle on the device's graph), configured alike; the plan is asserted first."""
    assert amd.small_plan(N, D)["cols"] == cols
    Y, psi = sr.inputs(N, D)
    lat = amd.Oscillink(Y, kneighbors=k, deterministic_k=True)
    ref = sr.oracle_on(orc, lat, Y, k)
    for L in (ref, lat):
        sr.configure(L, psi, gates, chain)
    return lat, ref


def _same_solve(got, want, lat, ref, what):
    assert got["iters"] == want["iters"], what
    hist = lat.residual_history()
    assert len(hist) == len(ref.history), what
    assert np.allclose(hist, ref.history, rtol=2e-2, atol=1e-7), what
    assert got["res"] == pytest.approx(want["res"], rel=2e-2, abs=1e-7), what


def _check_against_oracle(lat, ref, cols, **settle_kw):
    """settle, a second settle from the first one's state, U*, receipt: the oracle's answers, by the expected path."""
    kw = dict(max_iters=12, tol=1e-3, **settle_kw)
    before = lat.build_info()["small_solves"]
    ustar_solves = lat.stats["ustar_solves"]
    for step in ("first settle", "second settle"):
        want = dict(ref.settle(**kw))
        got = dict(lat.settle(**kw))
        _same_solve(got, want, lat, ref, step)
        assert relerr(lat.U, ref.U) < 2e-5, step
    want_us = ref.solve_Ustar()
    got_us = lat.solve_Ustar()
    _same_solve(lat.last_ustar, ref.last_ustar, lat, ref, "U*")
    assert relerr(got_us, want_us) < 2e-5
    rec = lat.receipt()
    assert rec["deltaH_total"] == pytest.approx(ref.deltaH(want_us), rel=TOL)
    assert rec["cg_iters"] == got["iters"] and rec["meta"]["ustar_iters"] == ref.last_ustar["iters"]
    assert lat.stats["ustar_solves"] == ustar_solves + 1  # (the receipt read the U* above: three solves were issued)
    assert lat.build_info()["small_solves"] - before == (3 if cols > 0 else 0)


@pytest.mark.parametrize("N,D,cols", SHAPES, ids=lambda v: str(v))
def test_every_width_and_planner_seam_against_oracle(amd, orc, N, D, cols):
    lat, ref = _pair(amd, orc, N, D, cols)
    assert lat.build_info()["small_solves"] == 0
    _check_against_oracle(lat, ref, cols)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("N,D,cols", VARIANT_SHAPES, ids=lambda v: str(v))
def test_operator_and_start_variants_against_oracle(amd, orc, N, D, cols, variant, monkeypatch):
    """Gates with entries exactly 0.0 and 1.0, a chain prior, both, no preconditioner, an inertia start, a cold start,
    degrees beyond one 8-entry fetch group (k = 12: a full group and a remainder), and the same solve on a second handle
    that takes the general multi-kernel path."""
    gates = sr.gates_with_exact_ends(N) if variant in ("gates", "gates_chain") else None
    chain = sr.chain_for(N) if variant in ("chain", "gates_chain") else None
    lat, ref = _pair(amd, orc, N, D, cols, k=12 if variant == "k12" else K, gates=gates, chain=chain)
    if variant == "k12":
        assert int(np.diff(lat.graph_csr()[0]).max()) > 8
    settle_kw = {"precond_none": dict(precond="none"), "inertia": dict(inertia=0.3),
                 "cold_start": dict(warm_start=False)}.get(variant, {})
    if variant != "general_path":
        _check_against_oracle(lat, ref, cols, **settle_kw)
        return
    monkeypatch.setenv("OSC_SMALL_PATH", "0")  # read when a handle is created
    Y, psi = sr.inputs(N, D)
    gen = amd.Oscillink(Y, kneighbors=K, deterministic_k=True)
    monkeypatch.delenv("OSC_SMALL_PATH")
    gen.set_query(psi)
    for step in range(2):
        a, b = dict(lat.settle(max_iters=12, tol=1e-3)), dict(gen.settle(max_iters=12, tol=1e-3))
        assert a["iters"] == b["iters"] and relerr(lat.U, gen.U) < 2e-5, step
    ua, ub = lat.solve_Ustar(), gen.solve_Ustar()
    assert lat.last_ustar["iters"] == gen.last_ustar["iters"] and relerr(ua, ub) < 2e-5
    assert gen.build_info()["small_solves"] == 0
    assert lat.build_info()["small_solves"] == (3 if cols > 0 else 0)


@pytest.mark.parametrize("N,D,cols,config", FP64_CASES, ids=lambda v: str(v))
def test_ustar_against_fp64_solution(amd, orc, N, D, cols, config):
    """U* at tol 1e-6 against a float64 direct solve of M x = rhs on the same graph (tests/_small_reference.py).

    The yardstick is the float32 oracle's own distance to that solution at the same tol and cap.  Kernel and oracle run
    the same recurrence in the same precision from the same start, so only the summation order differs (the kernel's
    column sums are float64): the kernel's distance may be at most twice the oracle's.  The factor 2 is an allowance,
    not a measurement.  On the CPU the oracle's distance at these shapes is 1.8e-7 .. 2.9e-7, the same at tol 1e-7 (it is
    the float32 floor of the recurrence, ten times the 2.5e-8 that rounding the float64 solution to float32 costs, so
    the ratio's denominator is far from zero) and 2.7e-7 .. 4.5e-7 at the default tol 1e-4.  Measured ratios on an MI355X:
    MEASURED_RATIOS above."""
    gates = sr.gates_with_exact_ends(N) if config == "gates_chain" else None
    chain = sr.chain_for(N) if config == "gates_chain" else None
    lat, ref = _pair(amd, orc, N, D, cols, gates=gates, chain=chain)
    Y, psi = sr.inputs(N, D)
    x64, direct_res = sr.ustar_fp64(orc, ref.A, Y, psi, gates, chain)
    assert direct_res < 1e-10
    want = ref.solve_Ustar(tol=1e-6, max_iters=64)
    got = lat.solve_Ustar(tol=1e-6, max_iters=64)
    d_ref, d_dev = relerr(want, x64), relerr(got, x64)
    print(f"\nfp64 check {N} x {D} {config}: cols {cols}, iterations oracle {ref.last_ustar['iters']} / device "
          f"{lat.last_ustar['iters']}, distance oracle {d_ref:.4e} / device {d_dev:.4e}, ratio {d_dev / d_ref:.3f}")
    assert lat.build_info()["small_solves"] == (1 if cols > 0 else 0)
    assert 1e-8 < d_ref < 2e-6  # the yardstick itself: at the float32 floor, not at zero and not unconverged
    assert d_dev <= 2.0 * d_ref


def test_iteration_cap_of_the_one_launch_solve(amd, orc):
    """Up to 4096 iterations the control words of the one-launch solve fit; one more takes the general path.  Both stop
    where the oracle stops (no run to the cap: past the float32 floor the implementations diverge chaotically)."""
    for max_iters, small in ((4096, 1), (4097, 0)):
        lat, ref = _pair(amd, orc, 300, 16, 4)
        want = dict(ref.settle(max_iters=max_iters, tol=1e-3))
        got = dict(lat.settle(max_iters=max_iters, tol=1e-3))
        _same_solve(got, want, lat, ref, max_iters)
        assert want["iters"] < 12 and relerr(lat.U, ref.U) < 2e-5
        assert lat.build_info()["small_solves"] == small, max_iters

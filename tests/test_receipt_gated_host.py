"""receipt_gated_many on the CPU: the float64 algebra the gated receipts stand on, and the
conditions that tests/test_gpu_receipt_gated_many.py puts on its INPUTS, checked with the oracle's graph and the float64
yardstick alone.  No GPU."""
import functools

import numpy as np
import pytest

from oracle import oscillink_oracle as orc
from tests import _bundle_gated as bg
from tests import _gated as yg
from tests import _receipt_gated as rg

LAMS = rg.LAMS


@functools.lru_cache(maxsize=None)
def _case(name):
    """(Y, P, G, A, sd) with the oracle's own graph and float64 diffusion gates in the fifth row"""
    N, D, kn, _, _, _ = rg.CASES[name]
    Y = rg.anchors(name)
    P = rg.queries(name, Y)
    ref = orc.OracleLattice(Y, kneighbors=kn, deterministic_k=True)
    A, sd = np.asarray(ref.A, np.float64), np.asarray(ref.sqrt_deg, np.float64)
    G = rg.given_gates(name, N)
    G[4] = yg.gates64(A, sd, Y, P[4], bg.GATE_BETA, bg.GATE_GAMMA)[0]
    return Y, P, G, A, sd


# ---- the algebra ----------------------------------------------------------------------------------------------------------
def test_deltaH_is_the_sum_of_the_columns_quadratic_forms():
    Y, P, G, A, sd = _case("seam_n97_d40")
    M = rg.gated_M(A, sd, G[0])
    E = np.random.default_rng(0).standard_normal(Y.shape)
    per_column = sum(float(E[:, c] @ (M @ E[:, c])) for c in range(E.shape[1]))
    assert np.isclose(per_column, float(np.sum(E * (M @ E))), rtol=1e-13, atol=0)
    assert np.isclose(per_column, float(np.trace(E.T @ M @ E)), rtol=1e-13, atol=0)


@pytest.mark.parametrize("dt", [1.0, 0.5])
def test_the_settle_system_is_the_panel_operator_with_primed_lambdas(dt):
    Y, P, G, A, sd = _case("seam_n97_d40")
    lamG, lamC, lamQ = LAMS
    primed = (1.0 + dt * lamG, dt * lamC, dt * lamQ)
    for g in G:
        S = rg.settle_system(rg.gated_M(A, sd, g), dt)
        assert np.allclose(S, rg.gated_M(A, sd, g, primed), rtol=0, atol=1e-14)
        # ... and so are their Jacobi diagonals: 1 + dt (lamG + lamQ g) = lamG' + lamQ' g
        assert np.allclose(rg.settle_diag(g, LAMS, dt), primed[0] + primed[2] * g.astype(np.float64), rtol=0, atol=1e-15)


@pytest.mark.parametrize("dt", [1.0, 0.5])
def test_the_settle_start_residual_needs_no_stored_rhs(dt):
    Y, P, G, A, sd = _case("seam_n97_d40")
    lamG, lamC, lamQ = LAMS
    W = np.eye(Y.shape[0]) - yg.laplacian64(A, sd)
    U = Y.astype(np.float64) + 0.3 * np.random.default_rng(1).standard_normal(Y.shape)
    for q in range(5):
        g, psi = G[q].astype(np.float64), P[q].astype(np.float64)
        want = rg.settle_rhs(Y, U, P[q], G[q], LAMS, dt) - rg.settle_system(rg.gated_M(A, sd, G[q]), dt) @ U
        r0 = dt * (lamG * (Y - U) + lamQ * g[:, None] * (psi[None, :] - U) + lamC * (W @ U - U))
        assert np.allclose(r0, want, rtol=0, atol=1e-12 * max(1.0, float(np.abs(want).max())))


# ---- the inputs' own conditions -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _null_census(name):
    """per query of a case: (null-point rows, rows with an edge, left-out share) of the yardstick"""
    Y, P, G, A, sd = _case(name)
    rows = rg.rows_with_edge(A)
    out = []
    for q in range(5):
        want = rg.yardstick(Y, Y, P[q], G[q], A, sd)  # (the margins are U*'s: the state does not enter)
        out.append((len({int(p["edge"][0]) for p in want["null_points"]}), int(rows.size),
                    rg.left_out_share(want["margin"], A)))
    return out


@pytest.mark.parametrize("name", list(rg.CASES))
def test_null_margins_leave_enough_rows_to_compare(name):
    for q, (nulls, rows, share) in enumerate(_null_census(name)):
        print(f"{name} q{q}: {nulls} null points on {rows} rows with an edge, left out {share:.4f}")
        assert share <= rg.LEFT_OUT_CAP, (name, q, share)


def test_the_z_rule_is_exercised_both_ways():
    census = [c for name in ("seam_n97_d40", "d64", "n33") for c in _null_census(name)]
    assert any(nulls >= 1 for nulls, _, _ in census), census
    assert any(rows - nulls >= 1 for nulls, rows, _ in census), census


@pytest.mark.parametrize("name,settle", [(rg.SETTLE_CASE, rg.SETTLE_DEFAULT), (rg.SETTLE_CASE, rg.SETTLE_CAPPED),
                                         (rg.LOOP_CASES[1], rg.SETTLE_DEFAULT)], ids=["default", "capped", "reordered"])
def test_settle_histories_keep_their_distance_from_tol(name, settle):
    Y, P, G, A, sd = _case(name)
    for q in range(5):
        M = rg.gated_M(A, sd, G[q])
        _, iters, res, hist = rg.settle64(M, Y, Y, P[q], G[q], LAMS, **settle)
        print(q, iters, [f"{h:.3e}" for h in hist[-2:]])
        assert len(hist) == iters and hist[-1] == res
        assert bg.history_clear_of_tol(hist, tol=settle["tol"]), (q, hist)


# ---- the Python layer and the entry point, with no device ---------------------------------------------------------------
class _Stub:
    """the attributes the call reads before it reaches the device; native calls are recorded"""

    def __init__(self, N=100, D=8, chain=None, comm=False):
        from oscillink_amd import OscillinkLattice

        self.N, self.D, self._has_comm, self._chain_nodes = N, D, comm, chain
        self._receipt_detail = "full"
        self._GATED_SETTLE_DEFAULTS = OscillinkLattice._GATED_SETTLE_DEFAULTS
        self.calls = []
        self._check_gate_rows = OscillinkLattice._check_gate_rows.__get__(self)

    def _call(self, name, *a):
        self.calls.append(name)

    def _push_params(self):
        self.calls.append("_push_params")

    def _log(self, *a):
        self.calls.append("log:" + a[0])


def _run(stub, *a, **kw):
    from oscillink_amd import OscillinkLattice

    return OscillinkLattice.receipt_gated_many(stub, *a, **kw)


def test_signature_and_native_calls():
    import inspect

    from oscillink_amd import OscillinkLattice

    names = list(inspect.signature(OscillinkLattice.receipt_gated_many).parameters)
    assert names == ["self", "psis", "gates", "settle", "bundle_k", "alpha", "tol", "max_iters", "as_arrays", "gate_beta",
                     "gate_gamma", "gate_method", "gate_tol", "gate_max_iters"]
    P = np.ones((3, 8), np.float32)
    stub = _Stub()
    out = _run(stub, P, np.ones((3, 100), np.float32), settle=True, bundle_k=4, as_arrays=True)
    assert stub.calls == ["_push_params", "osc_receipt_gated_many", "log:receipt_gated_many"]
    assert {"deltaH", "null_offsets", "ustar_iters", "ustar_res", "settle_iters", "settle_res", "ids", "score",
            "align"} <= set(out)
    assert out["ids"].shape == (3, 4) and stub.last_receipt_gated["settle_iters"].shape == (3,)
    out = _run(_Stub(), P, np.ones((3, 100), np.float32), as_arrays=True)
    assert "settle_iters" not in out and "ids" not in out


def test_argument_errors_come_before_any_device_work():
    P = np.ones((3, 8), np.float32)
    G = np.ones((3, 100), np.float32)

    def refused(exc, match, *a, stub=None, **kw):
        stub = stub or _Stub()
        with pytest.raises(exc, match=match):
            _run(stub, *a, **kw)
        assert stub.calls == []

    bad = G.copy()
    bad[2, 4] = np.nan
    refused(ValueError, "query 2: gates must be finite", P, bad)
    bad = G.copy()
    bad[1, 0] = -1.0
    refused(ValueError, "query 1: gates must be >= 0", P, gates=bad)
    refused(ValueError, "set_gates", P, G[0])
    refused(ValueError, r"\(3, 100\) array", P, G[:2])
    refused(ValueError, "'diffusion'", P, "diffuse")
    refused(ValueError, "gate_gamma must be > 0", P, "diffusion", gate_gamma=0.0)
    refused(ValueError, "max_iters must be >= 1", P, G, max_iters=0)
    refused(ValueError, "unknown keys", P, G, settle={"dt": 1.0, "iters": 3})
    refused(ValueError, "dt must be > 0", P, G, settle={"dt": 0.0})
    refused(ValueError, "max_iters must be >= 1", P, G, settle={"max_iters": 0})
    refused(ValueError, "settle must be", P, G, settle=3)
    refused(ValueError, "bundle_k", P, G, bundle_k=-1)
    refused(NotImplementedError, "chain of its own", P, G, stub=_Stub(chain=[0, 1]))
    refused(NotImplementedError, "communicator", P, G, stub=_Stub(comm=True))


def test_entry_point_is_declared_with_its_reference_seam_and_rejects_a_null_handle():
    import os

    from oscillink_amd import _build, _native as nat

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "oscillink_hip.h")).read()
    assert "int osc_receipt_gated_many(osc_handle h, " in header
    assert "lattice.py:159-230, 298-455" in header and "receipts.py:10-83" in header
    assert "receipt_gated_kernels.hip" in _build.SOURCES and "receipt_gated_plan.hpp" in _build.HEADERS
    _build.build()
    lib = nat.lib()
    assert lib.osc_receipt_gated_many(None, None, 0, None, 0, 1.0, 0.1, 0, 1e-4, 256, 1e-4, 256, 0, 1.0, 12, 1e-3, 1, 3.0, 0, 0,
                                      0.5, 0.5, None, None, None, None, None, None, None, None, None, None, None, None, 0,
                                      None, None, None, None, None, None, None) == nat.OSC_E_INVALID

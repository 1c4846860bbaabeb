"""bundle_gated_many on the CPU: the conditions that tests/test_gpu_bundle_gated_many.py puts on
its INPUTS, checked with the oracle's graph and the float64 yardstick alone, and the float64 algebra the gated path
stands on.  No GPU."""
import numpy as np
import pytest

from oracle import oscillink_oracle as orc
from tests import _bundle_gated as bg
from tests import _gated as yg
from tests import _queries as yq

LAMS = (1.0, 0.5, 4.0)


def _case(name):
    """(Y, P, G, A, sd, oracle lattice) with the oracle's own graph and float64 diffusion gates in the fifth row"""
    N, D, kn, k, _, _ = bg.CASES[name]
    Y = bg.anchors(name)
    P = bg.queries(name, Y)
    ref = orc.OracleLattice(Y, kneighbors=kn, deterministic_k=True)
    A, sd = np.asarray(ref.A, np.float64), np.asarray(ref.sqrt_deg, np.float64)
    G = bg.given_gates(name, N)
    G[4] = yg.gates64(A, sd, Y, P[4], bg.GATE_BETA, bg.GATE_GAMMA)[0]
    return Y, P, G, A, sd, ref


@pytest.mark.parametrize("name", list(bg.CASES))
def test_near_tie_cap_holds_for_the_yardstick(name):
    Y, P, G, A, sd, _ = _case(name)
    k = bg.CASES[name][3]
    cut = 0
    for q in range(5):
        _, U, ids, _, _, margins = bg.yardstick(Y, A, sd, P[q], G[q], LAMS, k)
        assert np.all(np.isfinite(U)) and len(ids) == min(k, Y.shape[0])
        cut += int(bg.cut_before_last(margins))
    print(f"{name}: {cut} of 5 yardstick id lists have a near tie before their last pick")
    assert cut <= 1


def test_oracle_histories_keep_their_distance_from_tol():
    Y, P, G, _, _, ref = _case(bg.ITERS_CASE)
    for q in range(5):
        ref.set_query(P[q], gates=G[q])
        ref.solve_Ustar(tol=bg.TOL, max_iters=bg.LOOP_ITERS)
        hist = list(ref.history)
        print(q, ref.last_ustar["iters"], [f"{h:.3e}" for h in hist[-2:]])
        assert ref.last_ustar["converged"], q
        assert bg.history_clear_of_tol(hist), (q, hist)
        # max_iters = 3 ends unconverged, clear of the stop
        assert len(hist) > 3 and min(hist[:3]) >= 1.05 * bg.TOL, (q, hist[:3])


def test_unit_gates_reproduce_the_ungated_basis_answer():
    Y, P, _, A, sd, _ = _case("seam_n97_d40")
    lamG, lamC, lamQ = LAMS
    ones = np.ones(Y.shape[0])
    M = yq.dense_M(A, sd, ones, lamG, lamC, lamQ)
    X, x = yq.basis(M, Y, ones, lamG, lamQ)
    for q in range(5):
        U = yq.ustar(M, Y, ones, P[q], lamG, lamQ)
        assert np.allclose(U, X + np.outer(x, P[q].astype(np.float64)), rtol=0, atol=1e-12)


@pytest.mark.parametrize("name", ["seam_n97_d40", "n2"])
def test_zero_gates_leave_M_positive_definite(name):
    Y, _, _, A, sd, _ = _case(name)
    lamG, lamC, lamQ = LAMS
    M = yq.dense_M(A, sd, np.zeros(Y.shape[0]), lamG, lamC, lamQ)
    assert np.allclose(M, M.T, rtol=0, atol=1e-15)
    # L_sym = I - D^-1/2 A D^-1/2 is positive semi-definite, so M = lamG I + lamC L_sym has no eigenvalue below lamG -- up
    # to the float32 rounding of sqrt_deg: each weight moves by at most 2^-23 of itself and |D^-1/2 A D^-1/2| <= 1, so an
    # eigenvalue of L_sym moves by less than 2^-22 (2^-20 leaves room for the eigensolver)
    assert np.linalg.eigvalsh(M).min() >= lamG - lamC * 2.0 ** -20


# ---- the Python layer and the entry point, with no device ---------------------------------------------------------------
class _Stub:
    """the attributes the two calls read before they reach the device; native calls are recorded"""

    def __init__(self, N=100, D=8, chain=None, comm=False):
        from oscillink_amd import OscillinkLattice

        self.N, self.D, self._has_comm, self._chain_nodes = N, D, comm, chain
        self.calls = []
        self._check_gate_rows = OscillinkLattice._check_gate_rows.__get__(self)

    def _call(self, name, *a):
        self.calls.append(name)

    def _ensure_query_basis(self, *a):
        self.calls.append("_ensure_query_basis")

    def _push_params(self):
        self.calls.append("_push_params")

    def _log(self, *a):
        pass


def _run(stub, *a, **kw):
    from oscillink_amd import OscillinkLattice

    return OscillinkLattice.bundle_gated_many(stub, *a, **kw)


def test_bundle_many_keeps_its_signature_and_its_native_calls():
    import inspect

    from oscillink_amd import OscillinkLattice

    assert "gates" not in inspect.signature(OscillinkLattice.bundle_many).parameters
    P = np.ones((3, 8), np.float32)
    stub = _Stub()
    OscillinkLattice.bundle_many(stub, P, k=4)
    assert stub.calls == ["_ensure_query_basis", "osc_bundle_many"]
    with pytest.raises(TypeError):
        OscillinkLattice.bundle_many(_Stub(), P, k=4, gates=np.ones((3, 100), np.float32))
    names = list(inspect.signature(OscillinkLattice.bundle_gated_many).parameters)
    assert names == ["self", "psis", "gates", "k", "alpha", "tol", "max_iters", "as_arrays", "gate_beta", "gate_gamma",
                     "gate_method", "gate_tol", "gate_max_iters"]
    stub = _Stub()
    _run(stub, P, np.ones((3, 100), np.float32), k=4)
    assert stub.calls == ["_push_params", "osc_bundle_gated_many"]
    assert stub.last_bundle_gated["gates"] is None and stub.last_bundle_gated["iters"].shape == (3,)


def test_gate_argument_errors_come_before_any_device_work():
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
    refused(ValueError, r"\(Q, 100\) array", P, G[:, :50])
    refused(ValueError, "'diffusion'", P, "diffuse")
    refused(ValueError, "gate_gamma must be > 0", P, "diffusion", gate_gamma=0.0)
    refused(ValueError, "gate_method", P, "diffusion", gate_method="lu")
    refused(ValueError, "max_iters must be >= 1", P, G, max_iters=0)
    refused(ValueError, "psis must be", np.ones((3, 9), np.float32), G)
    refused(NotImplementedError, "chain of its own", P, G, stub=_Stub(chain=[0, 1]))
    refused(NotImplementedError, "communicator", P, G, stub=_Stub(comm=True))
    # per-query gates and chain priors do not combine: no call takes both
    refused(TypeError, "chains", P, G, chains=[0, 1, 2], lamP=0.2)


def test_entry_points_are_declared_with_their_reference_seam_and_reject_a_null_handle():
    import os

    from oscillink_amd import _build, _native as nat

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "oscillink_hip.h")).read()
    assert "int osc_bundle_gated_many(osc_handle h, " in header and "int osc_ustar_gated_many(osc_handle h, " in header
    assert "lattice.py:114-120, 245-263, 530-568" in header and "OSC_GATED_CHUNK" in header
    _build.build()
    lib = nat.lib()
    assert lib.osc_bundle_gated_many(None, None, 0, None, 0, 1.0, 0.1, 0, 1e-4, 256, 1e-4, 256, 8, 0.5, 0.5, None, None, None,
                                     None, None) == nat.OSC_E_INVALID
    assert lib.osc_ustar_gated_many(None, None, 0, None, 1e-4, 256, None, None, None) == nat.OSC_E_INVALID

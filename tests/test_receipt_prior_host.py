"""osc_receipt_prior_many and receipt_many(chains=..., lamP=...) without a device: the library exports
the entry point, a NULL handle is refused, and the Python arguments are checked before any device work."""
import ctypes
import inspect
import os

import numpy as np
import pytest


def test_library_exports_the_entry_point_and_native_lists_it():
    from oscillink_amd import _build, _native as nat

    _build.build()
    lib = nat.lib()
    header = open(os.path.join(os.path.dirname(_build.HERE), "include", "oscillink_hip.h")).read()
    assert hasattr(lib, "osc_receipt_prior_many")
    res, args = nat.SIGNATURES["osc_receipt_prior_many"]
    assert res is ctypes.c_int and len(args) == 25 and args[0] is nat.Handle
    assert "int osc_receipt_prior_many(osc_handle h, " in header
    assert "lattice.py:298-455" in header and "receipts.py:10-83" in header and "lattice.py:129-150" in header


def test_rejects_a_null_handle_without_a_device():
    from oscillink_amd import _build, _native as nat

    _build.build()
    lib = nat.lib()
    assert lib.osc_receipt_prior_many(None, None, 0, None, None, None, 0.2, 1e-4, 256, 1, 3.0, 0, None, None, None, None, None,
                                      None, None, None, None, None, 0, None, None) == nat.OSC_E_INVALID


def test_signature_keeps_todays_call_and_adds_three_keywords():
    from oscillink_amd import OscillinkLattice

    sig = inspect.signature(OscillinkLattice.receipt_many)
    names = list(sig.parameters)
    assert names == ["self", "psis", "tol", "max_iters", "as_arrays", "chains", "lamP", "chain_weights"]
    for n in names[2:]:
        assert sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY
    for n in names[5:]:
        assert sig.parameters[n].default is None
    assert sig.parameters["tol"].default == 1e-4 and sig.parameters["max_iters"].default == 256
    assert sig.parameters["as_arrays"].default is False


class _Stub:
    """the attributes receipt_many reads before it reaches the device; any native call fails the test"""

    _receipt_detail = "full"

    def __init__(self, N=100, D=8, chain=None, comm=False):
        self.N, self.D, self._has_comm, self._chain_nodes = N, D, comm, chain

    def _call(self, *a):
        raise AssertionError("device work before the arguments were checked")

    _ensure_query_basis = _ensure_shifted_basis = _push_params = _call


def _run(stub, *a, **kw):
    from oscillink_amd import OscillinkLattice

    return OscillinkLattice.receipt_many(stub, *a, **kw)


def test_python_argument_errors_come_before_any_device_work():
    P = np.ones((3, 8), np.float32)
    ok = [0, 1, 2]
    with pytest.raises(ValueError, match="chains given without lamP"):
        _run(_Stub(), P, chains=ok)
    with pytest.raises(ValueError, match="lamP given without chains"):
        _run(_Stub(), P, lamP=0.2)
    with pytest.raises(ValueError, match="chain_weights given without chains and lamP"):
        _run(_Stub(), P, chain_weights=[1.0, 1.0])
    with pytest.raises(ValueError, match="lamP must be >= 0"):
        _run(_Stub(), P, chains=ok, lamP=-1e-3)
    with pytest.raises(ValueError, match="lamP must be >= 0"):
        _run(_Stub(), P, chains=ok, lamP=float("nan"))
    with pytest.raises(ValueError, match="lamP must be >= 0"):
        _run(_Stub(), P, chains=ok, lamP=float("inf"))
    with pytest.raises(ValueError, match="receipt_many with lamP: the lattice has a chain of its own \\(clear_chain first\\)"):
        _run(_Stub(chain=[0, 1]), P, chains=ok, lamP=0.2)
    with pytest.raises(ValueError, match="at most 64 distinct nodes, got 65"):
        _run(_Stub(), P, chains=list(range(65)), lamP=0.2)
    with pytest.raises(ValueError, match="query 1: with lamP a chain has at most 64 distinct"):
        _run(_Stub(), P, chains=[ok, list(range(65)), ok], lamP=0.0)
    with pytest.raises(ValueError, match="at most 1024"):
        _run(_Stub(), P, chains=[0, 1] * 512 + [0], lamP=0.2)
    with pytest.raises(ValueError, match="chain: weights length must equal"):
        _run(_Stub(), P, chains=ok, lamP=0.2, chain_weights=[1.0])
    with pytest.raises(ValueError, match="query 2: weights length must equal"):
        _run(_Stub(), P, chains=[ok, ok, ok], lamP=0.2, chain_weights=[None, [1.0, 2.0], [1.0]])
    with pytest.raises(ValueError, match="chain weights must be finite"):
        _run(_Stub(), P, chains=ok, lamP=0.2, chain_weights=[1.0, float("inf")])
    with pytest.raises(ValueError, match="hold 3 entries parallel to chains"):
        _run(_Stub(), P, chains=[ok, ok, ok], lamP=0.2, chain_weights=[[1.0, 1.0]] * 2)
    with pytest.raises(ValueError):  # a non-finite query, as in the plain call
        _run(_Stub(), np.full((3, 8), np.nan, np.float32), chains=ok, lamP=0.2)
    with pytest.raises(NotImplementedError, match=r"receipt_many: lattices with a communicator \(sharded / multi-rank\) are not"):
        _run(_Stub(comm=True), P, chains=ok, lamP=0.2)

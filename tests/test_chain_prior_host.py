"""osc_query_basis_shifted / osc_chain_prior_many and chain_receipt_many(lamP=...) without a device:
the library exports both entry points, a NULL handle is refused, and the Python arguments are checked before any device
work."""
import ctypes
import inspect
import os

import numpy as np
import pytest


def test_library_exports_both_entry_points_and_native_lists_them():
    from oscillink_amd import _build, _native as nat

    _build.build()
    lib = nat.lib()
    header = open(os.path.join(os.path.dirname(_build.HERE), "include", "oscillink_hip.h")).read()
    for name, nargs in (("osc_query_basis_shifted", 9), ("osc_chain_prior_many", 20)):
        assert hasattr(lib, name)
        res, args = nat.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs and args[0] is nat.Handle
        assert f"int {name}(osc_handle h, " in header


def test_both_reject_a_null_handle_without_a_device():
    from oscillink_amd import _build, _native as nat

    _build.build()
    lib = nat.lib()
    assert lib.osc_query_basis_shifted(None, 0.2, 1e-4, 256, 1.0, 1, None, None, None) == nat.OSC_E_INVALID
    assert lib.osc_chain_prior_many(None, None, 0, None, None, None, 0.2, 1e-4, 256, 2.5, None, None, None, None, None, None,
                                    None, None, None, None) == nat.OSC_E_INVALID


def test_signature_keeps_todays_call_and_adds_the_two_keywords():
    from oscillink_amd import OscillinkLattice

    sig = inspect.signature(OscillinkLattice.chain_receipt_many)
    names = list(sig.parameters)
    assert names == ["self", "psis", "chains", "z_th", "tol", "max_iters", "as_arrays", "lamP", "chain_weights"]
    for n in names[4:]:
        assert sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters["lamP"].default is None and sig.parameters["chain_weights"].default is None


class _Stub:
    """the attributes chain_receipt_many reads before it reaches the device; any native call fails the test"""

    def __init__(self, N=100, D=8, chain=None, comm=False):
        self.N, self.D, self._has_comm, self._chain_nodes = N, D, comm, chain

    def _call(self, *a):
        raise AssertionError("device work before the arguments were checked")

    _ensure_query_basis = _ensure_shifted_basis = _push_params = _call


def _run(stub, *a, **kw):
    from oscillink_amd import OscillinkLattice

    return OscillinkLattice.chain_receipt_many(stub, *a, **kw)


def test_python_argument_errors_come_before_any_device_work():
    P = np.ones((3, 8), np.float32)
    ok = [0, 1, 2]
    with pytest.raises(ValueError, match="chain_weights given without lamP"):
        _run(_Stub(), P, ok, chain_weights=[1.0, 1.0])
    with pytest.raises(ValueError, match="lamP must be >= 0"):
        _run(_Stub(), P, ok, lamP=-1e-3)
    with pytest.raises(ValueError, match="lamP must be >= 0"):
        _run(_Stub(), P, ok, lamP=float("nan"))
    with pytest.raises(ValueError, match="clear_chain first"):
        _run(_Stub(chain=[0, 1]), P, ok, lamP=0.2)
    with pytest.raises(ValueError, match="at most 64 distinct nodes, got 65"):
        _run(_Stub(), P, list(range(65)), lamP=0.2)
    with pytest.raises(ValueError, match="query 1: with lamP a chain has at most 64 distinct"):
        _run(_Stub(), P, [ok, list(range(65)), ok], lamP=0.0)
    with pytest.raises(ValueError, match="at most 1024"):
        _run(_Stub(), P, [0, 1] * 512 + [0], lamP=0.2)
    with pytest.raises(ValueError, match="chain: weights length must equal"):
        _run(_Stub(), P, ok, lamP=0.2, chain_weights=[1.0])
    with pytest.raises(ValueError, match="query 2: weights length must equal"):
        _run(_Stub(), P, [ok, ok, ok], lamP=0.2, chain_weights=[None, [1.0, 2.0], [1.0]])
    with pytest.raises(ValueError, match="chain weights must be finite"):
        _run(_Stub(), P, ok, lamP=0.2, chain_weights=[1.0, float("inf")])
    with pytest.raises(ValueError, match="hold 3 entries parallel to chains"):
        _run(_Stub(), P, [ok, ok, ok], lamP=0.2, chain_weights=[[1.0, 1.0]] * 2)
    with pytest.raises(NotImplementedError, match=r"communicator \(sharded / multi-rank\) are not supported"):
        _run(_Stub(comm=True), P, ok, lamP=0.2)


def test_shared_weight_parsing_is_corpus_refines():
    from oscillink_amd import _receipts as rc
    from oscillink_amd.corpus import Corpus

    blk = Corpus._chains([[0, 1, 2], None, [3, 4]], [[0.5, 2.0], None, None], 0.2, 2.5, 3, 10)
    assert blk["weights"].tolist() == [0.5, 2.0, 1.0]
    lists = [[0, 1, 2], [3, 4]]
    eo = np.array([0, 2, 3], np.int64)
    assert rc.chain_prior_weights([[0.5, 2.0], None], lists, lists, eo).tolist() == [0.5, 2.0, 1.0]
    assert rc.chain_prior_weights(None, lists, lists, eo) is None
    assert rc.chain_prior_weights([None, None], lists, lists, eo) is None
    shared = [[0, 1, 2]] * 2
    assert rc.chain_prior_weights([0.5, 2.0], [0, 1, 2], shared, np.array([0, 2, 4])).tolist() == [0.5, 2.0, 0.5, 2.0]

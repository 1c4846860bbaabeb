"""osc_gates_many / diffusion_gates_many without a device: the library exports the entry point, a
NULL handle is refused, and the Python surface has the signatures the batched gate call is documented with."""
import ctypes
import inspect
import os


def test_library_exports_osc_gates_many_and_native_lists_it():
    from oscillink_amd import _build, _native as nat

    _build.build()
    lib = nat.lib()
    assert hasattr(lib, "osc_gates_many")
    res, args = nat.SIGNATURES["osc_gates_many"]
    assert res is ctypes.c_int and len(args) == 12 and args[0] is nat.Handle
    header = open(os.path.join(os.path.dirname(_build.HERE), "include", "oscillink_hip.h")).read()
    assert "int osc_gates_many(osc_handle h, const float* psis, int32_t Q, float beta, float gamma" in header
    assert "preprocess/diffusion.py:104-124, 130-151" in header


def test_osc_gates_many_rejects_a_null_handle_without_a_device():
    from oscillink_amd import _build, _native as nat

    _build.build()
    lib = nat.lib()
    assert lib.osc_gates_many(None, None, 0, 1.0, 0.1, 0, 1e-4, 256, 1, None, None, None) == nat.OSC_E_INVALID
    h = nat.Handle()  # a NULL handle value passed by ctypes as such
    assert lib.osc_gates_many(h, None, 0, 1.0, 0.1, 1, 1e-4, 256, 1, None, None, None) == nat.OSC_E_INVALID
    assert ctypes.sizeof(h) == ctypes.sizeof(ctypes.c_void_p)


def test_python_surface_has_the_batched_gate_calls():
    import oscillink_amd
    from oscillink_amd import OscillinkLattice, compute_diffusion_gates, compute_diffusion_gates_many

    assert "compute_diffusion_gates_many" in oscillink_amd.__all__
    sig = inspect.signature(OscillinkLattice.diffusion_gates_many)
    names = list(sig.parameters)
    assert names == ["self", "psis", "beta", "gamma", "method", "tol", "max_iters", "clamp"]
    for n in names[2:]:
        assert sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY
    got = {n: sig.parameters[n].default for n in names[2:]}
    assert got == dict(beta=1.0, gamma=0.1, method="direct", tol=1e-4, max_iters=256, clamp=True)
    # the free function takes compute_diffusion_gates' arguments, with psis in psi's place
    one = inspect.signature(compute_diffusion_gates).parameters
    many = inspect.signature(compute_diffusion_gates_many).parameters
    assert [("psis" if n == "psi" else n) for n in one] == list(many)
    for n in one:
        if n not in ("Y", "psi"):
            assert many[n].kind is inspect.Parameter.KEYWORD_ONLY and many[n].default == one[n].default


def test_the_free_function_checks_its_arguments_like_the_single_call():
    import numpy as np
    import pytest

    from oscillink_amd import compute_diffusion_gates_many

    Y = np.ones((4, 3), np.float32)
    P = np.ones((2, 3), np.float32)
    with pytest.raises(ValueError, match="Y must be 2D"):
        compute_diffusion_gates_many(Y[0], P)
    with pytest.raises(ValueError, match="psi dimension mismatch"):
        compute_diffusion_gates_many(Y, P[:, :2])
    with pytest.raises(ValueError, match="gamma must be > 0"):
        compute_diffusion_gates_many(Y, P, gamma=0.0)
    with pytest.raises(ValueError, match="kneighbors must be >=1"):
        compute_diffusion_gates_many(Y, P, kneighbors=0)
    with pytest.raises(ValueError, match="unsupported similarity"):
        compute_diffusion_gates_many(Y, P, similarity="dot")

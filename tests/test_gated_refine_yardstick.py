"""The float64 yardstick of the gated refine tests (tests/_gated.gates64) against the oracle's diffusion gates, on the
corpora the GPU tests use; and the new entry points' NULL-handle behaviour.  No device."""
import ctypes

import numpy as np
import pytest

from tests import _gated as yg

MIN_SPREAD = 1e-2  # fp32 round-off / spread is the gates' error: below this the comparison says nothing


@pytest.mark.parametrize("top_k,k,kw,beta,gamma", yg.SETTINGS)
def test_gates64_against_the_oracle(top_k, k, kw, beta, gamma):
    from oracle import oscillink_oracle as orc

    Y, P = yg.corpus(top_k, k)
    cos = yg.host_cos(Y, P)
    lk = yg.lattice_kw(kw)
    for q in range(P.shape[0]):
        cand = np.lexsort((np.arange(Y.shape[0]), -cos[q]))[:top_k]
        Yc = Y[cand]
        lat = orc.OracleLattice(Yc, **lk)
        g64, raw, s = yg.gates64(np.asarray(lat.A), lat.sqrt_deg, Yc, P[q], beta, gamma)
        spread = float(raw.max() - raw.min())
        assert spread >= MIN_SPREAD, (q, spread)
        common = dict(kneighbors=lk["kneighbors"], row_cap_val=lk["row_cap_val"], beta=beta, gamma=gamma)
        direct = orc.diffusion_gates(Yc, P[q], method="direct", **common)
        cg = orc.diffusion_gates(Yc, P[q], method="cg", tol=1e-7 * max(1.0, float(np.linalg.norm(s))), max_iters=2048,
                                 **common)
        print(f"top_k={top_k} q={q} spread={spread:.4f} |direct-64|={np.abs(direct - g64).max():.2e} "
              f"|cg-64|={np.abs(cg - g64).max():.2e}")
        assert direct.dtype == np.float32 and g64.min() == 0.0 and g64.max() == 1.0
        np.testing.assert_allclose(direct, g64, atol=1e-4, rtol=0)
        np.testing.assert_allclose(cg, g64, atol=1e-4, rtol=0)


def test_gates64_uniform_fallbacks():
    A = np.zeros((1, 1))
    g, raw, s = yg.gates64(A, np.ones(1), np.ones((1, 4), np.float32), np.ones(4, np.float32), 1.0, 0.15)
    assert np.array_equal(g, np.ones(1))
    A = np.array([[0.0, 0.5], [0.5, 0.0]])
    g, raw, s = yg.gates64(A, np.sqrt(np.array([0.5, 0.5])), np.eye(2, dtype=np.float32), np.zeros(2, np.float32), 1.0, 0.1)
    assert np.array_equal(s, np.zeros(2)) and np.array_equal(g, np.ones(2))


def test_gated_entry_points_reject_a_null_handle_without_a_device():
    from oscillink_amd import _build, _native as nat

    _build.build()
    lib = nat.lib()
    assert lib.osc_corpus_gates(None, None, 0, 1, None, 6, 1.0, 1.0, 0.1, 0, 1e-4, 256, 1, None, None, None,
                                None) == nat.OSC_E_INVALID
    assert lib.osc_corpus_refine_gated(None, None, 0, 1, None, None, 1.0, 0.1, 0, 1e-4, 256, 6, 1.0, 1.0, 0.5, 4.0, 1e-4, 64,
                                       8, 0.5, None, None, None, None, None, None, None, None, None) == nat.OSC_E_INVALID
    h = nat.Handle()  # a NULL handle value passed by ctypes as such
    assert lib.osc_corpus_gates(h, None, 0, 1, None, 6, 1.0, 1.0, 0.1, 0, 1e-4, 256, 1, None, None, None,
                                None) == nat.OSC_E_INVALID
    assert ctypes.sizeof(h) == ctypes.sizeof(ctypes.c_void_p)


def test_validation_precedes_the_device():
    """The Python-side checks of the gate arguments need no handle beyond an object: they run before any native call."""
    from oscillink_amd.corpus import Corpus

    for bad, name in ((dict(gamma=0.0), "gamma"), (dict(gamma=float("nan")), "gamma"), (dict(beta=float("inf")), "beta"),
                      (dict(method="lu"), "method"), (dict(max_iters=0), "max_iters")):
        args = dict(beta=1.0, gamma=0.1, method="direct", max_iters=256)
        args.update(bad)
        with pytest.raises(ValueError, match=name):
            Corpus._gate_settings(**args)
    with pytest.raises(ValueError, match="gate_gamma"):
        Corpus._gate_settings(1.0, -1.0, "cg", 4, prefix="gate_")
    assert Corpus._gate_settings(1.2, 0.15, "cg", 7) == (1.2, 0.15, 1, 7)


def test_non_finite_gates_are_returned_with_a_warning_naming_the_query():
    from oscillink_amd.corpus import Corpus

    g = np.ones((3, 4), np.float32)
    g[1, 2] = np.nan
    with pytest.warns(RuntimeWarning, match="query 1 .*iters=7"):
        Corpus._warn_non_finite(g, np.array([3, 7, 3], np.int32), np.array([0.0, np.nan, 0.0], np.float32), "refine_many")
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("error")
        Corpus._warn_non_finite(np.ones((3, 4), np.float32), np.zeros(3, np.int32), np.zeros(3, np.float32), "refine_many")

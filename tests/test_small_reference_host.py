"""The float64 yardstick of tests/test_gpu_small_solve.py (tests/_small_reference.py) against the oracle it is meant to
restate, on the CPU: the matrix it assembles is the operator `OracleLattice.M_mul` applies, with and without gates and a
chain, and the oracle's own U* lies at float32 distance from its solution.  No GPU."""
import numpy as np
import pytest

from oracle import oscillink_oracle as orc
from tests import _small_reference as sr
from tests._cases import relerr


@pytest.mark.parametrize("config", ["plain", "gates", "chain", "gates_chain"])
def test_fp64_solution_solves_the_oracles_system(config):
    N, D = 600, 20
    Y, psi = sr.inputs(N, D, seed=3)
    ref = orc.OracleLattice(Y, kneighbors=8, deterministic_k=True, dense=False)
    gates = sr.gates_with_exact_ends(N) if "gates" in config else None
    chain = sr.chain_for(N) if "chain" in config else None
    sr.configure(ref, psi, gates, chain)
    if gates is not None:
        assert gates.min() == 0.0 and gates.max() == 1.0
    x64, res = sr.ustar_fp64(orc, ref.A, Y, psi, gates, chain)
    assert res < 1e-11
    # the oracle's operator (float32) applied to the float64 solution gives the oracle's right-hand side
    assert relerr(ref.M_mul(x64.astype(np.float32)), ref._rhs()) < 5e-7
    # ... and its own solve lands at float32 distance from it, ever closer as tol tightens down to the float32 floor
    d4 = relerr(ref.solve_Ustar(tol=1e-4, max_iters=64), x64)
    d6 = relerr(ref.solve_Ustar(tol=1e-6, max_iters=64), x64)
    assert 1e-8 < d6 <= d4 < 5e-6

"""refine_many(receipts="full") at config 3's shape (100 000 x 768, Q = 256, top_k 100, k 8, kneighbors 6), ungated and with
diffusion gates (gamma 0.15): 16 sampled queries through the loop check of test_gpu_refine_receipts.py.  An iteration-count
difference is accepted only where the loop's deciding residual lies within 1e-3 relative of its tolerance."""
import numpy as np
import pytest

from tests.test_gpu_refine_receipts import check_against_loop

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("gate_kw", [{}, {"gates": "diffusion", "gate_beta": 1.0, "gate_gamma": 0.15}], ids=["ungated", "gated"])
def test_config3_receipts_against_loop(gate_kw):
    import oscillink_amd as amd

    rng = np.random.default_rng(2024)
    Y = rng.standard_normal((100_000, 768)).astype(np.float32)
    P = (Y[rng.integers(0, 100_000, 256)] + 0.5 * rng.standard_normal((256, 768))).astype(np.float32)
    pick = np.sort(rng.choice(256, 16, replace=False))
    check_against_loop(amd, Y, P, 100, 8, 0.5, {"kneighbors": 6}, gate_kw, "config3-" + ("gated" if gate_kw else "ungated"),
                       queries=[int(q) for q in pick], allow_iter_exception=True)

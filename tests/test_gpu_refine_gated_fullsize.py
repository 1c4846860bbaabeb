"""The gated refine at config 3's shape (100 000 x 768, top_k 100, kneighbors 6, k 8, Q = 256, gamma 0.15): 16 sampled
queries through the gate check and the given-gates check of test_gpu_refine_gated.py."""
import numpy as np
import pytest

from tests.test_gpu_refine_gated import GATED_KEYS, check_gates, check_given_gates

pytestmark = pytest.mark.gpu


def test_config3_gated_refine_against_loop():
    import oscillink_amd as amd

    rng = np.random.default_rng(2024)
    Y = rng.standard_normal((100_000, 768)).astype(np.float32)
    P = (Y[rng.integers(0, 100_000, 256)] + 0.5 * rng.standard_normal((256, 768))).astype(np.float32)
    kw = {"kneighbors": 6}
    with amd.Corpus(Y) as c:
        res = c.refine_many(P, 100, 8, 0.5, as_arrays=True, gates="diffusion", gate_beta=1.0, gate_gamma=0.15, **kw)
        assert sorted(res) == sorted(GATED_KEYS)
        assert res["ids"].shape == (256, 8) and res["gates"].shape == (256, 100)
        pick = np.sort(rng.choice(256, 16, replace=False))
        d = check_gates(amd, c, Y, P[pick], 100, kw, 1.0, 0.15)
        assert np.array_equal(d["gates"], res["gates"][pick]) and np.array_equal(d["candidates"], res["candidates"][pick])
        # check 4 with its condition in force: >= 90 % of the picks compared, and the yardstick's gated picks differ from
        # the ungated ones on a compared step that the device follows (float64 on the CPU, these 16 queries: 127/128
        # picks compared, one near tie; gated picks differ from ungated for 16 of 16 queries)
        sub = check_given_gates(amd, c, Y, P[pick], d["candidates"], d["gates"], 100, 8, 0.5, kw)
        for key in ("ids", "local", "score", "align", "ustar_iters", "ustar_res"):
            assert np.array_equal(sub[key], res[key][pick]), key

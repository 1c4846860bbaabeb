"""Corpus.refine_many at config 3's shape (100 000 x 768, top_k 100, kneighbors 6, k 8, Q = 256): 16 sampled queries
against the per-query loop of the reference's retrieval scripts."""
import numpy as np
import pytest

from tests.test_gpu_refine_many import _compare

pytestmark = pytest.mark.gpu


def test_config3_refine_many_against_loop():
    import oscillink_amd as amd

    rng = np.random.default_rng(2024)
    Y = rng.standard_normal((100_000, 768)).astype(np.float32)
    P = (Y[rng.integers(0, 100_000, 256)] + 0.5 * rng.standard_normal((256, 768))).astype(np.float32)
    with amd.Corpus(Y) as c:
        res = c.refine_many(P, 100, 8, 0.5, kneighbors=6, as_arrays=True)
        assert res["ids"].shape == (256, 8)
        pick = np.sort(rng.choice(256, 16, replace=False))
        sub = {key: v[pick] for key, v in res.items()}
        _compare(amd, Y, P[pick], sub, 100, 8, 0.5, {"kneighbors": 6})

"""receipt_many at config 3's shape (N = 100 000, D = 768, k = 32), full detail, 4 queries (psi0 among them) against the
per-query loop: energies within 1e-4, null-point lists identical except on rows whose decision is a float64 near tie from
the loop's own U* rows, state_sig identical."""
import numpy as np
import pytest

from tests import _receipt_yardstick as yr

pytestmark = pytest.mark.gpu


def _margins(lat, rows):
    """float64 null-decision margins of `rows` (API ids) from the resident U* (the loop's), fetched row by row"""
    rowptr, col, a, _, sd = lat.graph_csr()
    out = {}
    for i in rows:
        js = col[rowptr[i]: rowptr[i + 1]]
        w = a[rowptr[i]: rowptr[i + 1]].astype(np.float64)
        keep = w > 0
        js, w = js[keep], w[keep]
        U = lat._fetch_rows(2, np.concatenate([[i], js]).astype(np.int32)).astype(np.float64)
        di = sd[np.concatenate([[i], js])].astype(np.float64)[:, None] + 1e-12
        Un = U / di
        R = lat.lamC * w * np.sum((Un[0][None, :] - Un[1:]) ** 2, axis=1)
        out[int(i)] = float(yr.null_margins(np.zeros(R.size, dtype=np.int64), R, lat.N)[0])
    return out


def test_config3_full_detail_against_loop():
    import oscillink_amd
    from oscillink_amd import _native

    assert _native.device_count() >= 1
    rng = np.random.default_rng(0)
    N, D = 100_000, 768
    Y = rng.standard_normal((N, D)).astype(np.float32)
    lat = oscillink_amd.Oscillink(Y, kneighbors=32, deterministic_k=True)
    psi0 = (Y[:32].mean(axis=0) / np.linalg.norm(Y[:32].mean(axis=0))).astype(np.float32)
    lat.set_query(psi0)
    lat.settle(max_iters=12, tol=1e-3)
    P = np.stack([psi0, rng.standard_normal(D), Y[123], rng.uniform(-1, 1, D)]).astype(np.float32)
    got = lat.receipt_many(P)
    assert lat.last_query_basis["converged"]
    for q in range(P.shape[0]):
        lat.set_query(P[q])
        lp = lat.receipt()
        g = got[q]
        for key in ("deltaH_total", "coh_drop_sum", "anchor_pen_sum", "query_term_sum"):
            assert g[key] == pytest.approx(lp[key], rel=1e-4), (q, key, g[key], lp[key])
        assert g["meta"]["state_sig"] == lp["meta"]["state_sig"]
        diff = yr.differing_rows(g["null_points"], lp["null_points"])
        assert len(diff) <= 1e-3 * N, (q, len(diff))
        if diff:
            m = _margins(lat, diff)
            assert all(v < 1e-3 for v in m.values()), (q, [(i, v) for i, v in m.items() if v >= 1e-3][:5])
        print(f"query {q}: {len(g['null_points'])} null points, {len(diff)} near-tie rows differ")

"""The yardstick of tests/test_gpu_refine_shapes.py, proved without a device: on every (D, top_k) of tests/_refine_shapes.py,
gated and ungated, the oracle's settle / U* / null points on the candidate lattices show the margins the GPU tests rely on.

  deciding residuals   no settle (tol 1e-3) or U* (tol 1e-4) residual of the oracle's histories lies within 10 % of its
                       tolerance, so the GPU tests demand identical iteration counts and accept no exception;
  null-point ties      at most 2 % of a shape's rows decide their null point inside the 1e-3 band.  (1536, 7) is exempt
                       from this: with K = 7 a single row of its 21 in the band is 4.8 %.  It is held to "no null points
                       at all" instead, for every query, gated and ungated;
  row coverage         every shape with top_k >= 64 has a null point in a row >= top_k - 2 and more than 0.6 top_k null
                       points in all, so the 256-row emit rounds and a cap of 300 do bite;
  bundle margins       every k = 8 pick is decided by more than the GPU test's near-tie band (1e-4), so the whole list is
                       compared there.

The second extra settings row (lamG 2, lamC 1.5, lamQ 0.5, row_cap 0.3, settle dt 0.5) runs on the corpus of (520, 64) as
it is: its closest deciding residual is printed below and passes the 10 % condition without a change of seed or lambdas."""
import numpy as np
import pytest

from tests import _gated as yg
from tests import _queries as yq
from tests import _receipt_yardstick as yr
from tests import _refine_shapes as rs

DECIDING = 0.10
NEAR = 1e-3
NEAR_FRACTION = 0.02
NEAR_TIE = 1e-4
CASES = [(D, tk, rs.K, {}, 1.0) for D, tk in rs.SHAPES] + [rs.EXTRA[1]]


@pytest.mark.parametrize("D,top_k,k,kw,dt", CASES)
def test_oracle_margins_on_the_shapes(D, top_k, k, kw, dt):
    from oracle import oscillink_oracle as orc

    Y, P = rs.cached_corpus(D, top_k)
    lk = yg.lattice_kw(kw)
    cos = yg.host_cos(Y, P)
    for gated in (False, True):
        tag = f"D={D} top_k={top_k} {'gated' if gated else 'ungated'}" + (f" {kw} dt={dt}" if kw else "")
        near = rows = total_nulls = 0
        worst = np.inf
        last_row = -1
        bundle_margin = np.inf
        for q in range(P.shape[0]):
            cand = np.lexsort((np.arange(Y.shape[0]), -cos[q]))[:top_k]
            Yc = Y[cand]
            g = None
            if gated:
                g = orc.diffusion_gates(Yc, P[q], kneighbors=lk["kneighbors"], row_cap_val=lk["row_cap_val"],
                                        beta=rs.GATE_BETA, gamma=rs.GATE_GAMMA)
            o = orc.OracleLattice(Yc, **lk)
            o.set_query(P[q], gates=g)
            s = dict(o.settle(dt=dt))
            hs = list(o.history)
            Us = o.solve_Ustar()
            hu = list(o.history)
            nulls = o.nulls(Us)
            dec = min(min(abs(x - 1e-3) / 1e-3 for x in hs), min(abs(x - 1e-4) / 1e-4 for x in hu))
            worst = min(worst, dec)
            A, sd = np.asarray(o.A, np.float64), np.asarray(o.sqrt_deg, np.float64)
            r, _, R = yr.edge_residuals(Us, A, sd, o.lamC)
            m = yr.null_margins(r, R, top_k)
            B = np.ones(top_k) if g is None else g.astype(np.float64)
            U64 = yq.ustar(yq.dense_M(A, sd, B, lk["lamG"], lk["lamC"], lk["lamQ"]), Yc, B, P[q], lk["lamG"], lk["lamQ"])
            margins = yq.bundle(Yc, U64, P[q], A, sd, lk["lamC"], k=k, alpha=rs.ALPHA)[3]
            bundle_margin = min(bundle_margin, min(margins))
            spread = ""
            if gated:  # whether the GPU test's gates-against-float64 comparison applies (its raw spread rule)
                raw = yg.gates64(A, sd, Yc, P[q], rs.GATE_BETA, rs.GATE_GAMMA)[1]
                spread = f" raw gate spread {float(raw.max() - raw.min()):.4f}"
            print(f"{tag} q={q}: settle {s['iters']} ustar {o.last_ustar['iters']} nulls {len(nulls)} near-tie rows "
                  f"{int(np.sum(m < NEAR))} closest deciding residual {dec:.4f} smallest bundle margin {min(margins):.3e}"
                  + spread)
            assert s["res"] <= 1e-3 and o.last_ustar["converged"], tag
            near += int(np.sum(m < NEAR))
            rows += top_k
            total_nulls += len(nulls)
            last_row = max([last_row] + [int(p["edge"][0]) for p in nulls])
            if (D, top_k) == (1536, 7):
                assert nulls == [], (tag, q)
            elif top_k >= 64:
                assert len(nulls) > 0.6 * top_k, (tag, q, len(nulls))
        print(f"{tag}: closest deciding residual {worst:.4f}, near-tie rows {near} of {rows}, null points {total_nulls} "
              f"({total_nulls / rows:.2f} of the rows), last null row {last_row}, smallest bundle margin {bundle_margin:.3e}")
        assert worst >= DECIDING, (tag, worst)
        if (D, top_k) != (1536, 7):  # exempt, see the module docstring; held to `nulls == []` above
            assert near <= NEAR_FRACTION * rows, (tag, near, rows)
        if top_k >= 64:
            assert last_row >= top_k - 2, (tag, last_row)
        assert bundle_margin >= NEAR_TIE, (tag, bundle_margin)


def test_shape_table_reaches_every_instantiation():
    """The table's own claims: every NC of cq_with_nc, the 5 -> 6 fall-through, pad columns, a ragged last group, both
    limits, and row counts of exactly one, partly and fully more than a round of 256."""
    nc = {(D, tk): (rs.ldn(D) + 255) // 256 for D, tk in rs.SHAPES}
    assert set(nc.values()) == {1, 2, 3, 4, 5, 6}
    assert rs.ldn(257) == 288 and rs.ldn(520) == 544 and rs.ldn(1290) == 1312 and rs.ldn(1536) == 1536
    assert nc[(1040, 100)] == nc[(1100, 300)] == 5 and nc[(1290, 100)] == nc[(1536, 1024)] == 6
    assert {tk for _, tk in rs.SHAPES} >= {7, 64, 100, 257, 300, 1024}
    for D, tk in rs.SHAPES:
        Y, P = rs.cached_corpus(D, tk)
        assert Y.shape == (rs.N_ROWS, D) and P.shape == (rs.N_QUERIES, D) and Y.dtype == P.dtype == np.float32

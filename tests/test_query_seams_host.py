"""CPU checks of the query-seam references (tests/_query_seams.py): the two references against each other, against the
existing yardsticks (tests/_queries.py, tests/_receipt_yardstick.py) and the oracle on small cases; the near-tie cap on
the oracle's graph for every table entry; and the float32 distances behind reference B's tolerance."""
import functools

import numpy as np
import pytest

from tests import _query_seams as qs
from tests import _queries as yq
from tests import _receipt_yardstick as yr

CASE_IDS = [c["id"] for c in qs.cases()]
SMALL = ["rows-n127", "queries-gates_chain_n333_d50_k7", "degree-hub65-d32", "degree-empty_rows-d32", "width-d5-plain"]


@functools.lru_cache(maxsize=None)
def _evaluated(case_id):
    """Per query of a table entry, on the oracle's graph: the float64 MMR margins (reference A) and the distances of the
    plain float32 evaluation from float64, for the fresh (U = Y) and the settled state."""
    c = qs.case(case_id)
    ref, s, P = qs.oracle_of(c)
    X, x = s.basis64()
    X32, x32 = X.astype(np.float32), x.astype(np.float32)
    ref.settle(max_iters=12, tol=1e-3)
    states = {"fresh": s.Y, "settled": ref.U.copy()}
    full, dist = [], {"score": 0.0, "align": 0.0, "sums": 0.0, "deltaH": 0.0}
    for q in range(P.shape[0]):
        Us = qs.ustar(X, x, P[q])
        Us32 = qs.ustar(X32, x32, P[q], np.float32)
        _, _, _, margins = qs.bundle64(s, Us, P[q])
        full.append(qs.full_steps(margins) == len(margins))
        sc, al = qs.scores(s, Us, P[q])
        sc32, al32 = qs.scores(s, Us32, P[q], dt=np.float32)
        dist["score"] = max(dist["score"], float(np.max(np.abs(sc32 - sc))))
        dist["align"] = max(dist["align"], float(np.max(np.abs(al32 - al))))
        for U in states.values():
            want = qs.receipt(s, U, Us, P[q], nulls=False)
            got = qs.receipt(s, U, Us32, P[q], dt=np.float32)
            dist["sums"] = max(dist["sums"], qs.sums_distance(got, want))
            dist["deltaH"] = max(dist["deltaH"], abs(got["deltaH"] - want["deltaH"]) / abs(want["deltaH"]))
    return np.array(full), dist


@pytest.mark.parametrize("case_id", SMALL)
def test_references_agree_on_small_cases(case_id):
    """The basis form U* = X + x psi^T equals a dense solve per query; `bundle64` / `receipt` on it equal the existing
    yardsticks, which solve per query; the oracle's own float32 CG lands on the same U*; and reference B's arithmetic
    (here: from reference A's basis rounded to float32) stays inside reference A's gates."""
    from oracle import oscillink_oracle as orc

    c = qs.case(case_id)
    ref, s, P = qs.oracle_of(c)
    P = P[:7]
    X, x = s.basis64()
    Xb, xb = X.astype(np.float32).astype(np.float64), x.astype(np.float32).astype(np.float64)
    ref.settle(max_iters=12, tol=1e-3)
    U = ref.U.copy()
    for q in range(P.shape[0]):
        Us = qs.ustar(X, x, P[q])
        direct = yq.ustar(s.M, s.Y, s.B, P[q], s.lamG, s.lamQ)
        assert np.max(np.abs(Us - direct)) <= 1e-10 * max(1.0, float(np.max(np.abs(direct)))), q
        ref.set_query(P[q])
        cg = ref.solve_Ustar(tol=1e-6, max_iters=256)
        assert np.linalg.norm(cg - Us) <= 2e-5 * np.linalg.norm(Us), q
        # bundles: the dense-adjacency yardstick and the all-rows scores
        ids, score, align, margins = qs.bundle64(s, Us, P[q])
        w_ids, w_score, w_align, w_margins = yq.bundle(s.Y, direct, P[q], s.A, s.sd, s.lamC, k=qs.K)
        assert ids == w_ids and np.allclose(margins, w_margins, rtol=0, atol=1e-9), q
        assert np.allclose(score, w_score, rtol=0, atol=1e-9) and np.allclose(align, w_align, rtol=0, atol=1e-9), q
        sc, al = qs.scores(s, Us, P[q])
        assert np.allclose(sc[ids], score, rtol=0, atol=1e-12) and np.allclose(al[ids], align, rtol=0, atol=1e-12), q
        # receipts: tests/_receipt_yardstick.py (oracle formulas, float32 per-node values and float32 U - U*)
        got = qs.receipt(s, U, Us, P[q])
        want = yr.receipt(s.Y, U, P[q], s.A, s.sd, s.B, s.lamG, s.lamC, s.lamQ, s.M)
        assert qs.sums_distance(got, want) <= 1e-6, q
        assert abs(got["deltaH"] - want["deltaH"]) <= 1e-5 * abs(want["deltaH"]), q
        assert np.allclose(got["margin"], want["margin"], rtol=1e-6, atol=1e-9), q
        differ = [i for i in set(got["nulls"]) | set(yr.null_edges(want["null_points"]))
                  if got["nulls"].get(i) != yr.null_edges(want["null_points"]).get(i)]
        assert all(want["margin"][i] < 1e-5 for i in differ), (q, differ)  # (the oracle's R is float32)
        unsettled = orc.deltaH_trace(s.Y.astype(np.float64), Us, lambda V: s.M @ V)
        assert abs(qs.receipt(s, s.Y, Us, P[q], nulls=False)["deltaH"] - unsettled) <= 1e-5 * abs(unsettled), q
        # reference B's evaluation from a float32 basis, inside reference A's gates
        Ub = qs.ustar(Xb, xb, P[q])
        b_ids, b_score, b_align, _ = qs.bundle64(s, Ub, P[q])
        n = qs.full_steps(margins)
        assert b_ids[:n] == ids[:n], q
        assert np.allclose(b_score[:n], score[:n], rtol=0, atol=qs.A_ATOL), q
        assert np.allclose(b_align[:n], align[:n], rtol=0, atol=qs.A_ATOL), q
        b = qs.receipt(s, U, Ub, P[q])
        assert qs.sums_distance(b, got) <= qs.A_RTOL and abs(b["deltaH"] - got["deltaH"]) <= qs.A_RTOL * abs(got["deltaH"]), q
        assert all(got["margin"][i] < qs.NEAR for i in set(b["nulls"]) | set(got["nulls"])
                   if b["nulls"].get(i) != got["nulls"].get(i)), q


@pytest.mark.parametrize("case_id", CASE_IDS)
def test_near_tie_cap_holds_for_every_entry(case_id):
    """At most one query in four of a batch is compared over fewer than all k steps, at least one in full: the margins
    are float64's, on the oracle's graph for the table's seeded inputs (the GPU test asserts it again on its graph)."""
    full, _ = _evaluated(case_id)
    counts = [n for n, _ in qs.QUERY_COUNTS] if case_id.startswith("queries-") else [full.size]
    for Q in counts:
        truncated = int(np.count_nonzero(~full[:Q]))
        print(f"{case_id} Q {Q}: {truncated} id lists end at a near tie")
        assert qs.cap_holds(truncated, Q), (case_id, Q, truncated)
        if case_id.startswith("queries-"):  # the subset that reference A is asked about keeps the cap too
            sel = qs.a_queries(Q)
            assert qs.cap_holds(int(np.count_nonzero(~full[sel])), len(sel)), (case_id, Q, sel)


@pytest.mark.parametrize("case_id", CASE_IDS)
def test_float32_distance_of_every_case(case_id):
    """The measurement behind `qs.B_TOL`: no entry's plain float32 evaluation lies further from float64 than recorded."""
    _, dist = _evaluated(case_id)
    print(f"{case_id}: float32 numpy from float64: " + ", ".join(f"{k} {v:.3e}" for k, v in dist.items()))
    for key, v in dist.items():
        assert v <= qs.F32_DIST[key], (case_id, key, v)


def test_recorded_distances_name_their_source():
    assert set(qs.F32_SOURCE) == set(qs.F32_DIST) and all(v in CASE_IDS for v in qs.F32_SOURCE.values())
    for key, cid in qs.F32_SOURCE.items():  # the recorded number is that entry's, to the digits recorded
        assert _evaluated(cid)[1][key] == pytest.approx(qs.F32_DIST[key], rel=5e-2), key


def test_tables_reach_what_they_name():
    """Shapes only: the arithmetic the table's comments rely on."""
    for D, _, _, _ in qs.WIDTHS:
        assert D <= 256 or (D + 255) // 256 >= 2
    assert {D % 4 for D, _, _, _ in qs.WIDTHS} == {0, 1, 3}
    assert {n for n, _ in qs.QUERY_COUNTS} >= {1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300}
    for kind in ("hub64", "hub65", "hub120", "hub128"):
        A = qs.injected_graph(kind, qs.DEG_N, 60)
        deg = np.diff(A.indptr)
        assert deg[qs.HUB] == int(kind[3:]) and deg.max() == deg[qs.HUB] and (A != A.T).nnz == 0
        assert A.data.min() >= 0.05 and A.data.max() <= 1.0
    A = qs.injected_graph("empty_rows", qs.DEG_N, 68)
    assert np.count_nonzero(np.diff(A.indptr) == 0) > qs.DEG_N // 2
    for N, Q in ((500, 257), (129, 12)):
        S = qs.mmr_scores(N, Q, 71)
        for col in qs.equal_columns(Q):
            assert np.all(S[:, col] == S[0, col])
        assert S[7, 4] == S[47, 4] == S[:, 4].max() and np.array_equal(S[8:40, 4], S[48:80, 4])

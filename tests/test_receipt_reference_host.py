"""The float64 yardstick of the receipt kernels (tests/_receipt_reference.py) against oracle/oscillink_oracle.py, and the
conditions the cases of tests/test_gpu_receipt_kernels.py and tests/test_gpu_mmr_kernels.py rest on, proven from float64 alone.
CPU only.

Per case: the stationary state comes from a float64 direct solve and is rounded to float32 (what a device holds); the
yardstick evaluated in float32 on those inputs stays within a QUARTER of every bound of the GPU tier; at z_th = the median z
both outcomes of the null decision occur and at most 2 % of the rows with an edge have a margin below 1e-3; the graph has the
degrees and the column chunks the case exists for.  MMR: at most one list in ten is cut short by a near tie, none before its
third pick."""
import numpy as np
import pytest

from tests import _queries as yq
from tests import _receipt_reference as RR

HEADROOM = 0.25
ORACLE_RTOL = 1e-12


@pytest.fixture(scope="module")
def evaluated():
    """name -> (case, yardstick in float64, the same in float32, z_th), each computed once."""
    cache = {}

    def get(name):
        if name not in cache:
            case = RR.build_case(name)
            Us = case.exact_ustar().astype(np.float32)
            args = (case.Y, Us, case.psi, case.B, case.rowptr, case.col, case.a, case.sqrt_deg(), *RR.LAMS)
            r64 = RR.receipt_reference(*args)
            r32 = RR.receipt_reference(*args, dtype=np.float32)
            cache[name] = ((case.N, case.D, case.ld, case.nch, case.pair), r64, r32, r64.median_z())
        return cache[name]

    return get


# ------------------------------------------------------------------------------------------------------- tie to the oracle
@pytest.mark.parametrize("name,gates", [("row_d7", True), ("row_isolated", False), ("row_hub", True)])
def test_yardstick_equals_the_oracle(name, gates, monkeypatch):
    """Both at the same float64 U* of a dense solve.  The oracle rounds its outputs (and R) to float32 at the end; its
    formulas are evaluated here with that rounding switched off, so that the agreement can be asked for at 1e-12."""
    from oracle import oscillink_oracle as orc

    monkeypatch.setattr(orc, "F32", np.float64)
    case = RR.build_case(name)
    assert case.N <= 400
    lamG, lamC, lamQ = RR.LAMS
    B = case.B if gates else np.ones(case.N, dtype=np.float32)
    A, sd = case.dense_A().astype(np.float64), case.sqrt_deg().astype(np.float64)
    Us = yq.ustar(yq.dense_M(A, sd, B, lamG, lamC, lamQ), case.Y, B, case.psi, lamG, lamQ)
    ref = RR.receipt_reference(case.Y, Us, case.psi, B, case.rowptr, case.col, case.a, case.sqrt_deg(), lamG, lamC, lamQ)
    coh, anchor, query = orc.per_node_components(case.Y.astype(np.float64), Us, A, sd, lamG, lamC, lamQ, B.astype(np.float64),
                                                 case.psi.astype(np.float64))
    assert coh.dtype == np.float64
    for got, want in ((ref.coh, coh), (ref.anchor, anchor), (ref.query, query)):
        assert np.all(np.abs(got - want) <= ORACLE_RTOL * np.abs(want))
    z_th = ref.median_z()
    is_null, _ = ref.decide(z_th)
    nulls = orc.null_points(Us, A, sd, lamC, z_th)
    assert 0 < len(nulls) < np.count_nonzero(ref.null_col >= 0)
    assert [p["edge"] for p in nulls] == [[int(i), int(ref.null_col[i])] for i in np.flatnonzero(is_null)]
    rows = np.flatnonzero(is_null)
    assert np.allclose([p["z"] for p in nulls], ref.null_z[rows], rtol=ORACLE_RTOL, atol=0.0)
    assert np.allclose([p["residual"] for p in nulls], ref.null_R[rows], rtol=ORACLE_RTOL, atol=0.0)
    # ... and the coherence drop of tests/_queries.py, the yardstick of the bundle tests
    assert np.allclose(ref.coh, yq.coherence_drop(case.Y, Us, case.graph, sd, lamC), rtol=1e-11, atol=0.0)


# ------------------------------------------------------------------------------------------ the conditions of the GPU tier
@pytest.mark.parametrize("name", sorted(RR.CASES))
def test_float32_stays_within_a_quarter_of_every_bound(evaluated, name):
    (N, D, ld, nch, pair), r64, r32, z_th = evaluated(name)
    is_null32, _ = r32.decide(z_th)
    rows = np.flatnonzero(is_null32)
    res = RR.compare((r32.coh, r32.anchor, r32.query, r32.sums), r64, z_th, rows, r32.null_col[rows], r32.null_z[rows], r32.null_R[rows],
                     frac=HEADROOM)
    print(name, f"N={N} D={D} ld={ld} nch={nch} pair={pair} z_th={z_th:.4f}",
          {k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()})
    assert RR.within_bounds(res) == []
    # both outcomes of the decision, in numbers: the median splits the rows with an edge
    assert res["nulls_among_compared"] > 0.4 * np.count_nonzero(r64.null_col >= 0)
    assert res["non_nulls_among_compared"] > 0.4 * np.count_nonzero(r64.null_col >= 0)
    # mag is what coh's error scales with, not coh: a difference of positive terms
    assert np.all(r64.mag[r64.null_col >= 0] > 0) and np.all(np.abs(r64.coh) <= r64.mag)


def test_the_cases_reach_every_template_and_form():
    got = {(RR.build_case(n).pair, RR.template(RR.build_case(n).nch), RR.build_case(n).nch) for n in RR.CASES
           if "hub" not in n}
    rows = {(t, nch) for pair, t, nch in got if not pair}
    pairs = {(t, nch) for pair, t, nch in got if pair}
    assert rows == {(1, 1), (2, 2), (3, 3), (4, 4), (6, 5), (6, 6), (0, 7), (0, 9)}
    assert pairs == {(1, 1), (2, 2), (3, 3), (4, 4), (6, 5), (6, 6)}
    assert RR.build_case("row_d50_ld64").ld == 64 and RR.build_case("row_d250_ld288").ld == 288  # pad columns: 14 and 38
    assert RR.build_case("pair_d1025").ld == 1056 and RR.build_case("pair_d257").ld == 260


def test_isolated_rows():
    case = RR.build_case("row_isolated")
    deg = np.diff(case.rowptr)
    assert case.N == 309 and np.all(deg[300:] == 0) and np.all(deg[:300] == 5)


@pytest.mark.parametrize("name", ["row_hub"] + RR.HUB_CASES)
def test_hub_graphs_have_the_degrees_they_exist_for(name):
    case = RR.build_case(name)
    fb = RR.finish_branches(case.rowptr, case.col)
    print(name, fb)
    assert fb["max_deg"] == 300 and fb["deg_over_128"] == 2 and fb["deg_65_128"] == 2
    assert fb["c0"] > 0 and fb["c1"] > 0 and fb["tail"] > 0     # mirror slots in c0, in c1 and behind them
    assert fb["max_lower_in_chunk"] > 4                         # several rounds of the four-in-flight loop
    deg = np.diff(case.rowptr)
    if name == "pair_hub_reversed":
        assert deg[-1] == 300 and fb["all_lower_chunks"] == 5   # the last row: 300 lower neighbours over five e0 chunks
        assert fb["high_rows_with_over_64_lower"] >= 1
        assert fb["max_lower_in_chunk"] == 64
    else:
        assert deg[0] == 300 and sorted(deg[[310, 320, 330]]) == [65, 100, 130]


@pytest.mark.parametrize("stars", [40, 600])
def test_star_twins_tie_at_the_centres_largest_residual(stars):
    case, centres, twins = RR.stars_case(stars, 16, 21)
    assert case.N == 7 * stars and case.pair == (stars == 600)
    assert np.all(np.diff(case.rowptr)[centres] == 6) and np.all(np.diff(case.rowptr)[twins.ravel()] == 1)
    a, b = twins[:, :, 0], twins[:, :, 1]  # a twin pair: the same anchor row, weight and gate
    assert np.all(a < b) and np.array_equal(case.Y[a], case.Y[b]) and np.array_equal(case.B[a], case.B[b])
    assert np.array_equal(case.a[case.rowptr[a]], case.a[case.rowptr[b]])
    assert np.any(a[:, 0] > centres) and np.any(b[:, 0] < centres)  # shuffled ids: twins on both sides of their centre
    Us = case.exact_ustar()
    assert np.allclose(Us[a], Us[b], rtol=1e-12, atol=1e-13)
    ref = RR.receipt_reference(case.Y, Us, case.psi, case.B, case.rowptr, case.col, case.a, case.sqrt_deg(), *RR.LAMS)
    for s, c in enumerate(centres):
        R = dict(zip(case.col[case.rowptr[c]: case.rowptr[c + 1]].tolist(), ref.R[case.rowptr[c]: case.rowptr[c + 1]]))
        far, rest = [R[int(twins[s, 0, t])] for t in range(2)], [R[int(j)] for j in twins[s, 1:].ravel()]
        assert abs(far[0] - far[1]) <= 1e-11 * far[0] and max(rest) < 0.9 * min(far), (s, far, rest)
        assert ref.null_z[c] > 1.0  # a null point at z_th = 0


# ------------------------------------------------------------------------------------------------------------------- MMR
def _cut(name):
    ids, margins = RR.mmr_reference(name)
    lam = RR.MMR_CASES[name][4]
    skip = 1 if lam == 1.0 else 0  # (lambda = 1: step 0 is an all-tie by construction, asserted as such by the GPU test)
    return RR.first_near_tie(margins[skip:]) + skip, len(ids)


def test_mmr_near_tie_cap():
    cuts = {name: _cut(name) for name in RR.MMR_CASES}
    short = {name: c for name, c in cuts.items() if c[0] < c[1]}
    print("lists cut short by a near tie:", short)
    assert len(short) <= len(cuts) / 10
    assert all(c[0] >= 2 for c in short.values())


def test_mmr_cases_are_what_they_claim():
    for name, (N, D, seed, k, lam, zero) in RR.MMR_CASES.items():
        ids, margins = RR.mmr_reference(name)
        assert len(ids) == min(k, N) and len(set(ids)) == len(ids)
    ids, margins = RR.mmr_reference("lambda1")
    assert ids[0] == 0 and margins[0] == 0.0
    N, D, seed, k, lam, zero = RR.MMR_CASES["lambda0"]
    assert N > 8192
    scores = RR.mmr_inputs(N, D, seed)[1]
    assert list(RR.mmr_reference("lambda0")[0]) == np.argsort(-scores.astype(np.float64), kind="stable")[:k].tolist()
    for name in ("exhaust_k_n", "exhaust_k_n_plus_5"):
        assert sorted(RR.mmr_reference(name)[0]) == list(range(257))
    assert RR.MMR_CASES["n65537_strided"][0] > 65536 and RR.MMR_CASES["exhaust_k_n_plus_5"][3] == 262


@pytest.mark.parametrize("N,D,seed", [(700, 10, 41), (2000, 24, 42)])
def test_mmr_duplicate_blocks_tie_exactly_in_float64(N, D, seed):
    """The exact-tie lists of the GPU test: inside a block of identical rows every step is an exact tie (margin 0.0) that the
    smallest remaining id wins; every other step is decided by more than the near-tie figure."""
    Y, scores, groups = RR.duplicate_blocks(N, D, seed)
    k = 24
    ids, margins = yq.mmr(Y, scores, k, 0.5)
    assert RR.picks_smallest_remaining(ids, groups)
    ties = [t for t, m in enumerate(margins) if m == 0.0]
    assert len(ties) >= 10
    assert all(m == 0.0 or m > RR.NEAR_TIE for m in margins)


def test_cosine_reference_guards():
    rows = np.array([[3.0, 4.0], [0.0, 0.0], [-1.0, 0.0]])
    assert np.allclose(RR.cosine_to(rows, [2.0, 0.0]), [0.6, 0.0, -1.0], rtol=1e-11, atol=0.0)
    assert np.array_equal(RR.cosine_to(rows, [0.0, 0.0]), [0.0, 0.0, 0.0])

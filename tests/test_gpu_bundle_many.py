"""Multi-query bundles: `bundle_many` against the reference's recorded bundles, a float64
yardstick (tests/_queries.py), this library's own per-query path and itself (batch composition, chunking, caching)."""

import numpy as np
import pytest

from tests import _queries as yq
from tests._cases import PARAM_CASES, ctor_kwargs, load_case, make_inputs, random_gates

pytestmark = pytest.mark.gpu

NEAR_TIE = 1e-4


@pytest.fixture(scope="module")
def amd():
    import oscillink_amd
    from oscillink_amd import _native

    assert _native.device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return oscillink_amd


def _fixture_lattice(amd, name):
    case = load_case(name)
    rc = case["recipe"]
    Y, psi = make_inputs(rc)
    lat = amd.Oscillink(Y, kneighbors=rc["k"], deterministic_k=True, **ctor_kwargs(rc))
    gates = None
    if rc["gates"] == "random":
        gates = random_gates(rc)
    elif rc["gates"] == "diffusion":
        gates = case["gates"]
    lat.set_query(psi, gates=gates)
    if rc["chain"]:
        lat.add_chain(rc["chain"], lamP=rc["lamP"])
    return lat, case, Y, psi


def _batch(Y, psi, seed=0):
    """the given psi first, then random queries, an anchor row and psi = 0 (7 queries)"""
    rng = np.random.default_rng(seed)
    D = Y.shape[1]
    rows = [psi, rng.standard_normal(D), 3.0 * rng.standard_normal(D), Y[5], rng.uniform(-1, 1, D),
            rng.standard_normal(D) / np.sqrt(D), np.zeros(D)]
    return np.stack(rows).astype(np.float32)


def _yardstick(lat):
    """float64 (M, A, sqrt_deg) of the lattice's own graph, gates, chain and lambdas"""
    rowptr, col, a, _, sd = lat.graph_csr()
    A = np.zeros((lat.N, lat.N))
    A[np.repeat(np.arange(lat.N), np.diff(rowptr)), col] = a
    Lp = lat.L_path if lat.lamP > 0 else None
    M = yq.dense_M(A, sd, lat.B_diag, lat.lamG, lat.lamC, lat.lamQ, lat.lamP, Lp)
    return M, A, sd


@pytest.mark.parametrize("name", ["c1_n80_d128_k8", "g1_n400_d64_k6_chain8", "gates_chain_n333_d50_k7"])
def test_fixture_query_first_in_batch(amd, name):
    lat, case, Y, psi = _fixture_lattice(amd, name)
    out = lat.bundle_many(_batch(Y, psi), k=6, alpha=0.5)
    assert len(out) == 7 and all(len(o) == 6 for o in out)
    assert [b["id"] for b in out[0]] == case["bundle_ids"].tolist()
    assert np.allclose([b["score"] for b in out[0]], case["bundle_score"], rtol=1e-3, atol=1e-4)
    assert np.allclose([b["align"] for b in out[0]], case["bundle_align"], rtol=1e-3, atol=1e-5)
    assert lat.last_query_basis["converged"]


@pytest.mark.parametrize("name", PARAM_CASES)
def test_param_cases_against_yardstick(amd, name):
    lat, case, Y, psi = _fixture_lattice(amd, name)
    P = _batch(Y, psi, seed=1)
    ids, score, align = lat.bundle_many(P, k=8, alpha=0.5, as_arrays=True)
    M, A, sd = _yardstick(lat)
    truncated = 0
    for q in range(P.shape[0]):
        U = yq.ustar(M, Y, lat.B_diag, P[q], lat.lamG, lat.lamQ)
        w_ids, w_score, w_align, margins = yq.bundle(Y, U, P[q], A, sd, lat.lamC, k=8)
        ok, cut = yq.same_until_near_tie(ids[q].tolist(), w_ids, margins, NEAR_TIE)
        assert ok, (q, ids[q].tolist(), w_ids, margins)
        truncated += int(cut)
        n = len(w_ids) if not cut else next(t for t, m in enumerate(margins) if m < NEAR_TIE)
        assert np.allclose(score[q, :n], w_score[:n], atol=2e-4, rtol=0), q
        assert np.allclose(align[q, :n], w_align[:n], atol=2e-4, rtol=0), q
    print(f"{name}: {truncated} of {P.shape[0]} id lists compared up to a near tie")


def test_matches_per_query_path_and_leaves_state(amd):
    lat, case, Y, psi = _fixture_lattice(amd, "gates_chain_n333_d50_k7")
    lat.settle(max_iters=12, tol=1e-3)
    rec0 = lat.receipt()
    U_star = lat.solve_Ustar().copy()
    st0, lu0, psi0, U0 = dict(lat.stats), dict(lat.last_ustar), lat.psi.copy(), lat.U.copy()
    P = _batch(Y, psi, seed=2)
    ids, score, align = lat.bundle_many(P, k=8, as_arrays=True)
    assert {k: v for k, v in lat.stats.items() if k.startswith("ustar_")} == {k: v for k, v in st0.items() if k.startswith("ustar_")}
    assert lat.stats["query_basis_solves"] == st0["query_basis_solves"] + 1
    assert lat.last_ustar == lu0
    assert np.array_equal(lat.psi, psi0) and np.array_equal(lat.U, U0)
    assert np.array_equal(lat.solve_Ustar(), U_star)
    rec1 = lat.receipt()
    for key in ("deltaH_total", "coh_drop_sum", "anchor_pen_sum", "query_term_sum", "null_points"):
        assert rec1[key] == rec0[key], key
    assert rec1["meta"]["state_sig"] == rec0["meta"]["state_sig"]
    M, A, sd = _yardstick(lat)
    for q in range(P.shape[0]):
        lat.set_query(P[q])
        bd = lat.bundle(k=8, alpha=0.5)
        U = yq.ustar(M, Y, lat.B_diag, P[q], lat.lamG, lat.lamQ)
        _, _, _, margins = yq.bundle(Y, U, P[q], A, sd, lat.lamC, k=8)
        ok, _ = yq.same_until_near_tie(ids[q].tolist(), [b["id"] for b in bd], margins, NEAR_TIE)
        assert ok, q


def test_implied_residual_within_contract(amd):
    from oracle import oscillink_oracle as orc

    lat, case, Y, psi = _fixture_lattice(amd, "g1_n400_d64_k6_chain8")
    P = _batch(Y, psi, seed=3)
    tol = 1e-4
    lat.bundle_many(P, tol=tol)
    X, x = lat.query_basis(tol=tol)
    assert lat.last_query_basis["converged"]
    rc = case["recipe"]
    ref = orc.OracleLattice(Y, kneighbors=rc["k"], deterministic_k=True, graph=lat.A)
    ref.set_query(psi, gates=lat.B_diag)
    ref.add_chain(rc["chain"], lamP=rc["lamP"])
    for q in range(P.shape[0]):
        U = X.astype(np.float64) + np.outer(x, P[q])
        R = lat.lamG * Y + lat.lamQ * lat.B_diag[:, None] * P[q][None, :] - ref.M_mul(U)
        assert np.max(np.linalg.norm(R, axis=0)) <= 2 * tol, q


def test_batch_independence_and_chunking(amd):
    from oscillink_amd import _native

    lat, case, Y, psi = _fixture_lattice(amd, "c1_n80_d128_k8")
    rng = np.random.default_rng(4)
    Q = _native.OSC_QUERY_CHUNK + 37
    P = rng.standard_normal((Q, Y.shape[1])).astype(np.float32)
    big = lat.bundle_many(P, k=8, as_arrays=True)
    for q in (0, 5, _native.OSC_QUERY_CHUNK - 1, _native.OSC_QUERY_CHUNK, Q - 1):
        alone = lat.bundle_many(P[q:q + 1], k=8, as_arrays=True)
        for a, b in zip(alone, big):
            assert np.array_equal(a[0], b[q]), q
    order = rng.permutation(Q)[:9]
    sub = lat.bundle_many(P[order], k=8, as_arrays=True)
    for t, q in enumerate(order):
        for a, b in zip(sub, big):
            assert np.array_equal(a[t], b[q])


def test_basis_caching(amd):
    lat, case, Y, psi = _fixture_lattice(amd, "gates_chain_n333_d50_k7")
    rc = case["recipe"]
    P = _batch(Y, psi, seed=5)
    st = lat.stats
    first = lat.bundle_many(P, as_arrays=True)
    n0 = st["query_basis_solves"]
    assert n0 == 1
    lat.bundle_many(P, as_arrays=True)
    lat.set_query(P[1])
    lat.bundle_many(P, as_arrays=True)
    assert st["query_basis_solves"] == n0
    # a larger |psi|_inf extends x only: X bit-identical, one more solve
    X0, _ = lat.query_basis()
    it_X = lat.last_query_basis["iters"]["X"]
    lat.bundle_many(10.0 * P, as_arrays=True)
    assert st["query_basis_solves"] == n0 + 1
    assert lat.last_query_basis["x_only"] and lat.last_query_basis["iters"]["X"] == it_X
    assert np.array_equal(lat.query_basis()[0], X0)
    assert lat.last_query_basis["psi_inf"] == pytest.approx(float(np.max(np.abs(10.0 * P))))

    def changed(fn):
        n = st["query_basis_solves"]
        fn()
        out = lat.bundle_many(P, as_arrays=True)
        assert st["query_basis_solves"] == n + 1, fn
        lat.bundle_many(P, as_arrays=True)
        assert st["query_basis_solves"] == n + 1, fn
        return out

    g = np.random.default_rng(6).uniform(0.2, 1.0, lat.N).astype(np.float32)
    after_gates = changed(lambda: lat.set_gates(g))
    assert not np.array_equal(after_gates[1], first[1])
    changed(lambda: lat.clear_chain())
    changed(lambda: lat.add_chain(rc["chain"], lamP=rc["lamP"]))
    changed(lambda: setattr(lat, "lamC", 0.8))
    changed(lambda: lat.rebuild_graph(kneighbors=rc["k"] + 1))
    A = lat.A
    changed(lambda: setattr(lat, "A", A))
    # answers follow the change: the per-query path on the final state agrees
    ids = lat.bundle_many(P[:2], k=6, as_arrays=True)[0]
    M, Ad, sd = _yardstick(lat)
    for q in range(2):
        U = yq.ustar(M, Y, lat.B_diag, P[q], lat.lamG, lat.lamQ)
        w_ids, _, _, margins = yq.bundle(Y, U, P[q], Ad, sd, lat.lamC, k=6)
        assert yq.same_until_near_tie(ids[q].tolist(), w_ids, margins, NEAR_TIE)[0]


def _route_lattice(amd, N, D, clustered=False, seed=7):
    rng = np.random.default_rng(seed)
    if clustered:
        centers = rng.standard_normal((N // 100, D)).astype(np.float32)
        Y = centers[np.arange(N) % centers.shape[0]] + 0.15 * rng.standard_normal((N, D)).astype(np.float32)
        Y = Y[rng.permutation(N)]
    else:
        Y = rng.standard_normal((N, D)).astype(np.float32)
    return amd.Oscillink(Y.astype(np.float32), kneighbors=8, deterministic_k=True), Y


@pytest.mark.parametrize("route", ["small", "mid", "blocked", "clustered"])
def test_routes_against_per_query_path(amd, route, monkeypatch):
    N, D, clustered = {"small": (300, 32, False), "mid": (4000, 64, False), "blocked": (20000, 64, False),
                       "clustered": (12000, 64, True)}[route]
    if clustered:
        monkeypatch.setenv("OSC_REORDER", "1")
    lat, Y = _route_lattice(amd, N, D, clustered)
    if clustered:
        assert lat.build_info()["reordered"]
    rng = np.random.default_rng(8)
    P = np.stack([Y[:32].mean(axis=0), rng.standard_normal(D), Y[17], rng.uniform(-1, 1, D)]).astype(np.float32)
    ids, score, align = lat.bundle_many(P, k=8, as_arrays=True)
    assert lat.last_query_basis["converged"]
    rowptr, col, a, _, sd = lat.graph_csr()
    for q in range(P.shape[0]):
        lat.set_query(P[q])
        bd = lat.bundle(k=8, alpha=0.5)
        want = [b["id"] for b in bd]
        # near ties from this library's own per-query U* (float64 MMR over its scores)
        _, _, _, margins = yq.bundle(Y, lat.solve_Ustar(), P[q], (rowptr, col, a), sd, lat.lamC, k=8)
        ok, cut = yq.same_until_near_tie(ids[q].tolist(), want, margins, NEAR_TIE)
        assert ok, (route, q, ids[q].tolist(), want, margins)
        n = len(want) if not cut else next(t for t, m in enumerate(margins) if m < NEAR_TIE)
        assert np.allclose(score[q, :n], [b["score"] for b in bd][:n], atol=2e-4), (route, q)
        assert np.allclose(align[q, :n], [b["align"] for b in bd][:n], atol=2e-4), (route, q)


def test_mmr_many_matches_mmr(amd):
    rng = np.random.default_rng(9)
    Y = rng.standard_normal((500, 48)).astype(np.float32)
    lat = amd.Oscillink(Y, kneighbors=6, deterministic_k=True)
    S = rng.standard_normal((500, 12)).astype(np.float32)
    S[:, 3] = 0.25  # every score tied
    S[:40, 4] = S[40:80, 4]  # pairs of exact ties
    S[:, 5] = np.round(S[:, 5], 1)
    got = lat._mmr_many(S, 10, 0.5)
    assert got.shape == (12, 10)
    for q in range(S.shape[1]):
        want = lat._mmr(S[:, q], 10, 0.5)
        _, margins = yq.mmr(Y, S[:, q], 10, 0.5)
        ok, _ = yq.same_until_near_tie(got[q].tolist(), want, margins, 1e-6)
        assert ok, (q, got[q].tolist(), want)
    assert got[3].tolist() == lat._mmr(S[:, 3], 10, 0.5)[:10]


def test_errors_and_edges(amd):
    lat, case, Y, psi = _fixture_lattice(amd, "c1_n80_d128_k8")
    D = Y.shape[1]
    with pytest.raises(ValueError):
        lat.bundle_many(np.zeros((3, D + 1), np.float32))
    with pytest.raises(ValueError):
        lat.bundle_many(np.zeros(D, np.float32))
    bad = np.zeros((4, D), np.float32)
    bad[2, 7] = np.nan
    with pytest.raises(ValueError, match="row 2"):
        lat.bundle_many(bad)
    assert lat.bundle_many(np.zeros((0, D), np.float32)) == []
    assert lat.bundle_many(np.ones((2, D), np.float32), k=0) == [[], []]
    big = lat.bundle_many(np.ones((2, D), np.float32), k=lat.N + 5, as_arrays=True)[0]
    assert big.shape == (2, lat.N) and sorted(big[0].tolist()) == list(range(lat.N))

    from oscillink_amd.sharding import run_loopback_ranks

    def rank(r, comm):
        l2 = amd.Oscillink(Y, kneighbors=8, deterministic_k=True, comm=comm)
        try:
            l2.bundle_many(np.ones((1, D), np.float32))
        except NotImplementedError:
            return "refused"
        return "ran"

    assert run_loopback_ranks(2, rank) == ["refused", "refused"]

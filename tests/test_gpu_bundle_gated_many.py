"""bundle_gated_many: Q gated U* solves as one panel CG, then the batched bundle.  Against
the float64 yardstick (tests/_queries.py with B = the query's gates) on the lattice's own graph, the oracle's iteration
counts, this library's per-query loop and itself (batch composition, chunking, the diffusion route).  The inputs'
own conditions (near-tie cap, distance of the oracle's residuals from tol) are checked on the CPU in
tests/test_bundle_gated_host.py."""
import numpy as np
import pytest

from tests import _bundle_gated as bg
from tests import _queries as yq

pytestmark = pytest.mark.gpu

NEAR_TIE = bg.NEAR_TIE


@pytest.fixture(scope="module")
def amd():
    import oscillink_amd
    from oscillink_amd import _native

    assert _native.device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return oscillink_amd


def _lattice(amd, name):
    Y = bg.anchors(name)
    return amd.Oscillink(Y, kneighbors=bg.CASES[name][2], deterministic_k=True), Y


def _inputs(lat, name, Y):
    """the five queries and their gates; the fifth row is that query's diffusion gates"""
    P = bg.queries(name, Y)
    G = bg.given_gates(name, lat.N)
    G[4] = lat.diffusion_gates_many(P[4:5], beta=bg.GATE_BETA, gamma=bg.GATE_GAMMA)["gates"][0]
    return P, G


_seam = {}


def _seam_case(amd):
    """case 1's lattice, inputs and batched answers, computed once for the tests that share them"""
    if not _seam:
        name = "seam_n97_d40"
        lat, Y = _lattice(amd, name)
        P, G = _inputs(lat, name, Y)
        out = lat.bundle_gated_many(P, k=bg.CASES[name][3], gates=G, as_arrays=True)
        rep = {k: (None if v is None else v.copy()) for k, v in lat.last_bundle_gated.items()}
        _seam.update(name=name, lat=lat, Y=Y, P=P, G=G, out=out, rep=rep)
    return _seam


def _lams(lat):
    return (lat.lamG, lat.lamC, lat.lamQ)


def _against_yardstick(lat, Y, P, G, k, out, U32, tol=bg.TOL):
    """per query: ids by the near-tie rule, score / align up to the cut within 2e-4, U within 1e-4 relative (max-norm),
    the implied residual within 2 tol; returns how many id lists were cut before their last pick"""
    ids, score, align = out
    A, sd = bg.dense_graph(lat.graph_csr(), lat.N)
    cut_early = 0
    for q in range(P.shape[0]):
        M, U, w_ids, w_score, w_align, margins = bg.yardstick(Y, A, sd, P[q], G[q], _lams(lat), k)
        ok, cut = yq.same_until_near_tie(ids[q].tolist(), w_ids, margins, NEAR_TIE)
        n = bg.first_near_tie(margins) if cut else len(w_ids)
        d_score = float(np.max(np.abs(score[q, :n] - w_score[:n]), initial=0.0))
        d_align = float(np.max(np.abs(align[q, :n] - w_align[:n]), initial=0.0))
        rel_U = float(np.max(np.abs(U32[q].astype(np.float64) - U)) / np.max(np.abs(U)))
        rhs = lat.lamG * Y.astype(np.float64) + lat.lamQ * G[q].astype(np.float64)[:, None] * P[q].astype(np.float64)[None, :]
        implied = float(np.max(np.linalg.norm(rhs - M @ U32[q].astype(np.float64), axis=0)))
        print(f"q{q}: compared {n} picks, |score| {d_score:.2e}, |align| {d_align:.2e}, U rel {rel_U:.2e}, "
              f"implied residual {implied:.2e}")
        assert ok, (q, ids[q].tolist(), w_ids, margins)
        assert d_score <= 2e-4 and d_align <= 2e-4, q
        assert rel_U <= 1e-4, q
        assert implied <= 2 * tol, q
        cut_early += int(bg.cut_before_last(margins))
    return cut_early


# cases 1-4: the row-part seam with a ragged slab, the other slab widths, tiny lattices, a reordered lattice
@pytest.mark.parametrize("name", list(bg.CASES))
def test_cases_against_yardstick(amd, name, monkeypatch):
    N, D, _, k, _, clustered = bg.CASES[name]
    if name == "seam_n97_d40":
        c = _seam_case(amd)
        lat, Y, P, G, out, rep = c["lat"], c["Y"], c["P"], c["G"], c["out"], c["rep"]
    else:
        if clustered:
            monkeypatch.setenv("OSC_REORDER", "1")
        lat, Y = _lattice(amd, name)
        if clustered:
            assert lat.build_info()["reordered"]
        P, G = _inputs(lat, name, Y)
        out = lat.bundle_gated_many(P, k=k, gates=G, as_arrays=True)  # gates in API row order
        rep = dict(lat.last_bundle_gated)
    assert out[0].shape == (5, min(k, N)) and rep["gates"] is None
    assert rep["converged"].all() and rep["iters"].max() <= bg.LOOP_ITERS
    U32, it_u, res_u = lat._ustar_gated_many(P, G, bg.TOL, 256)
    assert U32.shape == (5, N, D) and U32.dtype == np.float32
    assert np.array_equal(it_u, rep["iters"]) and np.array_equal(res_u, rep["res"])
    cut = _against_yardstick(lat, Y, P, G, k, out, U32)
    print(f"{name}: {cut} of 5 id lists compared up to a near tie before their last pick")
    assert cut <= 1


# case 5
def test_diffusion_route_equals_given_diffusion_gates(amd):
    c = _seam_case(amd)
    lat, P = c["lat"], c["P"]
    kw = dict(beta=1.2, gamma=0.15, method="cg", tol=1e-5, max_iters=300)
    Gd = lat.diffusion_gates_many(P, **kw)["gates"]
    given = lat.bundle_gated_many(P, k=6, gates=Gd, as_arrays=True)
    rep_given = dict(lat.last_bundle_gated)
    events = []
    lat.set_logger(lambda ev, payload: events.append(ev))
    routed = lat.bundle_gated_many(P, "diffusion", k=6, as_arrays=True, gate_beta=1.2, gate_gamma=0.15, gate_method="cg",
                                   gate_tol=1e-5, gate_max_iters=300)
    lat.set_logger(None)
    assert events.count("bundle_gated_many") == 1
    for a, b in zip(given, routed):
        assert np.array_equal(a, b)
    assert np.array_equal(lat.last_bundle_gated["gates"], Gd) and lat.last_bundle_gated["gates"].dtype == np.float32
    assert rep_given["gates"] is None
    for key in ("iters", "res", "converged"):
        assert np.array_equal(lat.last_bundle_gated[key], rep_given[key]), key
    # the list form carries the same numbers
    dicts = lat.bundle_gated_many(P, k=6, gates=Gd)
    assert [[b["id"] for b in d] for d in dicts] == given[0].tolist()


# case 6
def test_loop_parity_and_state(amd):
    c = _seam_case(amd)
    name, Y, P, G, (ids, _, _) = c["name"], c["Y"], c["P"], c["G"], c["out"]
    lat, _ = _lattice(amd, name)
    g0 = np.random.default_rng(3).uniform(0.2, 1.0, lat.N).astype(np.float32)
    lat.set_query(P[0], gates=g0)
    lat.settle(max_iters=12, tol=1e-3)
    lat.bundle_many(P[:2], k=6)  # a resident query basis and its record
    rec0 = lat.receipt()
    U_star = lat.solve_Ustar().copy()
    st0, lu0, qb0 = dict(lat.stats), dict(lat.last_ustar), dict(lat.last_query_basis)
    psi0, U0, B0 = lat.psi.copy(), lat.U.copy(), lat.B_diag.copy()
    got = lat.bundle_gated_many(P, k=6, gates=G, as_arrays=True)
    for a, b in zip(got, c["out"]):  # the lattice's own gates are not read
        assert np.array_equal(a, b)
    assert dict(lat.stats) == st0 and lat.last_ustar == lu0 and lat.last_query_basis == qb0
    assert np.array_equal(lat.psi, psi0) and np.array_equal(lat.U, U0) and np.array_equal(lat.B_diag, B0)
    assert np.array_equal(lat.solve_Ustar(), U_star)
    rec1 = lat.receipt()
    for key in ("deltaH_total", "coh_drop_sum", "anchor_pen_sum", "query_term_sum", "null_points"):
        assert rec1[key] == rec0[key], key
    assert rec1["meta"]["state_sig"] == rec0["meta"]["state_sig"]
    loop, _ = _lattice(amd, name)
    A, sd = bg.dense_graph(loop.graph_csr(), loop.N)
    for q in range(5):
        loop.set_query(P[q], gates=G[q])
        want = [b["id"] for b in loop.bundle(k=6, alpha=0.5)]
        margins = bg.yardstick(Y, A, sd, P[q], G[q], _lams(loop), 6)[5]
        assert yq.same_until_near_tie(ids[q].tolist(), want, margins, NEAR_TIE)[0], (q, ids[q].tolist(), want, margins)


# case 7
def test_iteration_counts_match_the_oracle(amd):
    from oracle import oscillink_oracle as orc

    c = _seam_case(amd)
    lat, Y, P, G = c["lat"], c["Y"], c["P"], c["G"]
    ref = orc.OracleLattice(Y, kneighbors=bg.CASES[c["name"]][2], deterministic_k=True, graph=lat.A)
    lat.bundle_gated_many(P, k=6, gates=G, tol=bg.TOL, max_iters=bg.LOOP_ITERS)
    full = {k: v.copy() for k, v in lat.last_bundle_gated.items() if v is not None}
    lat.bundle_gated_many(P, k=6, gates=G, tol=bg.TOL, max_iters=3)  # no exception
    short = lat.last_bundle_gated
    for q in range(5):
        ref.set_query(P[q], gates=G[q])
        ref.solve_Ustar(tol=bg.TOL, max_iters=bg.LOOP_ITERS)
        hist = list(ref.history)
        print(f"q{q}: iters {int(full['iters'][q])} (oracle {ref.last_ustar['iters']}), res {float(full['res'][q]):.3e} "
              f"(oracle {hist[-1]:.3e}); after 3: {float(short['res'][q]):.3e} (oracle {hist[2]:.3e})")
        assert int(full["iters"][q]) == ref.last_ustar["iters"], q
        assert bool(full["converged"][q]) and float(full["res"][q]) <= bg.TOL
        assert int(short["iters"][q]) == 3 and not bool(short["converged"][q]), q
        assert np.isclose(float(short["res"][q]), hist[2], rtol=2e-2, atol=0), q
    assert np.array_equal(full["iters"], c["rep"]["iters"])  # the default max_iters = 256 changes nothing for these


# case 8
def test_batch_independence_and_chunking(amd, monkeypatch):
    c = _seam_case(amd)
    lat, P, G, whole, rep = c["lat"], c["P"], c["G"], c["out"], c["rep"]

    def run(sel):
        out = lat.bundle_gated_many(P[sel], k=6, gates=G[sel], as_arrays=True)
        return out + (lat.last_bundle_gated["iters"].copy(), lat.last_bundle_gated["res"].copy())

    want = whole + (rep["iters"], rep["res"])
    monkeypatch.setenv("OSC_GATED_CHUNK", "2")  # chunks of 2, 2, 1
    for a, b in zip(run(np.arange(5)), want):
        assert np.array_equal(a, b)
    monkeypatch.delenv("OSC_GATED_CHUNK")
    for q in range(5):
        for a, b in zip(run(np.array([q])), want):
            assert np.array_equal(a[0], b[q]), q
    order = np.array([3, 0, 4, 2, 1])
    for a, b in zip(run(order), want):
        assert np.array_equal(a, b[order])


def test_non_finite_rows_stay_in_their_query(amd):
    c = _seam_case(amd)
    lat, P, G, whole = c["lat"], c["P"], c["G"], c["out"]
    others = [0, 1, 3, 4]
    Pn = P.copy()
    Pn[2, 7] = np.nan
    out = lat.bundle_gated_many(Pn, k=6, gates=G, as_arrays=True)
    for a, b in zip(out, whole):
        assert np.array_equal(a[others], b[others])
    assert not np.isfinite(out[1][2]).any() and not bool(lat.last_bundle_gated["converged"][2])
    # NaN gates cannot be passed to bundle_gated_many (ValueError); the solve itself keeps them inside their query
    U, it, res = lat._ustar_gated_many(P, G, bg.TOL, 64)
    Gn = G.copy()
    Gn[1, 3] = np.nan
    Un, itn, resn = lat._ustar_gated_many(P, Gn, bg.TOL, 64)
    keep = [0, 2, 3, 4]
    assert np.array_equal(Un[keep], U[keep]) and np.array_equal(itn[keep], it[keep]) and np.array_equal(resn[keep], res[keep])
    assert not np.isfinite(Un[1]).all() and itn[1] == 64
    # non-finite diffusion gates (from a non-finite query): the warning of diffusion_gates_many, the other queries untouched
    clean = lat.bundle_gated_many(P, k=6, gates="diffusion", as_arrays=True)
    with pytest.warns(RuntimeWarning, match="query 2"):
        dirty = lat.bundle_gated_many(Pn, k=6, gates="diffusion", as_arrays=True)
    for a, b in zip(dirty, clean):
        assert np.array_equal(a[others], b[others])
    assert not np.isfinite(lat.last_bundle_gated["gates"][2]).all()


# case 9
def test_all_ones_gates_against_the_ungated_call(amd):
    c = _seam_case(amd)
    lat, Y, P = c["lat"], c["Y"], c["P"]
    assert np.array_equal(lat.B_diag, np.ones(lat.N, np.float32))
    ones = np.ones((5, lat.N), np.float32)
    gated = lat.bundle_gated_many(P, k=6, gates=ones, as_arrays=True)
    plain = lat.bundle_many(P, k=6, as_arrays=True)
    A, sd = bg.dense_graph(lat.graph_csr(), lat.N)
    for q in range(5):
        margins = bg.yardstick(Y, A, sd, P[q], ones[q], _lams(lat), 6)[5]
        ok, cut = yq.same_until_near_tie(gated[0][q].tolist(), plain[0][q].tolist(), margins, NEAR_TIE)
        assert ok, (q, gated[0][q].tolist(), plain[0][q].tolist(), margins)
        n = bg.first_near_tie(margins) if cut else 6
        assert np.allclose(gated[1][q, :n], plain[1][q, :n], atol=2e-4, rtol=0), q
        assert np.allclose(gated[2][q, :n], plain[2][q, :n], atol=2e-4, rtol=0), q


# case 10
def test_errors_and_edges(amd):
    c = _seam_case(amd)
    lat, Y, P, G = c["lat"], c["Y"], c["P"], c["G"]
    N, D = Y.shape
    assert lat.bundle_gated_many(np.zeros((0, D), np.float32), gates=np.zeros((0, N), np.float32)) == []
    assert lat.bundle_gated_many(np.zeros((0, D), np.float32), gates="diffusion") == []
    assert lat.bundle_gated_many(P[:2], k=0, gates=G[:2]) == [[], []]
    assert lat.last_bundle_gated["iters"].shape == (2,) and lat.last_bundle_gated["converged"].all()
    big = lat.bundle_gated_many(P[:2], k=N + 5, gates=G[:2], as_arrays=True)[0]
    assert big.shape == (2, N) and sorted(big[0].tolist()) == list(range(N))
    bad = G.copy()
    bad[3, 5] = np.inf
    with pytest.raises(ValueError, match="query 3"):
        lat.bundle_gated_many(P, gates=bad)
    bad = G.copy()
    bad[1, 0] = -0.5
    bad[4, 0] = np.nan
    with pytest.raises(ValueError, match="query 1"):
        lat.bundle_gated_many(P, gates=bad)
    with pytest.raises(ValueError, match="set_gates"):
        lat.bundle_gated_many(P, gates=G[0])
    with pytest.raises(ValueError):
        lat.bundle_gated_many(P, gates=G[:4])
    with pytest.raises(ValueError):
        lat.bundle_gated_many(P, gates=G[:, :-1])
    with pytest.raises(ValueError):
        lat.bundle_gated_many(P, gates="diffuse")
    with pytest.raises(ValueError):
        lat.bundle_gated_many(P, gates="diffusion", gate_gamma=0.0)
    # per-query gates and chain priors do not combine: no call takes both
    with pytest.raises(TypeError):
        lat.bundle_gated_many(P, gates=G, chains=[0, 1, 2], lamP=0.2)
    with pytest.raises(TypeError):
        lat.bundle_many(P, gates=G)
    chained, _ = _lattice(amd, c["name"])
    chained.add_chain([0, 1, 2], lamP=0.2)
    with pytest.raises(NotImplementedError):
        chained.bundle_gated_many(P, gates=G)

    from oscillink_amd.sharding import run_loopback_ranks

    def rank(r, comm):
        l2 = amd.Oscillink(Y, kneighbors=6, deterministic_k=True, comm=comm)
        try:
            l2.bundle_gated_many(P, gates=G)
        except NotImplementedError:
            return "refused"
        return "ran"

    assert run_loopback_ranks(2, rank) == ["refused", "refused"]

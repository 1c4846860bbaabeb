"""receipt_gated_many: per-query gated receipts, settle and bundle in one call.  Against the
float64 yardstick (tests/_receipt_yardstick.py under M_q, tests/_receipt_gated.py's float64 settle) on the lattice's own
graph, this library's per-query loop, bundle_gated_many and itself (batch composition, chunking, the diffusion route).
The inputs' own conditions (null-point margins, distance of the settle's residuals from tol) are checked on the CPU in
tests/test_receipt_gated_host.py."""
import numpy as np
import pytest

from tests import _bundle_gated as bg
from tests import _receipt_gated as rg

pytestmark = pytest.mark.gpu

SUMS = ("coh_drop_sum", "anchor_pen_sum", "query_term_sum")
ARRAY_SCALARS = ("deltaH", "coh_drop_sum", "anchor_pen_sum", "query_term_sum", "null_total", "ustar_iters", "ustar_res")
ARRAY_NULLS = ("null_i", "null_j", "null_z", "null_r")


@pytest.fixture(scope="module")
def amd():
    import oscillink_amd
    from oscillink_amd import _native

    assert _native.device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return oscillink_amd


@pytest.fixture(autouse=True)
def _plain_env(monkeypatch):
    for key in ("OSCILLINK_RECEIPT_NULL_CAP", "OSCILLINK_RECEIPT_DYNAMICS", "OSC_GATED_CHUNK"):
        monkeypatch.delenv(key, raising=False)


_cases = {}


def _case(amd, name, monkeypatch):
    """the case's anchors, queries, gates (the fifth row: that query's diffusion gates), dense graph and float64 yardstick
    receipts from U = Y, computed once; lattices are built per test"""
    if name not in _cases:
        lat, Y = _lattice(amd, name, monkeypatch)
        P = rg.queries(name, Y)
        G = rg.given_gates(name, lat.N)
        G[4] = lat.diffusion_gates_many(P[4:5], beta=bg.GATE_BETA, gamma=bg.GATE_GAMMA)["gates"][0]
        A, sd = rg.dense_graph(lat.graph_csr(), lat.N)
        want = [rg.yardstick(Y, Y, P[q], G[q], A, sd, _lams(lat)) for q in range(5)]
        _cases[name] = dict(Y=Y, P=P, G=G, A=A, sd=sd, want=want)
    return _cases[name]


def _lattice(amd, name, monkeypatch):
    clustered = rg.CASES[name][5]
    if clustered:
        monkeypatch.setenv("OSC_REORDER", "1")
    Y = rg.anchors(name)
    lat = amd.Oscillink(Y, kneighbors=rg.CASES[name][2], deterministic_k=True)
    if clustered:
        assert lat.build_info()["reordered"]
    return lat, Y


def _lams(lat):
    return (lat.lamG, lat.lamC, lat.lamQ)


def _deltaH64(c, q, U, lams):
    """tr((U - U*)^T M_q (U - U*)) in float64 from the case's yardstick U*"""
    E = np.asarray(U, np.float64) - c["want"][q]["Ustar"]
    return float(np.sum(E * (rg.gated_M(c["A"], c["sd"], c["G"][q], lams) @ E)))


def _check_energies(rec, want, dH, who):
    print(f"{who}: deltaH {rec['deltaH_total']:.6g} (yardstick {dH:.6g}), " +
          ", ".join(f"{k} {rec[k]:.6g} ({want[k]:.6g})" for k in SUMS))
    assert rg.close(rec["deltaH_total"], dH), (who, rec["deltaH_total"], dH)
    for key in SUMS:
        assert rg.close(rec[key], want[key]), (who, key, rec[key], want[key])


# 1: settle=None, full detail, every case, U at Y and after one settle()
@pytest.mark.parametrize("state", ["fresh", "settled"])
@pytest.mark.parametrize("name", list(rg.CASES))
def test_cases_against_yardstick(amd, name, state, monkeypatch):
    c = _case(amd, name, monkeypatch)
    lat, Y = _lattice(amd, name, monkeypatch)
    if state == "settled":
        lat.settle()
    got = lat.receipt_gated_many(c["P"], c["G"])
    assert len(got) == 5 and lat.last_receipt_gated["converged"].all() and lat.last_receipt_gated["settle_iters"] is None
    U = lat.U
    for q in range(5):
        want = c["want"][q]
        _check_energies(got[q], want, _deltaH64(c, q, U, _lams(lat)), f"{name} {state} q{q}")
        share = rg.check_nulls(got[q]["null_points"], want["null_points"], want["margin"], c["A"])
        print(f"{name} {state} q{q}: {len(got[q]['null_points'])} null points, left out {share:.4f}")
        assert share <= rg.LEFT_OUT_CAP, (q, share)
        assert got[q]["cg_iters"] == int(lat.last.get("iters") or 0)
        m = got[q]["meta"]
        assert m["ustar_source"] == "gated_panel" and m["ustar_cached"] is False and m["ustar_converged"] is True
        assert m["ustar_iters"] == int(lat.last_receipt_gated["iters"][q])
        assert m["gates_min"] == float(np.min(c["G"][q])) and m["gates_mean"] == float(np.mean(c["G"][q]))


# 2: with settle, against the float64 settle followed by the yardstick receipt
@pytest.mark.parametrize("name,settle", [(rg.SETTLE_CASE, True), (rg.SETTLE_CASE, rg.SETTLE_CAPPED),
                                         (rg.LOOP_CASES[1], True)], ids=["default", "capped", "reordered"])
def test_settle_against_yardstick(amd, name, settle, monkeypatch):
    c = _case(amd, name, monkeypatch)
    lat, Y = _lattice(amd, name, monkeypatch)
    st = rg.SETTLE_DEFAULT if settle is True else settle
    got = lat.receipt_gated_many(c["P"], c["G"], settle=settle)
    rep = lat.last_receipt_gated
    for q in range(5):
        M = rg.gated_M(c["A"], c["sd"], c["G"][q], _lams(lat))
        Uq, iters, res, hist = rg.settle64(M, Y, Y, c["P"][q], c["G"][q], _lams(lat), **st)
        print(f"{name} q{q}: cg_iters {got[q]['cg_iters']} (float64 {iters}), residual {got[q]['residual']:.3e} ({res:.3e})")
        assert got[q]["cg_iters"] == iters == int(rep["settle_iters"][q]), q
        assert abs(got[q]["residual"] - res) <= 2 * st["tol"], q
        assert got[q]["residual"] == float(rep["settle_res"][q])
        assert (got[q]["residual"] <= st["tol"]) == (res <= st["tol"])
        _check_energies(got[q], c["want"][q], _deltaH64(c, q, Uq, _lams(lat)), f"{name} q{q}")
        assert got[q]["t_ms"] > 0 and got[q]["meta"]["last_settle_ms"] == got[q]["t_ms"]
    assert np.array_equal(lat.U, Y)  # no settled state is written back


# 3: every record equals set_query(gates); [settle();] receipt() on a second lattice; the first lattice's state is untouched
@pytest.mark.parametrize("mode", [None, "minimal", "extended"])
@pytest.mark.parametrize("detail", ["light", "full"])
@pytest.mark.parametrize("name", list(rg.LOOP_CASES))
def test_loop_parity_and_state(amd, name, detail, mode, monkeypatch):
    from oscillink_amd.receipts import verify_receipt

    c = _case(amd, name, monkeypatch)
    P, G = c["P"], c["G"]
    lat, Y = _lattice(amd, name, monkeypatch)
    loop, _ = _lattice(amd, name, monkeypatch)
    for l in (lat, loop):
        l.set_receipt_detail(detail)
        if mode:
            l.set_receipt_secret("s3cret")
            l.set_signature_mode(mode)
    # a lattice with a query, gates, a U* cache, a query basis and receipts of its own, its state back at U = Y
    g0 = np.random.default_rng(3).uniform(0.2, 1.0, lat.N).astype(np.float32)
    lat.set_query(P[0], gates=g0)
    lat.bundle_many(P[:2], k=2)
    rec0 = lat.receipt()
    U_star = lat.solve_Ustar().copy()
    st0, last0, lu0, qb0 = dict(lat.stats), dict(lat.last), dict(lat.last_ustar), dict(lat.last_query_basis)
    psi0, U0, B0 = lat.psi.copy(), lat.U.copy(), lat.B_diag.copy()
    for settle in (None, True):
        got = lat.receipt_gated_many(P, G, settle=settle)
        for q in range(5):
            loop.reset_U()
            loop.set_query(P[q], gates=G[q])
            if settle:
                loop.settle()
            want = loop.receipt()
            g = got[q]
            assert set(g) == set(want) and list(g) == list(want)
            assert set(g["meta"]) == set(want["meta"]) | {"ustar_source"}
            assert g["version"] == want["version"] and g["cg_iters"] == want["cg_iters"], (q, g["cg_iters"], want["cg_iters"])
            assert abs(g["residual"] - want["residual"]) <= 2e-3
            for key in ("deltaH_total",) + SUMS:
                assert rg.close(g[key], want[key]), (q, key, g[key], want[key])
            for key in ("state_sig", "receipt_detail", "gates_min", "gates_max", "gates_mean", "gates_uniform", "avg_degree",
                        "edge_density", "ustar_converged"):
                assert g["meta"][key] == want["meta"][key], (q, key)
            margin = c["want"][q]["margin"]
            bad = [i for i in rg.differing_rows(g["null_points"], want["null_points"]) if margin[i] >= rg.MARGIN]
            assert not bad, (q, bad[:5])
            if detail == "light":
                assert g["null_points"] == [] and all(g[k] == 0.0 for k in SUMS)
            if mode:
                assert verify_receipt(g, "s3cret") and not verify_receipt(g, "other")
                pay = g["meta"]["signature"]["payload"]
                assert pay["mode"] == mode and pay["state_sig"] == want["meta"]["state_sig"]
                assert pay["deltaH_total"] == g["deltaH_total"]
            else:
                assert "signature" not in g["meta"]
        assert dict(lat.stats) == st0 and lat.last == last0 and lat.last_ustar == lu0 and lat.last_query_basis == qb0
        lat._U_host = None  # (read the device's U again)
        assert np.array_equal(lat.psi, psi0) and np.array_equal(lat.U, U0) and np.array_equal(lat.B_diag, B0)
    assert np.array_equal(lat.solve_Ustar(), U_star)
    rec1 = lat.receipt()
    for key in ("deltaH_total", "null_points") + SUMS:
        assert rec1[key] == rec0[key], key
    assert rec1["meta"]["state_sig"] == rec0["meta"]["state_sig"]


def _arrays(lat, P, G, **kw):
    out = lat.receipt_gated_many(P, G, as_arrays=True, **kw)
    return {k: np.array(v, copy=True) for k, v in out.items()}


def _query_of(arrs, t):
    """query t's entries of an as_arrays dict, bytes included"""
    s, e = int(arrs["null_offsets"][t]), int(arrs["null_offsets"][t + 1])
    out = {k: arrs[k][t].tobytes() for k in arrs if k not in ARRAY_NULLS and k != "null_offsets"}
    out.update({k: arrs[k][s:e].tobytes() for k in ARRAY_NULLS})
    return out


# 4: the bundle of the same solve is bundle_gated_many's; the receipts do not depend on it
def test_bundle_k_equals_bundle_gated_many(amd, monkeypatch):
    c = _case(amd, rg.SETTLE_CASE, monkeypatch)
    P, G = c["P"], c["G"]
    lat, _ = _lattice(amd, rg.SETTLE_CASE, monkeypatch)
    k = rg.CASES[rg.SETTLE_CASE][3]
    ids, score, align = lat.bundle_gated_many(P, G, k=k, alpha=0.4, as_arrays=True)
    rep = {key: lat.last_bundle_gated[key].copy() for key in ("iters", "res")}
    for settle in (None, True):
        with_b = _arrays(lat, P, G, settle=settle, bundle_k=k, alpha=0.4)
        without = _arrays(lat, P, G, settle=settle)
        assert np.array_equal(with_b["ids"], ids) and with_b["ids"].dtype == np.int32
        assert with_b["score"].tobytes() == score.tobytes() and with_b["align"].tobytes() == align.tobytes()
        assert np.array_equal(with_b["ustar_iters"], rep["iters"]) and with_b["ustar_res"].tobytes() == rep["res"].tobytes()
        assert set(with_b) == set(without) | {"ids", "score", "align"}
        for key in without:
            assert with_b[key].tobytes() == without[key].tobytes(), (settle, key)
        assert ("settle_iters" in without) == bool(settle)
    recs, bundles = lat.receipt_gated_many(P, G, bundle_k=k, alpha=0.4)
    assert [[b["id"] for b in d] for d in bundles] == ids.tolist() and len(recs) == 5
    plain = lat.receipt_gated_many(P, G)
    assert [r["deltaH_total"] for r in recs] == [r["deltaH_total"] for r in plain]


# 5: alone / permuted / in chunks of two, with settle and a non-finite query in the batch
@pytest.mark.parametrize("name", list(rg.LOOP_CASES))
def test_batch_independence_and_chunking(amd, name, monkeypatch):
    c = _case(amd, name, monkeypatch)
    P, G = c["P"], c["G"]
    lat, _ = _lattice(amd, name, monkeypatch)
    kw = dict(settle=True, bundle_k=4)
    whole = _arrays(lat, P, G, **kw)
    assert int(whole["null_total"].sum()) > 0
    monkeypatch.setenv("OSC_GATED_CHUNK", "2")  # chunks of 2, 2, 1
    chunked = _arrays(lat, P, G, **kw)
    monkeypatch.delenv("OSC_GATED_CHUNK")
    assert set(chunked) == set(whole)
    for key in whole:
        assert chunked[key].tobytes() == whole[key].tobytes(), key
    for q in range(5):
        assert _query_of(_arrays(lat, P[q:q + 1], G[q:q + 1], **kw), 0) == _query_of(whole, q), q
    order = np.array([3, 0, 4, 2, 1])
    perm = _arrays(lat, P[order], G[order], **kw)
    for t, q in enumerate(order):
        assert _query_of(perm, t) == _query_of(whole, int(q)), q
    # a non-finite query stays inside its own query
    others = [0, 1, 3, 4]
    Pn = P.copy()
    Pn[2, min(7, P.shape[1] - 1)] = np.nan
    dirty = _arrays(lat, Pn, G, **kw)
    for q in others:
        assert _query_of(dirty, q) == _query_of(whole, q), q
    assert not np.isfinite(dirty["deltaH"][2]) and not np.isfinite(dirty["score"][2]).any()
    assert int(dirty["null_total"][2]) == 0 and not bool(lat.last_receipt_gated["converged"][2])
    # non-finite diffusion gates (from the non-finite query): the warning of diffusion_gates_many, the other queries untouched
    clean = _arrays(lat, P, "diffusion", **kw)
    with pytest.warns(RuntimeWarning, match="query 2"):
        dirty = _arrays(lat, Pn, "diffusion", **kw)
    for q in others:
        assert _query_of(dirty, q) == _query_of(clean, q), q
    assert not np.isfinite(dirty["deltaH"][2]) and not np.isfinite(lat.last_receipt_gated["gates"][2]).all()


# 6: the diffusion route is the array route; all-ones gates agree with receipt_many
def test_diffusion_route_and_all_ones_gates(amd, monkeypatch):
    c = _case(amd, rg.SETTLE_CASE, monkeypatch)
    P = c["P"]
    lat, _ = _lattice(amd, rg.SETTLE_CASE, monkeypatch)
    gkw = dict(beta=1.2, gamma=0.15, method="cg", tol=1e-5, max_iters=300)
    Gd = lat.diffusion_gates_many(P, **gkw)["gates"]
    given = _arrays(lat, P, Gd, settle=True, bundle_k=4)
    assert lat.last_receipt_gated["gates"] is None
    events = []
    lat.set_logger(lambda ev, payload: events.append(ev))
    routed = _arrays(lat, P, "diffusion", settle=True, bundle_k=4, gate_beta=1.2, gate_gamma=0.15, gate_method="cg",
                     gate_tol=1e-5, gate_max_iters=300)
    lat.set_logger(None)
    assert events.count("receipt_gated_many") == 1
    assert set(given) == set(routed)
    for key in given:
        assert given[key].tobytes() == routed[key].tobytes(), key
    assert np.array_equal(lat.last_receipt_gated["gates"], Gd)
    recs_given = lat.receipt_gated_many(P, Gd)
    recs_routed = lat.receipt_gated_many(P, "diffusion", gate_beta=1.2, gate_gamma=0.15, gate_method="cg", gate_tol=1e-5,
                                         gate_max_iters=300)
    for a, b in zip(recs_given, recs_routed):
        assert a["meta"]["state_sig"] == b["meta"]["state_sig"] and a["deltaH_total"] == b["deltaH_total"]
    # all-ones gates: a different algorithm (the query basis) on the same operator
    assert np.array_equal(lat.B_diag, np.ones(lat.N, np.float32))
    lat.settle()
    gated = lat.receipt_gated_many(P, np.ones((5, lat.N), np.float32))
    plain = lat.receipt_many(P)
    margins = [rg.yardstick(c["Y"], c["Y"], P[q], np.ones(lat.N, np.float32), c["A"], c["sd"], _lams(lat))["margin"]
               for q in range(5)]
    for q in range(5):
        for key in ("deltaH_total",) + SUMS:
            assert rg.close(gated[q][key], plain[q][key]), (q, key, gated[q][key], plain[q][key])
        assert gated[q]["meta"]["state_sig"] == plain[q]["meta"]["state_sig"]
        assert gated[q]["cg_iters"] == plain[q]["cg_iters"] and gated[q]["residual"] == plain[q]["residual"]
        bad = [i for i in rg.differing_rows(gated[q]["null_points"], plain[q]["null_points"]) if margins[q][i] >= rg.MARGIN]
        assert not bad, (q, bad[:5])


# 7
def test_null_cap(amd, monkeypatch):
    c = _case(amd, rg.SETTLE_CASE, monkeypatch)
    P, G = c["P"], c["G"]
    lat, _ = _lattice(amd, rg.SETTLE_CASE, monkeypatch)
    full = lat.receipt_gated_many(P, G)
    arrays_full = _arrays(lat, P, G)
    monkeypatch.setenv("OSCILLINK_RECEIPT_NULL_CAP", "3")
    capped = lat.receipt_gated_many(P, G)
    arrays = _arrays(lat, P, G)
    assert any(len(f["null_points"]) > 3 for f in full)
    for q in range(5):
        nulls = full[q]["null_points"]
        tot = len(nulls)
        z = np.array([p["z"] for p in nulls], dtype=np.float32)
        keep = [nulls[i] for i in np.argsort(-z, kind="stable")[:3]] if tot > 3 else nulls
        assert capped[q]["null_points"] == keep, q
        assert capped[q]["meta"]["null_points_summary"] == {"total_null_points": tot, "returned_null_points": min(3, tot),
                                                            "null_cap_applied": tot > 3}
        assert int(arrays["null_total"][q]) == tot == int(arrays_full["null_total"][q])
        s, e = int(arrays["null_offsets"][q]), int(arrays["null_offsets"][q + 1])
        assert [[int(i), int(j)] for i, j in zip(arrays["null_i"][s:e], arrays["null_j"][s:e])] == [p["edge"] for p in keep]
        for key, akey in (("deltaH_total", "deltaH"),) + tuple((k, k) for k in SUMS):
            assert float(arrays[akey][q]) == capped[q][key] == full[q][key]


# 8
def test_errors_and_edges(amd, monkeypatch):
    c = _case(amd, rg.SETTLE_CASE, monkeypatch)
    Y, P, G = c["Y"], c["P"], c["G"]
    lat, _ = _lattice(amd, rg.SETTLE_CASE, monkeypatch)
    N, D = Y.shape
    none_p, none_g = np.zeros((0, D), np.float32), np.zeros((0, N), np.float32)
    assert lat.receipt_gated_many(none_p, none_g) == []
    assert lat.receipt_gated_many(none_p, "diffusion", settle=True) == []
    assert lat.receipt_gated_many(none_p, none_g, bundle_k=3) == ([], [])
    empty = lat.receipt_gated_many(none_p, none_g, settle=True, bundle_k=3, as_arrays=True)
    assert empty["deltaH"].shape == (0,) and empty["null_offsets"].tolist() == [0] and empty["ids"].shape == (0, 3)
    assert empty["settle_iters"].shape == (0,)
    recs, bundles = lat.receipt_gated_many(P[:2], G[:2], bundle_k=0)
    assert bundles == [[], []] and len(recs) == 2
    big = lat.receipt_gated_many(P[:2], G[:2], bundle_k=N + 5, as_arrays=True)["ids"]
    assert big.shape == (2, N) and sorted(big[0].tolist()) == list(range(N))
    bad = G.copy()
    bad[3, 5] = np.inf
    with pytest.raises(ValueError, match="query 3"):
        lat.receipt_gated_many(P, bad)
    bad = G.copy()
    bad[1, 0] = -0.5
    with pytest.raises(ValueError, match="query 1"):
        lat.receipt_gated_many(P, bad)
    with pytest.raises(ValueError, match="set_gates"):
        lat.receipt_gated_many(P, G[0])
    for wrong in (G[:4], G[:, :-1], "diffuse"):
        with pytest.raises(ValueError):
            lat.receipt_gated_many(P, wrong)
    with pytest.raises(ValueError):
        lat.receipt_gated_many(P, "diffusion", gate_gamma=0.0)
    with pytest.raises(ValueError, match="unknown keys"):
        lat.receipt_gated_many(P, G, settle={"dt": 1.0, "steps": 3})
    with pytest.raises(ValueError):
        lat.receipt_gated_many(P, G, settle={"dt": -1.0})
    with pytest.raises(ValueError):
        lat.receipt_gated_many(P, G, max_iters=0)
    with pytest.raises(TypeError):
        lat.receipt_gated_many(P, G, chains=[0, 1, 2], lamP=0.2)
    chained, _ = _lattice(amd, rg.SETTLE_CASE, monkeypatch)
    chained.add_chain([0, 1, 2], lamP=0.2)
    with pytest.raises(NotImplementedError):
        chained.receipt_gated_many(P, G)

    from oscillink_amd.sharding import run_loopback_ranks

    def rank(r, comm):
        l2 = amd.Oscillink(Y, kneighbors=6, deterministic_k=True, comm=comm)
        try:
            l2.receipt_gated_many(P, G)
        except NotImplementedError:
            return "refused"
        return "ran"

    assert run_loopback_ranks(2, rank) == ["refused", "refused"]


def test_dynamics_meta_passes_through(amd, monkeypatch):
    monkeypatch.setenv("OSCILLINK_RECEIPT_DYNAMICS", "1")
    c = _case(amd, rg.SETTLE_CASE, monkeypatch)
    lat, _ = _lattice(amd, rg.SETTLE_CASE, monkeypatch)
    lat.settle()
    want = lat.receipt()["meta"]["dynamics"]
    for rec in lat.receipt_gated_many(c["P"], c["G"]):
        assert rec["meta"]["dynamics"] == want

"""Multi-query receipts: `receipt_many` against a float64 yardstick (tests/_receipt_yardstick.py),
this library's own per-query loop (`set_query(psi); receipt()`) and itself (batch composition, chunking, caching)."""

import numpy as np
import pytest

from tests import _queries as yq
from tests import _receipt_yardstick as yr
from tests._cases import PARAM_CASES, ctor_kwargs, load_case, make_inputs, random_gates

pytestmark = pytest.mark.gpu

NEAR = 1e-3
SUMS = ("coh_drop_sum", "anchor_pen_sum", "query_term_sum")
SAME_AS_LOOP = ("version", "cg_iters", "residual", "t_ms")
META_SAME_AS_LOOP = ("graph_build_ms", "last_settle_ms", "avg_degree", "edge_density", "gates_min", "gates_max",
                     "gates_mean", "gates_uniform", "receipt_detail", "state_sig")


@pytest.fixture(scope="module")
def amd():
    import oscillink_amd
    from oscillink_amd import _native

    assert _native.device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return oscillink_amd


@pytest.fixture(autouse=True)
def _plain_env(monkeypatch):
    for k in ("OSCILLINK_RECEIPT_NULL_CAP", "OSCILLINK_RECEIPT_DYNAMICS"):
        monkeypatch.delenv(k, raising=False)


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
    """psi0 first, then random queries, an anchor row and psi = 0 (6 queries)"""
    rng = np.random.default_rng(seed)
    D = Y.shape[1]
    rows = [psi, rng.standard_normal(D), 3.0 * rng.standard_normal(D), Y[5], rng.uniform(-1, 1, D), np.zeros(D)]
    return np.stack(rows).astype(np.float32)


def _yardstick(lat):
    rowptr, col, a, _, sd = lat.graph_csr()
    A = np.zeros((lat.N, lat.N))
    A[np.repeat(np.arange(lat.N), np.diff(rowptr)), col] = a
    Lp = lat.L_path if lat.lamP > 0 else None
    M = yq.dense_M(A, sd, lat.B_diag, lat.lamG, lat.lamC, lat.lamQ, lat.lamP, Lp)
    return M, A, sd


def _set_state(lat, state):
    if state == "settled":
        lat.settle(max_iters=12, tol=1e-3)
    elif state == "stationary":
        lat.U = lat.solve_Ustar()


def _loop(lat, P):
    """the per-query path; psi restored afterwards"""
    psi0 = lat.psi.copy()
    out = []
    for q in range(P.shape[0]):
        lat.set_query(P[q])
        out.append(lat.receipt())
    lat.set_query(psi0)
    return out


def _check_against_loop(got, loop, *, nulls_equal):
    for key in SAME_AS_LOOP:
        assert got[key] == loop[key], key
    for key in META_SAME_AS_LOOP:
        assert got["meta"][key] == loop["meta"][key], key
    assert set(got) == set(loop)
    assert set(got["meta"]) == set(loop["meta"]) | {"ustar_source"}
    assert got["meta"]["ustar_source"] == "query_basis"
    if nulls_equal:
        assert got["meta"]["null_points_summary"] == loop["meta"]["null_points_summary"]


@pytest.mark.parametrize("state", ["fresh", "settled", "stationary"])
@pytest.mark.parametrize("name", ["c1_n80_d128_k8", "g1_n400_d64_k6_chain8", "gates_chain_n333_d50_k7",
                                  "c5mini_n600_d96_k12"] + PARAM_CASES)
def test_fixtures_against_yardstick_and_loop(amd, name, state):
    lat, case, Y, psi = _fixture_lattice(amd, name)
    _set_state(lat, state)
    P = _batch(Y, psi)
    got = lat.receipt_many(P)
    assert len(got) == P.shape[0]
    loop = _loop(lat, P)
    M, A, sd = _yardstick(lat)
    U = lat.U.astype(np.float64)
    for q in range(P.shape[0]):
        want = yr.receipt(Y, U, P[q], A, sd, lat.B_diag, lat.lamG, lat.lamC, lat.lamQ, M)
        g, lp = got[q], loop[q]
        scale = max(abs(want["anchor_pen_sum"]) + abs(want["query_term_sum"]), 1e-12)
        for key in SUMS:
            assert abs(g[key] - want[key]) <= 1e-4 * max(abs(want[key]), 1e-3 * scale), (q, key, g[key], want[key])
        dH, wd, ld = g["deltaH_total"], want["deltaH"], lp["deltaH_total"]
        if state == "stationary":  # deltaH(psi0) ~ 0 (every psi when lamQ = 0): no worse than the loop's own error
            E = Y.astype(np.float64) - want["Ustar"]
            h_fresh = float(np.sum(E * (M @ E)))
            assert abs(dH - wd) <= max(1e-4 * abs(wd), 2 * abs(ld - wd) + 1e-7 * h_fresh), (q, dH, wd, ld)
        else:
            assert abs(dH - wd) <= 1e-4 * abs(wd), (q, dH, wd)
        bad = [i for i in yr.differing_rows(g["null_points"], want["null_points"]) if want["margin"][i] >= NEAR]
        assert not bad, (q, bad[:5])
        same = not yr.differing_rows(g["null_points"], lp["null_points"])
        _check_against_loop(g, lp, nulls_equal=same)
        if lat.lamC == 0:
            assert g["null_points"] == [] and g["meta"]["null_points_summary"]["total_null_points"] == 0
    # light detail: deltaH only, bit for bit the full call's
    lat.set_receipt_detail("light")
    light = lat.receipt_many(P)
    for q in range(P.shape[0]):
        assert light[q]["deltaH_total"] == got[q]["deltaH_total"]
        assert light[q]["null_points"] == [] and all(light[q][k] == 0.0 for k in SUMS)
        assert light[q]["meta"]["receipt_detail"] == "light"
        assert light[q]["meta"]["null_points_summary"] == {"total_null_points": 0, "returned_null_points": 0,
                                                           "null_cap_applied": False}


@pytest.mark.parametrize("mode", ["minimal", "extended"])
def test_signatures(amd, mode):
    from oscillink_amd.receipts import verify_receipt, verify_receipt_mode

    lat, case, Y, psi = _fixture_lattice(amd, "gates_chain_n333_d50_k7")
    lat.set_receipt_secret("s3cret")
    lat.set_signature_mode(mode)
    P = _batch(Y, psi, seed=1)
    got = lat.receipt_many(P)
    loop = _loop(lat, P)
    for g, lp in zip(got, loop):
        assert verify_receipt(g, "s3cret") and not verify_receipt(g, "other")
        ok, payload = verify_receipt_mode(g, "s3cret", require_mode=mode)
        assert ok
        assert payload["state_sig"] == g["meta"]["state_sig"] == lp["meta"]["state_sig"]
        assert payload["deltaH_total"] == g["deltaH_total"]
        if mode == "extended":
            for key in ("ustar_iters", "ustar_res", "ustar_converged"):
                assert payload[key] == g["meta"][key]
            assert payload["params"] == lp["meta"]["signature"]["payload"]["params"]
            assert payload["graph"] == lp["meta"]["signature"]["payload"]["graph"]


def _stable_cap(nulls, cap):
    z = np.array([p["z"] for p in nulls], dtype=np.float32)
    return [nulls[i] for i in np.argsort(-z, kind="stable")[:cap]]


@pytest.mark.parametrize("cap", [1, 5, 40])
def test_null_cap(amd, cap, monkeypatch):
    lat, case, Y, psi = _fixture_lattice(amd, "c5mini_n600_d96_k12")
    P = _batch(Y, psi, seed=2)
    full = lat.receipt_many(P)
    arrays_full = lat.receipt_many(P, as_arrays=True)
    monkeypatch.setenv("OSCILLINK_RECEIPT_NULL_CAP", str(cap))
    capped = lat.receipt_many(P)
    arrays = lat.receipt_many(P, as_arrays=True)
    for q in range(P.shape[0]):
        tot = len(full[q]["null_points"])
        assert capped[q]["null_points"] == (_stable_cap(full[q]["null_points"], cap) if tot > cap else full[q]["null_points"])
        assert capped[q]["meta"]["null_points_summary"] == {"total_null_points": tot,
                                                            "returned_null_points": min(cap, tot),
                                                            "null_cap_applied": tot > cap}
        s, e = int(arrays["null_offsets"][q]), int(arrays["null_offsets"][q + 1])
        assert [[int(i), int(j)] for i, j in zip(arrays["null_i"][s:e], arrays["null_j"][s:e])] == \
            [p["edge"] for p in capped[q]["null_points"]]
        assert arrays["null_z"][s:e].astype(float).tolist() == [p["z"] for p in capped[q]["null_points"]]
        assert arrays["null_r"][s:e].astype(float).tolist() == [p["residual"] for p in capped[q]["null_points"]]
        assert int(arrays["null_total"][q]) == tot == int(arrays_full["null_total"][q])
        for key, akey in (("deltaH_total", "deltaH"), ("coh_drop_sum", "coh_drop_sum"),
                          ("anchor_pen_sum", "anchor_pen_sum"), ("query_term_sum", "query_term_sum")):
            assert float(arrays[akey][q]) == capped[q][key] == full[q][key]
    assert any(len(f["null_points"]) > cap for f in full)


def test_leaves_state_alone(amd):
    lat, case, Y, psi = _fixture_lattice(amd, "gates_chain_n333_d50_k7")
    lat.settle(max_iters=12, tol=1e-3)
    rec0 = lat.receipt()
    U_star = lat.solve_Ustar().copy()
    hist0 = lat.residual_history()
    st0, lu0, last0, psi0, U0 = dict(lat.stats), dict(lat.last_ustar), dict(lat.last), lat.psi.copy(), lat.U.copy()
    P = _batch(Y, psi, seed=3)
    lat.receipt_many(P)
    lat.receipt_many(P, as_arrays=True)
    assert {k: v for k, v in lat.stats.items() if k.startswith("ustar_")} == \
        {k: v for k, v in st0.items() if k.startswith("ustar_")}
    assert lat.stats["query_basis_solves"] == st0["query_basis_solves"] + 1
    assert lat.last_ustar == lu0 and lat.last == last0
    assert lat.residual_history() == hist0
    assert np.array_equal(lat.psi, psi0) and np.array_equal(lat.U, U0)
    assert np.array_equal(lat.solve_Ustar(), U_star)
    rec1 = lat.receipt()
    for key in ("deltaH_total", "coh_drop_sum", "anchor_pen_sum", "query_term_sum", "null_points"):
        assert rec1[key] == rec0[key], key
    assert rec1["meta"]["state_sig"] == rec0["meta"]["state_sig"]


def test_basis_caching_and_meta(amd):
    lat, case, Y, psi = _fixture_lattice(amd, "gates_chain_n333_d50_k7")
    rc = case["recipe"]
    P = _batch(Y, psi, seed=4)
    st = lat.stats
    events = []
    lat.set_logger(lambda ev, payload: events.append(ev))
    lat.bundle_many(P, as_arrays=True)
    assert st["query_basis_solves"] == 1
    got = lat.receipt_many(P)
    assert st["query_basis_solves"] == 1 and events.count("receipt_many") == 1
    qb = lat.last_query_basis
    for q, g in enumerate(got):
        m = g["meta"]
        assert m["ustar_cached"] and m["ustar_solve_ms"] == 0.0
        assert m["ustar_iters"] == qb["iters"]["X"]
        res = qb["res"]["X"] + float(np.max(np.abs(P[q]))) * qb["res"]["x"]
        assert m["ustar_res"] == pytest.approx(res, rel=1e-12) and m["ustar_converged"] == (res <= 1e-4)
        assert m["ustar_solves"] == st["ustar_solves"] and m["ustar_cache_hits"] == st["ustar_cache_hits"]
    # a larger |psi|_inf extends x only
    lat.receipt_many(10.0 * P)
    assert st["query_basis_solves"] == 2 and lat.last_query_basis["x_only"]

    def changed(fn):
        n = st["query_basis_solves"]
        fn()
        out = lat.receipt_many(P)
        assert st["query_basis_solves"] == n + 1, fn
        assert not out[0]["meta"]["ustar_cached"] and out[0]["meta"]["ustar_solve_ms"] > 0.0
        lat.receipt_many(P)
        assert st["query_basis_solves"] == n + 1, fn
        return out

    g = np.random.default_rng(6).uniform(0.2, 1.0, lat.N).astype(np.float32)
    changed(lambda: lat.set_gates(g))
    changed(lambda: lat.clear_chain())
    changed(lambda: lat.add_chain(rc["chain"], lamP=rc["lamP"]))
    changed(lambda: setattr(lat, "lamC", 0.8))
    after = changed(lambda: lat.rebuild_graph(kneighbors=rc["k"] + 1))
    # the answers follow the change
    loop = _loop(lat, P[:3])
    for q in range(3):
        assert after[q]["meta"]["state_sig"] == loop[q]["meta"]["state_sig"]
        assert after[q]["deltaH_total"] == pytest.approx(loop[q]["deltaH_total"], rel=1e-4)
        assert after[q]["anchor_pen_sum"] == pytest.approx(loop[q]["anchor_pen_sum"], rel=1e-4)


def test_batch_independence_and_chunking(amd):
    from oscillink_amd import _native

    lat, case, Y, psi = _fixture_lattice(amd, "c1_n80_d128_k8")
    lat.settle(max_iters=12, tol=1e-3)
    rng = np.random.default_rng(7)
    Q = _native.OSC_QUERY_CHUNK + 44
    P = rng.standard_normal((Q, Y.shape[1])).astype(np.float32)
    big = lat.receipt_many(P, as_arrays=True)

    def one(arrs, t):
        s, e = int(arrs["null_offsets"][t]), int(arrs["null_offsets"][t + 1])
        return ([float(arrs[k][t]) for k in ("deltaH", "coh_drop_sum", "anchor_pen_sum", "query_term_sum")],
                int(arrs["null_total"][t]), [arrs[k][s:e].tolist() for k in ("null_i", "null_j", "null_z", "null_r")])

    for q in (0, 5, _native.OSC_QUERY_CHUNK - 1, _native.OSC_QUERY_CHUNK, Q - 1):
        assert one(lat.receipt_many(P[q:q + 1], as_arrays=True), 0) == one(big, q), q
    order = rng.permutation(Q)[:9]
    sub = lat.receipt_many(P[order], as_arrays=True)
    for t, q in enumerate(order):
        assert one(sub, t) == one(big, q)


def _route_lattice(amd, N, D, clustered=False, seed=7):
    rng = np.random.default_rng(seed)
    if clustered:
        centers = rng.standard_normal((N // 100, D)).astype(np.float32)
        Y = centers[np.arange(N) % centers.shape[0]] + 0.15 * rng.standard_normal((N, D)).astype(np.float32)
        Y = Y[rng.permutation(N)]
    else:
        Y = rng.standard_normal((N, D)).astype(np.float32)
    return amd.Oscillink(Y.astype(np.float32), kneighbors=8, deterministic_k=True), Y


def loop_margins(lat, Ustar):
    """per-row null-decision margins in float64 from the loop's own U* rows"""
    rowptr, col, a, _, sd = lat.graph_csr()
    r = np.repeat(np.arange(lat.N), np.diff(rowptr))
    keep = a > 0
    r, c, w = r[keep], col[keep], a[keep].astype(np.float64)
    Un = Ustar.astype(np.float64) / (sd.astype(np.float64)[:, None] + 1e-12)
    d = Un[r] - Un[c]
    return yr.null_margins(r, lat.lamC * w * np.einsum("ij,ij->i", d, d), lat.N)


@pytest.mark.parametrize("route", ["small", "mid", "blocked", "clustered"])
def test_routes_against_loop(amd, route, monkeypatch):
    N, D, clustered = {"small": (300, 32, False), "mid": (4000, 64, False), "blocked": (20000, 64, False),
                       "clustered": (12000, 64, True)}[route]
    if clustered:
        monkeypatch.setenv("OSC_REORDER", "1")
    lat, Y = _route_lattice(amd, N, D, clustered)
    if clustered:
        assert lat.build_info()["reordered"]
    lat.settle(max_iters=8, tol=1e-3)
    rng = np.random.default_rng(8)
    P = np.stack([Y[:32].mean(axis=0), rng.standard_normal(D), Y[17], rng.uniform(-1, 1, D)]).astype(np.float32)
    got = lat.receipt_many(P)
    assert lat.last_query_basis["converged"]
    psi0 = lat.psi.copy()
    for q in range(P.shape[0]):
        lat.set_query(P[q])
        lp = lat.receipt()
        g = got[q]
        for key in ("deltaH_total",) + SUMS:
            assert g[key] == pytest.approx(lp[key], rel=1e-4, abs=1e-4 * abs(lp["anchor_pen_sum"])), (route, q, key)
        diff = yr.differing_rows(g["null_points"], lp["null_points"])
        if diff:
            margin = loop_margins(lat, lat.solve_Ustar())
            assert all(margin[i] < NEAR for i in diff), (route, q, [(i, margin[i]) for i in diff[:5]])
        _check_against_loop(g, lp, nulls_equal=not diff)
    lat.set_query(psi0)
    if route == "mid":  # a cap above the device selection's limit: sorted on the host, same contract
        monkeypatch.setenv("OSCILLINK_RECEIPT_NULL_CAP", "1500")
        capped = lat.receipt_many(P)
        for q in range(P.shape[0]):
            tot = len(got[q]["null_points"])
            want = _stable_cap(got[q]["null_points"], 1500) if tot > 1500 else got[q]["null_points"]
            assert capped[q]["null_points"] == want
        assert any(len(g["null_points"]) > 1500 for g in got)


def test_errors_and_edges(amd):
    lat, case, Y, psi = _fixture_lattice(amd, "c1_n80_d128_k8")
    D = Y.shape[1]
    with pytest.raises(ValueError):
        lat.receipt_many(np.zeros((3, D + 1), np.float32))
    with pytest.raises(ValueError):
        lat.receipt_many(np.zeros(D, np.float32))
    bad = np.zeros((4, D), np.float32)
    bad[1, 3] = np.inf
    with pytest.raises(ValueError, match="row 1"):
        lat.receipt_many(bad)
    assert lat.receipt_many(np.zeros((0, D), np.float32)) == []
    empty = lat.receipt_many(np.zeros((0, D), np.float32), as_arrays=True)
    assert empty["deltaH"].shape == (0,) and empty["null_offsets"].tolist() == [0]
    assert lat.stats["query_basis_solves"] == 0

    from oscillink_amd.sharding import run_loopback_ranks

    def rank(r, comm):
        l2 = amd.Oscillink(Y, kneighbors=8, deterministic_k=True, comm=comm)
        try:
            l2.receipt_many(np.ones((1, D), np.float32))
        except NotImplementedError:
            return "refused"
        return "ran"

    assert run_loopback_ranks(2, rank) == ["refused", "refused"]


def test_dynamics_meta_passes_through(amd, monkeypatch):
    monkeypatch.setenv("OSCILLINK_RECEIPT_DYNAMICS", "1")
    lat, case, Y, psi = _fixture_lattice(amd, "g1_n400_d64_k6_chain8")
    lat.settle(max_iters=12, tol=1e-3)
    P = _batch(Y, psi, seed=9)
    got = lat.receipt_many(P)
    loop = _loop(lat, P)
    for g, lp in zip(got, loop):
        assert g["meta"]["dynamics"] == lp["meta"]["dynamics"]

"""chain_gated_many: per-query gates with a per-query chain prior, the whole request sequence in
one call.  Against the float64 yardstick of tests/_chain_gated.py on the lattice's own graph, this library's six-call loop
on a second lattice, the batched calls that cover a part of the combination (receipt_gated_many at lamP = 0; receipt_many,
chain_receipt_many and bundle_many with chains= and lamP= under all-ones gates) and itself (batch composition, chunking).
The inputs' own conditions are checked on the CPU in tests/test_chain_gated_host.py; the z-score rules are those of
tests/test_gpu_chain_receipt_many.py."""
import numpy as np
import pytest

from tests import _chain_gated as cg
from tests import _queries as yq
from tests.test_gpu_chain_receipt_many import check_yardstick
from tests.test_gpu_refine_chains import check_chain

pytestmark = pytest.mark.gpu

SUMS = ("coh_drop_sum", "anchor_pen_sum", "query_term_sum")
ARRAY_NULLS = ("null_i", "null_j", "null_z", "null_r")
CHAIN_EDGES = ("chain_z_struct", "chain_z_path", "chain_r_struct", "chain_r_path")
CHAIN_SCALARS = ("chain_gain", "chain_verdict", "chain_weakest_k", "chain_weakest_z")


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


def _lattice(amd, name, monkeypatch):
    clustered = cg.CASES[name][5]
    if clustered:
        monkeypatch.setenv("OSC_REORDER", "1")
    Y = cg.anchors(name)
    lat = amd.Oscillink(Y, kneighbors=cg.CASES[name][2], deterministic_k=True)
    if clustered:
        assert lat.build_info()["reordered"]
    return lat, Y


def _lams(lat):
    return (lat.lamG, lat.lamC, lat.lamQ)


_cases, _yards = {}, {}


def _case(amd, name, monkeypatch):
    """the case's anchors, queries, gates (the fifth row: that query's diffusion gates), dense graph and chains, once"""
    if name not in _cases:
        lat, Y = _lattice(amd, name, monkeypatch)
        P = cg.queries(name, Y)
        G = cg.given_gates(name, lat.N)
        G[4] = lat.diffusion_gates_many(P[4:5], beta=cg.bg.GATE_BETA, gamma=cg.bg.GATE_GAMMA)["gates"][0]
        A, sd = cg.rg.dense_graph(lat.graph_csr(), lat.N)
        chains, weights = cg.query_chains(name, A)
        _cases[name] = dict(Y=Y, P=P, G=G, A=A, sd=sd, chains=chains, weights=weights, k=cg.CASES[name][3])
    return _cases[name]


def _yard(c, key, lamP, chains=None, weights=None, G=None):
    """the float64 yardstick of the case's five queries from U = Y under lamP (and other chains or gates), once per key"""
    if key not in _yards:
        chains, weights = chains or c["chains"], weights or c["weights"]
        G = c["G"] if G is None else G
        _yards[key] = [cg.yardstick(c["Y"], c["Y"], c["P"][q], G[q], c["A"], c["sd"], lamP, chains[q], weights[q], c["k"])
                       for q in range(5)]
    return _yards[key]


def _check_receipt(rec, y, U, c, who):
    """deltaH and the three sums at PARITY, the null points by check_nulls"""
    want = y["receipt"]
    dH = cg.deltaH64(y["M"], U, want["Ustar"])
    print(f"{who}: deltaH {rec['deltaH_total']:.6g} (yardstick {dH:.6g}), " +
          ", ".join(f"{k} {rec[k]:.6g} ({want[k]:.6g})" for k in SUMS))
    assert cg.close(rec["deltaH_total"], dH), (who, rec["deltaH_total"], dH)
    for key in SUMS:
        assert cg.close(rec[key], want[key]), (who, key, rec[key], want[key])
    share = cg.check_nulls(rec["null_points"], want["null_points"], want["margin"], c["A"])
    assert share <= cg.LEFT_OUT_CAP, (who, share)


def _check_bundle(ids, y, who):
    ok, _ = yq.same_until_near_tie([int(i) for i in ids], [int(i) for i in y["ids"]], y["margins"], cg.NEAR_TIE)
    assert ok, (who, list(ids), list(y["ids"]), y["margins"])


def _arrays(lat, P, G, chains, lamP, **kw):
    out = lat.chain_gated_many(P, G, chains, lamP, as_arrays=True, **kw)
    return {k: np.array(v, copy=True) for k, v in out.items()}


def _query_of(arrs, t):
    """query t's entries of an as_arrays dict, bytes included"""
    s, e = int(arrs["null_offsets"][t]), int(arrs["null_offsets"][t + 1])
    cs, ce = int(arrs["chain_offsets"][t]), int(arrs["chain_offsets"][t + 1])
    out = {k: arrs[k][t].tobytes() for k in arrs if k not in ARRAY_NULLS + CHAIN_EDGES + ("null_offsets", "chain_offsets")}
    out.update({k: arrs[k][s:e].tobytes() for k in ARRAY_NULLS})
    out.update({k: arrs[k][cs:ce].tobytes() for k in CHAIN_EDGES})
    return out


# 1: every case, lamP 0.2 and 0.5, U at Y and after one settle(), against the float64 yardstick
@pytest.mark.parametrize("state", ["fresh", "settled"])
@pytest.mark.parametrize("lamP", cg.LAMPS)
@pytest.mark.parametrize("name", list(cg.CASES))
def test_cases_against_yardstick(amd, name, lamP, state, monkeypatch):
    c = _case(amd, name, monkeypatch)
    lat, Y = _lattice(amd, name, monkeypatch)
    if state == "settled":
        lat.settle()
    yard = _yard(c, (name, lamP), lamP)
    recs, crecs, bundles = lat.chain_gated_many(c["P"], c["G"], c["chains"], lamP, chain_weights=c["weights"],
                                                bundle_k=c["k"])
    assert len(recs) == len(crecs) == len(bundles) == 5 and lat.last_chain_gated["converged"].all()
    assert lat.last_chain_gated["lamP"] == lamP and lat.last_chain_gated["settle_iters"] is None
    arrs = {z_th: _arrays(lat, c["P"], c["G"], c["chains"], lamP, chain_weights=c["weights"], z_th=z_th) for z_th in cg.Z_THS}
    U = lat.U
    for q in range(5):
        who = f"{name} lamP {lamP} {state} q{q} {cg.kinds_of(name)[q]}"
        _check_receipt(recs[q], yard[q], U, c, who)
        for z_th in cg.Z_THS:
            worst = check_yardstick(who, q, arrs[z_th], c["chains"][q], yard[q]["chain"], z_th)
        print(f"{who}: chain deviations in units of their bounds {worst}")
        _check_bundle([b["id"] for b in bundles[q]], yard[q], who)
        m = recs[q]["meta"]
        assert m["ustar_source"] == "gated_panel" and m["ustar_cached"] is False and m["ustar_converged"] is True
        assert recs[q]["cg_iters"] == int(lat.last.get("iters") or 0)
        assert crecs[q]["verdict"] == bool(arrs[cg.Z_THS[0]]["chain_verdict"][q])
        assert [e["edge"] for e in crecs[q]["edges"]] == [list(p) for p in zip(c["chains"][q], c["chains"][q][1:])]


# 2: every record equals the six-call loop on a second lattice; the first lattice's state is untouched
@pytest.mark.parametrize("mode", [None, "minimal", "extended"])
@pytest.mark.parametrize("detail", ["light", "full"])
@pytest.mark.parametrize("name", list(cg.LOOP_CASES))
def test_loop_parity_and_state(amd, name, detail, mode, monkeypatch):
    from oscillink_amd.receipts import verify_receipt

    c = _case(amd, name, monkeypatch)
    P, G, chains, weights, k, lamP = c["P"], c["G"], c["chains"], c["weights"], c["k"], cg.LOOP_LAMP
    yard = _yard(c, (name, lamP), lamP)
    lat, Y = _lattice(amd, name, monkeypatch)
    loop, _ = _lattice(amd, name, monkeypatch)
    for l in (lat, loop):
        l.set_receipt_detail(detail)
        if mode:
            l.set_receipt_secret("s3cret")
            l.set_signature_mode(mode)
    # a lattice with a query, gates, a U* cache, both query bases and receipts of its own, its state back at U = Y
    g0 = np.random.default_rng(3).uniform(0.2, 1.0, lat.N).astype(np.float32)
    lat.set_query(P[0], gates=g0)
    lat.bundle_many(P[:2], k=2)
    lat.chain_receipt_many(P[:2], chains[0], lamP=0.3)
    rec0 = lat.receipt()
    U_star = lat.solve_Ustar().copy()
    st0, last0, lu0, qb0 = dict(lat.stats), dict(lat.last), dict(lat.last_ustar), dict(lat.last_query_basis)
    sb0 = dict(lat.last_shifted_basis)
    psi0, U0, B0 = lat.psi.copy(), lat.U.copy(), lat.B_diag.copy()
    for settle in (None, True):
        got, cgot, bgot = lat.chain_gated_many(P, G, chains, lamP, chain_weights=weights, settle=settle, bundle_k=k,
                                               max_iters=cg.bg.LOOP_ITERS)
        carr = _arrays(lat, P, G, chains, lamP, chain_weights=weights, settle=settle, max_iters=cg.bg.LOOP_ITERS)
        for q in range(5):
            loop.clear_chain()
            loop.reset_U()
            loop.add_chain(chains[q], lamP, weights[q])
            loop.set_query(P[q], gates=G[q])
            if settle:
                loop.settle()
            want, cwant, bwant = loop.receipt(), loop.chain_receipt(chains[q], 2.5), loop.bundle(k, 0.5)
            g = got[q]
            assert set(g) == set(want) and list(g) == list(want)
            assert set(g["meta"]) == set(want["meta"]) | {"ustar_source"}
            assert g["version"] == want["version"] and g["cg_iters"] == want["cg_iters"], (q, g["cg_iters"], want["cg_iters"])
            assert g["meta"]["ustar_iters"] == want["meta"]["ustar_iters"], (q, g["meta"]["ustar_iters"], want["meta"])
            assert abs(g["residual"] - want["residual"]) <= 2e-3
            for key in ("deltaH_total",) + SUMS:
                assert cg.close(g[key], want[key]), (q, key, g[key], want[key])
            for key in ("state_sig", "receipt_detail", "gates_min", "gates_max", "gates_mean", "gates_uniform", "avg_degree",
                        "edge_density", "ustar_converged"):
                assert g["meta"][key] == want["meta"][key], (q, key)
            margin = yard[q]["receipt"]["margin"]
            bad = [i for i in cg.rg.differing_rows(g["null_points"], want["null_points"]) if margin[i] >= cg.MARGIN]
            assert not bad, (q, bad[:5])
            if detail == "light":
                assert g["null_points"] == [] and all(g[key] == 0.0 for key in SUMS)
            if mode:
                assert verify_receipt(g, "s3cret") and not verify_receipt(g, "other")
                pay = g["meta"]["signature"]["payload"]
                assert pay["mode"] == mode and pay["state_sig"] == want["meta"]["state_sig"]
                assert pay["deltaH_total"] == g["deltaH_total"]
                if mode == "extended":
                    assert pay["params"] == want["meta"]["signature"]["payload"]["params"] and pay["params"]["lamP"] == lamP
            else:
                assert "signature" not in g["meta"]
            # the chain receipt against the loop's dict, by the project's loop-against-batch rule
            # (tests/test_gpu_refine_chains.check_chain, as tests/test_gpu_chain_receipt_many.check_loop applies it)
            check_chain(f"{name} settle {settle}", q, carr, chains[q], {"chain": cwant, "y64": yard[q]["chain"]},
                        {"chain_receipt": cgot[q]})
            assert list(cgot[q]) == list(cwant) and list(cgot[q]["weakest_link"]) == list(cwant["weakest_link"])
            ok, _ = yq.same_until_near_tie([b["id"] for b in bgot[q]], [b["id"] for b in bwant], yard[q]["margins"], cg.NEAR_TIE)
            assert ok, (q, bgot[q], bwant)
        assert dict(lat.stats) == st0 and lat.last == last0 and lat.last_ustar == lu0 and lat.last_query_basis == qb0
        assert lat.last_shifted_basis == sb0
        lat._U_host = None  # (read the device's U again)
        assert np.array_equal(lat.psi, psi0) and np.array_equal(lat.U, U0) and np.array_equal(lat.B_diag, B0)
    assert np.array_equal(lat.solve_Ustar(), U_star)
    rec1 = lat.receipt()
    for key in ("deltaH_total", "null_points") + SUMS:
        assert rec1[key] == rec0[key], key
    assert rec1["meta"]["state_sig"] == rec0["meta"]["state_sig"]


# 3: lamP = 0: the receipts and bundles are receipt_gated_many's bytes; the chain receipt is still computed
@pytest.mark.parametrize("settle", [None, True], ids=["held", "settle"])
def test_lamP_zero_is_receipt_gated_many_bit_for_bit(amd, settle, monkeypatch):
    name = cg.SETTLE_CASE
    c = _case(amd, name, monkeypatch)
    lat, Y = _lattice(amd, name, monkeypatch)
    k = c["k"]
    plain = {key: np.array(v, copy=True) for key, v in
             lat.receipt_gated_many(c["P"], c["G"], settle=settle, bundle_k=k, as_arrays=True).items()}
    got = _arrays(lat, c["P"], c["G"], c["chains"], 0.0, chain_weights=c["weights"], settle=settle, bundle_k=k)
    assert set(got) == set(plain) | set(CHAIN_EDGES) | set(CHAIN_SCALARS) | {"chain_offsets"}
    for key in plain:
        assert got[key].tobytes() == plain[key].tobytes() and got[key].dtype == plain[key].dtype, key
    # the chain arrays are those of U*_q without a prior (but on the weighted path of the argument)
    yard = _yard(c, (name, 0.0), 0.0)
    for q in range(5):  # (U*_q does not depend on the settle)
        check_yardstick(f"{name} lamP 0 q{q}", q, got, c["chains"][q], yard[q]["chain"], 2.5)
    recs, crecs = lat.chain_gated_many(c["P"], c["G"], c["chains"], 0.0, chain_weights=c["weights"], settle=settle)
    want = lat.receipt_gated_many(c["P"], c["G"], settle=settle)
    for q in range(5):
        assert recs[q]["deltaH_total"] == want[q]["deltaH_total"] and recs[q]["null_points"] == want[q]["null_points"]
        assert recs[q]["meta"]["state_sig"] != want[q]["meta"]["state_sig"]  # (chain_present and the chain's length)
        assert len(crecs[q]["edges"]) == len(c["chains"][q]) - 1


# 4: all-ones gates and short chains: the low-rank calls on the same operator
def test_all_ones_gates_agree_with_the_low_rank_calls(amd, monkeypatch):
    name, lamP = cg.SETTLE_CASE, cg.LAMPS[0]
    c = _case(amd, name, monkeypatch)
    P, chains, weights, k = c["P"], c["chains"], c["weights"], c["k"]
    lat, Y = _lattice(amd, name, monkeypatch)
    ones = np.ones((5, lat.N), np.float32)
    lat.settle()
    recs, crecs, bundles = lat.chain_gated_many(P, ones, chains, lamP, chain_weights=weights, bundle_k=k)
    arr = _arrays(lat, P, ones, chains, lamP, chain_weights=weights)
    plain = lat.receipt_many(P, chains=chains, lamP=lamP, chain_weights=weights)
    carr = lat.chain_receipt_many(P, chains, lamP=lamP, chain_weights=weights, as_arrays=True)
    bplain = lat.bundle_many(P, k=k, chains=chains, lamP=lamP, chain_weights=weights, as_arrays=True)
    yard = _yard(c, (name, lamP, "ones"), lamP, G=ones)
    for q in range(5):
        for key in ("deltaH_total",) + SUMS:
            assert cg.close(recs[q][key], plain[q][key]), (q, key, recs[q][key], plain[q][key])
        assert recs[q]["meta"]["state_sig"] == plain[q]["meta"]["state_sig"]
        assert recs[q]["cg_iters"] == plain[q]["cg_iters"] and recs[q]["residual"] == plain[q]["residual"]
        margin = yard[q]["receipt"]["margin"]
        bad = [i for i in cg.rg.differing_rows(recs[q]["null_points"], plain[q]["null_points"]) if margin[i] >= cg.MARGIN]
        assert not bad, (q, bad[:5])
        # both calls within the z rules of the same float64 values
        check_yardstick(f"gated q{q}", q, arr, chains[q], yard[q]["chain"], 2.5)
        check_yardstick(f"low-rank q{q}", q, carr, chains[q], yard[q]["chain"], 2.5)
        assert bool(arr["chain_verdict"][q]) == bool(carr["chain_verdict"][q])
        ok, _ = yq.same_until_near_tie([b["id"] for b in bundles[q]], bplain[0][q].tolist(), yard[q]["margins"], cg.NEAR_TIE)
        assert ok, (q, bundles[q], bplain[0][q].tolist())


# 5: alone / reversed / in chunks of one and three; shared and own chains in one batch; a frozen query stays frozen
def test_batch_independence_and_chunking(amd, monkeypatch):
    name, lamP = cg.SETTLE_CASE, cg.LAMPS[0]
    c = _case(amd, name, monkeypatch)
    P, G = c["P"], c["G"]
    ch = cg.chains(name, c["A"])
    chains = [ch["walk"][0], ch["mixed"][0], ch["walk"][0], ch["revisit"][0], ch["walk"][0]]  # three queries share a chain
    weights = [None, ch["mixed"][1], None, ch["revisit"][1], None]
    lat, _ = _lattice(amd, name, monkeypatch)
    kw = dict(settle=True, bundle_k=4)

    def run(order):
        return _arrays(lat, P[order], G[order], [chains[q] for q in order], lamP, chain_weights=[weights[q] for q in order], **kw)

    whole = run(list(range(5)))
    # the queries end at different iterations: a query frozen early sees later applies of the others' paths
    assert len(set(whole["ustar_iters"].tolist())) > 1 or len(set(whole["settle_iters"].tolist())) > 1, whole["ustar_iters"]
    assert int(whole["null_total"].sum()) > 0
    for chunk in ("1", "3"):
        monkeypatch.setenv("OSC_GATED_CHUNK", chunk)
        chunked = run(list(range(5)))
        monkeypatch.delenv("OSC_GATED_CHUNK")
        assert set(chunked) == set(whole)
        for key in whole:
            assert chunked[key].tobytes() == whole[key].tobytes(), (chunk, key)
    for q in range(5):
        assert _query_of(run([q]), 0) == _query_of(whole, q), q
    rev = run([4, 3, 2, 1, 0])
    for t, q in enumerate([4, 3, 2, 1, 0]):
        assert _query_of(rev, t) == _query_of(whole, q), q
    # a non-finite query stays inside its own query
    Pn = P.copy()
    Pn[2, min(7, P.shape[1] - 1)] = np.nan
    dirty = _arrays(lat, Pn, G, chains, lamP, chain_weights=weights, **kw)
    for q in (0, 1, 3, 4):
        assert _query_of(dirty, q) == _query_of(whole, q), q
    assert not np.isfinite(dirty["deltaH"][2]) and not np.isfinite(dirty["score"][2]).any()
    assert not np.isfinite(dirty["chain_gain"][2]) and not bool(lat.last_chain_gated["converged"][2])


# 6: the path seams on the reordered case: more than one fix unit, [a, a], the weight-0 edge, the two-weight revisit
def test_path_seams(amd, monkeypatch):
    name, lamP = cg.SEAM_CASE, cg.SETTLE_LAMP
    c = _case(amd, name, monkeypatch)
    chains, weights = cg.seam_chains(c["A"])
    assert len(chains[0]) == 1024 and len(set(chains[0])) > cg.fix_rows()  # (the plan's cut: two fix units)
    lat, Y = _lattice(amd, name, monkeypatch)
    yard = _yard(c, (name, lamP, "seams"), lamP, chains=chains, weights=weights)
    recs, crecs, bundles = lat.chain_gated_many(c["P"], c["G"], chains, lamP, chain_weights=weights, bundle_k=c["k"])
    arrs = {z_th: _arrays(lat, c["P"], c["G"], chains, lamP, chain_weights=weights, z_th=z_th) for z_th in cg.Z_THS}
    assert lat.last_chain_gated["converged"].all()
    for q in range(5):
        who = f"seam q{q} ({len(chains[q])} nodes)"
        _check_receipt(recs[q], yard[q], Y, c, who)
        # (the laps at 2.5 alone: tests/test_chain_gated_host.py::test_seam_chains_meet_the_same_conditions says why)
        for z_th in cg.Z_THS[:1] if len(chains[q]) == 1024 else cg.Z_THS:
            worst = check_yardstick(who, q, arrs[z_th], chains[q], yard[q]["chain"], z_th)
        print(f"{who}: chain deviations in units of their bounds {worst}")
        _check_bundle([b["id"] for b in bundles[q]], yard[q], who)


# 7: with settle, against the float64 settle under M_q followed by the yardstick receipt
@pytest.mark.parametrize("settle", [True, cg.SETTLE_CAPPED], ids=["default", "capped"])
def test_settle_against_yardstick(amd, settle, monkeypatch):
    name, lamP = cg.SETTLE_CASE, cg.SETTLE_LAMP
    c = _case(amd, name, monkeypatch)
    lat, Y = _lattice(amd, name, monkeypatch)
    st = cg.SETTLE_DEFAULT if settle is True else settle
    yard = _yard(c, (name, lamP), lamP)
    got, _ = lat.chain_gated_many(c["P"], c["G"], c["chains"], lamP, chain_weights=c["weights"], settle=settle)
    rep = lat.last_chain_gated
    for q in range(5):
        Uq, iters, res, hist = cg.settle64(yard[q]["M"], Y, Y, c["P"][q], c["G"][q], lamP, _lams(lat), **st)
        print(f"q{q}: cg_iters {got[q]['cg_iters']} (float64 {iters}), residual {got[q]['residual']:.3e} ({res:.3e})")
        assert got[q]["cg_iters"] == iters == int(rep["settle_iters"][q]), q
        assert abs(got[q]["residual"] - res) <= 2 * st["tol"], q
        assert got[q]["residual"] == float(rep["settle_res"][q])
        assert (got[q]["residual"] <= st["tol"]) == (res <= st["tol"])
        _check_receipt(got[q], yard[q], Uq, c, f"settle q{q}")
        assert got[q]["t_ms"] > 0 and got[q]["meta"]["last_settle_ms"] == got[q]["t_ms"]
    assert np.array_equal(lat.U, Y)  # no settled state is written back


# 8
def test_errors_and_edges(amd, monkeypatch):
    name = cg.SETTLE_CASE
    c = _case(amd, name, monkeypatch)
    Y, P, G, chains = c["Y"], c["P"], c["G"], c["chains"]
    lat, _ = _lattice(amd, name, monkeypatch)
    N, D = Y.shape
    none_p, none_g = np.zeros((0, D), np.float32), np.zeros((0, N), np.float32)
    assert lat.chain_gated_many(none_p, none_g, []) == ([], [])
    assert lat.chain_gated_many(none_p, "diffusion", [0, 1], settle=True, bundle_k=3) == ([], [], [])
    empty = lat.chain_gated_many(none_p, none_g, [], settle=True, bundle_k=3, as_arrays=True)
    assert empty["deltaH"].shape == (0,) and empty["null_offsets"].tolist() == [0] and empty["ids"].shape == (0, 3)
    assert empty["chain_offsets"].tolist() == [0] and empty["chain_z_struct"].shape == (0,) and empty["chain_gain"].shape == (0,)
    assert empty["chain_verdict"].dtype == np.bool_ and empty["settle_iters"].shape == (0,)
    for bad, match in (([0, N], "out of bounds"), ([3], "at least two"), ([0, 1] * 512 + [0], "at most 1024")):
        with pytest.raises(ValueError, match=match):
            lat.chain_gated_many(P, G, bad)
    with pytest.raises(ValueError, match="weights length"):
        lat.chain_gated_many(P, G, [0, 1, 2], chain_weights=[1.0])
    with pytest.raises(ValueError, match="lamP must be >= 0"):
        lat.chain_gated_many(P, G, chains, -0.5)
    ok = lat.chain_gated_many(P[:1], G[:1], [list(range(N)) * 10 + [0, 1, 2]][:1], as_arrays=True)  # 973 nodes, 97 distinct
    assert ok["chain_offsets"].tolist() == [0, 10 * N + 2] and np.isfinite(ok["deltaH"]).all()
    chained, _ = _lattice(amd, name, monkeypatch)
    chained.add_chain([0, 1, 2], lamP=0.2)
    with pytest.raises(NotImplementedError):
        chained.chain_gated_many(P, G, chains)

    from oscillink_amd.sharding import run_loopback_ranks

    def rank(r, comm):
        l2 = amd.Oscillink(Y, kneighbors=6, deterministic_k=True, comm=comm)
        try:
            l2.chain_gated_many(P, G, chains)
        except NotImplementedError:
            return "refused"
        return "ran"

    assert run_loopback_ranks(2, rank) == ["refused", "refused"]

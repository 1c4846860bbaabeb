"""Chain priors in receipt_many: `receipt_many(psis, chains=..., lamP=...)` against the float64
yardstick -- tests/_receipt_yardstick.py on the dense M + lamP L_path,q -- against this library's own loop
`add_chain(chain_q, lamP, weights_q); set_query(psi_q); receipt()` on a second lattice, and against itself (batch
composition, passes, chunks, state).

deltaH and the three sums: 1e-4 relative to the yardstick, a sum floored at 1e-3 of |anchor| + |query| as in
tests/test_gpu_receipt_many.py.  Null points equal the yardstick's except on rows whose float64 margin (`null_margins`) is below
NEAR = 1e-3, and those are at most 2 % of a query's rows; with lamC = 0 nothing is excused.  The wall-clock fields of a
record (graph_build_ms, last_settle_ms, t_ms) belong to the lattice that made it and are not compared across two lattices."""
import numpy as np
import pytest

from tests import _receipt_prior as rp
from tests import test_gpu_chain_receipt_many as tcm
from tests.test_gpu_bundle_prior_many import Yard, _own
from tests.test_gpu_receipt_many import META_SAME_AS_LOOP, NEAR, SAME_AS_LOOP, SUMS, _batch, _stable_cap

cm, yr = rp.cm, rp.yr
pytestmark = pytest.mark.gpu

TOL = 1e-4
REL = 1e-4
NEAR_SHARE = 0.02
CLOCKS = ("graph_build_ms", "last_settle_ms", "t_ms")


@pytest.fixture(scope="module")
def amd():
    import oscillink_amd
    from oscillink_amd import _native

    assert _native.device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return oscillink_amd


@pytest.fixture(autouse=True)
def _plain_env(monkeypatch):
    for k in ("OSCILLINK_RECEIPT_NULL_CAP", "OSCILLINK_RECEIPT_DYNAMICS", "OSC_CHAIN_PRIOR_COLS"):
        monkeypatch.delenv(k, raising=False)


def _per_query(chains, weights, Q):
    shared = bool(chains) and not isinstance(chains[0], (list, tuple))
    chs = [chains] * Q if shared else chains
    wts = [weights] * Q if shared or weights is None else weights
    return chs, wts


def _loop(lat2, P, chs, wts, lamP):
    psi0 = lat2.psi.copy()
    out = []
    for q in range(P.shape[0]):
        lat2.add_chain(chs[q], lamP=lamP, weights=wts[q])
        lat2.set_query(P[q])
        out.append(lat2.receipt())
    lat2.clear_chain()
    lat2.set_query(psi0)
    return out


def _want(yard, U, psi, chain, weights, lamP):
    Lp = rp.path_terms(yard.N, chain, weights)[0]
    return yr.receipt(yard.Y.astype(np.float32), U, psi, yard.A, yard.sd, yard.B, yard.lamG, yard.lamC, yard.lamQ,
                      yard.M + lamP * Lp)


def _dev(got, want):
    """relative deviation of deltaH and of each sum (floored) from the yardstick"""
    scale = max(abs(want["anchor_pen_sum"]) + abs(want["query_term_sum"]), 1e-12)
    out = {"deltaH": abs(got["deltaH_total"] - want["deltaH"]) / max(abs(want["deltaH"]), 1e-300)}
    for key in SUMS:
        out[key] = abs(got[key] - want[key]) / max(abs(want[key]), 1e-3 * scale)
    return out


def _check(tag, lat, lat2, yard, P, chains, weights, lamP, worst):
    """the batch against the yardstick and the loop; `worst` collects the largest deviations of both"""
    Q = P.shape[0]
    chs, wts = _per_query(chains, weights, Q)
    got = lat.receipt_many(P, chains=chains, lamP=lamP, chain_weights=weights)
    pr = lat.last_receipt_prior
    assert pr["lamP"] == lamP and pr["res"].dtype == np.float32 and pr["iters"].dtype == np.int32
    assert pr["res"].shape == (Q,) and np.all(pr["res"] <= TOL), (tag, pr["res"].tolist())
    loop = _loop(lat2, P, chs, wts, lamP) if lat2 is not None else [None] * Q
    U = lat.U.astype(np.float64)
    for q in range(Q):
        want = _want(yard, U, P[q], chs[q], wts[q], lamP)
        g, lp = got[q], loop[q]
        d = _dev(g, want)
        print(f"{tag}: query {q}: batch " + ", ".join(f"{k} {v:.3g}" for k, v in d.items()))
        for k, v in d.items():
            worst["batch"] = max(worst["batch"], v)
            assert v <= REL, (tag, q, k, v, g["deltaH_total"] if k == "deltaH" else g[k], want[k])
        diff = yr.differing_rows(g["null_points"], want["null_points"])
        if yard.lamC == 0:
            assert g["null_points"] == [] and g["meta"]["null_points_summary"]["total_null_points"] == 0
        else:
            bad = [i for i in diff if want["margin"][i] >= NEAR]
            assert not bad, (tag, q, bad[:5])
            assert len(diff) <= NEAR_SHARE * yard.N, (tag, q, len(diff))
        m = g["meta"]
        assert m["ustar_source"] == "chain_prior_basis" and m["ustar_res"] == float(pr["res"][q])
        assert m["ustar_converged"] is True and m["ustar_iters"] == lat.last_shifted_basis["iters"]["X"]
        if lp is None:
            continue
        dl = _dev(lp, want)
        worst["loop"] = max(worst["loop"], max(dl.values()))
        assert set(g) == set(lp) and set(m) == set(lp["meta"]) | {"ustar_source"}
        for key in SAME_AS_LOOP:
            if key not in CLOCKS:
                assert g[key] == lp[key], (tag, q, key)
        for key in META_SAME_AS_LOOP:
            if key not in CLOCKS:
                assert m[key] == lp["meta"][key], (tag, q, key)
        if not yr.differing_rows(g["null_points"], lp["null_points"]):
            assert m["null_points_summary"] == lp["meta"]["null_points_summary"]
    return got


def _pair(amd, inp, state):
    lat, lat2 = tcm._lattice(amd, inp, False), tcm._lattice(amd, inp, False)
    if state == "settled":
        lat.settle(max_iters=12, tol=1e-3)
        lat2.settle(max_iters=12, tol=1e-3)
        lat2.U = lat.U
    elif state == "stationary":
        lat.U = lat.solve_Ustar()
        lat2.U = lat.U
    return lat, lat2


@pytest.mark.parametrize("state", ["fresh", "settled", "stationary"])
@pytest.mark.parametrize("name", cm.FIXTURES)
def test_fixtures_against_yardstick_and_loop(amd, name, state):
    inp = cm.inputs(name)
    lat, lat2 = _pair(amd, inp, state)
    yard = Yard(lat, inp["Y"])
    P = _batch(inp["Y"], inp["psi"])
    Q = P.shape[0]
    assert Q == 6 and not P[5].any()
    ch = cm.chains(inp)
    chs, wts = _own(yard, Q)
    worst = {"batch": 0.0, "loop": 0.0}
    full = {}
    for lamP in (0.2, 0.5):
        for bname, c, w in (("shared walk", ch["walk"], None), ("shared weighted mixed", ch["mixed"], cm.OWN_WEIGHTS),
                            ("per query", chs, wts)):
            full[(lamP, bname)] = _check(f"{name}/{state}/lamP {lamP}/{bname}", lat, lat2, yard, P, c, w, lamP, worst)
    print(f"{name}/{state}: worst deviation from the yardstick: batch {worst['batch']:.3g}, loop {worst['loop']:.3g}")
    # light detail: deltaH only, bit for bit the full call's
    lat.set_receipt_detail("light")
    light = lat.receipt_many(P, chains=chs, lamP=0.5, chain_weights=wts)
    for q in range(Q):
        assert light[q]["deltaH_total"] == full[(0.5, "per query")][q]["deltaH_total"]
        assert light[q]["null_points"] == [] and all(light[q][k] == 0.0 for k in SUMS)
        assert light[q]["meta"]["receipt_detail"] == "light"
        assert light[q]["meta"]["null_points_summary"] == {"total_null_points": 0, "returned_null_points": 0,
                                                           "null_cap_applied": False}
    lat.close()
    lat2.close()


@pytest.mark.parametrize("mode", ["minimal", "extended"])
def test_signatures(amd, mode):
    from oscillink_amd.receipts import verify_receipt, verify_receipt_mode

    inp = cm.inputs("gates_chain_n333_d50_k7")
    lat, lat2 = _pair(amd, inp, "fresh")
    for x in (lat, lat2):
        x.set_receipt_secret("s3cret")
        x.set_signature_mode(mode)
    P = _batch(inp["Y"], inp["psi"], seed=1)
    chain = cm.chains(inp)["mixed"]  # 7 nodes, 4 distinct: chain_len is the raw length
    got = lat.receipt_many(P, chains=chain, lamP=0.3, chain_weights=cm.OWN_WEIGHTS)
    loop = _loop(lat2, P, [chain] * P.shape[0], [cm.OWN_WEIGHTS] * P.shape[0], 0.3)
    for g, lp in zip(got, loop):
        assert verify_receipt(g, "s3cret") and not verify_receipt(g, "other")
        ok, payload = verify_receipt_mode(g, "s3cret", require_mode=mode)
        assert ok
        assert payload["state_sig"] == g["meta"]["state_sig"] == lp["meta"]["state_sig"]
        assert payload["deltaH_total"] == g["deltaH_total"]
        if mode == "extended":
            for key in ("ustar_iters", "ustar_res", "ustar_converged"):
                assert payload[key] == g["meta"][key]
            assert payload["params"] == lp["meta"]["signature"]["payload"]["params"] and payload["params"]["lamP"] == 0.3
            assert payload["graph"] == lp["meta"]["signature"]["payload"]["graph"]
    lat.close()
    lat2.close()


def test_smallest_shapes_that_can_break_the_kernels(amd):
    inp = cm.inputs("gates_chain_n333_d50_k7")  # N = 333 (partial steps, waves and workgroups), D = 50 (ld padding), gates
    lat, lat2 = _pair(amd, inp, "settled")
    assert lat.N % 32 != 0 and inp["Y"].shape[1] % 4 != 0
    yard = Yard(lat, inp["Y"])
    P = _batch(inp["Y"], inp["psi"])[[0, 1, 5]]  # psi0, a random query, psi = 0
    worst = {"batch": 0.0, "loop": 0.0}
    kw = dict(lamP=0.3, as_arrays=True)
    # 31 / 32 / 33 distinct nodes in one pass (the panel's slab width), as one chain and as chains that share nodes
    for m in (31, 32, 33):
        chain = rp.spread(yard.rowptr, yard.col, m)
        assert len(set(chain)) == m
        _check(f"one chain of {m}", lat, lat2 if m == 33 else None, yard, P, chain, None, 0.3, worst)
        parts = [chain[:12], chain[10:24], chain[22:] + chain[:2]]
        assert len(set(sum(parts, []))) == m
        _check(f"{m} nodes in three chains", lat, None, yard, P, parts, None, 0.3, worst)
        arr = lat.receipt_many(P, chains=parts, **kw)
        for q in range(3):  # ... and each of them alone gives the same bytes
            alone = lat.receipt_many(P[q:q + 1], chains=[parts[q]], **kw)
            for key in ("deltaH", "coh_drop_sum", "anchor_pen_sum", "query_term_sum", "null_total", "chain_prior_res"):
                assert alone[key][0].tobytes() == arr[key][q].tobytes(), (m, q, key)
            s, e = int(arr["null_offsets"][q]), int(arr["null_offsets"][q + 1])
            for key in ("null_i", "null_j", "null_z", "null_r"):
                assert alone[key].tobytes() == arr[key][s:e].tobytes(), (m, q, key)
    # m = 64 with weights and a revisit; m = 1; 65 is refused before any device work
    c64 = rp.spread(yard.rowptr, yard.col, 64, start=7)
    w64 = [0.25 + (t % 5) * 0.5 for t in range(64)]
    _check("m = 64", lat, lat2, yard, P[:2], c64 + [c64[0]], w64, 0.5, worst)
    _check("m = 1", lat, lat2, yard, P, [c64[3], c64[3]], None, 0.5, worst)
    print(f"seams: worst deviation from the yardstick: batch {worst['batch']:.3g}, loop {worst['loop']:.3g}")
    n0 = lat.shifted_basis_solves
    with pytest.raises(ValueError, match="at most 64 distinct"):
        lat.receipt_many(P, chains=rp.spread(yard.rowptr, yard.col, 65), lamP=0.9)
    assert lat.shifted_basis_solves == n0
    lat.close()
    lat2.close()


def test_isolated_chain_node(amd):
    rng = np.random.default_rng(13)
    Y = rng.standard_normal((40, 19)).astype(np.float32)
    lats = []
    for _ in range(2):
        lat = amd.Oscillink(Y, kneighbors=4, deterministic_k=True)
        rowptr, col, a = lat.graph_csr()[:3]
        rows = np.repeat(np.arange(40), np.diff(rowptr))
        keep = (rows != 3) & (col != 3)
        cnt = np.bincount(rows[keep], minlength=40)
        lat.set_graph_csr(np.concatenate([[0], np.cumsum(cnt)]), col[keep], a[keep])
        lat.set_query(Y[:8].mean(axis=0))
        lats.append(lat)
    lat, lat2 = lats
    yard = Yard(lat, Y)
    assert yard.rowptr[4] == yard.rowptr[3]
    w = cm.walk(yard.rowptr, yard.col, 0, 3)
    P = rng.standard_normal((3, 19)).astype(np.float32)
    worst = {"batch": 0.0, "loop": 0.0}
    _check("isolated row on the chain", lat, lat2, yard, P, w + [3, 3, w[0]], None, 0.4, worst)
    _check("[3, 3]: m = 1 on the isolated row", lat, lat2, yard, P, [3, 3], None, 0.4, worst)
    lat.close()
    lat2.close()


@pytest.mark.parametrize("cap", [3, 1100])
def test_null_cap(amd, cap, monkeypatch):
    from tests import _gated

    Y = _gated.corpus(100, 16)[0]  # 2000 x 96 clustered rows: more null points than either cap
    assert Y.shape == (2000, 96)
    lat = amd.Oscillink(Y, kneighbors=8, deterministic_k=True)
    lat.set_query(Y[:32].mean(axis=0))
    rowptr, col = lat.graph_csr()[:2]
    rng = np.random.default_rng(2)
    P = np.stack([Y[:32].mean(axis=0), rng.standard_normal(Y.shape[1])]).astype(np.float32)
    starts = [s for s in (0, 700, 701, 702, 703) if len(cm.walk(rowptr, col, s)) >= 3][:2]
    chs = [cm.walk(rowptr, col, s) for s in starts]
    assert len(chs) == 2
    kw = dict(chains=chs, lamP=0.3)
    full = lat.receipt_many(P, **kw)
    monkeypatch.setenv("OSCILLINK_RECEIPT_NULL_CAP", str(cap))
    capped = lat.receipt_many(P, **kw)
    arrays = lat.receipt_many(P, as_arrays=True, **kw)
    for q in range(P.shape[0]):
        tot = len(full[q]["null_points"])
        assert capped[q]["null_points"] == (_stable_cap(full[q]["null_points"], cap) if tot > cap else full[q]["null_points"])
        assert capped[q]["meta"]["null_points_summary"] == {"total_null_points": tot, "returned_null_points": min(cap, tot),
                                                            "null_cap_applied": tot > cap}
        s, e = int(arrays["null_offsets"][q]), int(arrays["null_offsets"][q + 1])
        assert [[int(i), int(j)] for i, j in zip(arrays["null_i"][s:e], arrays["null_j"][s:e])] == \
            [p["edge"] for p in capped[q]["null_points"]]
        assert int(arrays["null_total"][q]) == tot
        assert float(arrays["deltaH"][q]) == capped[q]["deltaH_total"] == full[q]["deltaH_total"]
    print(f"cap {cap}: null points per query {[len(f['null_points']) for f in full]}")
    assert any(len(f["null_points"]) > cap for f in full)  # (above 1 024 the selection is the host's stable sort)
    lat.close()


def test_bfs_permuted_lattice(amd, monkeypatch):
    from tests import _gated

    monkeypatch.setenv("OSC_REORDER", "1")
    Y = _gated.corpus(100, 8)[0]
    assert Y.shape == (2000, 96)
    lat = amd.Oscillink(Y, kneighbors=8, deterministic_k=True)
    lat2 = amd.Oscillink(Y, kneighbors=8, deterministic_k=True)
    assert lat.build_info()["reordered"]
    for x in (lat, lat2):
        x.set_query(Y[:32].mean(axis=0))
    yard = Yard(lat, Y)
    rng = np.random.default_rng(3)
    P = np.stack([Y[:32].mean(axis=0), rng.standard_normal(96)]).astype(np.float32)
    chs = [cm.walk(yard.rowptr, yard.col, s) for s in (0, 1999)]
    worst = {"batch": 0.0, "loop": 0.0}
    _check("bfs order", lat, lat2, yard, P, chs, [None, [1.0, 0.5, 2.0, 0.7, 0.3]], 0.3, worst)
    lat.close()
    lat2.close()


def test_bit_identity_across_batches_passes_and_chunks(amd, monkeypatch):
    from oscillink_amd import _native

    inp = cm.inputs("c1_n80_d128_k8")
    lat = tcm._lattice(amd, inp, False)
    lat.settle(max_iters=12, tol=1e-3)
    rowptr, col = inp["csr"][:2]
    N, D = inp["Y"].shape
    rng = np.random.default_rng(21)
    Q = _native.OSC_QUERY_CHUNK + 44
    P = rng.standard_normal((Q, D)).astype(np.float32)
    chains, weights = [], []
    for q in range(Q):
        w = cm.walk(rowptr, col, q % N, 2 + q % 8)
        chains.append(cm.mixed(w) if q % 16 == 3 and len(w) >= 3 else w)
        weights.append([0.5 + 0.125 * ((q + t) % 9) for t in range(len(chains[-1]) - 1)] if q % 3 == 0 else None)
    assert {len(set(c)) for c in chains} >= set(range(2, 10))
    kw = dict(lamP=0.35, as_arrays=True)
    per_q = ("deltaH", "coh_drop_sum", "anchor_pen_sum", "query_term_sum", "null_total", "chain_prior_res", "chain_prior_iters")

    def same(a, qa, b, qb):
        for key in per_q:
            if a[key][qa].tobytes() != b[key][qb].tobytes():
                return key
        sa, ea = int(a["null_offsets"][qa]), int(a["null_offsets"][qa + 1])
        sb, eb = int(b["null_offsets"][qb]), int(b["null_offsets"][qb + 1])
        for key in ("null_i", "null_j", "null_z", "null_r"):
            if a[key][sa:ea].tobytes() != b[key][sb:eb].tobytes():
                return key
        return None

    big = lat.receipt_many(P, chains=chains, chain_weights=weights, **kw)
    assert np.all(big["chain_prior_res"] <= TOL) and int(big["null_total"].sum()) > 0
    solves = lat.shifted_basis_solves
    for q in (0, 5, _native.OSC_QUERY_CHUNK - 1, _native.OSC_QUERY_CHUNK, Q - 1):
        one = lat.receipt_many(P[q:q + 1], chains=[chains[q]], chain_weights=[weights[q]], **kw)
        assert same(one, 0, big, q) is None, (q, same(one, 0, big, q))
    back = lat.receipt_many(P[::-1].copy(), chains=chains[::-1], chain_weights=weights[::-1], **kw)
    for q in range(Q):
        assert same(back, Q - 1 - q, big, q) is None, (q, same(back, Q - 1 - q, big, q))
    shared = lat.receipt_many(P, chains=chains[6], chain_weights=weights[6], **kw)
    repeated = lat.receipt_many(P, chains=[chains[6]] * Q, chain_weights=[weights[6]] * Q, **kw)
    assert weights[6] is not None
    assert all(shared[key].tobytes() == repeated[key].tobytes() for key in shared)
    assert same(shared, 6, big, 6) is None
    # a forced small pass: at most 8 panel columns a pass (a chain here has at most 9 distinct nodes: such a pass is one query)
    monkeypatch.setenv("OSC_CHAIN_PRIOR_COLS", "8")
    small = lat.receipt_many(P[:60], chains=chains[:60], chain_weights=weights[:60], **kw)
    monkeypatch.delenv("OSC_CHAIN_PRIOR_COLS")
    for q in range(60):
        assert same(small, q, big, q) is None, (q, same(small, q, big, q))
    assert lat.shifted_basis_solves == solves  # the resident shifted basis served all of it
    lat.close()


@pytest.mark.parametrize("order", ["receipt first", "receipt last"])
def test_leaves_state_alone_and_shares_the_shifted_slot(amd, order):
    inp = cm.inputs("gates_chain_n333_d50_k7")
    lat = tcm._lattice(amd, inp, False)
    lat.settle(max_iters=12, tol=1e-3)
    lat.solve_Ustar()  # a resident U* and its signature
    P = _batch(inp["Y"], inp["psi"])
    chain = cm.chains(inp)["walk"]
    plain0 = lat.receipt_many(P, as_arrays=True)
    if order == "receipt last":
        lat.chain_receipt_many(P, chain, lamP=0.3, as_arrays=True)
        lat.bundle_many(P, k=8, chains=chain, lamP=0.3, as_arrays=True)
        assert lat.shifted_basis_solves == 1
    events = []
    lat.set_logger(lambda ev, payload: events.append((ev, payload)))
    st0, psi0, U0, sig0, key0 = dict(lat.stats), lat.psi.copy(), lat.U.copy(), lat._Ustar_sig, lat._qb_key
    lu0, last0, hist0 = dict(lat.last_ustar), dict(lat.last), list(lat.residual_history())
    assert sig0 is not None and key0 is not None
    a = lat.receipt_many(P, chains=chain, lamP=0.3, as_arrays=True)
    assert lat.shifted_basis_solves == 1
    b = lat.receipt_many(P, chains=[chain] * P.shape[0], lamP=0.3)
    assert [r["deltaH_total"] for r in b] == a["deltaH"].tolist()
    assert [ev for ev, pl in events if ev == "receipt_many" and pl.get("lamP") == 0.3]
    if order == "receipt first":
        lat.chain_receipt_many(P, chain, lamP=0.3, as_arrays=True)
        lat.bundle_many(P, k=8, chains=chain, lamP=0.3, as_arrays=True)
        assert lat.shifted_basis_solves == 1
    assert lat.stats == st0 and np.array_equal(lat.psi, psi0) and np.array_equal(lat.U, U0)
    assert lat._Ustar_sig == sig0 and lat._qb_key == key0 and lat.last_ustar == lu0 and lat.last == last0
    assert list(lat.residual_history()) == hist0
    assert a["deltaH"].tobytes() != plain0["deltaH"].tobytes()  # the prior is in the answer
    plain1 = lat.receipt_many(P, as_arrays=True)
    assert all(plain0[key].tobytes() == plain1[key].tobytes() for key in plain0)
    zero = lat.receipt_many(P, chains=chain, lamP=0.0, as_arrays=True)
    assert all(plain0[key].tobytes() == zero[key].tobytes() for key in plain0)
    assert np.all(zero["chain_prior_iters"] == 0) and np.all(zero["chain_prior_res"] <= TOL)
    assert lat.shifted_basis_solves == 1 and lat.stats["query_basis_solves"] == st0["query_basis_solves"]
    assert not [ev for ev, _ in events if ev in ("shifted_basis_solve", "query_basis_solve")][order == "receipt first":]
    assert not [ev for ev, _ in events if ev == "chain_prior_convergence_warn"]
    zrec = lat.receipt_many(P[:2], chains=chain, lamP=0.0)
    assert zrec[0]["meta"]["ustar_source"] == "chain_prior_basis" and zrec[0]["meta"]["state_sig"] != \
        lat.receipt_many(P[:2])[0]["meta"]["state_sig"]
    lat.add_chain(chain, lamP=0.2)
    with pytest.raises(ValueError, match="clear_chain"):
        lat.receipt_many(P, chains=chain, lamP=0.2)
    lat.clear_chain()
    assert lat.receipt_many(np.zeros((0, P.shape[1]), np.float32), chains=[], lamP=0.2) == []
    lat.close()


def test_reference_answer(amd):
    """The reference's own answer for the request add_chain(recipe chain, recipe lamP); set_query(psi); receipt() at the
    fixture's recorded state U: its recorded deltaH, sums, state signature and null-point edge list, from a lattice that
    carries no chain."""
    from tests._cases import load_case

    name = "g1_n400_d64_k6_chain8"
    inp = cm.inputs(name)
    case = load_case(name)
    assert inp["chain"] and inp["lamP"] > 0
    lat = tcm._lattice(amd, inp, False)
    lat.U = case["U"]
    yard = Yard(lat, inp["Y"])
    chain = [int(c) for c in inp["chain"]]
    got = lat.receipt_many(inp["psi"][None, :], chains=chain, lamP=float(inp["lamP"]))[0]
    want = _want(yard, case["U"].astype(np.float64), inp["psi"], chain, None, float(inp["lamP"]))
    ref = {"deltaH": float(case["deltaH"]), **{k: float(case[k]) for k in SUMS}}
    d = _dev(got, ref)
    print("reference answer: " + ", ".join(f"{k} {v:.3g}" for k, v in d.items()))
    assert all(v <= REL for v in d.values()), d
    assert got["meta"]["state_sig"] == str(case["state_sig"])
    ref_edges = {int(i): int(j) for i, j in case["null_edges"]}
    assert len(ref_edges) == int(case["n_nulls"])
    mine = yr.null_edges(got["null_points"])
    diff = sorted(i for i in set(mine) | set(ref_edges) if mine.get(i) != ref_edges.get(i))
    assert all(want["margin"][i] < NEAR for i in diff) and len(diff) <= NEAR_SHARE * lat.N, diff[:5]
    lat.close()

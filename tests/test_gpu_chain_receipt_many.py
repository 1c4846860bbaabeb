"""Multi-query chain receipts: `chain_receipt_many` against the float64 yardstick on the exact dense
U*(psi_q) (tests/_chain_many.py), this library's own per-query loop (`set_query(psi); chain_receipt(chain, z_th)`) and itself
(batch composition, chunking, the shared-chain form, state).

Tolerances are tests/test_gpu_refine_chains.check_chain's: z within 1e-4 (|R_ij| + |mu_i|) / sigma_i of the reference's value,
r within 1e-4 relative, the gain within 1e-4 of the sum of the magnitudes it adds up, the verdict equal, the weakest link's k
equal unless the top-two gap is below 1e-3 (on gates_chain's own chain [5, 9, 2, 9, 40] the gap is 1e-13 by construction).
tests/test_chain_many_host.py proves on the CPU that no edge's max(z) of the fixture cases is closer than 1 % to a threshold.
Measured on the CPU: solving U* by CG at tol 1e-4 instead of exactly moves z by at most 4e-6 of its bound, r by at most 4e-6
relative and the gain by at most 1.1e-7 of its magnitude, so the 1e-4 bounds leave 25 x over what the solve contributes."""
import numpy as np
import pytest

from tests import _chain_many as cm
from tests import test_gpu_receipt_many as trm
from tests import test_gpu_refine_chains as trc

pytestmark = pytest.mark.gpu

KEYS = trc.CHAIN_KEYS
REL = 1e-4


@pytest.fixture(scope="module")
def amd():
    import oscillink_amd
    from oscillink_amd import _native

    assert _native.device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return oscillink_amd


def _lattice(amd, inp, own):
    lat = amd.Oscillink(inp["Y"], **inp["kw"])
    lat.set_query(inp["psi"], gates=inp["gates"])
    if own:
        ch, ws, lamP = cm.own_chain(inp)
        lat.add_chain(ch, lamP=lamP, weights=ws)
    return lat


def _loop(lat, P, chain, z_ths, ustar=False):
    """the per-query path at every threshold (one U* solve per query); psi restored afterwards"""
    psi0 = lat.psi.copy()
    out = []
    for q in range(P.shape[0]):
        lat.set_query(P[q])
        rec = {z_th: lat.chain_receipt(chain, z_th) for z_th in z_ths}
        if ustar:
            rec["Us"] = lat.solve_Ustar().copy()
        out.append(rec)
    lat.set_query(psi0)
    return out


def check_yardstick(tag, q, arr, chain, y, z_th):
    """query q's arrays against the float64 yardstick; the worst deviations in units of their bounds"""
    s, e = int(arr["chain_offsets"][q]), int(arr["chain_offsets"][q + 1])
    assert e - s == len(chain) - 1
    worst = {"z": 0.0, "r": 0.0}
    for name in ("struct", "path"):
        gz, gr = arr["chain_z_" + name][s:e].astype(np.float64), arr["chain_r_" + name][s:e].astype(np.float64)
        wz, wr, bound = y["z_" + name], y["r_" + name], REL * y["bound_" + name]
        worst["z"] = max(worst["z"], float(np.max(np.abs(gz - wz) / np.maximum(bound, 1e-300))))
        worst["r"] = max(worst["r"], float(np.max(np.abs(gr - wr) / np.maximum(REL * np.abs(wr), 1e-300))))
        assert np.all(np.abs(gz - wz) <= bound), (tag, q, name, gz.tolist(), wz.tolist(), bound.tolist())
        assert np.all(np.abs(gr - wr) <= REL * np.abs(wr)), (tag, q, name, gr.tolist(), wr.tolist())
    gain = float(arr["chain_gain"][q])
    worst["gain"] = abs(gain - y["gain"]) / max(REL * y["gain_magnitude"], 1e-300)
    assert abs(gain - y["gain"]) <= REL * y["gain_magnitude"], (tag, q, gain, y["gain"], y["gain_magnitude"])
    assert bool(arr["chain_verdict"][q]) == bool(np.all(y["zmax"] <= z_th)), (tag, q, z_th, y["zmax"].tolist())
    wk, wz = cm.weakest(y["zmax"])
    k = int(arr["chain_weakest_k"][q])
    assert abs(float(arr["chain_weakest_z"][q]) - wz) <= REL * abs(wz), (tag, q, float(arr["chain_weakest_z"][q]), wz)
    assert 0 <= k < e - s and abs(y["zmax"][k] - wz) <= REL * abs(wz), (tag, q, k, y["zmax"].tolist())
    top = np.sort(y["zmax"])[::-1]
    if len(top) == 1 or top[0] - top[1] > 1e-3 * abs(top[0]):
        assert k == wk, (tag, q, k, wk, y["zmax"].tolist())
    return worst


def check_loop(tag, q, arr, chain, loop_rec, y, dct):
    """... and against the loop's dict, with the dict form (test_gpu_refine_chains.check_chain)"""
    trc.check_chain(tag, q, arr, chain, {"chain": loop_rec, "y64": y}, {"chain_receipt": dct})
    assert list(dct) == list(loop_rec) and list(dct["weakest_link"]) == list(loop_rec["weakest_link"])


def check_dtypes(arr, Q, n_edges):
    assert set(arr) == set(KEYS)
    assert arr["chain_offsets"].dtype == np.int64 and arr["chain_offsets"].shape == (Q + 1,)
    assert arr["chain_gain"].dtype == np.float64 and arr["chain_verdict"].dtype == np.bool_
    assert arr["chain_weakest_k"].dtype == np.int32 and arr["chain_weakest_z"].dtype == np.float32
    assert all(arr[k].dtype == np.float32 and arr[k].shape == (n_edges,) for k in trc.EDGE_KEYS)
    assert all(arr[k].shape == (Q,) for k in KEYS[5:])


@pytest.mark.parametrize("own", [False, True], ids=["plain", "own"])
@pytest.mark.parametrize("name", cm.FIXTURES)
def test_fixtures_against_yardstick_and_loop(amd, name, own):
    inp = cm.inputs(name)
    lat = _lattice(amd, inp, own)
    rowptr, col, a, _, sd = lat.graph_csr()
    assert np.array_equal(rowptr, inp["csr"][0]) and np.array_equal(col, inp["csr"][1])  # the chains the CPU proof covers
    y = cm.Yardstick(inp, own, csr=(rowptr, col, a), sqrt_deg=sd)
    P = cm.queries(inp)
    Q = P.shape[0]
    worst = {"z": 0.0, "r": 0.0, "gain": 0.0}
    for cname, chain in cm.chains(inp).items():
        loop = _loop(lat, P, chain, cm.Z_THS)
        y64 = [y.chain(P[q], chain) for q in range(Q)]
        for z_th in cm.Z_THS:
            arr = lat.chain_receipt_many(P, chain, z_th, as_arrays=True)
            dcts = lat.chain_receipt_many(P, chain, z_th)
            check_dtypes(arr, Q, Q * (len(chain) - 1))
            assert len(dcts) == Q
            for q in range(Q):
                tag = f"{name}/{'own' if own else 'plain'}/{cname}/z_th {z_th}"
                w = check_yardstick(tag, q, arr, chain, y64[q], z_th)
                worst = {k: max(worst[k], w[k]) for k in worst}
                check_loop(tag, q, arr, chain, loop[q][z_th], y64[q], dcts[q])
    print(f"{name} {'own' if own else 'plain'}: worst deviation from the yardstick in units of the bound: z {worst['z']:.3g}, "
          f"r {worst['r']:.3g}, gain {worst['gain']:.3g}")
    lat.close()


def test_leaves_state_alone(amd):
    inp = cm.inputs("gates_chain_n333_d50_k7")
    lat = _lattice(amd, inp, True)
    lat.settle(max_iters=12, tol=1e-3)
    lat.chain_receipt(inp["chain"])  # a resident U* and its signature
    events = []
    lat.set_logger(lambda ev, payload: events.append((ev, payload)))
    P = cm.queries(inp)
    chain = cm.chains(inp)["walk"]
    st0, psi0, U0, sig0, lu0, last0 = dict(lat.stats), lat.psi.copy(), lat.U.copy(), lat._Ustar_sig, dict(lat.last_ustar), dict(lat.last)
    assert sig0 is not None
    a = lat.chain_receipt_many(P, chain, as_arrays=True)
    assert lat.stats["query_basis_solves"] == st0["query_basis_solves"] + 1
    b = lat.chain_receipt_many(P, [chain] * P.shape[0])
    assert lat.stats["query_basis_solves"] == st0["query_basis_solves"] + 1  # a second call solves no basis
    for key in ("ustar_solves", "ustar_cache_hits"):
        assert lat.stats[key] == st0[key], key
    assert np.array_equal(lat.psi, psi0) and np.array_equal(lat.U, U0) and lat._Ustar_sig == sig0
    assert lat.last_ustar == lu0 and lat.last == last0
    mine = [p for ev, p in events if ev == "chain_receipt_many"]
    assert mine == [{"Q": 6, "edges": 30, "basis_solved": True}, {"Q": 6, "edges": 30, "basis_solved": False}]
    assert [d["coherence_gain"] for d in b] == a["chain_gain"].tolist()
    hits = lat.stats["ustar_cache_hits"]
    lat.chain_receipt(inp["chain"])  # the lattice's own U* is still the resident one
    assert lat.stats["ustar_solves"] == st0["ustar_solves"] and lat.stats["ustar_cache_hits"] == hits + 1
    lat.receipt_many(P[:2])  # ... and the basis serves the other batched calls
    assert lat.stats["query_basis_solves"] == st0["query_basis_solves"] + 1


def per_query(arr, q):
    s, e = int(arr["chain_offsets"][q]), int(arr["chain_offsets"][q + 1])
    return {k: arr[k][s:e].tobytes() if k in trc.EDGE_KEYS else arr[k][q:q + 1].tobytes() for k in KEYS[1:]}


def test_batch_composition_and_chunking(amd):
    from oscillink_amd import _native

    inp = cm.inputs("c1_n80_d128_k8")
    lat = _lattice(amd, inp, False)
    rowptr, col = inp["csr"][:2]
    N, D = inp["Y"].shape
    rng = np.random.default_rng(21)
    Q = _native.OSC_QUERY_CHUNK + 44
    P = rng.standard_normal((Q, D)).astype(np.float32)
    chains = []
    for q in range(Q):  # lengths 2 to 9; every sixteenth chain with a self-step, a revisited edge and a non-edge
        w = cm.walk(rowptr, col, q % N, 2 + q % 8)
        chains.append(cm.mixed(w) if q % 16 == 3 else w)
    assert {len(c) for c in chains} == set(range(2, 10))
    big = lat.chain_receipt_many(P, chains, as_arrays=True)
    assert big["chain_offsets"].tolist() == np.concatenate([[0], np.cumsum([len(c) - 1 for c in chains])]).tolist()
    check_dtypes(big, Q, sum(len(c) - 1 for c in chains))
    for q in (0, 5, _native.OSC_QUERY_CHUNK - 1, _native.OSC_QUERY_CHUNK, Q - 1):
        assert per_query(lat.chain_receipt_many(P[q:q + 1], [chains[q]], as_arrays=True), 0) == per_query(big, q), q
    back = lat.chain_receipt_many(P[::-1].copy(), chains[::-1], as_arrays=True)
    for q in range(Q):
        assert per_query(back, Q - 1 - q) == per_query(big, q), q
    shared = lat.chain_receipt_many(P, chains[7], as_arrays=True)
    repeated = lat.chain_receipt_many(P, [chains[7]] * Q, as_arrays=True)
    for key in KEYS:
        assert shared[key].tobytes() == repeated[key].tobytes(), key
    assert per_query(shared, 7) == per_query(big, 7)
    dcts = lat.chain_receipt_many(P, chains)
    for q in range(Q):
        s = int(big["chain_offsets"][q])
        d = dcts[q]
        assert d["verdict"] == bool(big["chain_verdict"][q]) and d["coherence_gain"] == float(big["chain_gain"][q])
        k = int(big["chain_weakest_k"][q])
        assert d["weakest_link"] == {"k": k, "edge": [chains[q][k], chains[q][k + 1]] if k >= 0 else [-1, -1],
                                     "zscore": float(big["chain_weakest_z"][q])}
        assert [(ed["k"], ed["edge"]) for ed in d["edges"]] == [(t, [chains[q][t], chains[q][t + 1]]) for t in range(len(chains[q]) - 1)]
        for t, ed in enumerate(d["edges"]):
            assert [ed[n] for n in ("z_struct", "z_path", "r_struct", "r_path")] == [float(big["chain_" + n][s + t]) for n in ("z_struct", "z_path", "r_struct", "r_path")]


def _against_loop(tag, lat, Y, P, chain, z_th=2.5):
    """the batch against the loop at check_chain's tolerances, the bounds from the loop's own U* rows (no dense solve)"""
    arr = lat.chain_receipt_many(P, chain, z_th, as_arrays=True)
    dcts = lat.chain_receipt_many(P, chain, z_th)
    loop = _loop(lat, P, chain, (z_th,), ustar=True)
    rowptr, col, a, _, sd = lat.graph_csr()
    path = (lat._chain_nodes, lat._chain_weights) if lat._chain_nodes is not None else (chain, None)
    for q in range(P.shape[0]):
        y = cm.chain_yardstick_rows(loop[q]["Us"], Y, (rowptr, col, a), sd, lat.lamC, path, chain)
        check_loop(tag, q, arr, chain, loop[q][z_th], y, dcts[q])
    return arr


@pytest.mark.parametrize("route", ["small", "mid", "clustered"])
def test_routes_against_loop(amd, route, monkeypatch):
    N, D, clustered = {"small": (300, 32, False), "mid": (4000, 64, False), "clustered": (12000, 64, True)}[route]
    if clustered:
        monkeypatch.setenv("OSC_REORDER", "1")
    lat, Y = trm._route_lattice(amd, N, D, clustered)
    if clustered:
        assert lat.build_info()["reordered"]
    rng = np.random.default_rng(8)
    P = np.stack([Y[:32].mean(axis=0), rng.standard_normal(D), Y[17], rng.uniform(-1, 1, D)]).astype(np.float32)
    rowptr, col = lat.graph_csr()[:2]
    for start in (0, N - 1):
        chain = cm.walk(rowptr, col, start)
        assert len(chain) == 6
        _against_loop(f"{route}/from {start}", lat, Y, P, chain)
        assert lat.last_query_basis["converged"]
    if route == "mid":  # the longest chain: 1024 nodes of a random walk with revisits
        long = [0]
        while len(long) < 1024:
            nb = col[rowptr[long[-1]]: rowptr[long[-1] + 1]]
            long.append(int(nb[rng.integers(nb.size)]))
        arr = _against_loop("mid/1024 nodes", lat, Y, P[:2], long)
        assert arr["chain_offsets"].tolist() == [0, 1023, 2046]
        lat.add_chain(cm.walk(rowptr, col, 5), lamP=0.3, weights=[1.0, 0.5, 2.0, 0.7, 0.3])  # a chain of its own, re-ordered rows or not
        _against_loop("mid/own chain", lat, Y, P[:2], cm.walk(rowptr, col, 0))
    if clustered:
        lat.add_chain(cm.walk(rowptr, col, 0)[::-1], lamP=0.3, weights=[1.0, 0.5, 2.0, 0.7, 0.3])
        _against_loop("clustered/own chain", lat, Y, P[:2], cm.walk(rowptr, col, 0))
    lat.close()


def test_edges_of_the_row_loop(amd):
    rng = np.random.default_rng(13)
    # a row without neighbours, and a chain through it
    Y = rng.standard_normal((40, 19)).astype(np.float32)
    lat = amd.Oscillink(Y, kneighbors=4, deterministic_k=True)
    rowptr, col, a = lat.graph_csr()[:3]
    keep = (np.repeat(np.arange(40), np.diff(rowptr)) != 3) & (col != 3)
    cnt = np.bincount(np.repeat(np.arange(40), np.diff(rowptr))[keep], minlength=40)
    lat.set_graph_csr(np.concatenate([[0], np.cumsum(cnt)]), col[keep], a[keep])
    rp2, col2 = lat.graph_csr()[:2]
    assert rp2[4] == rp2[3]
    w = cm.walk(rp2, col2, 0, 3)
    P = rng.standard_normal((3, 19)).astype(np.float32)
    arr = _against_loop("isolated row", lat, Y, P, w + [3, 3, w[0]])
    s = int(arr["chain_offsets"][1])
    assert arr["chain_r_struct"][s + 2: s + 5].tolist() == [0.0, 0.0, 0.0] and arr["chain_z_struct"][s + 3] == 0.0
    _against_loop("two nodes", lat, Y, P, [w[0], w[1]])
    _against_loop("two nodes, no edge", lat, Y, P, [3, 3])
    lat.close()
    # 7 rows, kneighbors 6, every row on the chain; max(z) <= sqrt(6) < 2.5 whatever the data
    Y7 = rng.standard_normal((7, 5)).astype(np.float32)
    lat = amd.Oscillink(Y7, kneighbors=6, deterministic_k=True)
    P7 = rng.standard_normal((3, 5)).astype(np.float32)
    arr = _against_loop("all7", lat, Y7, P7, [6, 0, 1, 2, 3, 4, 5])
    assert arr["chain_verdict"].tolist() == [True] * 3
    lat.close()


def test_errors(amd):
    inp = cm.inputs("c1_n80_d128_k8")
    lat = _lattice(amd, inp, False)
    N, D = inp["Y"].shape
    P = cm.queries(inp)
    ok = [0, 1, 2]
    for bad in ([0, -1], [0, N], [[0, 1]] * 5 + [[0, N]]):
        with pytest.raises(ValueError, match="out of bounds"):
            lat.chain_receipt_many(P, bad)
    with pytest.raises(ValueError, match="at least two"):
        lat.chain_receipt_many(P, [5])
    with pytest.raises(ValueError, match="at most 1024"):
        lat.chain_receipt_many(P, [0, 1] * 512 + [0])
    with pytest.raises(ValueError, match="hold 6 chains"):
        lat.chain_receipt_many(P, [ok] * 5)
    with pytest.raises(ValueError):
        lat.chain_receipt_many(np.zeros((3, D + 1), np.float32), ok)
    with pytest.raises(ValueError):
        lat.chain_receipt_many(np.zeros(D, np.float32), ok)
    assert lat.stats["query_basis_solves"] == 0
    assert lat.chain_receipt_many(np.zeros((0, D), np.float32), ok) == []
    assert lat.chain_receipt_many(np.zeros((0, D), np.float32), []) == []
    empty = lat.chain_receipt_many(np.zeros((0, D), np.float32), [], as_arrays=True)
    check_dtypes(empty, 0, 0)
    assert empty["chain_offsets"].tolist() == [0] and lat.stats["query_basis_solves"] == 0
    # the C entry point's own checks
    import ctypes as C
    from oscillink_amd import _native as nat

    z = np.zeros(8, np.float32)
    g, iv = np.zeros(2, np.float64), np.zeros(2, np.int32)

    def raw(offsets, nodes, Q=1):
        return nat.lib().osc_chain_receipt_many(lat._h, nat.f32(P), Q, nat.i64(np.asarray(offsets, np.int64)),
                                                nat.i32(np.asarray(nodes, np.int32)), 2.5, nat.f32(z), nat.f32(z), nat.f32(z),
                                                nat.f32(z), g.ctypes.data_as(C.POINTER(C.c_double)), nat.i32(iv), nat.i32(iv),
                                                nat.f32(z[:2]))

    assert raw([0, 2], [0, 1]) == nat.OSC_E_STATE  # no basis yet
    good = lat.chain_receipt_many(P, ok, as_arrays=True)
    assert raw([0, 2], [0, 1]) == nat.OSC_OK
    for offsets, nodes in (([0, 2], [0, N]), ([0, 2], [-1, 0]), ([0, 1], [0, 1]), ([1, 3], [0, 1, 2]), ([0, 2, 3], [0, 1, 2])):
        assert raw(offsets, nodes, Q=len(offsets) - 1) == nat.OSC_E_INVALID, (offsets, nodes)
    # a query row with a NaN changes no other query's bytes
    bad = P.copy()
    bad[2, 7] = np.nan
    got = lat.chain_receipt_many(bad, ok, as_arrays=True)
    for q in range(P.shape[0]):
        if q != 2:
            assert per_query(got, q) == per_query(good, q), q
    s, e = int(got["chain_offsets"][2]), int(got["chain_offsets"][3])
    assert np.all(np.isnan(got["chain_z_struct"][s:e])) and not bool(got["chain_verdict"][2])
    assert int(got["chain_weakest_k"][2]) == -1 and float(got["chain_weakest_z"][2]) == -1.0
    assert lat.chain_receipt_many(bad, ok)[2]["weakest_link"] == {"k": -1, "edge": [-1, -1], "zscore": -1.0}
    lat.close()

    from oscillink_amd.sharding import run_loopback_ranks

    def rank(r, comm):
        l2 = amd.Oscillink(inp["Y"], kneighbors=8, deterministic_k=True, comm=comm)
        try:
            l2.chain_receipt_many(np.ones((1, D), np.float32), ok)
        except NotImplementedError:
            return "refused"
        return "ran"

    assert run_loopback_ranks(2, rank) == ["refused", "refused"]

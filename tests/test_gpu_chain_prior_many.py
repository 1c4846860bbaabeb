"""Per-query chain priors on a resident lattice: `chain_receipt_many(psis, chains, lamP=...)` against
the float64 yardstick -- chain_receipt's formulas on the exact dense U* of M + lamP L_path,q -- against this library's own loop
`add_chain(chain_q, lamP, weights_q); set_query(psi_q); chain_receipt(chain_q, z_th)` on a second lattice, and against itself
(batch composition, passes, chunks, state).

The bounds are tests/test_gpu_chain_receipt_many's, imported unchanged (REL = 1e-4): the implied U*_q meets the same stop test
as the loop's U*, `chain_prior_res <= tol` being that statement, so the batch owes the yardstick no more than the loop does."""
import numpy as np
import pytest

from tests import _chain_many as cm
from tests import _queries as yq
from tests import _refine_chains as rc
from tests import test_gpu_chain_receipt_many as tcm
from tests import test_gpu_receipt_many as trm

pytestmark = pytest.mark.gpu

KEYS = tcm.KEYS
PRIOR_KEYS = ("chain_prior_res", "chain_prior_iters")
LAMPS = (0.0, 0.2, 0.5)
TOL = 1e-4


@pytest.fixture(scope="module")
def amd():
    import oscillink_amd
    from oscillink_amd import _native

    assert _native.device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return oscillink_amd


def per_query(arr, q):
    out = tcm.per_query(arr, q)
    out.update({k: arr[k][q:q + 1].tobytes() for k in PRIOR_KEYS})
    return out


def _loop(lat2, P, chains, weights, lamP, z_ths, ustar=False):
    """the reference's pair per query on the second lattice: the chain in the operator, then its receipt"""
    out = []
    for q in range(P.shape[0]):
        lat2.add_chain(chains[q], lamP=lamP, weights=weights[q])
        lat2.set_query(P[q])
        rec = {z_th: lat2.chain_receipt(chains[q], z_th) for z_th in z_ths}
        if ustar:
            rec["Us"] = lat2.solve_Ustar().copy()
        out.append(rec)
    lat2.clear_chain()
    return out


class Dense:
    """the exact dense basis of M + lamP L_path per distinct (chain, weights, lamP) of a fixture, float64"""

    def __init__(self, inp, csr, sd):
        Y = inp["Y"]
        kw = inp["kw"]
        self.Y, self.N, self.csr, self.sd = Y, Y.shape[0], csr, sd
        self.A = cm.dense_adj(csr, self.N)
        self.lamG, self.lamC, self.lamQ = kw.get("lamG", 1.0), kw.get("lamC", 0.5), kw.get("lamQ", 4.0)
        self.B = np.ones(self.N, np.float32) if inp["gates"] is None else inp["gates"]
        self.cache = {}

    def basis(self, chain, weights, lamP):
        key = (tuple(chain), None if weights is None else tuple(weights), lamP)
        if key not in self.cache:
            Ap = rc.path_adjacency(self.N, chain, weights)
            d = Ap.astype(np.float64).sum(axis=1)
            dm = 1.0 / np.sqrt(np.maximum(d, 1e-12))
            Lp = np.eye(self.N) - (Ap * dm[:, None]) * dm[None, :]
            M = yq.dense_M(self.A, self.sd, self.B, self.lamG, self.lamC, self.lamQ, lamP, Lp)
            self.cache[key] = yq.basis(M, self.Y, self.B, self.lamG, self.lamQ)
        return self.cache[key]

    def yardstick(self, psi, chain, weights, lamP):
        X, x = self.basis(chain, weights, lamP)
        Us = X + x[:, None] * np.asarray(psi, np.float64)[None, :]
        return cm.chain_yardstick_rows(Us, self.Y, self.csr, self.sd, self.lamC, (chain, weights), chain)


def _cases(inp):
    ch = cm.chains(inp)
    a = ch["walk"][2]
    return {"walk": (ch["walk"], None), "mixed": (ch["mixed"], cm.OWN_WEIGHTS), "aa": ([a, a], None)}


def _check_prior(arr, Q, lamP, tag):
    assert arr["chain_prior_res"].dtype == np.float32 and arr["chain_prior_res"].shape == (Q,)
    assert arr["chain_prior_iters"].dtype == np.int32 and arr["chain_prior_iters"].shape == (Q,)
    assert np.all(arr["chain_prior_res"] <= TOL), (tag, arr["chain_prior_res"].tolist())
    if lamP > 0:
        assert np.all(arr["chain_prior_iters"] >= 1), (tag, arr["chain_prior_iters"].tolist())
    else:
        assert np.all(arr["chain_prior_iters"] == 0), (tag, arr["chain_prior_iters"].tolist())


@pytest.mark.parametrize("name", cm.FIXTURES)
def test_fixtures_against_yardstick_and_loop(amd, name):
    inp = cm.inputs(name)
    lat, lat2 = tcm._lattice(amd, inp, False), tcm._lattice(amd, inp, False)
    rowptr, col, a, _, sd = lat.graph_csr()
    dense = Dense(inp, (rowptr, col, a), sd)
    P = cm.queries(inp)
    Q = P.shape[0]
    cases = _cases(inp)
    # per query: the three chains in turn, weights on every other one
    names = [list(cases)[q % 3] for q in range(Q)]
    own_ch = [cases[n][0] for n in names]
    own_w = [cases[names[q]][1] if q < 3 else ([0.5 + 0.25 * t for t in range(len(own_ch[q]) - 1)] if q % 2 else None)
             for q in range(Q)]
    worst = {"z": 0.0, "r": 0.0, "gain": 0.0}
    worst_loop = {"z": 0.0, "r": 0.0, "gain": 0.0}
    for lamP in LAMPS:
        batches = [(f"shared {n}", [c] * Q, [w] * Q, dict(chains=c, chain_weights=w)) for n, (c, w) in cases.items()]
        batches.append(("per query", own_ch, own_w, dict(chains=own_ch, chain_weights=own_w)))
        for bname, chs, wts, kw in batches:
            loop = _loop(lat2, P, chs, wts, lamP, cm.Z_THS)
            y64 = [dense.yardstick(P[q], chs[q], wts[q], lamP) for q in range(Q)]
            for z_th in cm.Z_THS:
                arr = lat.chain_receipt_many(P, kw["chains"], z_th, lamP=lamP, chain_weights=kw["chain_weights"], as_arrays=True)
                dcts = lat.chain_receipt_many(P, kw["chains"], z_th, lamP=lamP, chain_weights=kw["chain_weights"])
                tag = f"{name}/lamP {lamP}/{bname}/z_th {z_th}"
                assert set(arr) == set(KEYS) | set(PRIOR_KEYS) and len(dcts) == Q
                _check_prior(arr, Q, lamP, tag)
                core = {k: arr[k] for k in KEYS}
                tcm.check_dtypes(core, Q, sum(len(c) - 1 for c in chs))
                for q in range(Q):
                    w = tcm.check_yardstick(tag, q, core, chs[q], y64[q], z_th)
                    worst = {k: max(worst[k], w[k]) for k in worst}
                    tcm.check_loop(tag, q, core, chs[q], loop[q][z_th], y64[q], dcts[q])
                    # the loop itself against the yardstick, in the same units
                    la = _loop_arrays(loop[q][z_th])
                    wl = tcm.check_yardstick(tag + "/loop", 0, la, chs[q], y64[q], z_th)
                    worst_loop = {k: max(worst_loop[k], wl[k]) for k in worst_loop}
    print(f"{name}: worst deviation from the yardstick in units of the bound: batch z {worst['z']:.3g}, r {worst['r']:.3g}, "
          f"gain {worst['gain']:.3g}; loop z {worst_loop['z']:.3g}, r {worst_loop['r']:.3g}, gain {worst_loop['gain']:.3g}")
    lat.close()
    lat2.close()


def _loop_arrays(rec):
    """a chain_receipt dict as one query's arrays"""
    ed = rec["edges"]
    f = lambda k: np.array([e[k] for e in ed], np.float32)  # noqa: E731
    return dict(chain_offsets=np.array([0, len(ed)], np.int64), chain_z_struct=f("z_struct"), chain_z_path=f("z_path"),
                chain_r_struct=f("r_struct"), chain_r_path=f("r_path"), chain_gain=np.array([rec["coherence_gain"]]),
                chain_verdict=np.array([rec["verdict"]]), chain_weakest_k=np.array([rec["weakest_link"]["k"]], np.int32),
                chain_weakest_z=np.array([rec["weakest_link"]["zscore"]], np.float32))


def _against_loop(tag, lat, lat2, Y, P, chs, wts, lamP, z_th=2.5):
    """the batch against the loop at check_chain's tolerances, the bounds from the loop's own U* rows (no dense solve)"""
    Q = P.shape[0]
    arr = lat.chain_receipt_many(P, chs, z_th, lamP=lamP, chain_weights=wts, as_arrays=True)
    dcts = lat.chain_receipt_many(P, chs, z_th, lamP=lamP, chain_weights=wts)
    wl = [None] * Q if wts is None else wts
    loop = _loop(lat2, P, chs, wl, lamP, (z_th,), ustar=True)
    rowptr, col, a, _, sd = lat.graph_csr()
    _check_prior(arr, Q, lamP, tag)
    for q in range(Q):
        y = cm.chain_yardstick_rows(loop[q]["Us"], Y, (rowptr, col, a), sd, lat.lamC, (chs[q], wl[q]), chs[q])
        tcm.check_loop(tag, q, {k: arr[k] for k in KEYS}, chs[q], loop[q][z_th], y, dcts[q])
    return arr


def _spread(rowptr, col, m, start=0):
    """m distinct nodes: a walk along the graph's edges from `start`, then the rows after it that are not on it"""
    w = cm.walk(rowptr, col, start)
    rest = [i for i in range(len(rowptr) - 1) if i not in set(w)]
    return (w + rest)[:m]


def test_smallest_shapes_that_can_break_the_kernels(amd):
    inp = cm.inputs("gates_chain_n333_d50_k7")  # N = 333: no multiple of 32, gates
    lat, lat2 = tcm._lattice(amd, inp, False), tcm._lattice(amd, inp, False)
    assert lat.N % 32 != 0
    rowptr, col = lat.graph_csr()[:2]
    Y, P = inp["Y"], cm.queries(inp)[:3]
    # 31 / 32 / 33 distinct nodes in one pass (the slab seam), as one chain and as chains that share nodes
    for m in (31, 32, 33):
        chain = _spread(rowptr, col, m)
        assert len(set(chain)) == m
        _against_loop(f"one chain of {m}", lat, lat2, Y, P, [chain] * 3, None, 0.3)
        parts = [chain[:12], chain[10:24], chain[22:] + chain[:2]]
        assert len(set(sum(parts, []))) == m
        arr = _against_loop(f"{m} nodes in three chains", lat, lat2, Y, P, parts, None, 0.3)
        for q in range(3):  # ... and each of them alone gives the same bytes
            alone = lat.chain_receipt_many(P[q:q + 1], [parts[q]], lamP=0.3, as_arrays=True)
            assert per_query(alone, 0) == per_query(arr, q), (m, q)
    # m = 64 with weights and a revisit; 65 is refused before any device work
    c64 = _spread(rowptr, col, 64, start=7)
    w64 = [0.25 + (t % 5) * 0.5 for t in range(64)]
    _against_loop("m = 64", lat, lat2, Y, P[:2], [c64 + [c64[0]]] * 2, [w64] * 2, 0.5)
    n0 = lat.shifted_basis_solves
    with pytest.raises(ValueError, match="at most 64 distinct"):
        lat.chain_receipt_many(P, _spread(rowptr, col, 65), lamP=0.9)
    assert lat.shifted_basis_solves == n0
    lat.close()
    lat2.close()


def test_isolated_node_and_m1(amd):
    rng = np.random.default_rng(13)
    Y = rng.standard_normal((40, 19)).astype(np.float32)
    lats = []
    for _ in range(2):
        lat = amd.Oscillink(Y, kneighbors=4, deterministic_k=True)
        rowptr, col, a = lat.graph_csr()[:3]
        keep = (np.repeat(np.arange(40), np.diff(rowptr)) != 3) & (col != 3)
        cnt = np.bincount(np.repeat(np.arange(40), np.diff(rowptr))[keep], minlength=40)
        lat.set_graph_csr(np.concatenate([[0], np.cumsum(cnt)]), col[keep], a[keep])
        lats.append(lat)
    lat, lat2 = lats
    rp2, col2 = lat.graph_csr()[:2]
    assert rp2[4] == rp2[3]
    w = cm.walk(rp2, col2, 0, 3)
    P = rng.standard_normal((3, 19)).astype(np.float32)
    _against_loop("isolated row", lat, lat2, Y, P, [w + [3, 3, w[0]]] * 3, None, 0.4)
    _against_loop("[3, 3]: m = 1 on the isolated row", lat, lat2, Y, P, [[3, 3]] * 3, None, 0.4)
    _against_loop("two nodes", lat, lat2, Y, P, [[w[0], w[1]]] * 3, [[2.0]] * 3, 0.4)
    lat.close()
    lat2.close()


def test_d768(amd):
    inp = cm.inputs("seed_n400_d768_k12")
    lat, lat2 = tcm._lattice(amd, inp, False), tcm._lattice(amd, inp, False)
    rowptr, col = lat.graph_csr()[:2]
    P = cm.queries(inp)[:3]
    chs = [cm.walk(rowptr, col, s) for s in (0, 100, 399)]
    _against_loop("D = 768", lat, lat2, inp["Y"], P, chs, [None, [1.0, 0.5, 2.0, 0.7, 0.3], None], 0.2)
    lat.close()
    lat2.close()


def test_bfs_permuted_lattice(amd, monkeypatch):
    from tests import _gated

    monkeypatch.setenv("OSC_REORDER", "1")
    Y = _gated.corpus(100, 8)[0]
    assert Y.shape == (2000, 96)
    lat = amd.Oscillink(Y, kneighbors=8, deterministic_k=True)
    lat2 = amd.Oscillink(Y, kneighbors=8, deterministic_k=True)
    assert lat.build_info()["reordered"]
    rng = np.random.default_rng(3)
    P = np.stack([Y[:32].mean(axis=0), rng.standard_normal(96), Y[17]]).astype(np.float32)
    rowptr, col = lat.graph_csr()[:2]
    chs = [cm.walk(rowptr, col, s) for s in (0, 1999, 1000)]
    _against_loop("bfs order", lat, lat2, Y, P, chs, None, 0.3)
    lat.close()
    lat2.close()


def test_route_clustered_12000(amd, monkeypatch):
    monkeypatch.setenv("OSC_REORDER", "1")
    lat, Y = trm._route_lattice(amd, 12000, 64, True)
    lat2, _ = trm._route_lattice(amd, 12000, 64, True)
    assert lat.build_info()["reordered"]
    rng = np.random.default_rng(8)
    P = np.stack([Y[:32].mean(axis=0), rng.standard_normal(64)]).astype(np.float32)
    rowptr, col = lat.graph_csr()[:2]
    chs = [cm.walk(rowptr, col, 0), cm.walk(rowptr, col, 11999)]
    _against_loop("clustered 12000", lat, lat2, Y, P, chs, [None, [1.0, 0.5, 2.0, 0.7, 0.3]], 0.3)
    assert lat.last_shifted_basis["converged"]
    lat.close()
    lat2.close()


def test_bit_identity_across_batches_passes_and_chunks(amd, monkeypatch):
    from oscillink_amd import _native

    inp = cm.inputs("c1_n80_d128_k8")
    lat = tcm._lattice(amd, inp, False)
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
    lamP = 0.35
    big = lat.chain_receipt_many(P, chains, lamP=lamP, chain_weights=weights, as_arrays=True)
    assert np.all(big["chain_prior_res"] <= TOL)
    solves = lat.shifted_basis_solves
    for q in (0, 5, _native.OSC_QUERY_CHUNK - 1, _native.OSC_QUERY_CHUNK, Q - 1):
        one = lat.chain_receipt_many(P[q:q + 1], [chains[q]], lamP=lamP, chain_weights=[weights[q]], as_arrays=True)
        assert per_query(one, 0) == per_query(big, q), q
    back = lat.chain_receipt_many(P[::-1].copy(), chains[::-1], lamP=lamP, chain_weights=weights[::-1], as_arrays=True)
    for q in range(Q):
        assert per_query(back, Q - 1 - q) == per_query(big, q), q
    shared = lat.chain_receipt_many(P, chains[6], lamP=lamP, chain_weights=weights[6], as_arrays=True)
    repeated = lat.chain_receipt_many(P, [chains[6]] * Q, lamP=lamP, chain_weights=[weights[6]] * Q, as_arrays=True)
    assert weights[6] is not None
    for key in KEYS + PRIOR_KEYS:
        assert shared[key].tobytes() == repeated[key].tobytes(), key
    assert per_query(shared, 6) == per_query(big, 6)
    # a forced small pass: at most 8 panel columns a pass (a chain here has at most 9 distinct nodes: such a pass is one query)
    monkeypatch.setenv("OSC_CHAIN_PRIOR_COLS", "8")
    small = lat.chain_receipt_many(P[:60], chains[:60], lamP=lamP, chain_weights=weights[:60], as_arrays=True)
    monkeypatch.delenv("OSC_CHAIN_PRIOR_COLS")
    for q in range(60):
        assert per_query(small, q) == per_query(big, q), q
    assert lat.shifted_basis_solves == solves  # the resident shifted basis served all of it
    # a non-finite query changes no other query's bytes
    bad = P[:6].copy()
    bad[2, 7] = np.nan
    got = lat.chain_receipt_many(bad, chains[:6], lamP=lamP, chain_weights=weights[:6], as_arrays=True)
    for q in range(6):
        if q != 2:
            assert per_query(got, q) == per_query(big, q), q
    s, e = int(got["chain_offsets"][2]), int(got["chain_offsets"][3])
    assert np.all(np.isnan(got["chain_z_struct"][s:e])) and not bool(got["chain_verdict"][2])
    lat.close()


def test_leaves_state_alone(amd):
    inp = cm.inputs("gates_chain_n333_d50_k7")
    lat = tcm._lattice(amd, inp, False)
    lat.settle(max_iters=12, tol=1e-3)
    lat.chain_receipt(cm.chains(inp)["walk"])  # a resident U* and its signature
    P = cm.queries(inp)
    chain = cm.chains(inp)["walk"]
    before = lat.chain_receipt_many(P, chain, as_arrays=True)
    events = []
    lat.set_logger(lambda ev, payload: events.append((ev, payload)))
    st0, psi0, U0, sig0, key0 = dict(lat.stats), lat.psi.copy(), lat.U.copy(), lat._Ustar_sig, lat._qb_key
    lu0, last0 = dict(lat.last_ustar), dict(lat.last)
    assert sig0 is not None and key0 is not None
    a = lat.chain_receipt_many(P, chain, lamP=0.3, as_arrays=True)
    assert lat.shifted_basis_solves == 1
    b = lat.chain_receipt_many(P, [chain] * P.shape[0], lamP=0.3)
    assert lat.shifted_basis_solves == 1  # a second call with the same lamP solves no basis
    assert [d["coherence_gain"] for d in b] == a["chain_gain"].tolist()
    assert list(b[0]) == list(lat.chain_receipt(chain))  # the dict form has chain_receipt's keys only
    after = lat.chain_receipt_many(P, chain, as_arrays=True)
    for key in KEYS:
        assert before[key].tobytes() == after[key].tobytes(), key
    assert set(after) == set(KEYS)
    hits = lat.stats["ustar_cache_hits"]
    assert lat.stats == {**st0, "ustar_cache_hits": hits} and hits == st0["ustar_cache_hits"] + 1  # (the chain_receipt above)
    assert np.array_equal(lat.psi, psi0) and np.array_equal(lat.U, U0) and lat._Ustar_sig == sig0 and lat._qb_key == key0
    assert lat.last_ustar == lu0 and lat.last == last0
    mine = [p for ev, p in events if ev == "chain_receipt_many"]
    assert mine == [{"Q": 6, "edges": 30, "basis_solved": True, "lamP": 0.3}, {"Q": 6, "edges": 30, "basis_solved": False, "lamP": 0.3},
                    {"Q": 6, "edges": 30, "basis_solved": False}]
    assert not [ev for ev, _ in events if ev == "chain_prior_convergence_warn"]
    assert lat.build_info()["shifted_basis_bytes"] > 0
    # lamP = 0: the resident unshifted basis, no Green's columns; with unit weights the bytes of the plain call
    zero = lat.chain_receipt_many(P, chain, lamP=0.0, as_arrays=True)
    for key in KEYS:
        assert zero[key].tobytes() == before[key].tobytes(), key
    assert lat.shifted_basis_solves == 1 and lat.stats["query_basis_solves"] == st0["query_basis_solves"]
    lat.close()


def test_errors(amd):
    inp = cm.inputs("c1_n80_d128_k8")
    lat = tcm._lattice(amd, inp, False)
    D = inp["Y"].shape[1]
    P = cm.queries(inp)
    ok = [0, 1, 2]
    with pytest.raises(ValueError, match="without lamP"):
        lat.chain_receipt_many(P, ok, chain_weights=[1.0, 1.0])
    with pytest.raises(ValueError, match="lamP must be >= 0"):
        lat.chain_receipt_many(P, ok, lamP=-0.1)
    with pytest.raises(ValueError, match="at most 64 distinct"):
        lat.chain_receipt_many(P, list(range(65)), lamP=0.2)
    with pytest.raises(ValueError, match="weights length"):
        lat.chain_receipt_many(P, ok, lamP=0.2, chain_weights=[1.0])
    with pytest.raises(ValueError, match="finite"):
        lat.chain_receipt_many(P, ok, lamP=0.2, chain_weights=[1.0, np.inf])
    with pytest.raises(ValueError, match="parallel to chains"):
        lat.chain_receipt_many(P, [ok] * 6, lamP=0.2, chain_weights=[[1.0, 1.0]] * 5)
    lat.chain_receipt_many(P, list(range(64)) + [0] * 100, lamP=0.2)  # 64 distinct nodes, repeats allowed
    lat.add_chain(ok, lamP=0.2)
    with pytest.raises(ValueError, match="clear_chain"):
        lat.chain_receipt_many(P, ok, lamP=0.2)
    lat.clear_chain()
    assert lat.chain_receipt_many(np.zeros((0, D), np.float32), [], lamP=0.2) == []
    empty = lat.chain_receipt_many(np.zeros((0, D), np.float32), [], lamP=0.2, as_arrays=True)
    assert empty["chain_prior_res"].shape == (0,) and empty["chain_prior_iters"].shape == (0,)
    lat.close()

    from oscillink_amd.sharding import run_loopback_ranks

    def rank(r, comm):
        l2 = amd.Oscillink(inp["Y"], kneighbors=8, deterministic_k=True, comm=comm)
        try:
            l2.chain_receipt_many(np.ones((1, D), np.float32), ok, lamP=0.2)
        except NotImplementedError as exc:
            return "refused" if "communicator (sharded / multi-rank) are not supported" in str(exc) else str(exc)
        return "ran"

    assert run_loopback_ranks(2, rank) == ["refused", "refused"]

"""Chain priors in bundle_many: `bundle_many(psis, k, alpha, chains=..., lamP=...)` against the float64
yardstick -- `yq.ustar` on the dense M + lamP L_path,q, then `yq.bundle` -- against this library's own loop
`add_chain(chain_q, lamP, weights_q); set_query(psi_q); bundle(k, alpha)` on a second lattice, and against itself (batch
composition, passes, chunks, state).

NEAR_TIE = 1e-4 and atol = 2e-4 are tests/test_gpu_bundle_many.py's.  At most a quarter of a test's queries may be cut short
by a near tie.  Where the loop itself is further than 2e-4 from the yardstick on a query, that query's bound is twice the
loop's deviation (the test prints where)."""
import numpy as np
import pytest

from tests import _bundle_prior as bp
from tests import _chain_many as cm
from tests import _queries as yq
from tests import test_gpu_chain_receipt_many as tcm
from tests.test_gpu_bundle_many import NEAR_TIE, _batch

pytestmark = pytest.mark.gpu

ATOL = 2e-4
TOL = 1e-4
K = 8


@pytest.fixture(scope="module")
def amd():
    import oscillink_amd
    from oscillink_amd import _native

    assert _native.device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return oscillink_amd


class Yard:
    """the float64 yardstick of a lattice without a chain of its own: its graph, gates and lambdas, dense"""

    def __init__(self, lat, Y):
        rowptr, col, a, _, sd = lat.graph_csr()
        self.Y, self.N = np.asarray(Y, np.float64), lat.N
        self.A, self.sd, self.B = cm.dense_adj((rowptr, col, a), lat.N), sd, np.asarray(lat.B_diag, np.float64)
        self.lamG, self.lamC, self.lamQ = lat.lamG, lat.lamC, lat.lamQ
        self.M = yq.dense_M(self.A, sd, self.B, self.lamG, self.lamC, self.lamQ)
        self.rowptr, self.col = rowptr, col

    def bundle(self, psi, chain, weights, lamP, k=K):
        Lp = bp.path_terms(self.N, chain, weights)[0]
        U = yq.ustar(self.M + lamP * Lp, self.Y, self.B, psi, self.lamG, self.lamQ)
        return yq.bundle(self.Y, U, psi, self.A, self.sd, self.lamC, k=k)


def _loop(lat2, P, chs, wts, lamP, k=K):
    out = []
    for q in range(P.shape[0]):
        lat2.add_chain(chs[q], lamP=lamP, weights=wts[q])
        lat2.set_query(P[q])
        bd = lat2.bundle(k=k, alpha=0.5)
        out.append(([b["id"] for b in bd], np.array([b["score"] for b in bd]), np.array([b["align"] for b in bd])))
    lat2.clear_chain()
    return out


class Tally:
    """near ties met by one test: at most a quarter of its queries may be cut short by one"""

    def __init__(self):
        self.truncated = self.queries = 0

    def check(self):
        assert 4 * self.truncated <= self.queries, (self.truncated, self.queries)


def _check(tag, lat, lat2, yard, P, chains, weights, lamP, *, tally, k=K):
    """the batch against the yardstick and the loop; returns (arrays, worst deviation of the batch, of the loop).  Every
    caller hands in its test's Tally and ends with `tally.check()`: the near-tie cap holds for every test of this file."""
    Q = P.shape[0]
    shared = bool(chains) and not isinstance(chains[0], (list, tuple))
    chs = [chains] * Q if shared else chains
    wts = [weights] * Q if shared or weights is None else weights
    ids, score, align = lat.bundle_many(P, k=k, alpha=0.5, chains=chains, lamP=lamP, chain_weights=weights, as_arrays=True)
    kk = min(k, lat.N)
    assert ids.shape == score.shape == align.shape == (Q, kk)
    assert ids.dtype == np.int32 and score.dtype == np.float32 and align.dtype == np.float32
    pr = lat.last_bundle_prior
    assert pr["lamP"] == lamP and pr["res"].dtype == np.float32 and pr["iters"].dtype == np.int32
    assert pr["res"].shape == (Q,) and np.all(pr["res"] <= TOL), (tag, pr["res"].tolist())
    assert np.all(pr["iters"] >= 1) if lamP > 0 else np.all(pr["iters"] == 0)
    loop = _loop(lat2, P, chs, wts, lamP, k) if lat2 is not None else None
    truncated, worst, worst_loop = 0, 0.0, 0.0
    for q in range(Q):
        w_ids, w_score, w_align, margins = yard.bundle(P[q], chs[q], wts[q], lamP, k)
        ok, cut = yq.same_until_near_tie(ids[q].tolist(), w_ids, margins, NEAR_TIE)
        assert ok, (tag, q, ids[q].tolist(), w_ids, margins)
        truncated += int(cut)
        n = len(w_ids) if not cut else next(t for t, m in enumerate(margins) if m < NEAR_TIE)
        bound = ATOL
        if loop is not None:
            l_ids, l_score, l_align = loop[q]
            okl, _ = yq.same_until_near_tie(ids[q].tolist(), l_ids, margins, NEAR_TIE)
            assert okl, (tag, q, ids[q].tolist(), l_ids, margins)
            nl = next((t for t in range(n) if l_ids[t] != w_ids[t]), n)
            dl = max(float(np.max(np.abs(l_score[:nl] - w_score[:nl]), initial=0.0)),
                     float(np.max(np.abs(l_align[:nl] - w_align[:nl]), initial=0.0)))
            worst_loop = max(worst_loop, dl)
            if dl > ATOL:
                bound = 2 * dl
                print(f"{tag}: query {q}: the loop is {dl:.3g} from the yardstick; bound {bound:.3g}")
        db = max(float(np.max(np.abs(score[q, :n] - w_score[:n]), initial=0.0)),
                 float(np.max(np.abs(align[q, :n] - w_align[:n]), initial=0.0)))
        print(f"{tag}: query {q}: batch {db:.3g} from the yardstick over {n} picks")
        worst = max(worst, db)
        assert db <= bound, (tag, q, db, bound)
    print(f"{tag}: {truncated} of {Q} id lists compared up to a near tie")
    tally.truncated += truncated
    tally.queries += Q
    return (ids, score, align), worst, worst_loop


def _own(yard, Q, n=6):
    """a chain per query walking the graph from different rows, weights on every other one"""
    chs = [cm.walk(yard.rowptr, yard.col, (37 * q) % yard.N, n) for q in range(Q)]
    chs[1] = cm.mixed(chs[1]) if len(chs[1]) >= 3 else chs[1]
    wts = [[0.5 + 0.25 * t for t in range(len(chs[q]) - 1)] if q % 2 else None for q in range(Q)]
    return chs, wts


@pytest.mark.parametrize("name", ["c1_n80_d128_k8", "g1_n400_d64_k6_chain8", "gates_chain_n333_d50_k7", "seed_n400_d768_k12"])
def test_fixtures_against_yardstick_and_loop(amd, name):
    inp = cm.inputs(name)
    lat, lat2 = tcm._lattice(amd, inp, False), tcm._lattice(amd, inp, False)  # (no chain of its own; gates kept)
    yard = Yard(lat, inp["Y"])
    P = _batch(inp["Y"], inp["psi"])
    Q = P.shape[0]
    assert Q == 7 and not P[6].any()
    w8 = bp.spread(yard.rowptr, yard.col, 8)
    chs, wts = _own(yard, Q)
    worst, worst_loop, tally = 0.0, 0.0, Tally()
    for lamP in (0.2, 0.5):
        for bname, c, w in (("shared", w8, None), ("shared weighted", w8, [1.0, 0.5, 2.0, 0.7, 0.3, 1.5, 0.25]),
                            ("per query", chs, wts)):
            _, wb, wl = _check(f"{name}/lamP {lamP}/{bname}", lat, lat2, yard, P, c, w, lamP, tally=tally)
            worst, worst_loop = max(worst, wb), max(worst_loop, wl)
    tally.check()
    print(f"{name}: worst deviation from the yardstick: batch {worst:.3g}, loop {worst_loop:.3g}")
    dicts = lat.bundle_many(P[:2], k=3, chains=w8, lamP=0.2)
    assert len(dicts) == 2 and all(list(b) == ["id", "score", "align"] for d in dicts for b in d) and len(dicts[0]) == 3
    lat.close()
    lat2.close()


def test_smallest_shapes_that_can_break_the_kernels(amd):
    inp = cm.inputs("gates_chain_n333_d50_k7")  # N = 333 (partial waves and workgroups), D = 50 (no multiple of 4), gates
    lat, lat2 = tcm._lattice(amd, inp, False), tcm._lattice(amd, inp, False)
    assert lat.N % 32 != 0 and inp["Y"].shape[1] % 4 != 0
    yard = Yard(lat, inp["Y"])
    P = _batch(inp["Y"], inp["psi"])[[0, 1, 3]]
    tally = Tally()
    # 31 / 32 / 33 distinct nodes in one pass (the panel's slab width), as one chain and as chains that share nodes
    for m in (31, 32, 33):
        chain = bp.spread(yard.rowptr, yard.col, m)
        assert len(set(chain)) == m
        _check(f"one chain of {m}", lat, lat2, yard, P, chain, None, 0.3, tally=tally)
        parts = [chain[:12], chain[10:24], chain[22:] + chain[:2]]
        assert len(set(sum(parts, []))) == m
        arr, _, _ = _check(f"{m} nodes in three chains", lat, None, yard, P, parts, None, 0.3, tally=tally)
        for q in range(3):  # ... and each of them alone gives the same bytes
            alone = lat.bundle_many(P[q:q + 1], k=K, chains=[parts[q]], lamP=0.3, as_arrays=True)
            assert all(a[0].tobytes() == b[q].tobytes() for a, b in zip(alone, arr)), (m, q)
    # m = 64 with weights and a revisit; m = 1; 65 is refused before any device work
    c64 = bp.spread(yard.rowptr, yard.col, 64, start=7)
    w64 = [0.25 + (t % 5) * 0.5 for t in range(64)]
    _check("m = 64", lat, lat2, yard, P[:2], c64 + [c64[0]], w64, 0.5, tally=tally)
    _check("m = 1", lat, lat2, yard, P, [c64[3], c64[3]], None, 0.5, tally=tally)
    tally.check()
    n0 = lat.shifted_basis_solves
    with pytest.raises(ValueError, match="at most 64 distinct"):
        lat.bundle_many(P, chains=bp.spread(yard.rowptr, yard.col, 65), lamP=0.9)
    assert lat.shifted_basis_solves == n0
    lat.close()
    lat2.close()


def test_k_at_least_n_and_lamc_zero(amd):
    inp = cm.inputs("c1_n80_d128_k8")  # N = 80: k >= N picks every row
    lat = tcm._lattice(amd, inp, False)
    yard = Yard(lat, inp["Y"])
    P = _batch(inp["Y"], inp["psi"])[:4]
    chain = bp.spread(yard.rowptr, yard.col, 8)
    tally = Tally()
    (ids, score, align), _, _ = _check("k >= N", lat, None, yard, P, chain, None, 0.2, k=100, tally=tally)
    tally.check()
    assert ids.shape == (4, 80) and all(sorted(ids[q].tolist()) == list(range(80)) for q in range(4))
    for q in range(4):  # every row is picked: score and align of each row against the yardstick's, by id
        w_ids, w_score, w_align, _ = yard.bundle(P[q], chain, None, 0.2, k=80)
        by = np.argsort(w_ids)
        mine = np.argsort(ids[q])
        assert np.allclose(score[q][mine], w_score[by], atol=ATOL, rtol=0) and np.allclose(align[q][mine], w_align[by], atol=ATOL, rtol=0)
    lat.close()
    inp = cm.inputs("lam_g03_c0_q0_n240_d40_k6")  # lamC = 0: M' is diagonal, the coherence term vanishes
    lat, lat2 = tcm._lattice(amd, inp, False), tcm._lattice(amd, inp, False)
    assert lat.lamC == 0
    yard = Yard(lat, inp["Y"])
    P = _batch(inp["Y"], inp["psi"])
    chs, wts = _own(yard, P.shape[0])
    tally = Tally()
    _check("lamC = 0", lat, lat2, yard, P, chs, wts, 0.5, tally=tally)
    tally.check()
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
        lats.append(lat)
    lat, lat2 = lats
    yard = Yard(lat, Y)
    assert yard.rowptr[4] == yard.rowptr[3]
    w = cm.walk(yard.rowptr, yard.col, 0, 3)
    P = rng.standard_normal((3, 19)).astype(np.float32)
    tally = Tally()
    _check("isolated row on the chain", lat, lat2, yard, P, w + [3, 3, w[0]], None, 0.4, tally=tally)
    _check("[3, 3]: m = 1 on the isolated row", lat, lat2, yard, P, [3, 3], None, 0.4, tally=tally)
    tally.check()
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
    yard = Yard(lat, Y)
    rng = np.random.default_rng(3)
    P = np.stack([Y[:32].mean(axis=0), rng.standard_normal(96)]).astype(np.float32)
    chs = [cm.walk(yard.rowptr, yard.col, s) for s in (0, 1999)]
    tally = Tally()
    _check("bfs order", lat, lat2, yard, P, chs, [None, [1.0, 0.5, 2.0, 0.7, 0.3]], 0.3, tally=tally)
    tally.check()
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
    kw = dict(k=K, lamP=lamP, as_arrays=True)

    def same(a, qa, b, qb):
        return all(x[qa].tobytes() == y[qb].tobytes() for x, y in zip(a, b))

    big = lat.bundle_many(P, chains=chains, chain_weights=weights, **kw)
    res_big = lat.last_bundle_prior["res"].copy()
    assert np.all(res_big <= TOL)
    solves = lat.shifted_basis_solves
    for q in (0, 5, _native.OSC_QUERY_CHUNK - 1, _native.OSC_QUERY_CHUNK, Q - 1):
        one = lat.bundle_many(P[q:q + 1], chains=[chains[q]], chain_weights=[weights[q]], **kw)
        assert same(one, 0, big, q), q
        assert lat.last_bundle_prior["res"].tobytes() == res_big[q:q + 1].tobytes()
    back = lat.bundle_many(P[::-1].copy(), chains=chains[::-1], chain_weights=weights[::-1], **kw)
    for q in range(Q):
        assert same(back, Q - 1 - q, big, q), q
    shared = lat.bundle_many(P, chains=chains[6], chain_weights=weights[6], **kw)
    repeated = lat.bundle_many(P, chains=[chains[6]] * Q, chain_weights=[weights[6]] * Q, **kw)
    assert weights[6] is not None
    assert all(x.tobytes() == y.tobytes() for x, y in zip(shared, repeated))
    assert same(shared, 6, big, 6)
    # a forced small pass: at most 8 panel columns a pass (a chain here has at most 9 distinct nodes: such a pass is one query)
    monkeypatch.setenv("OSC_CHAIN_PRIOR_COLS", "8")
    small = lat.bundle_many(P[:60], chains=chains[:60], chain_weights=weights[:60], **kw)
    monkeypatch.delenv("OSC_CHAIN_PRIOR_COLS")
    for q in range(60):
        assert same(small, q, big, q), q
    assert lat.shifted_basis_solves == solves  # the resident shifted basis served all of it
    lat.close()


def test_leaves_state_alone_and_shares_the_shifted_slot(amd):
    inp = cm.inputs("gates_chain_n333_d50_k7")
    lat = tcm._lattice(amd, inp, False)
    lat.settle(max_iters=12, tol=1e-3)
    lat.solve_Ustar()  # a resident U* and its signature
    P = _batch(inp["Y"], inp["psi"])
    chain = cm.chains(inp)["walk"]
    plain0 = lat.bundle_many(P, k=K, as_arrays=True)
    cr0 = lat.chain_receipt_many(P, chain, lamP=0.3, as_arrays=True)
    assert lat.shifted_basis_solves == 1
    bytes0 = lat.build_info()["shifted_basis_bytes"]
    events = []
    lat.set_logger(lambda ev, payload: events.append((ev, payload)))
    st0, psi0, U0, sig0, key0 = dict(lat.stats), lat.psi.copy(), lat.U.copy(), lat._Ustar_sig, lat._qb_key
    lu0, last0 = dict(lat.last_ustar), dict(lat.last)
    assert sig0 is not None and key0 is not None
    a = lat.bundle_many(P, k=K, chains=chain, lamP=0.3, as_arrays=True)
    assert lat.shifted_basis_solves == 1  # chain_receipt_many's basis, the same slot and key
    b = lat.bundle_many(P, k=K, chains=[chain] * P.shape[0], lamP=0.3)
    assert [[d["id"] for d in bq] for bq in b] == a[0].tolist()
    assert lat.stats == st0 and np.array_equal(lat.psi, psi0) and np.array_equal(lat.U, U0)
    assert lat._Ustar_sig == sig0 and lat._qb_key == key0 and lat.last_ustar == lu0 and lat.last == last0
    assert not any(x.tobytes() == y.tobytes() for x, y in zip(a[1:], plain0[1:]))  # the prior is in the answer
    plain1 = lat.bundle_many(P, k=K, as_arrays=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(plain0, plain1))
    cr1 = lat.chain_receipt_many(P, chain, lamP=0.3, as_arrays=True)
    assert lat.shifted_basis_solves == 1
    for key in cr0:
        assert cr0[key].tobytes() == cr1[key].tobytes(), key
    zero = lat.bundle_many(P, k=K, chains=chain, lamP=0.0, as_arrays=True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(plain0, zero))
    assert np.all(lat.last_bundle_prior["iters"] == 0) and np.all(lat.last_bundle_prior["res"] <= TOL)
    assert lat.shifted_basis_solves == 1 and lat.stats["query_basis_solves"] == st0["query_basis_solves"]
    assert lat.build_info()["shifted_basis_bytes"] == bytes0 + 28 * lat.N  # s, |X'|^2, c0, c2 beside the basis
    assert not [ev for ev, _ in events if ev in ("shifted_basis_solve", "query_basis_solve")]  # no basis solved in between
    assert not [ev for ev, _ in events if ev == "chain_prior_convergence_warn"]
    lat.add_chain(chain, lamP=0.2)
    with pytest.raises(ValueError, match="clear_chain"):
        lat.bundle_many(P, chains=chain, lamP=0.2)
    lat.clear_chain()
    D = P.shape[1]
    assert lat.bundle_many(np.zeros((0, D), np.float32), chains=[], lamP=0.2) == []
    lat.close()

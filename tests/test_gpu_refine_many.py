"""Corpus.search / Corpus.refine_many against a float64 search, the candidate lattice's own graph
bit for bit, the per-query loop of the reference's retrieval scripts, the float64 yardstick and the oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _queries as yq

pytestmark = pytest.mark.gpu

NEAR_TIE = 1e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def amd():
    import oscillink_amd

    return oscillink_amd


def _corpora(D=64, N=600, seed=0):
    rng = np.random.default_rng(seed)
    gauss = rng.standard_normal((N, D)).astype(np.float32)
    centers = rng.standard_normal((8, D)).astype(np.float32) * 3
    clustered = (centers[rng.integers(0, 8, N)] + 0.3 * rng.standard_normal((N, D))).astype(np.float32)
    dup = gauss.copy()
    dup[1::7] = dup[0::7][: dup[1::7].shape[0]]
    zero = gauss.copy()
    zero[::11] = 0.0
    return {"gauss": gauss, "clustered": clustered, "dup": dup, "zero": zero}


def _queries(Y, Q=6, seed=1):
    rng = np.random.default_rng(seed)
    P = rng.standard_normal((Q, Y.shape[1])).astype(np.float32)
    P[0] = 0.0
    P[1] = Y[5]
    return P


def _host_cos(Y, P):
    Yd = Y.astype(np.float64)
    Yn = Yd / (np.linalg.norm(Yd, axis=1, keepdims=True) + 1e-12)
    Pd = P.astype(np.float64)
    return (Yn @ Pd.T).T / (np.linalg.norm(Pd, axis=1, keepdims=True) + 1e-12)


def _check_search(amd, Y, P, top_ks, atol):
    with amd.Corpus(Y) as c:
        for top_k in top_ks:
            ids, cos = c.search(P, top_k)
            ref = _host_cos(Y, P)
            err = float(np.abs(cos - np.take_along_axis(ref, ids, 1)).max())
            print(f"D={Y.shape[1]} top_k={top_k}: max |cos - float64| {err:.3e}")
            for q in range(P.shape[0]):
                want = np.lexsort((np.arange(Y.shape[0]), -ref[q]))[:top_k]
                np.testing.assert_allclose(cos[q], ref[q][ids[q]], atol=atol)
                assert np.all(np.diff(cos[q]) <= 0)
                kth = ref[q][want[-1]]
                for g, w in zip(ids[q], want):
                    if g != w:  # only inside the tie class of the K-th place
                        assert abs(ref[q][g] - kth) <= atol or abs(ref[q][g] - ref[q][w]) <= atol
                assert len(set(ids[q].tolist())) == len(ids[q])


@pytest.mark.parametrize("name", ["gauss", "clustered", "dup", "zero"])
def test_search_against_float64(amd, name):
    Y = _corpora()[name]
    P = _queries(Y)
    _check_search(amd, Y, P, (1, 10, 100), 1e-6)


# Twice the largest |cos - float64| of a plain float32 numpy `Yn @ psi` (rows and query normalised in float32) on the
# corpora below, measured on the CPU: 6.55e-07 (D = 257, clustered; 5.70e-07 at D = 1290, 4.24e-07 at D = 1536).
WIDE_ATOL = 2 * 6.55e-7


@pytest.mark.parametrize("D", [257, 1290, 1536])
@pytest.mark.parametrize("name", ["gauss", "clustered", "dup", "zero"])
def test_search_against_float64_wide(amd, name, D):
    """The search GEMM and select beyond D = 64: pad columns (257 -> ldn 288, 1290 -> 1312), the widest rows (1536) and the
    largest top_k (1024 of 1100 rows)."""
    Y = _corpora(D=D, N=1100)[name]
    P = _queries(Y)
    _check_search(amd, Y, P, (1, 100, 1024), WIDE_ATOL)


def _loop(amd, Y, cand, psi, k, alpha, **kw):
    lat = amd.Oscillink(Y[cand], **kw)
    lat.set_query(psi)
    out = lat.bundle(k, alpha)
    it = dict(lat.last_ustar, hist=lat.residual_history())
    rowptr, col, a, w, sd = lat.graph_csr()
    lat.close()
    return out, it, (rowptr, col, a, w, sd)


GRAPH_CASES = [(tk, kn, cap, D) for D in (50, 128, 768, 1536) for tk in (1, 2, 7, 64, 100, 1024)
               for kn in (1, 6, 16, 64, 2000) for cap in (1.0, 0.3)
               if min(kn, max(1, tk - 1)) <= 128 and (D in (50, 128) or tk in (7, 100, 1024))]


@pytest.mark.parametrize("D", [50, 128, 768, 1536])
def test_candidate_graph_bit_identical(amd, D):
    rng = np.random.default_rng(D)
    Y = rng.standard_normal((1100, D)).astype(np.float32)
    psi = rng.standard_normal(D).astype(np.float32)
    with amd.Corpus(Y) as c:
        for tk, kn, cap, d in GRAPH_CASES:
            if d != D:
                continue
            cand = c.search(psi[None, :], tk)[0][0]
            got = c._candidate_graph(psi, tk, kn, cap)
            lat = amd.Oscillink(Y[cand], kneighbors=kn, row_cap_val=cap)
            want = lat.graph_csr()
            lat.close()
            for g, w, nm in zip(got, want, ("rowptr", "col", "a", "w", "sqrt_deg")):
                assert np.array_equal(np.asarray(g), np.asarray(w)), (tk, kn, cap, D, nm)
            got2 = c._candidate_graph(cand, tk, kn, cap)
            for g, w in zip(got2, got):
                assert np.array_equal(g, w)


def _compare(amd, Y, P, res, top_k, k, alpha, kw):
    kw_loop = dict(kneighbors=kw.get("kneighbors", 6), row_cap_val=kw.get("row_cap_val", 1.0), lamG=kw.get("lamG", 1.0),
                   lamC=kw.get("lamC", 0.5), lamQ=kw.get("lamQ", 4.0))
    exceptions = []
    for q in range(P.shape[0]):
        cand = res["candidates"][q]
        out, it, csr = _loop(amd, Y, cand, P[q], k, alpha, **kw_loop)
        Yc = Y[cand]
        M = yq.dense_M(yq_dense(csr, len(cand)), csr[4], np.ones(len(cand)), kw_loop["lamG"], kw_loop["lamC"],
                       kw_loop["lamQ"])
        U = yq.ustar(M, Yc, np.ones(len(cand)), P[q], kw_loop["lamG"], kw_loop["lamQ"])
        _, _, _, margins = yq.bundle(Yc, U, P[q], csr[:3], csr[4], kw_loop["lamC"], k=k, alpha=alpha)
        want = [int(cand[b["id"]]) for b in out]
        got = res["ids"][q].tolist()
        ok, cut = yq.same_until_near_tie(got, want, margins, NEAR_TIE)
        assert ok, (q, got, want)
        n = len(want)
        for t in range(n):
            if margins[t] < NEAR_TIE:
                break
            assert abs(res["score"][q][t] - out[t]["score"]) <= 1e-4
            assert abs(res["align"][q][t] - out[t]["align"]) <= 1e-5
        if int(res["ustar_iters"][q]) != it["iters"]:
            gi, wi = int(res["ustar_iters"][q]), it["iters"]
            exceptions.append((q, gi, wi, it["hist"][min(gi, wi) - 1]))
    for q, gi, wi, deciding in exceptions:  # only where the loop's deciding residual sits at tol
        print(f"ustar_iters exception: query {q}: {gi} vs loop {wi} (loop residual {deciding:.6e} at iteration {min(gi, wi)})")
        assert abs(deciding - 1e-4) <= 1e-3 * 1e-4, (q, gi, wi, deciding)


def yq_dense(csr, n):
    rowptr, col, a = csr[0], csr[1], csr[2]
    A = np.zeros((n, n))
    r = np.repeat(np.arange(n), np.diff(rowptr))
    A[r, col] = a
    return A


@pytest.mark.parametrize("top_k,k,alpha,kw", [
    (100, 8, 0.5, {}),
    (64, 1, 0.0, {"kneighbors": 16}),
    (64, 64, 1.0, {"lamC": 0.0, "lamQ": 0.0}),
    (30, 40, 0.5, {"lamG": 2.0, "lamC": 1.5, "lamQ": 0.5, "row_cap_val": 0.3}),
    (7, 8, 0.5, {"kneighbors": 2000}),
])
def test_refine_many_against_loop(amd, top_k, k, alpha, kw):
    rng = np.random.default_rng(top_k + k)
    centers = rng.standard_normal((6, 96)).astype(np.float32) * 2
    Y = (centers[rng.integers(0, 6, 2000)] + 0.5 * rng.standard_normal((2000, 96))).astype(np.float32)
    P = rng.standard_normal((5, 96)).astype(np.float32)
    with amd.Corpus(Y) as c:
        res = c.refine_many(P, top_k, k, alpha, as_arrays=True, **kw)
        assert res["ids"].shape == (5, min(k, top_k))
        assert res["candidates"].shape == (5, top_k)
        assert np.array_equal(res["candidates"], c.search(P, top_k)[0])
        _compare(amd, Y, P, res, top_k, k, alpha, kw)
        lists = c.refine_many(P, top_k, k, alpha, **kw)
        assert [[d["id"] for d in l] for l in lists] == res["ids"].tolist()


def test_float64_yardstick_and_oracle(amd):
    from oracle import oscillink_oracle as orc

    rng = np.random.default_rng(3)
    Y = rng.standard_normal((400, 32)).astype(np.float32)
    P = rng.standard_normal((3, 32)).astype(np.float32)
    with amd.Corpus(Y) as c:
        res = c.refine_many(P, 40, 6, 0.5, as_arrays=True)
        for q in range(3):
            cand = res["candidates"][q]
            rowptr, col, a, w, sd = c._candidate_graph(cand, 40)
            Yc = Y[cand]
            A = yq_dense((rowptr, col, a), 40)
            M = yq.dense_M(A, sd, np.ones(40), 1.0, 0.5, 4.0)
            U = yq.ustar(M, Yc, np.ones(40), P[q], 1.0, 4.0)
            ids, score, align, margins = yq.bundle(Yc, U, P[q], (rowptr, col, a), sd, 0.5, k=6, alpha=0.5)
            ok, _ = yq.same_until_near_tie(res["local"][q].tolist(), ids, margins, NEAR_TIE)
            assert ok
            np.testing.assert_allclose(res["align"][q][:3], align[:3], atol=1e-4)
        cand = res["candidates"][0]
        ref = orc.OracleLattice(Y[cand], kneighbors=6)
        ref.set_query(P[0])
        Us = ref.solve_Ustar()
        assert ref.last_ustar["iters"] == int(res["ustar_iters"][0])
        ids, score, align, margins = yq.bundle(Y[cand], Us, P[0], np.asarray(ref.A), ref.sqrt_deg, 0.5, k=6, alpha=0.5)
        ok, _ = yq.same_until_near_tie(res["local"][0].tolist(), ids, margins, NEAR_TIE)
        assert ok
        np.testing.assert_allclose(res["score"][0][:2], score[:2], atol=1e-4)


def test_independence_and_chunking(amd):
    rng = np.random.default_rng(5)
    Y = rng.standard_normal((1500, 64)).astype(np.float32)
    P = rng.standard_normal((9, 64)).astype(np.float32)
    keys = ("ids", "local", "score", "align", "candidates", "ustar_iters", "ustar_res")
    with amd.Corpus(Y) as c:
        full = c.refine_many(P, 50, 8, as_arrays=True)
        for q in (0, 8, 4):
            alone = c.refine_many(P[q:q + 1], 50, 8, as_arrays=True)
            for key in keys:
                assert np.array_equal(alone[key][0], full[key][q]), (q, key)
        given = c.refine_many(P, 50, 8, candidates=full["candidates"], as_arrays=True)
        for key in keys:
            assert np.array_equal(given[key], full[key]), key
    # OSC_CORPUS_CHUNK is read at creation: a fresh process with chunks of 4 queries
    code = ("import numpy as np, sys; sys.path.insert(0, %r); from oscillink_amd import Corpus; "
            "rng = np.random.default_rng(5); Y = rng.standard_normal((1500, 64)).astype(np.float32); "
            "P = rng.standard_normal((9, 64)).astype(np.float32); c = Corpus(Y); assert c.info(50)['chunk'] == 4; "
            "r = c.refine_many(P, 50, 8, as_arrays=True); "
            "np.savez(sys.argv[1], **r)") % ROOT
    import tempfile

    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "r.npz")
        env = dict(os.environ, OSC_CORPUS_CHUNK="4")
        r = subprocess.run([sys.executable, "-c", code, out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:]
        chunked = np.load(out)
        for key in keys:
            assert np.array_equal(chunked[key], full[key]), key


def test_errors_and_edges(amd):
    rng = np.random.default_rng(9)
    Y = rng.standard_normal((300, 16)).astype(np.float32)
    P = rng.standard_normal((2, 16)).astype(np.float32)
    bad = Y.copy()
    bad[3, 2] = np.nan
    with pytest.raises(ValueError, match="finite"):
        amd.Corpus(bad)
    c = amd.Corpus(Y)
    with pytest.raises(ValueError, match="top_k"):
        c.refine_many(P, 0)
    with pytest.raises(ValueError, match="top_k"):
        c.search(P, 1025)
    with pytest.raises(ValueError, match="128"):
        c.refine_many(P, 300, kneighbors=200)
    with pytest.raises(ValueError, match="psis"):
        c.refine_many(P[:, :8], 10)
    Pn = P.copy()
    Pn[1, 0] = np.inf
    with pytest.raises(ValueError, match="finite"):
        c.refine_many(Pn, 10)
    with pytest.raises(ValueError, match="candidates"):
        c.refine_many(P, 10, candidates=np.zeros((2, 9), dtype=np.int32))
    with pytest.raises(ValueError, match="candidates"):
        c.refine_many(P, 10, candidates=np.full((2, 10), 300, dtype=np.int32))
    rep = np.tile(np.arange(10, dtype=np.int32), (2, 1))
    rep[1, 3] = 4
    with pytest.raises(ValueError, match="repeated"):
        c.refine_many(P, 10, candidates=rep)
    empty = c.refine_many(np.zeros((0, 16), np.float32), 10, as_arrays=True)
    assert empty["ids"].shape == (0, 8)
    assert c.refine_many(np.zeros((0, 16), np.float32), 10) == []
    r = c.refine_many(P, 5, k=50, as_arrays=True)  # k clamped to K
    assert r["ids"].shape == (2, 5) and sorted(r["local"][0].tolist()) == list(range(5))
    r1 = c.refine_many(P, 1, k=3, as_arrays=True)
    assert r1["ids"].shape == (2, 1) and np.array_equal(r1["ids"][:, 0], r1["candidates"][:, 0])
    c.close()
    with pytest.raises(ValueError, match="closed"):
        c.refine_many(P, 10)

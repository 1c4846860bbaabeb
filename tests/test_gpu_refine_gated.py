"""Corpus.refine_many(gates=...) and Corpus.diffusion_gates_many (the gated form) against the
float64 yardstick of tests/_gated.py, the per-query loop `Oscillink(Y[cand]); compute_diffusion_gates(..., lattice=lat);
set_query(psi, gates=g); bundle(k, alpha)` and the oracle's CG, on test_refine_many_against_loop's corpus and settings."""
import os
import subprocess
import sys
import tempfile
import warnings

import numpy as np
import pytest

from tests import _gated as yg
from tests import _queries as yq

pytestmark = pytest.mark.gpu

NEAR_TIE = 1e-4
GATE_ATOL = 1e-4  # what tests/test_gpu_parity.py holds the single-lattice gates to
USTAR_TOL = 1e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNGATED_KEYS = ("ids", "local", "score", "align", "candidates", "ustar_iters", "ustar_res")
GATED_KEYS = UNGATED_KEYS + ("gates", "gate_iters", "gate_res")


@pytest.fixture(scope="module")
def amd():
    import oscillink_amd

    return oscillink_amd


def _gate_kw(kw, beta, gamma):
    return dict(kneighbors=kw.get("kneighbors", 6), row_cap_val=kw.get("row_cap_val", 1.0), beta=beta, gamma=gamma)


def _refine_gate_kw(beta, gamma, **more):
    return dict(gates="diffusion", gate_beta=beta, gate_gamma=gamma, **more)


def check_gates(amd, c, Y, P, top_k, kw, beta, gamma):
    """Check 1 of the gated tests, shared with the full-size test: the batch's gates against float64 on the device's own
    graph, against the loop, and the cg iteration counts against the oracle's CG.

    Both methods are held to the loop's gates of the same method (atol 1e-4).  Against float64, method="direct" is compared
    as it is; method="cg" is compared through a third run, `tight` (cg at tol 1e-7 max(1, |s|), 2048 iterations -- the
    setting the CPU yardstick test uses for the oracle's cg), because cg stopped at the caller's absolute residual of 1e-4
    is by definition not within 1e-4 of the exact solve once the error is divided by a small spread max h - min h.  The
    run at tol 1e-4 is the one whose iteration count is compared with the oracle's."""
    from oracle import oscillink_oracle as orc

    gk = _gate_kw(kw, beta, gamma)
    lk = yg.lattice_kw(kw)
    direct = c.diffusion_gates_many(P, top_k, method="direct", **gk)
    cg = c.diffusion_gates_many(P, top_k, method="cg", tol=1e-4, max_iters=256, **gk)
    raw = c.diffusion_gates_many(P, top_k, method="direct", clamp=False, **gk)
    Q, K = direct["gates"].shape
    assert direct["gates"].dtype == np.float32 and cg["gates"].dtype == np.float32
    assert np.array_equal(direct["candidates"], c.search(P, top_k)[0])
    assert np.array_equal(cg["candidates"], direct["candidates"])
    exceptions = []
    for q in range(Q):
        cand = direct["candidates"][q]
        Yc = Y[cand]
        csr = c._candidate_graph(cand, top_k, gk["kneighbors"], gk["row_cap_val"])
        A = yg.dense_adj(csr, K)
        g64, raw64, s = yg.gates64(A, csr[4], Yc, P[q], beta, gamma)
        lat = amd.Oscillink(Yc, **lk)
        loop_direct = amd.compute_diffusion_gates(Yc, P[q], method="direct", lattice=lat, **gk)
        loop_cg = amd.compute_diffusion_gates(Yc, P[q], method="cg", tol=1e-4, max_iters=256, lattice=lat, **gk)
        lat.close()
        stol = 1e-7 * max(1.0, float(np.linalg.norm(s)))
        tight = c.diffusion_gates_many(P[q:q + 1], top_k, method="cg", tol=stol, max_iters=2048, candidates=cand[None, :],
                                       **gk)
        spread = float(raw64.max() - raw64.min())
        print(f"top_k={top_k} q={q} spread={spread:.4f} iters direct/cg/tight={int(direct['iters'][q])}/"
              f"{int(cg['iters'][q])}/{int(tight['iters'][0])} |direct-64|={np.abs(direct['gates'][q] - g64).max():.2e} "
              f"|tight-64|={np.abs(tight['gates'][0] - g64).max():.2e} "
              f"|direct-loop|={np.abs(direct['gates'][q] - loop_direct).max():.2e} "
              f"|cg-loop|={np.abs(cg['gates'][q] - loop_cg).max():.2e}")
        np.testing.assert_allclose(direct["gates"][q], g64, atol=GATE_ATOL, rtol=0)
        np.testing.assert_allclose(tight["gates"][0], g64, atol=GATE_ATOL, rtol=0)
        np.testing.assert_allclose(direct["gates"][q], loop_direct, atol=GATE_ATOL, rtol=0)
        np.testing.assert_allclose(cg["gates"][q], loop_cg, atol=GATE_ATOL, rtol=0)
        assert spread >= 1e-12  # every lattice here is non-uniform: min 0 and max 1 exactly
        for got in (direct["gates"][q], cg["gates"][q], tight["gates"][0]):
            assert got.min() == 0.0 and got.max() == 1.0
        np.testing.assert_allclose(raw["gates"][q], raw64, atol=1e-4 * float(np.abs(raw64).max()), rtol=0)
        _, want_it, hist = yg.oracle_cg(orc, A, csr[4], s, gamma, 1e-4, 256)
        got_it = int(cg["iters"][q])
        if got_it != want_it:
            exceptions.append((q, got_it, want_it, hist[min(got_it, want_it) - 1]))
    for q, gi, wi, deciding in exceptions:  # only where the oracle's deciding residual sits at tol
        print(f"gate_iters exception: query {q}: {gi} vs oracle {wi} (oracle residual {deciding:.6e} at iteration "
              f"{min(gi, wi)})")
        assert abs(deciding - 1e-4) <= 1e-3 * 1e-4, (q, gi, wi, deciding)
    return direct


def check_given_gates(amd, c, Y, P, cand, g, top_k, k, alpha, kw):
    """Check 4, shared with the full-size test: refine_many(gates=g, candidates=cand) against the gated loop and the
    float64 yardstick with B = g[q], under test_gpu_refine_many._compare's criteria."""
    lk = yg.lattice_kw(kw)
    res = c.refine_many(P, top_k, k, alpha, candidates=cand, gates=g, as_arrays=True, **kw)
    assert np.array_equal(res["gates"], g) and np.array_equal(res["candidates"], cand)
    assert not res["gate_iters"].any() and not res["gate_res"].any()
    total = compared = 0
    differs = follows = False
    exceptions = []
    for q in range(P.shape[0]):
        Yc = Y[cand[q]]
        lat = amd.Oscillink(Yc, **lk)
        lat.set_query(P[q], gates=g[q])
        out = lat.bundle(k, alpha)
        it = dict(lat.last_ustar, hist=lat.residual_history())
        csr = lat.graph_csr()
        lat.close()
        K = len(cand[q])
        A = yg.dense_adj(csr, K)
        B = g[q].astype(np.float64)
        M = yq.dense_M(A, csr[4], B, lk["lamG"], lk["lamC"], lk["lamQ"])
        U = yq.ustar(M, Yc, B, P[q], lk["lamG"], lk["lamQ"])
        ids64, _, _, margins = yq.bundle(Yc, U, P[q], csr[:3], csr[4], lk["lamC"], k=k, alpha=alpha)
        M1 = yq.dense_M(A, csr[4], np.ones(K), lk["lamG"], lk["lamC"], lk["lamQ"])
        U1 = yq.ustar(M1, Yc, np.ones(K), P[q], lk["lamG"], lk["lamQ"])
        ids1, _, _, _ = yq.bundle(Yc, U1, P[q], csr[:3], csr[4], lk["lamC"], k=k, alpha=alpha)
        got_local = res["local"][q].tolist()
        got = res["ids"][q].tolist()
        want = [int(cand[q][b["id"]]) for b in out]
        ok, _ = yq.same_until_near_tie(got, want, margins, NEAR_TIE)
        assert ok, (q, got, want)
        ok, _ = yq.same_until_near_tie(got_local, ids64, margins, NEAR_TIE)
        assert ok, (q, got_local, ids64)
        cut = next((t for t, m in enumerate(margins) if m < NEAR_TIE), len(want))
        total += len(want)
        compared += cut
        for t in range(cut):
            assert abs(res["score"][q][t] - out[t]["score"]) <= 1e-4
            assert abs(res["align"][q][t] - out[t]["align"]) <= 1e-5
            if ids64[t] != ids1[t]:
                differs = True
                follows = follows or got_local[t] == ids64[t]
        if int(res["ustar_iters"][q]) != it["iters"]:
            gi, wi = int(res["ustar_iters"][q]), it["iters"]
            exceptions.append((q, gi, wi, it["hist"][min(gi, wi) - 1]))
    for q, gi, wi, deciding in exceptions:  # only where the loop's deciding residual sits at tol
        print(f"ustar_iters exception: query {q}: {gi} vs loop {wi} (loop residual {deciding:.6e} at iteration {min(gi, wi)})")
        assert abs(deciding - USTAR_TOL) <= 1e-3 * USTAR_TOL, (q, gi, wi, deciding)
    print(f"top_k={top_k}: compared {compared}/{total} picks; gated picks differ from ungated on a compared step: {differs}")
    assert compared >= 0.9 * total, (compared, total)  # near ties cannot hide a failure
    assert differs and follows  # a gate that is silently ignored fails here
    return res


@pytest.mark.parametrize("top_k,k,kw,beta,gamma", yg.SETTINGS)
def test_gates_against_float64_loop_and_oracle(amd, top_k, k, kw, beta, gamma):
    Y, P = yg.corpus(top_k, k)
    with amd.Corpus(Y) as c:
        check_gates(amd, c, Y, P, top_k, kw, beta, gamma)


@pytest.mark.parametrize("top_k,k,kw,beta,gamma", yg.SETTINGS)
def test_gates_of_ones_are_the_ungated_path(amd, top_k, k, kw, beta, gamma):
    Y, P = yg.corpus(top_k, k)
    with amd.Corpus(Y) as c:
        plain = c.refine_many(P, top_k, k, 0.5, as_arrays=True, **kw)
        assert sorted(plain) == sorted(UNGATED_KEYS)
        ones = c.refine_many(P, top_k, k, 0.5, as_arrays=True, gates=np.ones((P.shape[0], top_k), np.float32), **kw)
        assert sorted(ones) == sorted(GATED_KEYS)
        for key in UNGATED_KEYS:
            assert np.array_equal(ones[key], plain[key]), key


def test_uniform_fallbacks(amd):
    Y, P = yg.corpus(100, 8)
    P = P.copy()
    P[0] = 0.0  # a zero query: s = 0
    cos = yg.host_cos(Y, P[2:3])[0]
    away = np.argsort(cos)[:40].astype(np.int32)  # candidates that all point away from query 2
    assert np.all(cos[away] <= 0.0)
    with amd.Corpus(Y) as c:
        gk = _refine_gate_kw(1.0, 0.15)
        zero = c.refine_many(P[:1], 50, 8, as_arrays=True, **gk)
        one = c.refine_many(P, 1, 3, as_arrays=True, **gk)
        neg = c.refine_many(P[2:3], 40, 8, candidates=away[None, :], as_arrays=True, **gk)
        for got, plain in ((zero, c.refine_many(P[:1], 50, 8, as_arrays=True)),
                           (one, c.refine_many(P, 1, 3, as_arrays=True)),
                           (neg, c.refine_many(P[2:3], 40, 8, candidates=away[None, :], as_arrays=True))):
            assert got["gates"].dtype == np.float32 and np.all(got["gates"] == 1.0)
            for key in UNGATED_KEYS:
                assert np.array_equal(got[key], plain[key]), key
        d = c.diffusion_gates_many(P[:1], 50, gamma=0.15)
        assert np.all(d["gates"] == 1.0) and np.all(np.isfinite(d["res"]))


@pytest.mark.parametrize("top_k,k,kw,beta,gamma", yg.SETTINGS)
def test_given_gates_against_loop_and_float64(amd, top_k, k, kw, beta, gamma):
    Y, P = yg.corpus(top_k, k)
    with amd.Corpus(Y) as c:
        d = c.diffusion_gates_many(P, top_k, method="direct", **_gate_kw(kw, beta, gamma))
        check_given_gates(amd, c, Y, P, d["candidates"], d["gates"], top_k, k, 0.5, kw)


@pytest.mark.parametrize("top_k,k,kw,beta,gamma", yg.SETTINGS)
def test_composition(amd, top_k, k, kw, beta, gamma):
    Y, P = yg.corpus(top_k, k)
    with amd.Corpus(Y) as c:
        for method in ("direct", "cg"):
            r = c.refine_many(P, top_k, k, 0.5, as_arrays=True, **kw, **_refine_gate_kw(beta, gamma, gate_method=method))
            given = c.refine_many(P, top_k, k, 0.5, as_arrays=True, gates=r["gates"], candidates=r["candidates"], **kw)
            for key in UNGATED_KEYS + ("gates",):
                assert np.array_equal(r[key], given[key]), (method, key)
            d = c.diffusion_gates_many(P, top_k, method=method, **_gate_kw(kw, beta, gamma))
            assert np.array_equal(d["gates"], r["gates"]) and np.array_equal(d["candidates"], r["candidates"])
            assert np.array_equal(d["iters"], r["gate_iters"]) and np.array_equal(d["res"], r["gate_res"])
            assert r["gate_iters"].min() >= 1
        lists = c.refine_many(P, top_k, k, 0.5, **kw, **_refine_gate_kw(beta, gamma))
        r = c.refine_many(P, top_k, k, 0.5, as_arrays=True, **kw, **_refine_gate_kw(beta, gamma))
        assert [[d["id"] for d in l] for l in lists] == r["ids"].tolist()


def test_independence_and_chunking(amd):
    rng = np.random.default_rng(5)
    Y = rng.standard_normal((1500, 64)).astype(np.float32)
    P = rng.standard_normal((9, 64)).astype(np.float32)
    gk = _refine_gate_kw(1.0, 0.15)
    with amd.Corpus(Y) as c:
        full = c.refine_many(P, 50, 8, as_arrays=True, **gk)
        assert sorted(full) == sorted(GATED_KEYS)
        for q in (0, 8, 4):
            alone = c.refine_many(P[q:q + 1], 50, 8, as_arrays=True, **gk)
            for key in GATED_KEYS:
                assert np.array_equal(alone[key][0], full[key][q]), (q, key)
        back = c.refine_many(P[::-1], 50, 8, as_arrays=True, **gk)
        for key in GATED_KEYS:
            assert np.array_equal(back[key][::-1], full[key]), key
    # OSC_CORPUS_CHUNK is read at creation: a fresh process with chunks of 4 queries
    code = ("import numpy as np, sys; sys.path.insert(0, %r); from oscillink_amd import Corpus; "
            "rng = np.random.default_rng(5); Y = rng.standard_normal((1500, 64)).astype(np.float32); "
            "P = rng.standard_normal((9, 64)).astype(np.float32); c = Corpus(Y); assert c.info(50)['chunk'] == 4; "
            "r = c.refine_many(P, 50, 8, as_arrays=True, gates='diffusion', gate_beta=1.0, gate_gamma=0.15); "
            "np.savez(sys.argv[1], **r)") % ROOT
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "r.npz")
        env = dict(os.environ, OSC_CORPUS_CHUNK="4")
        r = subprocess.run([sys.executable, "-c", code, out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:]
        chunked = np.load(out)
        for key in GATED_KEYS:
            assert np.array_equal(chunked[key], full[key]), key


def test_errors_and_edges(amd):
    from oscillink_amd import _native as nat

    rng = np.random.default_rng(9)
    Y = rng.standard_normal((300, 16)).astype(np.float32)
    P = rng.standard_normal((2, 16)).astype(np.float32)
    c = amd.Corpus(Y)
    for bad, name in ((dict(gate_gamma=0.0), "gate_gamma"), (dict(gate_gamma=-1.0), "gate_gamma"),
                      (dict(gate_beta=float("nan")), "gate_beta"), (dict(gate_method="lu"), "gate_method"),
                      (dict(gate_max_iters=0), "gate_max_iters")):
        with pytest.raises(ValueError, match=name):
            c.refine_many(P, 10, gates="diffusion", **bad)
    for bad, name in ((dict(gamma=0.0), "gamma"), (dict(beta=float("inf")), "beta"), (dict(method="lu"), "method"),
                      (dict(max_iters=0), "max_iters")):
        with pytest.raises(ValueError, match=name):
            c.diffusion_gates_many(P, 10, **bad)
    with pytest.raises(ValueError, match="gates"):
        c.refine_many(P, 10, gates="heat")
    with pytest.raises(ValueError, match="gates"):
        c.refine_many(P, 10, gates=np.ones((2, 9), np.float32))
    g = np.ones((2, 10), np.float32)
    g[1, 3] = np.nan
    with pytest.raises(ValueError, match="gates.*finite"):
        c.refine_many(P, 10, gates=g)
    g[1, 3] = -0.5
    with pytest.raises(ValueError, match="gates.*>= 0"):
        c.refine_many(P, 10, gates=g)
    with pytest.raises(ValueError, match="candidates"):
        c.diffusion_gates_many(P, 10, candidates=np.zeros((2, 9), dtype=np.int32))
    # the C entry points: the same checks behind the Python ones, and NULL buffers
    L = nat.lib()
    cand = np.zeros((2, 10), np.int32)
    gates = np.zeros((2, 10), np.float32)
    it = np.zeros(2, np.int32)
    rs = np.zeros(2, np.float32)
    assert L.osc_corpus_gates(c._h, nat.f32(P), 2, 10, None, 6, 1.0, 1.0, 0.1, 0, 1e-4, 256, 1, nat.i32(cand), None,
                              nat.i32(it), nat.f32(rs)) == nat.OSC_E_INVALID
    assert b"NULL buffer" in L.osc_corpus_last_error(c._h)
    assert L.osc_corpus_gates(c._h, nat.f32(P), 2, 10, None, 6, 1.0, 1.0, 0.0, 0, 1e-4, 256, 1, nat.i32(cand),
                              nat.f32(gates), nat.i32(it), nat.f32(rs)) == nat.OSC_E_INVALID
    assert b"gamma" in L.osc_corpus_last_error(c._h)
    assert L.osc_corpus_refine_gated(c._h, nat.f32(P), 2, 10, None, None, 1.0, 0.1, 0, 1e-4, 256, 6, 1.0, 1.0, 0.5, 4.0,
                                     1e-4, 64, 0, 0.5, nat.i32(cand), None, None, None, None, nat.i32(it), nat.f32(rs),
                                     nat.i32(it), nat.f32(rs)) == nat.OSC_E_INVALID
    assert b"NULL buffer" in L.osc_corpus_last_error(c._h)
    g[1, 3] = -0.5
    assert L.osc_corpus_refine_gated(c._h, nat.f32(P), 2, 10, None, nat.f32(g), 1.0, 0.1, 0, 1e-4, 256, 6, 1.0, 1.0, 0.5,
                                     4.0, 1e-4, 64, 0, 0.5, nat.i32(cand), nat.f32(gates), None, None, None, nat.i32(it),
                                     nat.f32(rs), nat.i32(it), nat.f32(rs)) == nat.OSC_E_INVALID
    assert b"gates" in L.osc_corpus_last_error(c._h)
    # edges
    empty = c.refine_many(np.zeros((0, 16), np.float32), 10, as_arrays=True, gates="diffusion")
    assert empty["ids"].shape == (0, 8) and empty["gates"].shape == (0, 10) and empty["gates"].dtype == np.float32
    assert empty["gate_iters"].shape == (0,) and empty["gate_res"].shape == (0,)
    empty = c.refine_many(np.zeros((0, 16), np.float32), 10, as_arrays=True, gates=np.zeros((0, 10), np.float32))
    assert empty["gates"].shape == (0, 10)
    assert c.refine_many(np.zeros((0, 16), np.float32), 10, gates="diffusion") == []
    d = c.diffusion_gates_many(np.zeros((0, 16), np.float32), 10)
    assert d["gates"].shape == (0, 10) and d["candidates"].shape == (0, 10) and d["iters"].shape == (0,)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # finite gates: no warning
        r = c.refine_many(P, 5, k=50, as_arrays=True, gates="diffusion")
    assert r["ids"].shape == (2, 5) and sorted(r["local"][0].tolist()) == list(range(5)) and r["gates"].shape == (2, 5)
    zero_gates = c.refine_many(P, 10, as_arrays=True, gates=np.zeros((2, 10), np.float32))  # B = 0 is legal (lamQ B = 0)
    assert np.all(np.isfinite(zero_gates["score"]))
    c.close()
    with pytest.raises(ValueError, match="closed"):
        c.refine_many(P, 10, gates="diffusion")
    with pytest.raises(ValueError, match="closed"):
        c.diffusion_gates_many(P, 10)

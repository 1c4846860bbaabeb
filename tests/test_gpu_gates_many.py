"""OscillinkLattice.diffusion_gates_many: the batched screened-diffusion gates of one lattice against
the per-query loop `compute_diffusion_gates(Y, psi_q, lattice=lat)`, the float64 yardstick of tests/_gated.py, the
oracle's CG and the reference fixture, plus the properties the batch adds: a stop per column, independence of a query from
the rest of its batch and from the chunking, and no change of the lattice's state.

Shapes: tests/_gated.corpus(100, 8) -- 2000 x 96 clustered anchors (63 row parts of 32 rows, the last one short), 5
queries -- on a kneighbors=6 lattice; Q = 1, 6, 33, 70 cover a single column, a partly filled slab, the first column of a
second slab and three slabs / three chunks of 32 with a partial last one."""
import warnings

import numpy as np
import pytest

from tests import _gated as yg
from tests._cases import load_case, make_inputs

pytestmark = pytest.mark.gpu

GATE_ATOL = 1e-4  # what tests/test_gpu_parity.py and tests/test_gpu_refine_gated.py hold the gates to
BETA_GAMMA = sorted({(s[3], s[4]) for s in yg.SETTINGS})


@pytest.fixture(scope="module")
def amd():
    import oscillink_amd

    return oscillink_amd


@pytest.fixture(scope="module")
def world(amd):
    """The shared lattice, its dense graph and the queries; nothing here is modified by a test."""
    Y, P = yg.corpus(100, 8)
    lat = amd.Oscillink(Y, kneighbors=6)
    csr = lat.graph_csr()
    A = yg.dense_adj(csr, Y.shape[0])
    rng = np.random.default_rng(7)
    inside = (Y[1234] + 0.05 * rng.standard_normal(96)).astype(np.float32)  # a query inside a cluster
    P70 = rng.standard_normal((70, 96)).astype(np.float32)
    P70[::7] = Y[rng.integers(0, 2000, 10)] + 0.2 * rng.standard_normal((10, 96)).astype(np.float32)
    yield dict(Y=Y, P=P, lat=lat, A=A, sd=csr[4], inside=inside, P70=P70)
    lat.close()


def _loop(amd, w, P, **kw):
    return np.stack([amd.compute_diffusion_gates(w["Y"], p, lattice=w["lat"], **kw) for p in P])


@pytest.mark.parametrize("beta,gamma", BETA_GAMMA)
def test_against_the_loop_float64_and_the_oracle(amd, world, beta, gamma):
    """check_gates' criteria (tests/test_gpu_refine_gated.py) on this lattice's own graph."""
    from oracle import oscillink_oracle as orc

    w, lat, P = world, world["lat"], world["P"]
    direct = lat.diffusion_gates_many(P, beta=beta, gamma=gamma, method="direct")
    cg = lat.diffusion_gates_many(P, beta=beta, gamma=gamma, method="cg", tol=1e-4, max_iters=256)
    loop_direct = _loop(amd, w, P, beta=beta, gamma=gamma, method="direct")
    loop_cg = _loop(amd, w, P, beta=beta, gamma=gamma, method="cg", tol=1e-4, max_iters=256)
    for out in (direct, cg):
        assert out["gates"].dtype == np.float32 and out["gates"].shape == (5, 2000)
        assert out["iters"].dtype == np.int32 and out["iters"].shape == (5,)
        assert out["res"].dtype == np.float32 and out["res"].shape == (5,)
    exceptions = []
    for q in range(5):
        g64, raw64, s = yg.gates64(w["A"], w["sd"], w["Y"], P[q], beta, gamma)
        spread = float(raw64.max() - raw64.min())
        print(f"beta={beta} gamma={gamma} q={q} spread={spread:.4f} iters direct/cg={int(direct['iters'][q])}/"
              f"{int(cg['iters'][q])} res direct/cg={float(direct['res'][q]):.3e}/{float(cg['res'][q]):.3e} "
              f"|direct-64|={np.abs(direct['gates'][q] - g64).max():.2e} "
              f"|direct-loop|={np.abs(direct['gates'][q] - loop_direct[q]).max():.2e} "
              f"|cg-loop|={np.abs(cg['gates'][q] - loop_cg[q]).max():.2e}")
        np.testing.assert_allclose(direct["gates"][q], g64, atol=GATE_ATOL, rtol=0)
        np.testing.assert_allclose(direct["gates"][q], loop_direct[q], atol=GATE_ATOL, rtol=0)
        np.testing.assert_allclose(cg["gates"][q], loop_cg[q], atol=GATE_ATOL, rtol=0)
        assert spread >= 1e-12  # non-uniform: min 0 and max 1 exactly
        for got in (direct["gates"][q], cg["gates"][q]):
            assert got.min() == 0.0 and got.max() == 1.0
        assert float(direct["res"][q]) <= 1e-7 * max(1.0, float(np.linalg.norm(s))) * (1 + 1e-6)
        _, want_it, hist = yg.oracle_cg(orc, w["A"], w["sd"], s, gamma, 1e-4, 256)
        got_it = int(cg["iters"][q])
        if got_it != want_it:
            exceptions.append((q, got_it, want_it, hist[min(got_it, want_it) - 1]))
    for q, gi, wi, deciding in exceptions:  # only where the oracle's deciding residual sits at tol
        print(f"iters exception: query {q}: {gi} vs oracle {wi} (oracle residual {deciding:.6e} at iteration {min(gi, wi)})")
        assert abs(deciding - 1e-4) <= 1e-3 * 1e-4, (q, gi, wi, deciding)
    assert len(exceptions) <= 1, exceptions


def test_reference_fixture(amd):
    case = load_case("c5mini_n600_d96_k12")
    rc = case["recipe"]
    Y, psi = make_inputs(rc)
    lat = amd.Oscillink(Y, kneighbors=rc["k"], deterministic_k=True)
    got = lat.diffusion_gates_many(psi[None], **rc["diffusion"])["gates"][0]  # (gamma and method)
    print(f"fixture: |gates - recorded|={np.abs(got - case['gates']).max():.2e}")
    np.testing.assert_allclose(got, case["gates"], atol=GATE_ATOL, rtol=0)
    free = amd.compute_diffusion_gates_many(Y, psi[None], kneighbors=rc["k"], deterministic_k=True, **rc["diffusion"])
    assert free.shape == (1, Y.shape[0]) and np.array_equal(free[0], got)
    lat.close()


def test_every_column_stops_on_its_own(amd, world):
    w, lat = world, world["lat"]
    P = np.vstack([w["P"], w["inside"][None]])
    out = lat.diffusion_gates_many(P, gamma=0.15, method="cg", tol=1e-4, max_iters=256)
    loop = _loop(amd, w, P, gamma=0.15, method="cg", tol=1e-4, max_iters=256)
    print("iters", out["iters"].tolist(), "res", out["res"].tolist(),
          "|batch-loop|", [float(np.abs(out["gates"][q] - loop[q]).max()) for q in range(6)])
    assert len(set(out["iters"].tolist())) >= 2  # else nothing here exercises the freeze
    for q in range(6):
        np.testing.assert_allclose(out["gates"][q], loop[q], atol=GATE_ATOL, rtol=0)
        assert float(out["res"][q]) <= 1e-4


@pytest.mark.parametrize("method", ["cg", "direct"])
def test_a_query_does_not_see_its_batch(amd, world, method, monkeypatch):
    lat, P = world["lat"], world["P70"]
    kw = dict(gamma=0.15, method=method, tol=1e-4, max_iters=256)
    monkeypatch.delenv("OSC_GATES_CHUNK", raising=False)
    whole = lat.diffusion_gates_many(P, **kw)
    assert whole["gates"].shape == (70, 2000) and np.isfinite(whole["gates"]).all()
    for q in (0, 31, 32, 69):
        one = lat.diffusion_gates_many(P[q:q + 1], **kw)
        assert np.array_equal(one["gates"][0], whole["gates"][q]), q
        assert one["iters"][0] == whole["iters"][q] and one["res"][0] == whole["res"][q]
    first33 = lat.diffusion_gates_many(P[:33], **kw)
    assert np.array_equal(first33["gates"], whole["gates"][:33])
    perm = np.random.default_rng(3).permutation(70)
    shuffled = lat.diffusion_gates_many(P[perm], **kw)
    for key in ("gates", "iters", "res"):
        assert np.array_equal(shuffled[key], whole[key][perm]), key
    monkeypatch.setenv("OSC_GATES_CHUNK", "32")  # three chunks, the last one of 6 queries
    chunked = lat.diffusion_gates_many(P, **kw)
    for key in ("gates", "iters", "res"):
        assert np.array_equal(chunked[key], whole[key]), key


def test_degenerate_columns(amd, world):
    w, lat, P = world, world["lat"], world["P"]
    Yn = w["Y"] / (np.linalg.norm(w["Y"], axis=1, keepdims=True) + 1e-12)
    neg = (-Yn.sum(axis=0)).astype(np.float32)
    assert yg.host_cos(w["Y"], neg).max() < -1e-3  # every cosine below zero, beyond float32 round-off
    batch = np.vstack([P[0], np.zeros(96, np.float32), P[1], neg, P[2]])
    for method in ("cg", "direct"):
        kw = dict(gamma=0.15, method=method)
        out = lat.diffusion_gates_many(batch, **kw)
        for q in (1, 3):
            assert np.array_equal(out["gates"][q], np.ones(2000, np.float32)) and out["iters"][q] == 1
            assert out["res"][q] == 0.0
        alone = lat.diffusion_gates_many(P[:3], **kw)
        for a, b in ((0, 0), (1, 2), (2, 4)):
            assert np.array_equal(alone["gates"][a], out["gates"][b]) and alone["iters"][a] == out["iters"][b]
    Y0 = w["Y"].copy()
    Y0[7] = 0.0
    lat0 = amd.Oscillink(Y0, kneighbors=6)
    g = lat0.diffusion_gates_many(P, gamma=0.15)["gates"]
    assert np.isfinite(g).all() and g.min() == 0.0 and g.max() == 1.0
    lat0.close()


def test_non_finite_gates_come_back_with_one_warning(amd, world):
    """A source of 3e38 overflows the float32 sums of the first iteration: the column never freezes, runs to max_iters and
    comes back as computed; the zero query beside it is untouched."""
    lat, P = world["lat"], world["P"]
    batch = np.vstack([np.zeros(96, np.float32), P[0], P[1]])
    with pytest.warns(RuntimeWarning, match=r"query 1 .*iters=3") as rec:
        out = lat.diffusion_gates_many(batch, beta=3e38, gamma=0.15, method="cg", max_iters=3)
    assert len([r for r in rec if issubclass(r.category, RuntimeWarning)]) == 1
    assert not np.isfinite(out["gates"][1]).all() and out["iters"].tolist() == [1, 3, 3]
    assert np.array_equal(out["gates"][0], np.ones(2000, np.float32))


def test_rows_come_back_in_api_order_from_a_permuted_lattice(amd, world, monkeypatch):
    monkeypatch.setenv("OSC_REORDER", "1")
    lat = amd.Oscillink(world["Y"], kneighbors=6)
    monkeypatch.delenv("OSC_REORDER")
    assert lat.build_info()["reordered"] == 1
    P = world["P"]
    for method in ("direct", "cg"):
        got = lat.diffusion_gates_many(P, gamma=0.15, method=method)["gates"]
        for q in range(5):
            want = amd.compute_diffusion_gates(world["Y"], P[q], gamma=0.15, method=method, lattice=lat)
            np.testing.assert_allclose(got[q], want, atol=GATE_ATOL, rtol=0)
        # and against the lattice stored in API order: the same graph, the same gates up to the order of the sums
        np.testing.assert_allclose(got, world["lat"].diffusion_gates_many(P, gamma=0.15, method=method)["gates"],
                                   atol=GATE_ATOL, rtol=0)
    lat.close()


def test_the_call_changes_no_state(amd, world):
    Y, P = world["Y"], world["P"]
    lat = amd.Oscillink(Y, kneighbors=6)
    lat.set_query(P[0])
    lat.settle(max_iters=12, tol=1e-4)
    first = lat.bundle_many(P, k=5, as_arrays=True)
    U, sig, info = lat.U.copy(), lat.receipt()["meta"]["state_sig"], lat.build_info()
    stats, last = dict(lat.stats), dict(lat.last)
    psi, B = lat._psi.copy(), lat.B_diag.copy()
    lat.diffusion_gates_many(P, gamma=0.15)
    lat.diffusion_gates_many(P, gamma=0.15, method="cg")
    lat._U_host = None  # read U from the device again
    assert np.array_equal(lat.U, U) and lat.receipt()["meta"]["state_sig"] == sig
    assert lat.build_info() == info and dict(lat.last) == last
    assert np.array_equal(lat._psi, psi) and np.array_equal(lat.B_diag, B)
    again = lat.bundle_many(P, k=5, as_arrays=True)
    assert lat.stats["query_basis_solves"] == stats["query_basis_solves"]  # the cached basis still serves
    for a, b in zip(first, again):
        assert np.array_equal(a, b)
    lat.close()


def test_errors_and_the_empty_batch(amd, world):
    from oscillink_amd import _native as nat

    lat, P, Y = world["lat"], world["P"], world["Y"]
    with pytest.raises(ValueError, match=r"psis must be a \(Q, 96\) array"):
        lat.diffusion_gates_many(P[:, :95])
    with pytest.raises(ValueError, match=r"psis must be a \(Q, 96\) array"):
        lat.diffusion_gates_many(P[0])
    bad = P.copy()
    bad[3, 5] = np.nan
    with pytest.raises(ValueError, match="psis row 3 is not finite"):
        lat.diffusion_gates_many(bad)
    with pytest.raises(ValueError, match="gamma must be > 0 for SPD"):
        lat.diffusion_gates_many(P, gamma=0.0)
    with pytest.raises(ValueError, match="max_iters must be >= 1"):
        lat.diffusion_gates_many(P, method="cg", max_iters=0)
    with pytest.raises(ValueError, match="method"):
        lat.diffusion_gates_many(P, method="lu")
    # the C entry point holds the same line for callers that bypass Python
    g = np.zeros((5, 2000), np.float32)
    lib = nat.lib()
    assert lib.osc_gates_many(lat._h, nat.f32(P), 5, 1.0, 0.0, 0, 1e-4, 256, 1, nat.f32(g), None, None) == nat.OSC_E_INVALID
    assert lib.osc_last_error(lat._h).decode() == "gamma must be > 0 for SPD"
    assert lib.osc_gates_many(lat._h, nat.f32(P), 5, 1.0, 0.1, 1, 1e-4, 0, 1, nat.f32(g), None, None) == nat.OSC_E_INVALID
    assert lib.osc_last_error(lat._h).decode() == "max_iters must be >= 1"
    assert lib.osc_gates_many(lat._h, nat.f32(P), 5, 1.0, 0.1, 2, 1e-4, 256, 1, nat.f32(g), None, None) == nat.OSC_E_INVALID
    empty = lat.diffusion_gates_many(np.zeros((0, 96), np.float32))
    assert empty["gates"].shape == (0, 2000) and empty["gates"].dtype == np.float32
    assert empty["iters"].shape == (0,) and empty["iters"].dtype == np.int32
    assert empty["res"].shape == (0,) and empty["res"].dtype == np.float32
    assert amd.compute_diffusion_gates_many(Y, np.zeros((0, 96), np.float32), lattice=lat).shape == (0, 2000)
    # a lattice without a graph: what the single call's solve raises
    bare = amd.Oscillink(Y[:50], kneighbors=6, _build_graph=False)
    with pytest.raises(nat.NativeError) as single:
        amd.compute_diffusion_gates(Y[:50], P[0], lattice=bare)
    with pytest.raises(nat.NativeError) as many:
        bare.diffusion_gates_many(P)
    assert many.value.status == single.value.status == nat.OSC_E_STATE
    # a communicator: bundle_many's wording
    bare._has_comm = True
    with pytest.raises(NotImplementedError, match=r"lattices with a communicator \(sharded / multi-rank\) are not supported"):
        bare.diffusion_gates_many(P)
    bare._has_comm = False
    bare.close()
    with pytest.raises((ValueError, RuntimeError)):
        bare.diffusion_gates_many(P)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # finite gates: no warning
        lat.diffusion_gates_many(P[:1])

"""The streamed second apply of an anchor start ("Cached third row sums"): on top of the streamed first
apply (tests/test_gpu_anchor_ap.py) the cached INIT pass also leaves T = A (A p1), formed from the anchors' third row sums
W (W (W Y)) and W (W 1), iteration 2's p update forms A p2 = (1 + beta1) A p1 - m alpha1 T beside p2 (k_update_p_ap2), and
that iteration launches no gathering matvec either.  It is the same A p2 rounded differently, so the reference everywhere
is a second handle on the same inputs that runs depth 1 (OSC_ANCHOR_AP=1, OSC_ANCHOR_AP2=0); the handle under test runs
with both switches at 1.  Iteration counts equal, residual histories to rtol 1e-5, U to 2e-6 relative (the bounds the
suite holds two routes to that differ by fp32 rounding; a CPU model of the route in fp32 gives 2.3e-6 / 3.2e-7), and
against the CPU oracle on the device-built graph the streamed route may be at most 2.5 times as far off as the gathered
one (OSC_ANCHOR_AP=0), measured in the same test: the model says 1.6-1.7, from the cancellation in (1 + beta1) A p1 -
m alpha1 T while the residual falls ~30 x per iteration.  Wherever the route must NOT be taken (per-row gates, a chain
prior, a start from a written U, OSC_ANCHOR_AP=0, max_iters = 1, auto mode below 96 000 rows) the two handles agree to the
bit.

Shapes: those of tests/test_gpu_anchor_ap.py (see there why)."""
import numpy as np
import pytest

from tests._cases import relerr
from tests._fullsize import oracle_solves

pytestmark = pytest.mark.gpu

SWITCHES = ("OSC_SPMM_XS", "OSC_REORDER", "OSC_SPMM_BLOCKED", "OSC_BLK_VARIANT", "OSC_BLK_INIT", "OSC_X_DEFER", "OSC_X_RING",
            "OSC_ANCHOR_SLAB", "OSC_ANCHOR_WY", "OSC_ANCHOR_AP", "OSC_ANCHOR_AP2", "OSC_BALANCE", "OSC_SMALL_PATH",
            "OSC_FAKE_COL_SHARD", "OSC_SHARD", "OSC_ROW_FAKE_SHARDS", "OSC_LD", "OSCILLINK_RECEIPT_DYNAMICS")
CHAIN = [5, 1, 19999, 9000, 7, 2]
KW = dict(max_iters=12, tol=1e-3)
U_TOL = 2e-6
HIST_RTOL = 1e-5
ORACLE_FACTOR = 2.5


@pytest.fixture(scope="module")
def amd():
    import oscillink_amd
    from oscillink_amd import _native

    assert _native.device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return oscillink_amd


@pytest.fixture(scope="module")
def orc():
    from oracle import oscillink_oracle

    return oscillink_oracle


def _inputs(N, D, seed=3):
    rng = np.random.default_rng(seed)
    Y = rng.standard_normal((N, D)).astype(np.float32)
    psi = rng.standard_normal(D).astype(np.float32)
    psi /= np.linalg.norm(psi)
    psi2 = rng.standard_normal(D).astype(np.float32)
    psi2 /= np.linalg.norm(psi2)
    gates = rng.uniform(0.1, 1.0, N).astype(np.float32)
    return Y, psi, psi2, gates


def _clean_env(monkeypatch):
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)


def _make(amd, monkeypatch, Y, psi, k, ap, ap2, gates=None, chain=None):
    for name, v in (("OSC_ANCHOR_AP", ap), ("OSC_ANCHOR_AP2", ap2)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)
    lat = amd.Oscillink(Y, kneighbors=k)
    lat.set_query(psi, gates=gates)
    if chain:
        lat.add_chain(chain, lamP=0.3)
    return lat


class _Pair:
    """Two lattices over the same inputs: `ref` at depth 1 (OSC_ANCHOR_AP=`ref_ap`, OSC_ANCHOR_AP2=0), `ap` under
    OSC_ANCHOR_AP=`ap` and OSC_ANCHOR_AP2=`ap2` (None: unset).  The solver's switches are fixed at creation."""

    def __init__(self, amd, monkeypatch, Y, psi, k, gates=None, chain=None, ap="1", ap2="1", ref_ap="1"):
        self.ref = _make(amd, monkeypatch, Y, psi, k, ref_ap, "0", gates, chain)
        self.ap = _make(amd, monkeypatch, Y, psi, k, ap, ap2, gates, chain)
        self.both = (self.ref, self.ap)

    def close(self):
        self.ref.close()
        self.ap.close()

    def counts(self):
        """(streamed second applies, cache builds) of `ap`; `ref` never takes the route"""
        r = self.ref.build_info()
        assert (r["streamed_second_applies"], r["anchor_ap2_bytes"], r["anchor_ap2_builds"], r["anchor_ap2_last_solve"]) == (0, 0, 0, 0), r
        a = self.ap.build_info()
        return a["streamed_second_applies"], a["anchor_ap2_builds"]


def _anchor_start(lat, **kw):
    lat.reset_U(wait=False)
    st = lat.settle(**dict(KW, **kw))
    return st["iters"], st["res"], lat.residual_history(), lat.U.copy()


def _agree(x, y, what):
    """y (depth 2) against x (depth 1): the same A p2 rounded differently"""
    assert x[0] == y[0], (what, "iters", x[0], y[0])
    hx, hy = np.asarray(x[2], dtype=np.float64), np.asarray(y[2], dtype=np.float64)
    e = relerr(y[3], x[3])
    print(f"{what}: iters {x[0]} history max rel {np.max(np.abs(hy - hx) / np.abs(hx)) if hx.size else 0.0:.3e} U rel {e:.3e}")
    assert np.allclose(hy, hx, rtol=HIST_RTOL, atol=0.0), (what, "history", x[2], y[2])
    assert e < U_TOL, (what, "U", e)


def _same(x, y, what):
    assert x[0] == y[0], (what, "iters", x[0], y[0])
    assert np.array_equal(x[2], y[2], equal_nan=True), (what, "history", x[2], y[2])
    assert np.array_equal(x[3], y[3], equal_nan=True), (what, "U")


def _both_start(pair, what, compare=_agree, **kw):
    """One anchor start on both lattices, compared; returns (second applies streamed, cache builds, matvecs saved against the
    depth-1 handle) of this solve."""
    s0, b0 = pair.counts()
    m0 = [lat.build_info()["blocked_applies"] for lat in pair.both]
    f0 = [lat.build_info()["streamed_first_applies"] for lat in pair.both]
    compare(_anchor_start(pair.ref, **kw), _anchor_start(pair.ap, **kw), what)
    s1, b1 = pair.counts()
    m1 = [lat.build_info()["blocked_applies"] for lat in pair.both]
    f1 = [lat.build_info()["streamed_first_applies"] for lat in pair.both]
    assert f1[0] - f0[0] == f1[1] - f0[1], (what, "first applies", f0, f1)  # (depth 1 is the same on both)
    if s1 - s0:
        assert pair.ap.build_info()["anchor_ap2_last_solve"] == 1 == pair.ap.build_info()["anchor_ap_last_solve"], what
    return s1 - s0, b1 - b0, (m1[0] - m0[0]) - (m1[1] - m0[1])


def _ustar(pair, what):
    s0, b0 = pair.counts()
    m0 = [lat.build_info()["blocked_applies"] for lat in pair.both]
    us = [lat.solve_Ustar(use_cache=False).copy() for lat in pair.both]
    hs = [np.asarray(lat.residual_history(), dtype=np.float64) for lat in pair.both]
    assert len(hs[0]) == len(hs[1]), (what, "U* iters", len(hs[0]), len(hs[1]))
    e = relerr(us[1], us[0])
    print(f"{what}: U* iters {len(hs[0])} history max rel {np.max(np.abs(hs[1] - hs[0]) / np.abs(hs[0])):.3e} U* rel {e:.3e}")
    assert np.allclose(hs[1], hs[0], rtol=HIST_RTOL, atol=0.0), (what, "U* history", hs)
    assert e < U_TOL, (what, "U*", e)
    s1, b1 = pair.counts()
    m1 = [lat.build_info()["blocked_applies"] for lat in pair.both]
    return s1 - s0, b1 - b0, (m1[0] - m0[0]) - (m1[1] - m0[1])


SHAPES = {
    "default": dict(N=20000, D=256),
    "wide_shape": dict(N=20000, D=256, env={"OSC_BLK_VARIANT": "3"}, shape=3),
    "ragged": dict(N=20011, D=200, env={"OSC_LD": "224", "OSC_SPMM_XS": "1"}),
    "column_window": dict(N=20000, D=256, env={"OSC_FAKE_COL_SHARD": "1/2"}, window=True),
    "balanced_rows": dict(N=20000, D=256, env={"OSC_BALANCE": "1"}, order="balanced"),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_streamed_second_apply_agrees_with_depth_one(amd, name, monkeypatch):
    """Build, the start that forms both caches, a third start, the U* solve, then other lams and another psi: the cache
    stays, every solve from the one that holds it on saves exactly one more blocked matvec than depth 1."""
    _clean_env(monkeypatch)
    spec = SHAPES[name]
    for k, v in spec.get("env", {}).items():
        monkeypatch.setenv(k, v)
    N, D = spec["N"], spec["D"]
    Y, psi, psi2, _ = _inputs(N, D)
    pair = _Pair(amd, monkeypatch, Y, psi, 16)
    try:
        if spec.get("window"):  # (the settles start from U's own copy: depth 1's bytes; the U* solves take the route)
            for trip in range(2):
                assert _both_start(pair, (name, "settle", trip), compare=_same) == (0, 0, 0)
            assert _ustar(pair, (name, "first")) == (0, 0, 0)
            assert pair.ap.build_info()["anchor_ap2_bytes"] == 0
            assert _ustar(pair, (name, "second")) == (1, 1, 1)
            assert _ustar(pair, (name, "third")) == (1, 0, 1)
            assert _both_start(pair, (name, "settle", 2), compare=_same) == (0, 0, 0)
            assert _ustar(pair, (name, "fourth")) == (1, 0, 1)
        else:
            assert _both_start(pair, (name, "first")) == (0, 0, 0)
            assert pair.ap.build_info()["anchor_ap2_bytes"] == 0
            assert _both_start(pair, (name, "second")) == (1, 1, 1)
            assert _both_start(pair, (name, "third")) == (1, 0, 1)
            assert _ustar(pair, name) == (1, 0, 1)
        for lat in pair.both:
            lat.set_query(psi2, gates=None)
            lat.lamC, lat.lamQ = 0.8, 2.5
        if spec.get("window"):
            assert _both_start(pair, (name, "other query and lams"), compare=_same) == (0, 0, 0)
        else:
            assert _both_start(pair, (name, "other query and lams")) == (1, 0, 1)
        assert _ustar(pair, (name, "other query and lams")) == (1, 0, 1)
        info = pair.ap.build_info()
        assert info["apply_src_blocks"] > 0 and info["small_solves"] == 0, info
        if "shape" in spec:
            assert info["apply_blocked_shape"] == spec["shape"], info
        if "order" in spec:
            assert info["order_kind"] == spec["order"], info
        assert info["anchor_ap_bytes"] == info["anchor_wy_bytes"] + N * 4 > 0, info
        assert info["anchor_ap2_bytes"] == 2 * info["anchor_wy_bytes"] + N * 4, info
        assert info["anchor_ap2_builds"] == 1 == info["anchor_ap_builds"], info
    finally:
        pair.close()


def test_against_the_cpu_oracle(amd, orc, monkeypatch):
    """The CPU oracle on the device-built graph, the device's iteration counts executed: the depth-2 route's error against it
    is at most 2.5 times the gathered route's (OSC_ANCHOR_AP=0), for the settle and for the U* solve."""
    import scipy.sparse as sp

    _clean_env(monkeypatch)
    N, D, k = 20000, 256, 16
    Y, psi, _, _ = _inputs(N, D, seed=5)
    pair = _Pair(amd, monkeypatch, Y, psi, k)
    gathered = _make(amd, monkeypatch, Y, psi, k, "0", "1")
    try:
        for trip in range(3):
            took = _both_start(pair, ("oracle", trip))
            g = _anchor_start(gathered)
        assert took == (1, 0, 1)
        assert gathered.build_info()["streamed_first_applies"] == 0 == gathered.build_info()["streamed_second_applies"]
        lats = (gathered, pair.ref, pair.ap)
        U = [g[3], pair.ref.U.copy(), pair.ap.U.copy()]
        iters = len(pair.ap.residual_history())
        assert iters == len(pair.ref.residual_history()) == g[0]
        s0, _ = pair.counts()
        Us = [lat.solve_Ustar(use_cache=False).copy() for lat in lats]
        assert pair.counts()[0] == s0 + 1
        uiters = len(pair.ap.residual_history())
        assert uiters == len(pair.ref.residual_history()) == len(gathered.residual_history())
        csr = pair.ref.graph_csr()[:3]
        assert all(np.array_equal(a, b) for a, b in zip(csr, pair.ap.graph_csr()[:3]))
        A = sp.csr_matrix((csr[2], csr[1], csr[0]), shape=(N, N), dtype=np.float32)
        ref = oracle_solves(orc, Y, psi, A, k=k, settle_iters=iters, settle_tol=1e-3, ustar_iters=uiters)
        for what, got, want in (("settle", U, ref["U"]), ("U*", Us, ref["Ustar"])):
            e_g, e_1, e_2 = (relerr(x, want) for x in got)
            print(f"oracle {what}: gathered {e_g:.3e} depth 1 {e_1:.3e} depth 2 {e_2:.3e} ratio {e_2 / e_g:.2f}")
            assert e_2 <= ORACLE_FACTOR * e_g, (what, e_g, e_1, e_2)
    finally:
        gathered.close()
        pair.close()


def test_uniform_gates_other_than_one_and_dt(amd, monkeypatch):
    _clean_env(monkeypatch)
    N, D = 20000, 256
    Y, psi, _, _ = _inputs(N, D, seed=6)
    pair = _Pair(amd, monkeypatch, Y, psi, 16, gates=np.full(N, 0.5, np.float32))
    try:
        assert _both_start(pair, "gates 0.5, first") == (0, 0, 0)
        assert _both_start(pair, "gates 0.5, second") == (1, 1, 1)
        assert _both_start(pair, "gates 0.5, third") == (1, 0, 1)
        assert _ustar(pair, "gates 0.5") == (1, 0, 1)
        for dt in (0.5, 2.0):
            assert _both_start(pair, f"gates 0.5, dt {dt}", dt=dt) == (1, 0, 1)
    finally:
        pair.close()


@pytest.mark.parametrize("ring", ["0", "2", "4"])
def test_stops_guesses_and_iteration_limits(amd, ring, monkeypatch):
    """Solves that stop at iteration 1 and at iteration 2 (tol from the reference's history), each first under a guess that is
    too long, then under the right one, then the next solve under one that is too short (the r update redone, iteration 2
    enqueued behind the residual); max_iters 1 (depth 1's bytes: the route needs a second iteration) and 2; with the
    direction ring off, at two and at four slots."""
    _clean_env(monkeypatch)
    monkeypatch.setenv("OSC_X_RING", ring)
    Y, psi, _, _ = _inputs(20000, 256, seed=12)
    pair = _Pair(amd, monkeypatch, Y, psi, 16)
    try:
        assert _both_start(pair, "first") == (0, 0, 0)
        assert _both_start(pair, "second") == (1, 1, 1)
        hist = pair.ref.residual_history()
        full = len(hist)
        assert full >= 4, hist
        tol1 = float(hist[0]) * 1.5  # (the residual falls ~30 x per iteration: far from either neighbour)
        tol2 = float(np.sqrt(hist[0] * hist[1]))
        info = pair.ap.build_info()
        assert info["x_ring_slots"] == (1 if ring == "0" else int(ring)), info
        steps = [("stop at 1, guess long", dict(tol=tol1), 1, 1), ("stop at 1, guess right", dict(tol=tol1), 1, 0),
                 ("stop at 2, guess short", dict(tol=tol2), 2, 1), ("stop at 2, guess right", dict(tol=tol2), 2, 1),
                 ("guess short at 2", {}, full, 1), ("guess right", {}, full, 1),
                 ("max_iters 2, guess long", dict(max_iters=2, tol=0.0), 2, 1), ("max_iters 2", dict(max_iters=2, tol=0.0), 2, 1),
                 ("guess short at max_iters 2", {}, full, 1)]
        for what, kw, iters, second in steps:
            took = _both_start(pair, (ring, what), **kw)
            assert took == (second, 0, second), (what, took)
            assert pair.ap.last["iters"] == iters, (what, pair.ap.last)
        for trip in range(2):
            assert _both_start(pair, (ring, "max_iters 1", trip), compare=_same, max_iters=1, tol=0.0) == (0, 0, 0)
            assert pair.ap.build_info()["anchor_ap2_last_solve"] == 0 and pair.ap.build_info()["anchor_ap_last_solve"] == 1
        assert _both_start(pair, (ring, "guess short at max_iters 1")) == (1, 0, 1)
    finally:
        pair.close()


@pytest.mark.parametrize("name", ["per_row_gates", "chain_prior", "written_U", "first_apply_off"])
def test_other_solver_inputs_keep_the_reference_bytes(amd, name, monkeypatch):
    """Per-row gates, a chain prior, a start from a written U and OSC_ANCHOR_AP=0 leave no depth-1 route to build on: the
    results are the other handle's bytes and nothing is formed."""
    _clean_env(monkeypatch)
    N, D = 20000, 256
    Y, psi, _, gates = _inputs(N, D, seed=7)
    off = "0" if name == "first_apply_off" else "1"
    pair = _Pair(amd, monkeypatch, Y, psi, 16, gates=gates if name == "per_row_gates" else None,
                 chain=CHAIN if name == "chain_prior" else None, ap=off, ref_ap=off)
    try:
        if name == "written_U":
            for trip in range(2):  # (the caches exist: the start below must not use them)
                _both_start(pair, (name, "anchor start", trip))
            U0 = (Y * np.float32(0.5)).astype(np.float32)
            for trip in range(2):
                s0, b0 = pair.counts()
                outs = []
                for lat in pair.both:
                    lat.U = U0
                    st = lat.settle(**KW)
                    outs.append((st["iters"], st["res"], lat.residual_history(), lat.U.copy()))
                _same(outs[0], outs[1], (name, trip))
                assert pair.counts() == (s0, b0) and pair.ap.build_info()["anchor_ap2_last_solve"] == 0
            return
        for trip in range(3):
            assert _both_start(pair, (name, trip), compare=_same) == (0, 0, 0)
        us = [lat.solve_Ustar(use_cache=False).copy() for lat in pair.both]
        assert np.array_equal(us[0], us[1])
        info = pair.ap.build_info()
        assert pair.counts() == (0, 0) and info["anchor_ap2_bytes"] == 0 and info["anchor_ap_bytes"] == 0, info
        if name == "per_row_gates":  # uniform gates again: the route opens
            for lat in pair.both:
                lat.set_gates(np.ones(N, np.float32))
            assert _both_start(pair, (name, "uniform again")) == (1, 1, 1)
    finally:
        pair.close()


def test_everything_that_drops_the_second_sums_drops_the_third(amd, monkeypatch):
    """The third row sums go with W.(W.Y): a rebuilt or injected graph, an append (a new handle), a new row order and a new
    column window drop them, the next anchor start gathers (and leaves W.Y behind), the one after it forms them anew."""
    from oscillink_amd import _native as nat
    from oscillink_amd import sharding

    _clean_env(monkeypatch)
    N, D = 20000, 256
    Y, psi, _, _ = _inputs(N, D, seed=8)
    pair = _Pair(amd, monkeypatch, Y, psi, 16)
    donor = amd.Oscillink(Y, kneighbors=9)
    try:
        assert _both_start(pair, "first") == (0, 0, 0)
        assert _both_start(pair, "second") == (1, 1, 1)
        full = (2 * N * 256 + N) * 4
        assert pair.ap.build_info()["anchor_ap2_bytes"] == full
        for lat in pair.both:
            lat.rebuild_graph(kneighbors=12)
        info = pair.ap.build_info()
        assert info["anchor_ap2_bytes"] == 0 == info["anchor_ap_bytes"] == info["anchor_wy_bytes"], info
        assert _both_start(pair, "after rebuild_graph") == (0, 0, 0)
        assert _both_start(pair, "second after rebuild_graph") == (1, 1, 1)
        rowptr, col, a = donor._host_csr()[:3]
        for lat in pair.both:
            lat.set_graph_csr(rowptr, col, a)
        assert pair.ap.build_info()["anchor_ap2_bytes"] == 0
        assert _both_start(pair, "after set_graph_csr") == (0, 0, 0)
        assert _both_start(pair, "second after set_graph_csr") == (1, 1, 1)
        assert pair.ap.build_info()["anchor_ap2_bytes"] == full
        monkeypatch.setenv("OSC_BALANCE", "1")  # (a rebuild reads the build switches again: a new row order)
        for lat in pair.both:
            lat.rebuild_graph(kneighbors=16)
        assert pair.ap.build_info()["order_kind"] == "balanced" and pair.ap.build_info()["anchor_ap2_bytes"] == 0
        assert _both_start(pair, "after the row order changed") == (0, 0, 0)
        assert _both_start(pair, "second after the row order changed") == (1, 1, 1)
        monkeypatch.delenv("OSC_BALANCE")
        more = _inputs(64, D, seed=9)[0]
        for lat, ap2 in zip(pair.both, ("0", "1")):  # (an append makes a new handle, which reads the solver's switches)
            monkeypatch.setenv("OSC_ANCHOR_AP2", ap2)
            lat.append(more)
        info = pair.ap.build_info()
        assert info["anchor_ap2_bytes"] == 0 == info["anchor_ap2_builds"] == info["streamed_second_applies"], info
        assert _both_start(pair, "after append") == (0, 0, 0)
        assert _both_start(pair, "second after append") == (1, 1, 1)
        assert pair.ap.build_info()["anchor_ap2_bytes"] == (2 * (N + 64) * 256 + N + 64) * 4
    finally:
        donor.close()
        pair.close()

    def rank_fn(rank, comm):
        uid, _, world = comm
        lat = amd.Oscillink(Y, kneighbors=16)
        try:
            lat.set_query(psi)
            for _ in range(2):
                lat.reset_U()
                lat.settle(**KW)
            before = lat.build_info()
            nat.check(nat.lib().osc_comm_init(lat._h, bytes(uid), int(rank), int(world)), lat._h, "osc_comm_init")
            return before, lat.build_info()
        finally:
            lat.close()

    monkeypatch.setenv("OSC_ANCHOR_AP", "1")
    monkeypatch.setenv("OSC_ANCHOR_AP2", "1")
    for before, after in sharding.run_loopback_ranks(2, rank_fn, timeout_s=120.0):
        assert before["streamed_second_applies"] == 1 and before["anchor_ap2_bytes"] == (2 * N * 256 + N) * 4, before
        assert after["anchor_ap2_bytes"] == 0 and after["anchor_ap_bytes"] == 0 and after["anchor_wy_bytes"] == 0, after


def test_nan_column(amd, monkeypatch):
    """A NaN in psi makes column 3 of the right-hand side NaN: that column stays NaN, the stop test is never met, the other
    columns are untouched -- at depth 2 as at depth 1."""
    _clean_env(monkeypatch)
    N, D = 20000, 256
    Y, psi, _, _ = _inputs(N, D, seed=9)
    psi = psi.copy()
    psi[3] = np.nan
    pair = _Pair(amd, monkeypatch, Y, psi, 16)
    try:
        for trip in range(3):
            s0, _ = pair.counts()
            out = [_anchor_start(lat, max_iters=5) for lat in pair.both]
            assert pair.counts()[0] - s0 == (1 if trip > 0 else 0)
            for iters, res, hist, U in out:
                assert iters == 5 and np.isnan(res) and np.isnan(hist).all(), (trip, iters, res, hist)
                assert np.isnan(U[:, 3]).all() and np.isfinite(np.delete(U, 3, axis=1)).all(), trip
            assert np.array_equal(np.isnan(out[0][3]), np.isnan(out[1][3]))
            assert relerr(np.delete(out[1][3], 3, axis=1), np.delete(out[0][3], 3, axis=1)) < U_TOL
    finally:
        pair.close()


def test_two_handles_give_the_same_bytes(amd, monkeypatch):
    _clean_env(monkeypatch)
    Y, psi, _, _ = _inputs(20000, 256, seed=10)
    lats = [_make(amd, monkeypatch, Y, psi, 16, "1", "1") for _ in range(2)]
    try:
        for trip in range(3):
            outs = [_anchor_start(lat) for lat in lats]
            _same(outs[0], outs[1], ("repeat", trip))
        us = [lat.solve_Ustar(use_cache=False).copy() for lat in lats]
        assert np.array_equal(us[0], us[1])
        assert all(lat.build_info()["streamed_second_applies"] == 3 for lat in lats)
    finally:
        for lat in lats:
            lat.close()


def test_an_unset_switch_leaves_small_lattices_at_depth_one(amd, monkeypatch):
    """Below 96 000 rows the default keeps depth 1 where OSC_ANCHOR_AP=1 forces that: the bytes of the OSC_ANCHOR_AP2=0
    handle, and OSC_ANCHOR_AP=1 alone keeps meaning exactly one matvec saved."""
    _clean_env(monkeypatch)
    Y, psi, _, _ = _inputs(20000, 256, seed=11)
    pair = _Pair(amd, monkeypatch, Y, psi, 16, ap2=None)
    try:
        for trip in range(3):
            assert _both_start(pair, ("unset", trip), compare=_same) == (0, 0, 0)
        info = pair.ap.build_info()
        assert info["streamed_first_applies"] == 2 and info["anchor_ap2_bytes"] == 0 and info["anchor_ap2_builds"] == 0, info
    finally:
        pair.close()

"""The streamed first apply of an anchor start ("Cached second row sums"): under uniform gates and
without a chain prior iteration 1's A p is a per-row scalar combination of psi, W Y and W (W Y), so from a lattice's second
anchor start on the cached INIT pass emits it (k_init_cached_ap) and that iteration's gathering matvec is not launched.  It
is the same A p rounded differently, so the reference everywhere is a second handle created under OSC_ANCHOR_AP=0 on the
same inputs (the gathered route): iteration counts equal, residual histories to rtol 1e-5, U to 2e-6 relative -- the bound
the suite holds two routes to that differ by fp32 summation order -- and against the CPU oracle on the device-built graph
the streamed route may be at most 1.5 times as far off as the gathered one.  Wherever the route must NOT be taken (per-row
gates, a chain prior, auto mode below 96 000 rows) the two handles agree to the bit.

Shapes: 20 000 x 256 at k = 16 is the smallest default plan with source blocks (tests/test_gpu_anchor_wy.py); the same
under OSC_BLK_VARIANT=3 (wide shape: other batch geometry); 20 011 x 200 (rows no multiple of a deal of groups, the last
slab 8 of 32 columns; below 24 576 rows a 200-column lattice gets the blocked plan only under OSC_SPMM_XS=1 with a 128-byte
row pitch, OSC_LD=224, as tests/test_gpu_block_balance.py forces it); the column window 128..256 of OSC_FAKE_COL_SHARD=1/2
(a windowed handle's U is a copy of the anchors, never their alias, so its settles start from U and only its U* solves are
anchor starts); OSC_BALANCE=1 (rows stored permuted)."""
import numpy as np
import pytest

from tests._cases import relerr
from tests._fullsize import oracle_solves

pytestmark = pytest.mark.gpu

SWITCHES = ("OSC_SPMM_XS", "OSC_REORDER", "OSC_SPMM_BLOCKED", "OSC_BLK_VARIANT", "OSC_BLK_INIT", "OSC_X_DEFER", "OSC_X_RING",
            "OSC_ANCHOR_SLAB", "OSC_ANCHOR_WY", "OSC_ANCHOR_AP", "OSC_BALANCE", "OSC_SMALL_PATH", "OSC_FAKE_COL_SHARD", "OSC_SHARD",
            "OSC_ROW_FAKE_SHARDS", "OSC_LD", "OSCILLINK_RECEIPT_DYNAMICS")
CHAIN = [5, 1, 19999, 9000, 7, 2]
KW = dict(max_iters=12, tol=1e-3)
U_TOL = 2e-6
HIST_RTOL = 1e-5


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


class _Pair:
    """Two lattices over the same inputs: `ref` created under OSC_ANCHOR_AP=0 (the gathered first apply), `ap` under
    `mode` ("1": the route wherever the cached INIT pass runs; None: auto mode)."""

    def __init__(self, amd, monkeypatch, Y, psi, k, gates=None, chain=None, mode="1"):
        def make():
            lat = amd.Oscillink(Y, kneighbors=k)
            lat.set_query(psi, gates=gates)
            if chain:
                lat.add_chain(chain, lamP=0.3)
            return lat

        monkeypatch.setenv("OSC_ANCHOR_AP", "0")
        self.ref = make()
        if mode is None:
            monkeypatch.delenv("OSC_ANCHOR_AP")
        else:
            monkeypatch.setenv("OSC_ANCHOR_AP", mode)
        self.ap = make()
        self.both = (self.ref, self.ap)

    def close(self):
        self.ref.close()
        self.ap.close()

    def counts(self):
        """(streamed first applies, cache builds) of `ap`; `ref` never takes the route"""
        r = self.ref.build_info()
        assert (r["streamed_first_applies"], r["anchor_ap_bytes"], r["anchor_ap_builds"], r["anchor_ap_last_solve"]) == (0, 0, 0, 0), r
        a = self.ap.build_info()
        return a["streamed_first_applies"], a["anchor_ap_builds"]


def _anchor_start(lat, **kw):
    lat.reset_U(wait=False)
    st = lat.settle(**dict(KW, **kw))
    return st["iters"], st["res"], lat.residual_history(), lat.U.copy()


def _agree(x, y, what):
    """y (streamed) against x (gathered): the same A p1 rounded differently"""
    assert x[0] == y[0], (what, "iters", x[0], y[0])
    assert np.allclose(y[2], x[2], rtol=HIST_RTOL, atol=0.0), (what, "history", x[2], y[2])
    e = relerr(y[3], x[3])
    assert e < U_TOL, (what, "U", e)


def _same(x, y, what):
    assert x[0] == y[0], (what, "iters", x[0], y[0])
    assert np.array_equal(x[2], y[2], equal_nan=True), (what, "history", x[2], y[2])
    assert np.array_equal(x[3], y[3], equal_nan=True), (what, "U")


def _both_start(pair, what, compare=_agree, **kw):
    """One anchor start on both lattices, compared; returns (streamed applies, cache builds, matvecs saved) of this solve."""
    s0, b0 = pair.counts()
    m0 = [lat.build_info()["blocked_applies"] for lat in pair.both]
    compare(_anchor_start(pair.ref, **kw), _anchor_start(pair.ap, **kw), what)
    s1, b1 = pair.counts()
    m1 = [lat.build_info()["blocked_applies"] for lat in pair.both]
    assert pair.ap.build_info()["anchor_ap_last_solve"] == s1 - s0, what
    return s1 - s0, b1 - b0, (m1[0] - m0[0]) - (m1[1] - m0[1])


def _ustar(pair, what):
    s0, b0 = pair.counts()
    us = [lat.solve_Ustar(use_cache=False).copy() for lat in pair.both]
    hs = [lat.residual_history() for lat in pair.both]
    assert len(hs[0]) == len(hs[1]), (what, "U* iters", len(hs[0]), len(hs[1]))
    assert np.allclose(hs[1], hs[0], rtol=HIST_RTOL, atol=0.0), (what, "U* history", hs)
    e = relerr(us[1], us[0])
    assert e < U_TOL, (what, "U*", e)
    s1, b1 = pair.counts()
    return s1 - s0, b1 - b0


SHAPES = {
    "default": dict(N=20000, D=256),
    "wide_shape": dict(N=20000, D=256, env={"OSC_BLK_VARIANT": "3"}, shape=3),
    "ragged": dict(N=20011, D=200, env={"OSC_LD": "224", "OSC_SPMM_XS": "1"}),
    "column_window": dict(N=20000, D=256, env={"OSC_FAKE_COL_SHARD": "1/2"}, window=True),
    "balanced_rows": dict(N=20000, D=256, env={"OSC_BALANCE": "1"}, order="balanced"),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_streamed_first_apply_agrees_with_the_gathered_one(amd, name, monkeypatch):
    """Build, the start that forms the cache, a third start, the U* solve, then other lams and another psi: the cache stays,
    every solve from the second on saves exactly one blocked matvec."""
    _clean_env(monkeypatch)
    spec = SHAPES[name]
    for k, v in spec.get("env", {}).items():
        monkeypatch.setenv(k, v)
    N, D = spec["N"], spec["D"]
    Y, psi, psi2, _ = _inputs(N, D)
    pair = _Pair(amd, monkeypatch, Y, psi, 16)
    try:
        if spec.get("window"):  # (the settles start from U's own copy: the gathered route's bytes; the U* solves take the route)
            for trip in range(2):
                assert _both_start(pair, (name, "settle", trip), compare=_same) == (0, 0, 0)
            assert _ustar(pair, (name, "first")) == (0, 0)
            assert pair.ap.build_info()["anchor_ap_bytes"] == 0
            assert _ustar(pair, (name, "second")) == (1, 1)
            assert _ustar(pair, (name, "third")) == (1, 0)
            assert _both_start(pair, (name, "settle", 2), compare=_same) == (0, 0, 0)
            assert _ustar(pair, (name, "fourth")) == (1, 0)
        else:
            assert _both_start(pair, (name, "first")) == (0, 0, 0)
            assert pair.ap.build_info()["anchor_ap_bytes"] == 0
            assert _both_start(pair, (name, "second")) == (1, 1, 1)
            assert _both_start(pair, (name, "third")) == (1, 0, 1)
            assert _ustar(pair, name) == (1, 0)
        for lat in pair.both:
            lat.set_query(psi2, gates=None)
            lat.lamC, lat.lamQ = 0.8, 2.5
        assert _both_start(pair, (name, "other query and lams"), compare=_same if spec.get("window") else _agree)[:2] == (0 if spec.get("window") else 1, 0)
        assert _ustar(pair, (name, "other query and lams")) == (1, 0)
        info = pair.ap.build_info()
        assert info["apply_src_blocks"] > 0 and info["small_solves"] == 0, info
        if "shape" in spec:
            assert info["apply_blocked_shape"] == spec["shape"], info
        if "order" in spec:
            assert info["order_kind"] == spec["order"], info
        assert info["anchor_ap_bytes"] == info["anchor_wy_bytes"] + N * 4 > 0, info
        assert info["cached_inits"] == pair.ref.build_info()["cached_inits"] == (4 if spec.get("window") else 5), info
    finally:
        pair.close()


def test_against_the_cpu_oracle(amd, orc, monkeypatch):
    """The CPU oracle on the device-built graph, the device's iteration counts executed: the streamed route's error against
    it is at most 1.5 times the gathered route's, for the settle and for the U* solve."""
    import scipy.sparse as sp

    _clean_env(monkeypatch)
    N, D, k = 20000, 256, 16
    Y, psi, _, _ = _inputs(N, D, seed=5)
    pair = _Pair(amd, monkeypatch, Y, psi, k)
    try:
        for trip in range(3):
            took = _both_start(pair, ("oracle", trip))
        assert took[0] == 1
        U = [lat.U.copy() for lat in pair.both]
        iters = len(pair.ap.residual_history())
        assert iters == len(pair.ref.residual_history())
        s0, _ = pair.counts()
        Us = [lat.solve_Ustar(use_cache=False).copy() for lat in pair.both]
        assert pair.counts()[0] == s0 + 1
        uiters = len(pair.ap.residual_history())
        assert uiters == len(pair.ref.residual_history())
        csr = pair.ref.graph_csr()[:3]
        assert all(np.array_equal(a, b) for a, b in zip(csr, pair.ap.graph_csr()[:3]))
        A = sp.csr_matrix((csr[2], csr[1], csr[0]), shape=(N, N), dtype=np.float32)
        ref = oracle_solves(orc, Y, psi, A, k=k, settle_iters=iters, settle_tol=1e-3, ustar_iters=uiters)
        for what, got, want in (("settle", U, ref["U"]), ("U*", Us, ref["Ustar"])):
            gathered, streamed = relerr(got[0], want), relerr(got[1], want)
            print(f"oracle {what}: gathered {gathered:.3e} streamed {streamed:.3e}")
            assert streamed <= 1.5 * gathered, (what, gathered, streamed)
    finally:
        pair.close()


def test_uniform_gates_other_than_one(amd, monkeypatch):
    _clean_env(monkeypatch)
    N, D = 20000, 256
    Y, psi, _, _ = _inputs(N, D, seed=6)
    pair = _Pair(amd, monkeypatch, Y, psi, 16, gates=np.full(N, 0.5, np.float32))
    try:
        assert _both_start(pair, "gates 0.5, first") == (0, 0, 0)
        assert _both_start(pair, "gates 0.5, second") == (1, 1, 1)
        assert _both_start(pair, "gates 0.5, third") == (1, 0, 1)
        assert _ustar(pair, "gates 0.5") == (1, 0)
    finally:
        pair.close()


@pytest.mark.parametrize("name", ["per_row_gates", "chain_prior"])
def test_other_solver_inputs_keep_the_gathered_apply(amd, name, monkeypatch):
    """Per-row gates make the combination's coefficients per-row inside the sum, a chain prior adds rows to the operator:
    neither takes the route, and the results are the other handle's bytes."""
    _clean_env(monkeypatch)
    N, D = 20000, 256
    Y, psi, _, gates = _inputs(N, D, seed=7)
    pair = _Pair(amd, monkeypatch, Y, psi, 16, gates=gates if name == "per_row_gates" else None,
                 chain=CHAIN if name == "chain_prior" else None)
    try:
        for trip in range(3):
            assert _both_start(pair, (name, trip), compare=_same) == (0, 0, 0)
        us = [lat.solve_Ustar(use_cache=False).copy() for lat in pair.both]
        assert np.array_equal(us[0], us[1])
        assert pair.counts() == (0, 0) and pair.ap.build_info()["anchor_ap_bytes"] == 0
        assert pair.ap.build_info()["cached_inits"] == 3
        if name == "per_row_gates":  # uniform gates again: the route opens
            for lat in pair.both:
                lat.set_gates(np.ones(N, np.float32))
            assert _both_start(pair, (name, "uniform again")) == (1, 1, 1)
    finally:
        pair.close()


def test_graph_changes_and_a_communicator_drop_the_cache(amd, monkeypatch):
    """The second row sums go with W.Y: a rebuilt or injected graph and a new column window drop both, the next anchor
    start gathers (and leaves W.Y behind), the one after it forms the second sums anew."""
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
        for lat in pair.both:
            lat.rebuild_graph(kneighbors=12)
        assert pair.ap.build_info()["anchor_ap_bytes"] == 0 == pair.ap.build_info()["anchor_wy_bytes"]
        assert _both_start(pair, "after rebuild_graph") == (0, 0, 0)
        assert _both_start(pair, "second after rebuild_graph") == (1, 1, 1)
        rowptr, col, a = donor._host_csr()[:3]
        for lat in pair.both:
            lat.set_graph_csr(rowptr, col, a)
        assert pair.ap.build_info()["anchor_ap_bytes"] == 0
        assert _both_start(pair, "after set_graph_csr") == (0, 0, 0)
        assert _both_start(pair, "second after set_graph_csr") == (1, 1, 1)
        assert pair.ap.build_info()["anchor_ap_bytes"] == (N * 256 + N) * 4
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
    for before, after in sharding.run_loopback_ranks(2, rank_fn, timeout_s=120.0):
        assert before["streamed_first_applies"] == 1 and before["anchor_ap_bytes"] == (N * 256 + N) * 4, before
        assert after["anchor_ap_bytes"] == 0 and after["anchor_wy_bytes"] == 0, after


def test_nan_column(amd, monkeypatch):
    """A NaN in psi makes column 3 of the right-hand side NaN: that column stays NaN, the stop test is never met, the other
    columns are untouched -- on the streamed route as on the gathered one."""
    _clean_env(monkeypatch)
    N, D = 20000, 256
    Y, psi, _, _ = _inputs(N, D, seed=9)
    psi = psi.copy()
    psi[3] = np.nan
    pair = _Pair(amd, monkeypatch, Y, psi, 16)
    try:
        out = None
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
    monkeypatch.setenv("OSC_ANCHOR_AP", "1")
    Y, psi, _, _ = _inputs(20000, 256, seed=10)
    lats = [amd.Oscillink(Y, kneighbors=16) for _ in range(2)]
    try:
        for trip in range(3):
            outs = []
            for lat in lats:
                if trip == 0:
                    lat.set_query(psi)
                outs.append(_anchor_start(lat))
            _same(outs[0], outs[1], ("repeat", trip))
        us = [lat.solve_Ustar(use_cache=False).copy() for lat in lats]
        assert np.array_equal(us[0], us[1])
        assert all(lat.build_info()["streamed_first_applies"] == 3 for lat in lats)
    finally:
        for lat in lats:
            lat.close()


def test_auto_mode_leaves_small_lattices_alone(amd, monkeypatch):
    """Below 96 000 rows the default keeps the gathered first apply: the bytes of the OSC_ANCHOR_AP=0 handle."""
    _clean_env(monkeypatch)
    Y, psi, _, _ = _inputs(20000, 256, seed=11)
    pair = _Pair(amd, monkeypatch, Y, psi, 16, mode=None)
    try:
        for trip in range(3):
            assert _both_start(pair, ("auto", trip), compare=_same) == (0, 0, 0)
        info = pair.ap.build_info()
        assert info["cached_inits"] == 2 and info["anchor_ap_bytes"] == 0 and info["anchor_ap_builds"] == 0, info
    finally:
        pair.close()

"""Iterations 1 and 2 of an anchor start inside its INIT pass ("Gram sums"): on top of the streamed second
apply (tests/test_gpu_anchor_ap2.py) the CG scalars of the first two iterations come from float64 Gram sums of the cached row
sums (k_anchor_gram_scalars), and one pass (k_init_two_steps) leaves r2, p3 and x2.  The vectors are depth 2's, formed with the
same operations; only alpha and beta are rounded from other sums.  So the reference everywhere is a second handle on the same
inputs at depth 2 (OSC_ANCHOR_AP=1 OSC_ANCHOR_AP2=1 OSC_ANCHOR_GRAM=0), the handle under test adds OSC_ANCHOR_GRAM=1, and both
get the same calls.  Iteration counts equal, residual histories to rtol 1e-5, U to 2e-6 relative (the suite's bounds for two
routes that differ by rounding; the CPU model of tests/host_logic/sweep_anchor_gram.cpp gives 3e-7 / 1e-7).  Against the CPU
oracle the route may be at most the 2.5 x of the gathered route that depth 2 is allowed.  Wherever the route must not run the
two handles agree to the bit.  The Gram sums are read back and compared with float64 numpy sums over Y and graph_csr() to 2e-6
(one row of 20 011 counted twice or not at all is 5e-5).

Shapes: those of tests/test_gpu_anchor_ap2.py."""
import numpy as np
import pytest

from tests._cases import relerr
from tests._fullsize import oracle_solves

pytestmark = pytest.mark.gpu

SWITCHES = ("OSC_SPMM_XS", "OSC_REORDER", "OSC_SPMM_BLOCKED", "OSC_BLK_VARIANT", "OSC_BLK_INIT", "OSC_X_DEFER", "OSC_X_RING",
            "OSC_ANCHOR_SLAB", "OSC_ANCHOR_WY", "OSC_ANCHOR_AP", "OSC_ANCHOR_AP2", "OSC_ANCHOR_GRAM", "OSC_BALANCE", "OSC_SMALL_PATH",
            "OSC_FAKE_COL_SHARD", "OSC_SHARD", "OSC_ROW_FAKE_SHARDS", "OSC_LD", "OSCILLINK_RECEIPT_DYNAMICS")
CHAIN = [5, 1, 19999, 9000, 7, 2]
KW = dict(max_iters=12, tol=1e-3)
U_TOL = 2e-6
HIST_RTOL = 1e-5
ORACLE_FACTOR = 2.5
GRAM_RTOL = 2e-6


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


def _make(amd, monkeypatch, Y, psi, k, gram, gates=None, chain=None, ap="1"):
    monkeypatch.setenv("OSC_ANCHOR_AP", ap)
    monkeypatch.setenv("OSC_ANCHOR_AP2", "1")
    if gram is None:
        monkeypatch.delenv("OSC_ANCHOR_GRAM", raising=False)
    else:
        monkeypatch.setenv("OSC_ANCHOR_GRAM", gram)
    lat = amd.Oscillink(Y, kneighbors=k)
    lat.set_query(psi, gates=gates)
    if chain:
        lat.add_chain(chain, lamP=0.3)
    return lat


class _Pair:
    """`ref` at depth 2 (OSC_ANCHOR_GRAM=0), `gram` under OSC_ANCHOR_GRAM=`gram` (None: unset); the switches are fixed at creation."""

    def __init__(self, amd, monkeypatch, Y, psi, k, gates=None, chain=None, gram="1"):
        self.ref = _make(amd, monkeypatch, Y, psi, k, "0", gates, chain)
        self.gram = _make(amd, monkeypatch, Y, psi, k, gram, gates, chain)
        self.both = (self.ref, self.gram)

    def close(self):
        self.ref.close()
        self.gram.close()

    def counts(self):
        """(fused solves, Gram builds, redos) of `gram`; `ref` never takes the route"""
        r = self.ref.build_info()
        assert (r["fused_two_step_solves"], r["anchor_gram_bytes"], r["anchor_gram_builds"], r["anchor_gram_last_solve"],
                r["anchor_gram_redos"]) == (0, 0, 0, 0, 0), r
        a = self.gram.build_info()
        return a["fused_two_step_solves"], a["anchor_gram_builds"], a["anchor_gram_redos"]


def _anchor_start(lat, **kw):
    lat.reset_U(wait=False)
    st = lat.settle(**dict(KW, **kw))
    return st["iters"], st["res"], lat.residual_history(), lat.U.copy()


def _agree(x, y, what):
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


def _diff(a, b):
    return tuple(y - x for x, y in zip(a, b))


def _both_start(pair, what, compare=_agree, **kw):
    """One anchor start on both lattices, compared; (fused solves, Gram builds, redos) of this solve.  The fused pass replaces
    two streamed iterations, never a matvec: both handles launch the same number of those."""
    c0 = pair.counts()
    m0 = [lat.build_info()["blocked_applies"] for lat in pair.both]
    compare(_anchor_start(pair.ref, **kw), _anchor_start(pair.gram, **kw), what)
    m1 = [lat.build_info()["blocked_applies"] for lat in pair.both]
    took = _diff(c0, pair.counts())
    if took[2] == 0:  # (a solve given up at iteration 2 had iteration 3's matvec enqueued, gated off)
        assert m1[0] - m0[0] == m1[1] - m0[1], (what, "matvecs", m0, m1)
    assert pair.gram.build_info()["anchor_gram_last_solve"] == took[0], what
    return took


def _ustar(pair, what, compare_exact=False):
    c0 = pair.counts()
    us = [lat.solve_Ustar(use_cache=False).copy() for lat in pair.both]
    hs = [np.asarray(lat.residual_history(), dtype=np.float64) for lat in pair.both]
    assert len(hs[0]) == len(hs[1]), (what, "U* iters", len(hs[0]), len(hs[1]))
    e = relerr(us[1], us[0])
    print(f"{what}: U* iters {len(hs[0])} history max rel {np.max(np.abs(hs[1] - hs[0]) / np.abs(hs[0])):.3e} U* rel {e:.3e}")
    if compare_exact:
        assert np.array_equal(hs[0], hs[1]) and np.array_equal(us[0], us[1]), what
    assert np.allclose(hs[1], hs[0], rtol=HIST_RTOL, atol=0.0), (what, "U* history", hs)
    assert e < U_TOL, (what, "U*", e)
    return _diff(c0, pair.counts())


def _numpy_gram(lat, Y, c0, c1):
    """The sums in float64 from Y and the device-built graph: (22, c1 - c0) and (6,) in the layout of osc_anchor_gram_read."""
    import scipy.sparse as sp

    N = Y.shape[0]
    rowptr, col, _, w = lat.graph_csr()[:4]
    W = sp.csr_matrix((w.astype(np.float64), col, rowptr), shape=(N, N))
    ys = [Y[:, c0:c1].astype(np.float64)]
    for _ in range(3):
        ys.append(W @ ys[-1])
    a = [np.ones(N)]
    for _ in range(2):
        a.append(W @ a[-1])
    per = [np.einsum("ij,ij->j", ys[j], ys[k]) for j in range(4) for k in range(j, 4)]
    per += [a[b] @ ys[j] for b in range(3) for j in range(4)]
    latt = [a[b] @ a[c] for b in range(3) for c in range(b, 3)]
    return np.asarray(per), np.asarray(latt)


def _check_gram(lat, Y, what, c0=0, c1=None):
    c1 = Y.shape[1] if c1 is None else c1
    g = lat.anchor_gram()
    ld = (g.size - 6) // 22
    assert g.size == 22 * ld + 6 and ld >= Y.shape[1], (what, g.size)
    got = g[:22 * ld].reshape(22, ld)
    per, latt = _numpy_gram(lat, Y, c0, c1)
    scale = np.abs(per).max(axis=1, keepdims=True)  # (a sum of mixed signs is judged against the size of its row of sums)
    err = np.max(np.abs(got[:, c0:c1] - per) / scale)
    err_l = np.max(np.abs(g[22 * ld:] - latt) / np.abs(latt))
    print(f"{what}: Gram sums max rel {err:.3e}, lattice sums {err_l:.3e}")
    assert err <= GRAM_RTOL and err_l <= GRAM_RTOL, (what, err, err_l)
    assert not got[:, :c0].any() and not got[:, c1:].any(), (what, "columns outside the window")


SHAPES = {
    "default": dict(N=20000, D=256),
    "wide_shape": dict(N=20000, D=256, env={"OSC_BLK_VARIANT": "3"}, shape=3),
    "ragged": dict(N=20011, D=200, env={"OSC_LD": "224", "OSC_SPMM_XS": "1"}),
    "column_window": dict(N=20000, D=256, env={"OSC_FAKE_COL_SHARD": "1/2"}, window=True),
    "balanced_rows": dict(N=20000, D=256, env={"OSC_BALANCE": "1"}, order="balanced"),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_fused_two_steps_agree_with_depth_two(amd, name, monkeypatch):
    """The first start gathers (a handle's first solve of a kind has no prediction: the reference's bytes), the second forms
    the row sums and the Gram sums and takes the route, later ones reuse them: under other lams, another psi, and with a
    tolerance that makes the solve run longer than predicted."""
    _clean_env(monkeypatch)
    spec = SHAPES[name]
    for k, v in spec.get("env", {}).items():
        monkeypatch.setenv(k, v)
    N, D = spec["N"], spec["D"]
    Y, psi, psi2, _ = _inputs(N, D)
    pair = _Pair(amd, monkeypatch, Y, psi, 16)
    try:
        if spec.get("window"):  # (the settles start from U's own copy: the reference's bytes; the U* solves take the route)
            for trip in range(2):
                assert _both_start(pair, (name, "settle", trip), compare=_same) == (0, 0, 0)
            assert _ustar(pair, (name, "first"), compare_exact=True) == (0, 0, 0)
            assert _ustar(pair, (name, "second")) == (1, 1, 0)
            assert _ustar(pair, (name, "third")) == (1, 0, 0)
            _check_gram(pair.gram, Y, name, 128, 256)
        else:
            assert _both_start(pair, (name, "first"), compare=_same) == (0, 0, 0)
            assert pair.gram.build_info()["anchor_gram_bytes"] == 0
            assert _both_start(pair, (name, "second")) == (1, 1, 0)
            assert _both_start(pair, (name, "third")) == (1, 0, 0)
            _check_gram(pair.gram, Y, name)
            assert _ustar(pair, (name, "U*, no prediction"), compare_exact=True) == (0, 0, 0)
            assert _ustar(pair, (name, "U*")) == (1, 0, 0)
            assert _both_start(pair, (name, "longer than predicted"), tol=1e-6) == (1, 0, 0)
            assert len(pair.gram.residual_history()) > 4
        for lat in pair.both:
            lat.set_query(psi2, gates=None)
            lat.lamC, lat.lamQ = 0.8, 2.5
        if not spec.get("window"):
            assert _both_start(pair, (name, "other query and lams")) == (1, 0, 0)
        assert _ustar(pair, (name, "other query and lams")) == (1, 0, 0)
        info = pair.gram.build_info()
        assert info["apply_src_blocks"] > 0 and info["small_solves"] == 0, info
        if "shape" in spec:
            assert info["apply_blocked_shape"] == spec["shape"], info
        if "order" in spec:
            assert info["order_kind"] == spec["order"], info
        ld = int(spec.get("env", {}).get("OSC_LD", D))
        assert info["anchor_gram_bytes"] == (22 * ld + 6) * 8 and info["anchor_gram_builds"] == 1, info
    finally:
        pair.close()


def test_against_the_cpu_oracle(amd, orc, monkeypatch):
    """The CPU oracle on the device-built graph, the device's iteration counts executed: the route's error against it is at most
    2.5 times the gathered route's (OSC_ANCHOR_AP=0) -- what depth 2 is allowed, whose vectors these are."""
    import scipy.sparse as sp

    _clean_env(monkeypatch)
    N, D, k = 20000, 256, 16
    Y, psi, _, _ = _inputs(N, D, seed=5)
    pair = _Pair(amd, monkeypatch, Y, psi, k)
    gathered = _make(amd, monkeypatch, Y, psi, k, "0", ap="0")
    try:
        for trip in range(3):
            took = _both_start(pair, ("oracle", trip), compare=_agree if trip >= 1 else _same)
            g = _anchor_start(gathered)
        assert took == (1, 0, 0)
        lats = (gathered, pair.ref, pair.gram)
        U = [g[3], pair.ref.U.copy(), pair.gram.U.copy()]
        iters = len(pair.gram.residual_history())
        assert iters == len(pair.ref.residual_history()) == g[0]
        c0 = pair.counts()
        for trip in range(2):
            Us = [lat.solve_Ustar(use_cache=False).copy() for lat in lats]
        assert _diff(c0, pair.counts()) == (1, 0, 0)
        uiters = len(pair.gram.residual_history())
        assert uiters == len(pair.ref.residual_history()) == len(gathered.residual_history())
        csr = pair.ref.graph_csr()[:3]
        assert all(np.array_equal(a, b) for a, b in zip(csr, pair.gram.graph_csr()[:3]))
        A = sp.csr_matrix((csr[2], csr[1], csr[0]), shape=(N, N), dtype=np.float32)
        ref = oracle_solves(orc, Y, psi, A, k=k, settle_iters=iters, settle_tol=1e-3, ustar_iters=uiters)
        for what, got, want in (("settle", U, ref["U"]), ("U*", Us, ref["Ustar"])):
            e_g, e_2, e_f = (relerr(x, want) for x in got)
            print(f"oracle {what}: gathered {e_g:.3e} depth 2 {e_2:.3e} fused {e_f:.3e} ratio to gathered {e_f / e_g:.2f} "
                  f"to depth 2 {e_f / e_2:.2f}")
            assert e_f <= ORACLE_FACTOR * e_g, (what, e_g, e_2, e_f)
    finally:
        gathered.close()
        pair.close()


def test_early_stops_are_solved_again_at_depth_two(amd, monkeypatch):
    """After a prediction of three or more, a tol between res1 and res2 stops the solve in 2 iterations and one above res1 in 1:
    the fused pass was gated off, the solve runs again at depth 2 -- the reference's bytes --, one redo is counted, and the next
    solve (prediction below 3) does not take the route."""
    _clean_env(monkeypatch)
    Y, psi, _, _ = _inputs(20000, 256, seed=12)
    pair = _Pair(amd, monkeypatch, Y, psi, 16)
    try:
        assert _both_start(pair, "first", compare=_same) == (0, 0, 0)
        assert _both_start(pair, "second") == (1, 1, 0)
        hist = pair.ref.residual_history()
        assert len(hist) >= 4, hist
        tol1 = float(hist[0]) * 1.5  # (the residual falls ~30 x per iteration: far from either neighbour)
        tol2 = float(np.sqrt(hist[0] * hist[1]))
        for what, tol, iters in (("stop at 2", tol2, 2), ("stop at 1", tol1, 1)):
            assert _both_start(pair, (what, "predicted long"), compare=_same, tol=tol) == (0, 0, 1), what
            assert pair.gram.last["iters"] == iters, (what, pair.gram.last)
            assert _both_start(pair, (what, "predicted short"), compare=_same, tol=tol) == (0, 0, 0), what
            assert _both_start(pair, (what, "guess short")) == (0, 0, 0), what  # (still predicted short: depth 2, runs long)
            assert _both_start(pair, (what, "route again")) == (1, 0, 0), what
    finally:
        pair.close()


@pytest.mark.parametrize("name", ["per_row_gates", "chain_prior", "written_U", "max_iters_2", "ring_off", "auto_small", "nan_anchor_row"])
def test_where_the_route_must_not_run_the_handles_agree_to_the_bit(amd, name, monkeypatch):
    _clean_env(monkeypatch)
    if name == "ring_off":
        monkeypatch.setenv("OSC_X_RING", "0")
    N, D = 20000, 256
    Y, psi, _, gates = _inputs(N, D, seed=7)
    if name == "nan_anchor_row":
        Y = Y.copy()
        Y[1234] = np.nan
    pair = _Pair(amd, monkeypatch, Y, psi, 16, gates=gates if name == "per_row_gates" else None,
                 chain=CHAIN if name == "chain_prior" else None, gram=None if name == "auto_small" else "1")
    try:
        if name == "written_U":
            for trip in range(2):  # (the sums exist: the start below must not use them)
                _both_start(pair, (name, "anchor start", trip), compare=_agree if trip == 1 else _same)
            U0 = (Y * np.float32(0.5)).astype(np.float32)
            for trip in range(2):
                c0 = pair.counts()
                outs = []
                for lat in pair.both:
                    lat.U = U0
                    st = lat.settle(**KW)
                    outs.append((st["iters"], st["res"], lat.residual_history(), lat.U.copy()))
                _same(outs[0], outs[1], (name, trip))
                assert pair.counts() == c0 and pair.gram.build_info()["anchor_gram_last_solve"] == 0
            return
        kw = dict(max_iters=2, tol=0.0) if name == "max_iters_2" else dict(max_iters=5) if name == "nan_anchor_row" else {}
        if name == "max_iters_2":  # (a prediction of three or more first)
            for trip in range(2):
                _both_start(pair, (name, "warm", trip), compare=_agree if trip == 1 else _same)
        c0 = pair.counts()
        for trip in range(4):
            took = _both_start(pair, (name, trip), compare=_same, **kw)
            # a NaN row makes every Gram sum NaN: the solve is given up before anything is written and run again at depth 2
            assert took == ((0, 1 if trip == 1 else 0, 1) if name == "nan_anchor_row" and trip >= 1 else (0, 0, 0)), (name, trip, took)
        us = [lat.solve_Ustar(use_cache=False).copy() for lat in pair.both]
        assert np.array_equal(us[0], us[1], equal_nan=True)
        if name not in ("nan_anchor_row", "max_iters_2"):
            assert pair.counts() == (0, 0, 0) and pair.gram.build_info()["anchor_gram_bytes"] == 0
        if name == "per_row_gates":  # uniform gates again: the route opens
            for lat in pair.both:
                lat.set_gates(np.ones(N, np.float32))
            assert _both_start(pair, (name, "uniform again")) == (1, 1, 0)
    finally:
        pair.close()


def test_two_runs_give_the_same_bytes(amd, monkeypatch):
    _clean_env(monkeypatch)
    Y, psi, _, _ = _inputs(20000, 256, seed=10)
    lats = [_make(amd, monkeypatch, Y, psi, 16, "1") for _ in range(2)]
    try:
        for trip in range(3):
            outs = [_anchor_start(lat) for lat in lats]
            _same(outs[0], outs[1], ("repeat", trip))
        assert np.array_equal(lats[0].anchor_gram(), lats[1].anchor_gram())
        for trip in range(2):
            us = [lat.solve_Ustar(use_cache=False).copy() for lat in lats]
        assert np.array_equal(us[0], us[1])
        assert all(lat.build_info()["fused_two_step_solves"] == 3 for lat in lats)
    finally:
        for lat in lats:
            lat.close()


def test_everything_that_drops_the_row_sums_drops_the_gram_sums(amd, monkeypatch):
    """rebuild_graph, append, remove and update drop the sums with W.(W.(W.Y)); they are formed anew by the next solve that
    takes the route, and the results agree with the reference, which went through the same calls."""
    _clean_env(monkeypatch)
    N, D = 20000, 256
    Y, psi, _, _ = _inputs(N, D, seed=8)
    pair = _Pair(amd, monkeypatch, Y, psi, 16)
    more = _inputs(64, D, seed=9)[0]

    def again(what, Ynow):
        assert pair.gram.build_info()["anchor_gram_bytes"] == 0, what
        assert _both_start(pair, (what, "gathers"), compare=_same)[:2] == (0, 0), what
        assert _both_start(pair, (what, "route"))[:2] == (1, 1), what
        _check_gram(pair.gram, Ynow, what)

    try:
        assert _both_start(pair, "first", compare=_same) == (0, 0, 0)
        assert _both_start(pair, "second") == (1, 1, 0)
        for lat in pair.both:
            lat.rebuild_graph(kneighbors=12)
        again("rebuild_graph", Y)
        for lat, gram in zip(pair.both, ("0", "1")):  # (append, remove and update may make a new handle, which reads the switches)
            monkeypatch.setenv("OSC_ANCHOR_GRAM", gram)
            lat.append(more)
        Y2 = np.concatenate([Y, more])
        again("append", Y2)
        for lat, gram in zip(pair.both, ("0", "1")):
            monkeypatch.setenv("OSC_ANCHOR_GRAM", gram)
            lat.remove(np.arange(N, N + 64))
        again("remove", Y)
        rows = np.array([3, 777, 19999])
        Y3 = Y.copy()
        Y3[rows] = more[:3]
        for lat, gram in zip(pair.both, ("0", "1")):
            monkeypatch.setenv("OSC_ANCHOR_GRAM", gram)
            lat.update(rows, more[:3])
        again("update", Y3)
    finally:
        pair.close()

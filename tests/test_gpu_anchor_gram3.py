"""Iteration 3 of an anchor start in one launch ("Three steps"): on top of the fused two-step INIT pass
(tests/test_gpu_anchor_gram.py) alpha3, beta3 and |r3| come from float64 sums of nine vectors (k_anchor_gram_scalars,
anchor_gram.hpp: three_steps), and the iteration's gathering matvec forms r3 and p4 in its epilogue (k_apply_blocked's FUSED form)
instead of storing A p3.  The vectors are the two-step route's, formed with the same operations; only alpha3 and beta3 are rounded
from other sums.  So the reference everywhere is a second handle on the same inputs on the two-step route (OSC_ANCHOR_GRAM=1
OSC_ANCHOR_GRAM3=0), the handle under test adds OSC_ANCHOR_GRAM3=1, and both get the same calls.  Iteration counts equal, residual
histories to rtol 1e-5, U to 2e-6 relative: the bounds tests/test_gpu_anchor_gram.py uses for two routes that differ by rounding.
The CPU model of tests/host_logic/sweep_anchor_gram3.cpp gives, against the two-step route, alpha3 3.2e-7, beta3 5.1e-7, res3
2.8e-7, res4 6.4e-7 (7.1e-7 against summed scalars) and x 9.6e-8: res4 stays below 2.5e-6, so the history bound is the suite's
1e-5 for every entry.  Against the CPU oracle the route may be at most the 2.5 x of the gathered route that the depth-2 and
two-step routes are allowed.  Wherever the route must not run the two handles agree to the bit.  The new sums are read back and
compared with float64 numpy sums over Y and graph_csr() to 2e-6 of the row's scale.

Shapes: those of tests/test_gpu_anchor_gram.py."""
import numpy as np
import pytest

from tests import test_gpu_anchor_gram as two
from tests._cases import relerr
from tests._fullsize import oracle_solves

pytestmark = pytest.mark.gpu

KW = two.KW
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


def _clean_env(monkeypatch):
    two._clean_env(monkeypatch)
    monkeypatch.delenv("OSC_ANCHOR_GRAM3", raising=False)


def _make(amd, monkeypatch, Y, psi, k, gram3, gates=None, chain=None, ap="1"):
    monkeypatch.setenv("OSC_ANCHOR_AP", ap)
    monkeypatch.setenv("OSC_ANCHOR_AP2", "1")
    monkeypatch.setenv("OSC_ANCHOR_GRAM", "1")
    if gram3 is None:
        monkeypatch.delenv("OSC_ANCHOR_GRAM3", raising=False)
    else:
        monkeypatch.setenv("OSC_ANCHOR_GRAM3", gram3)
    lat = amd.Oscillink(Y, kneighbors=k)
    lat.set_query(psi, gates=gates)
    if chain:
        lat.add_chain(chain, lamP=0.3)
    return lat


class _Pair:
    """`ref` on the two-step route (OSC_ANCHOR_GRAM3=0), `three` under OSC_ANCHOR_GRAM3=`gram3` (None: unset)."""

    def __init__(self, amd, monkeypatch, Y, psi, k, gates=None, chain=None, gram3="1"):
        self.ref = _make(amd, monkeypatch, Y, psi, k, "0", gates, chain)
        self.three = _make(amd, monkeypatch, Y, psi, k, gram3, gates, chain)
        self.both = (self.ref, self.three)

    def close(self):
        self.ref.close()
        self.three.close()

    def counts(self):
        """(three-step solves, builds of the new sums) of `three`; `ref` never takes the route"""
        r = self.ref.build_info()
        assert (r["fused_three_step_solves"], r["anchor_gram3_bytes"], r["anchor_gram3_builds"], r["anchor_gram3_last_solve"]) == (0, 0, 0, 0), r
        a = self.three.build_info()
        return a["fused_three_step_solves"], a["anchor_gram3_builds"]


def _both_start(pair, what, compare=two._agree, **kw):
    """One anchor start on both lattices, compared; (three-step solves, builds) of this solve.  The fused launch counts as the
    matvec it is: both handles advance blocked_applies equally, and take the two-step route (or not) together."""
    c0 = pair.counts()
    i0 = [lat.build_info() for lat in pair.both]
    compare(two._anchor_start(pair.ref, **kw), two._anchor_start(pair.three, **kw), what)
    i1 = [lat.build_info() for lat in pair.both]
    for key in ("blocked_applies", "fused_two_step_solves", "anchor_gram_redos"):
        assert i1[0][key] - i0[0][key] == i1[1][key] - i0[1][key], (what, key, i0, i1)
    took = two._diff(c0, pair.counts())
    assert i1[1]["anchor_gram3_last_solve"] == took[0], what
    return took


def _ustar(pair, what, compare_exact=False):
    c0 = pair.counts()
    m0 = [lat.build_info()["blocked_applies"] for lat in pair.both]
    us = [lat.solve_Ustar(use_cache=False).copy() for lat in pair.both]
    m1 = [lat.build_info()["blocked_applies"] for lat in pair.both]
    hs = [np.asarray(lat.residual_history(), dtype=np.float64) for lat in pair.both]
    assert len(hs[0]) == len(hs[1]), (what, "U* iters", len(hs[0]), len(hs[1]))
    assert m1[0] - m0[0] == m1[1] - m0[1], (what, "matvecs", m0, m1)
    e = relerr(us[1], us[0])
    print(f"{what}: U* iters {len(hs[0])} history max rel {np.max(np.abs(hs[1] - hs[0]) / np.abs(hs[0])):.3e} U* rel {e:.3e}")
    if compare_exact:
        assert np.array_equal(hs[0], hs[1]) and np.array_equal(us[0], us[1]), what
    assert np.allclose(hs[1], hs[0], rtol=two.HIST_RTOL, atol=0.0), (what, "U* history", hs)
    assert e < two.U_TOL, (what, "U*", e)
    return two._diff(c0, pair.counts())


def _numpy_gram3(lat, Y, c0, c1):
    """The third step's sums in float64 from Y and the device-built graph: (13, c1 - c0) and (4,) in the layout of
    osc_anchor_gram3_read."""
    import scipy.sparse as sp

    N = Y.shape[0]
    rowptr, col, _, w = lat.graph_csr()[:4]
    W = sp.csr_matrix((w.astype(np.float64), col, rowptr), shape=(N, N))
    ys = [Y[:, c0:c1].astype(np.float64)]
    for _ in range(4):
        ys.append(W @ ys[-1])
    a = [np.ones(N)]
    for _ in range(3):
        a.append(W @ a[-1])
    per = [np.einsum("ij,ij->j", ys[j], ys[4]) for j in range(5)]
    per += [a[b] @ ys[4] for b in range(4)]
    per += [a[3] @ ys[j] for j in range(4)]
    latt = [a[b] @ a[3] for b in range(4)]
    return np.asarray(per), np.asarray(latt)


def _check_gram3(lat, Y, what, c0=0, c1=None):
    c1 = Y.shape[1] if c1 is None else c1
    g = lat.anchor_gram3()
    ld = (g.size - 4) // 13
    assert g.size == 13 * ld + 4 and ld >= Y.shape[1], (what, g.size)
    assert lat.build_info()["anchor_gram3_bytes"] == (13 * ld + 4) * 8 + 4 * Y.shape[0], what
    got = g[:13 * ld].reshape(13, ld)
    per, latt = _numpy_gram3(lat, Y, c0, c1)
    scale = np.abs(per).max(axis=1, keepdims=True)  # (a sum of mixed signs is judged against the size of its row of sums)
    err = np.max(np.abs(got[:, c0:c1] - per) / scale)
    err_l = np.max(np.abs(g[13 * ld:] - latt) / np.abs(latt))
    print(f"{what}: third-step sums max rel {err:.3e}, lattice sums {err_l:.3e}")
    assert err <= GRAM_RTOL and err_l <= GRAM_RTOL, (what, err, err_l)
    assert not got[:, :c0].any() and not got[:, c1:].any(), (what, "columns outside the window")


@pytest.mark.parametrize("name", sorted(two.SHAPES))
def test_three_steps_agree_with_two(amd, name, monkeypatch):
    """The first start gathers (no prediction), the second forms every cached array and the sums and takes the route, later ones
    reuse them: under a tolerance between res2 and res3 (the solve ends in iteration 3 and the fused launch is gated off: x = x2 +
    alpha3 p3), behind that prediction of 3 (iteration 4 is enqueued late), with a tolerance that makes the solve run past 4
    iterations, and under other lams and another psi."""
    _clean_env(monkeypatch)
    spec = two.SHAPES[name]
    for k, v in spec.get("env", {}).items():
        monkeypatch.setenv(k, v)
    N, D = spec["N"], spec["D"]
    Y, psi, psi2, _ = two._inputs(N, D)
    pair = _Pair(amd, monkeypatch, Y, psi, 16)
    try:
        if spec.get("window"):  # (the settles start from U's own copy: the reference's bytes; the U* solves take the route)
            for trip in range(2):
                assert _both_start(pair, (name, "settle", trip), compare=two._same) == (0, 0)
            assert _ustar(pair, (name, "first"), compare_exact=True) == (0, 0)
            assert _ustar(pair, (name, "second")) == (1, 1)
            assert _ustar(pair, (name, "third")) == (1, 0)
            _check_gram3(pair.three, Y, name, 128, 256)
        else:
            assert _both_start(pair, (name, "first"), compare=two._same) == (0, 0)
            assert pair.three.build_info()["anchor_gram3_bytes"] == 0
            assert _both_start(pair, (name, "second")) == (1, 1)
            assert _both_start(pair, (name, "third")) == (1, 0)
            _check_gram3(pair.three, Y, name)
            hist = pair.ref.residual_history()
            assert len(hist) >= 4, hist
            tol3 = float(np.sqrt(hist[1] * hist[2]))  # (the residual falls ~30 x per iteration: far from either neighbour)
            assert _both_start(pair, (name, "ends in iteration 3"), tol=tol3) == (1, 0)
            assert pair.three.last["iters"] == 3, pair.three.last
            assert _both_start(pair, (name, "predicted 3, runs 4")) == (1, 0)
            assert pair.three.last["iters"] == len(hist)
            assert _ustar(pair, (name, "U*, no prediction"), compare_exact=True) == (0, 0)
            assert _ustar(pair, (name, "U*")) == (1, 0)
            assert _both_start(pair, (name, "longer than predicted"), tol=1e-6) == (1, 0)
            assert len(pair.three.residual_history()) > 4
        for lat in pair.both:
            lat.set_query(psi2, gates=None)
            lat.lamC, lat.lamQ = 0.8, 2.5
        if not spec.get("window"):
            assert _both_start(pair, (name, "other query and lams")) == (1, 0)
        assert _ustar(pair, (name, "other query and lams")) == (1, 0)
        info = pair.three.build_info()
        assert info["apply_src_blocks"] > 0 and info["small_solves"] == 0, info
        if "shape" in spec:
            assert info["apply_blocked_shape"] == spec["shape"], info
        if "order" in spec:
            assert info["order_kind"] == spec["order"], info
        assert info["anchor_gram3_builds"] == 1 and info["anchor_gram_builds"] == 1, info
    finally:
        pair.close()


def test_against_the_cpu_oracle(amd, orc, monkeypatch):
    """The CPU oracle on the device-built graph, the device's iteration counts executed: the route's error against it is at most
    2.5 times the gathered route's (OSC_ANCHOR_AP=0)."""
    import scipy.sparse as sp

    _clean_env(monkeypatch)
    N, D, k = 20000, 256, 16
    Y, psi, _, _ = two._inputs(N, D, seed=5)
    pair = _Pair(amd, monkeypatch, Y, psi, k)
    gathered = _make(amd, monkeypatch, Y, psi, k, "0", ap="0")
    try:
        for trip in range(3):
            took = _both_start(pair, ("oracle", trip), compare=two._agree if trip >= 1 else two._same)
            g = two._anchor_start(gathered)
        assert took == (1, 0)
        lats = (gathered, pair.ref, pair.three)
        U = [g[3], pair.ref.U.copy(), pair.three.U.copy()]
        iters = len(pair.three.residual_history())
        assert iters == len(pair.ref.residual_history()) == g[0]
        c0 = pair.counts()
        for trip in range(2):
            Us = [lat.solve_Ustar(use_cache=False).copy() for lat in lats]
        assert two._diff(c0, pair.counts()) == (1, 0)
        uiters = len(pair.three.residual_history())
        assert uiters == len(pair.ref.residual_history()) == len(gathered.residual_history())
        csr = pair.ref.graph_csr()[:3]
        assert all(np.array_equal(a, b) for a, b in zip(csr, pair.three.graph_csr()[:3]))
        A = sp.csr_matrix((csr[2], csr[1], csr[0]), shape=(N, N), dtype=np.float32)
        ref = oracle_solves(orc, Y, psi, A, k=k, settle_iters=iters, settle_tol=1e-3, ustar_iters=uiters)
        for what, got, want in (("settle", U, ref["U"]), ("U*", Us, ref["Ustar"])):
            e_g, e_2, e_3 = (relerr(x, want) for x in got)
            print(f"oracle {what}: gathered {e_g:.3e} two steps {e_2:.3e} three steps {e_3:.3e} ratio to gathered {e_3 / e_g:.2f} "
                  f"to two steps {e_3 / e_2:.2f}")
            assert e_3 <= ORACLE_FACTOR * e_g, (what, e_g, e_2, e_3)
    finally:
        gathered.close()
        pair.close()


@pytest.mark.parametrize("name", ["per_row_gates", "chain_prior", "written_U", "max_iters_2", "ring_off", "auto_small", "nan_anchor_row"])
def test_where_the_route_must_not_run_the_handles_agree_to_the_bit(amd, name, monkeypatch):
    _clean_env(monkeypatch)
    if name == "ring_off":
        monkeypatch.setenv("OSC_X_RING", "0")
    N, D = 20000, 256
    Y, psi, _, gates = two._inputs(N, D, seed=7)
    if name == "nan_anchor_row":
        Y = Y.copy()
        Y[1234] = np.nan
    pair = _Pair(amd, monkeypatch, Y, psi, 16, gates=gates if name == "per_row_gates" else None,
                 chain=two.CHAIN if name == "chain_prior" else None, gram3=None if name == "auto_small" else "1")
    try:
        if name == "written_U":
            for trip in range(2):  # (the sums exist: the start below must not use them)
                _both_start(pair, (name, "anchor start", trip), compare=two._agree if trip == 1 else two._same)
            U0 = (Y * np.float32(0.5)).astype(np.float32)
            for trip in range(2):
                c0 = pair.counts()
                outs = []
                for lat in pair.both:
                    lat.U = U0
                    st = lat.settle(**KW)
                    outs.append((st["iters"], st["res"], lat.residual_history(), lat.U.copy()))
                two._same(outs[0], outs[1], (name, trip))
                assert pair.counts() == c0 and pair.three.build_info()["anchor_gram3_last_solve"] == 0
            return
        kw = dict(max_iters=2, tol=0.0) if name == "max_iters_2" else dict(max_iters=5) if name == "nan_anchor_row" else {}
        if name == "max_iters_2":  # (a prediction of three or more first)
            for trip in range(2):
                _both_start(pair, (name, "warm", trip), compare=two._agree if trip == 1 else two._same)
        c0 = pair.counts()
        redos0 = pair.three.build_info()["anchor_gram_redos"]
        for trip in range(4):
            took = _both_start(pair, (name, trip), compare=two._same, **kw)
            # a NaN row makes every sum NaN: the solve is given up before anything is written and run again at depth 2 -- one redo,
            # as on the two-step route (the sums were formed once, by the first solve that asked for the route)
            assert took == ((0, 1 if trip == 1 else 0) if name == "nan_anchor_row" else (0, 0)), (name, trip, took)
        if name == "nan_anchor_row":
            assert pair.three.build_info()["anchor_gram_redos"] - redos0 == 3 == pair.ref.build_info()["anchor_gram_redos"]
        us = [lat.solve_Ustar(use_cache=False).copy() for lat in pair.both]
        assert np.array_equal(us[0], us[1], equal_nan=True)
        if name not in ("nan_anchor_row", "max_iters_2"):
            assert pair.counts() == (0, 0) and pair.three.build_info()["anchor_gram3_bytes"] == 0
    finally:
        pair.close()


def test_two_runs_give_the_same_bytes(amd, monkeypatch):
    _clean_env(monkeypatch)
    Y, psi, _, _ = two._inputs(20000, 256, seed=10)
    lats = [_make(amd, monkeypatch, Y, psi, 16, "1") for _ in range(2)]
    try:
        for trip in range(3):
            outs = [two._anchor_start(lat) for lat in lats]
            two._same(outs[0], outs[1], ("repeat", trip))
        assert np.array_equal(lats[0].anchor_gram3(), lats[1].anchor_gram3())
        for trip in range(2):
            us = [lat.solve_Ustar(use_cache=False).copy() for lat in lats]
        assert np.array_equal(us[0], us[1])
        assert all(lat.build_info()["fused_three_step_solves"] == 3 for lat in lats)
    finally:
        for lat in lats:
            lat.close()


def test_everything_that_drops_the_row_sums_drops_the_new_sums(amd, monkeypatch):
    """rebuild_graph, append, remove and update drop the new sums with the old ones; they are formed anew by the next solve that
    takes the route, and the results agree with the reference, which went through the same calls."""
    _clean_env(monkeypatch)
    N, D = 20000, 256
    Y, psi, _, _ = two._inputs(N, D, seed=8)
    pair = _Pair(amd, monkeypatch, Y, psi, 16)
    more = two._inputs(64, D, seed=9)[0]

    def again(what, Ynow):
        info = pair.three.build_info()
        assert info["anchor_gram3_bytes"] == 0 and info["anchor_gram_bytes"] == 0, what
        assert _both_start(pair, (what, "gathers"), compare=two._same) == (0, 0), what
        assert _both_start(pair, (what, "route")) == (1, 1), what
        _check_gram3(pair.three, Ynow, what)

    try:
        assert _both_start(pair, "first", compare=two._same) == (0, 0)
        assert _both_start(pair, "second") == (1, 1)
        for lat in pair.both:
            lat.rebuild_graph(kneighbors=12)
        again("rebuild_graph", Y)
        for lat, g3 in zip(pair.both, ("0", "1")):  # (append, remove and update may make a new handle, which reads the switches)
            monkeypatch.setenv("OSC_ANCHOR_GRAM3", g3)
            lat.append(more)
        again("append", np.concatenate([Y, more]))
        for lat, g3 in zip(pair.both, ("0", "1")):
            monkeypatch.setenv("OSC_ANCHOR_GRAM3", g3)
            lat.remove(np.arange(N, N + 64))
        again("remove", Y)
        rows = np.array([3, 777, 19999])
        Y3 = Y.copy()
        Y3[rows] = more[:3]
        for lat, g3 in zip(pair.both, ("0", "1")):
            monkeypatch.setenv("OSC_ANCHOR_GRAM3", g3)
            lat.update(rows, more[:3])
        again("update", Y3)
    finally:
        pair.close()

"""An anchor start that ends in iteration 4 without a fourth matvec ("Four steps"): on top of the three-step
route (tests/test_gpu_anchor_gram3.py) alpha4 and |r4| come from float64 sums of eleven vectors (k_anchor_gram_scalars,
anchor_gram.hpp: four_steps), and where the published residuals show the solve to end in iteration 4, iteration 3's gathering
matvec writes x4 = x3 + alpha4 p4 from its epilogue (k_apply_blocked's FUSED_LAST form) and iteration 4 launches nothing.  The
vectors are the three-step route's, formed with the same operations; only alpha4 and the fourth residual are rounded from other
sums.  So the reference everywhere is a second handle on the same inputs under OSC_ANCHOR_GRAM4=0, the handle under test runs
under OSC_ANCHOR_GRAM4=1, and both get the same calls.  Where the route is taken: iteration counts equal, residual histories to
rtol 1e-5, U to 2e-6 relative (the suite's bounds for two routes that differ by rounding), one blocked apply less.  The CPU
model of tests/host_logic/sweep_anchor_gram4.cpp gives, against the three-step route, alpha4 6.4e-7, res4 5.5e-7 and x4 9.3e-8
(7.3e-7 and 2.2e-7 against summed scalars; tests/test_anchor_gram4_host.py).  Wherever the route must not run -- stops in 1, 2,
3 and beyond 4, max_iters = 3, per-row gates, a chain prior, a warm start -- the two handles agree to the bit and their
counters are equal.  Against the CPU oracle the route may be at most the siblings' 2.5 x of the gathered route.  The new sums are
read back and compared with float64 numpy sums over Y and graph_csr() to 2e-6 of the row's scale.

Shapes: those of tests/test_gpu_anchor_gram.py."""
import numpy as np
import pytest

from tests import test_gpu_anchor_gram as two
from tests import test_gpu_anchor_gram3 as three
from tests._cases import relerr
from tests._fullsize import oracle_solves

pytestmark = pytest.mark.gpu

ORACLE_FACTOR = 2.5
GRAM_RTOL = 2e-6
COUNTERS = ("blocked_applies", "fused_two_step_solves", "fused_three_step_solves", "anchor_gram_redos")
LAST_SOLVE = ("x_ring_slots", "x_ring_passes", "x_ring_flushes", "anchor_gram_last_solve", "anchor_gram3_last_solve")


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
    three._clean_env(monkeypatch)
    monkeypatch.delenv("OSC_ANCHOR_GRAM4", raising=False)


def _make(amd, monkeypatch, Y, psi, k, gram4, gates=None, chain=None, ap="1"):
    if gram4 is None:
        monkeypatch.delenv("OSC_ANCHOR_GRAM4", raising=False)
    else:
        monkeypatch.setenv("OSC_ANCHOR_GRAM4", gram4)
    return three._make(amd, monkeypatch, Y, psi, k, "1", gates, chain, ap)


class _Pair:
    """`ref` on the three-step route (OSC_ANCHOR_GRAM4=0), `four` under OSC_ANCHOR_GRAM4=`gram4` (None: unset)."""

    def __init__(self, amd, monkeypatch, Y, psi, k, gates=None, chain=None, gram4="1"):
        self.ref = _make(amd, monkeypatch, Y, psi, k, "0", gates, chain)
        self.four = _make(amd, monkeypatch, Y, psi, k, gram4, gates, chain)
        self.both = (self.ref, self.four)

    def close(self):
        self.ref.close()
        self.four.close()

    def counts(self):
        """(four-step solves, builds of the new sums) of `four`; `ref` never plans the route"""
        r = self.ref.build_info()
        assert (r["fused_four_step_solves"], r["anchor_gram4_bytes"], r["anchor_gram4_builds"], r["anchor_gram4_last_solve"]) == (0, 0, 0, 0), r
        a = self.four.build_info()
        return a["fused_four_step_solves"], a["anchor_gram4_builds"]


def _both_start(pair, what, compare=two._agree, one_less=False, **kw):
    """One anchor start on both lattices, compared; (four-step solves, builds) of this solve.  A solve that takes the route
    launches one blocked apply, the settle's only one, and no x pass; the reference launches iteration 4's as well -- one_less:
    and nothing else, its prediction being 4 (behind another prediction it also counts the gated-off matvec of a speculative
    iteration 5, which the route does not enqueue).  Every other solve advances every counter equally."""
    c0 = pair.counts()
    i0 = [lat.build_info() for lat in pair.both]
    compare(two._anchor_start(pair.ref, **kw), two._anchor_start(pair.four, **kw), what)
    i1 = [lat.build_info() for lat in pair.both]
    took = two._diff(c0, pair.counts())
    d = [{key: i1[j][key] - i0[j][key] for key in COUNTERS} for j in range(2)]
    assert i1[1]["anchor_gram4_last_solve"] == took[0], what
    if took[0]:
        assert d[1]["blocked_applies"] == 1 and d[0]["blocked_applies"] in ((2,) if one_less else (2, 3)), (what, d)
        assert i1[1]["x_ring_passes"] == 0 and i1[1]["anchor_gram3_last_solve"] == 1, (what, i1[1])
        for key in ("fused_two_step_solves", "fused_three_step_solves", "anchor_gram_redos"):
            assert d[0][key] == d[1][key], (what, key, d)
    else:
        assert d[0] == d[1], (what, d)
        for key in LAST_SOLVE:
            assert i1[0][key] == i1[1][key], (what, key, i1)
    return took


def _numpy_gram4(lat, Y, c0, c1):
    """The fourth step's sums in float64 from Y and the device-built graph: (16, c1 - c0) and (5,) in the layout of
    osc_anchor_gram4_read."""
    import scipy.sparse as sp

    N = Y.shape[0]
    rowptr, col, _, w = lat.graph_csr()[:4]
    W = sp.csr_matrix((w.astype(np.float64), col, rowptr), shape=(N, N))
    ys = [Y[:, c0:c1].astype(np.float64)]
    for _ in range(5):
        ys.append(W @ ys[-1])
    a = [np.ones(N)]
    for _ in range(4):
        a.append(W @ a[-1])
    per = [np.einsum("ij,ij->j", ys[j], ys[5]) for j in range(6)]
    per += [a[b] @ ys[5] for b in range(5)]
    per += [a[4] @ ys[j] for j in range(5)]
    latt = [a[b] @ a[4] for b in range(5)]
    return np.asarray(per), np.asarray(latt)


def _check_gram4(lat, Y, what, c0=0, c1=None):
    c1 = Y.shape[1] if c1 is None else c1
    g = lat.anchor_gram4()
    ld = (g.size - 5) // 16
    assert g.size == 16 * ld + 5 and ld >= Y.shape[1], (what, g.size)
    assert lat.build_info()["anchor_gram4_bytes"] == (16 * ld + 5) * 8, what
    got = g[:16 * ld].reshape(16, ld)
    per, latt = _numpy_gram4(lat, Y, c0, c1)
    scale = np.abs(per).max(axis=1, keepdims=True)  # (a sum of mixed signs is judged against the size of its row of sums)
    err = np.max(np.abs(got[:, c0:c1] - per) / scale)
    err_l = np.max(np.abs(g[16 * ld:] - latt) / np.abs(latt))
    print(f"{what}: fourth-step sums max rel {err:.3e}, lattice sums {err_l:.3e}")
    assert err <= GRAM_RTOL and err_l <= GRAM_RTOL, (what, err, err_l)
    assert not got[:, :c0].any() and not got[:, c1:].any(), (what, "columns outside the window")


def _tols(hist):
    """Tolerances that end a solve with this residual history in iteration 1, 2, 3 and 4: the geometric means of neighbouring
    residuals (the residual falls ~30 x per iteration: far from either neighbour), and twice the first residual."""
    assert len(hist) >= 4, hist
    return {1: 2.0 * float(hist[0]), 2: float(np.sqrt(hist[0] * hist[1])), 3: float(np.sqrt(hist[1] * hist[2])),
            4: float(np.sqrt(hist[2] * hist[3]))}


@pytest.mark.parametrize("name", sorted(two.SHAPES))
def test_a_solve_that_ends_in_iteration_four_needs_one_matvec(amd, name, monkeypatch):
    """The first start gathers (no prediction), the second takes the three-step route and forms the new sums, and under a
    tolerance between the reference's residuals 3 and 4 the solve ends in iteration 4 on the route: again behind that
    prediction, behind a prediction of 3 (iteration 4 is enqueued late: nothing is launched for it) and of 5.  Then the solves
    the route must decline: stops in 3, 2 and 1, beyond 4 (the published fourth residual is taken back), max_iters = 3."""
    _clean_env(monkeypatch)
    spec = two.SHAPES[name]
    for k, v in spec.get("env", {}).items():
        monkeypatch.setenv(k, v)
    N, D = spec["N"], spec["D"]
    Y, psi, psi2, _ = two._inputs(N, D)
    pair = _Pair(amd, monkeypatch, Y, psi, 16)
    try:
        if spec.get("window"):  # (the settles start from U's own copy: the reference's bytes; the U* solves plan the route)
            for trip in range(2):
                assert _both_start(pair, (name, "settle", trip), compare=two._same) == (0, 0)
            for trip in range(3):
                us = [lat.solve_Ustar(use_cache=False).copy() for lat in pair.both]
                hs = [np.asarray(lat.residual_history(), dtype=np.float64) for lat in pair.both]
                assert len(hs[0]) == len(hs[1]), (name, trip, hs)
                assert np.allclose(hs[1], hs[0], rtol=two.HIST_RTOL, atol=0.0), (name, trip, hs)
                assert relerr(us[1], us[0]) < two.U_TOL, (name, trip)
            assert pair.counts()[1] == 1
            _check_gram4(pair.four, Y, name, 128, 256)
            return
        assert _both_start(pair, (name, "first"), compare=two._same) == (0, 0)
        assert pair.four.build_info()["anchor_gram4_bytes"] == 0
        took = _both_start(pair, (name, "second"))
        assert took[1] == 1, took
        _check_gram4(pair.four, Y, name)
        tol = _tols(pair.ref.residual_history())
        assert _both_start(pair, (name, "ends in iteration 4"), tol=tol[4])[0] == 1
        assert pair.four.last["iters"] == 4 == pair.ref.last["iters"], pair.four.last
        assert _both_start(pair, (name, "again, predicted 4"), one_less=True, tol=tol[4]) == (1, 0)
        assert _both_start(pair, (name, "ends in iteration 3"), compare=two._same, tol=tol[3]) == (0, 0)
        assert pair.four.last["iters"] == 3
        assert _both_start(pair, (name, "predicted 3, ends in 4"), tol=tol[4]) == (1, 0)
        assert _both_start(pair, (name, "beyond 4"), compare=two._same, tol=1e-6) == (0, 0)
        assert len(pair.four.residual_history()) > 4
        assert _both_start(pair, (name, "predicted longer, ends in 4"), tol=tol[4]) == (1, 0)
        assert _both_start(pair, (name, "max_iters 3"), compare=two._same, max_iters=3, tol=tol[4]) == (0, 0)
        assert _both_start(pair, (name, "ends in iteration 2"), compare=two._same, tol=tol[2]) == (0, 0)
        assert pair.four.last["iters"] == 2
        assert _both_start(pair, (name, "ends in iteration 1"), compare=two._same, tol=tol[1]) == (0, 0)
        assert pair.four.last["iters"] == 1
        for lat in pair.both:
            lat.set_query(psi2, gates=None)
            lat.lamC, lat.lamQ = 0.8, 2.5
        _both_start(pair, (name, "other query and lams, prediction"), compare=two._same, tol=1e-6)
        tol = _tols(pair.ref.residual_history())
        assert _both_start(pair, (name, "other query and lams"), tol=tol[4]) == (1, 0)
        info = pair.four.build_info()
        assert info["apply_src_blocks"] > 0 and info["small_solves"] == 0, info
        if "shape" in spec:
            assert info["apply_blocked_shape"] == spec["shape"], info
        if "order" in spec:
            assert info["order_kind"] == spec["order"], info
        assert info["anchor_gram4_builds"] == 1 and info["anchor_gram3_builds"] == 1, info
    finally:
        pair.close()


@pytest.mark.parametrize("slots", [2, 3])
def test_small_rings_move_the_alphas_out_of_alpha4s_way(amd, slots, monkeypatch):
    """With two ring slots alpha4 takes alpha2's slot (and alpha3 alpha1's), with three alpha1's: the INIT pass, their only
    reader, finds them in free rows of the r . z partials.  Same bounds as above; the declined solves to the bit."""
    _clean_env(monkeypatch)
    monkeypatch.setenv("OSC_X_RING", str(slots))
    Y, psi, _, _ = two._inputs(20000, 256, seed=11)
    pair = _Pair(amd, monkeypatch, Y, psi, 16)
    try:
        assert _both_start(pair, (slots, "first"), compare=two._same, tol=1e-6) == (0, 0)
        assert _both_start(pair, (slots, "second"), compare=two._same, tol=1e-6) == (0, 1)
        assert pair.four.build_info()["x_ring_slots"] == slots
        tol = _tols(pair.ref.residual_history())
        assert _both_start(pair, (slots, "ends in iteration 4"), tol=tol[4]) == (1, 0)
        assert _both_start(pair, (slots, "again"), one_less=True, tol=tol[4]) == (1, 0)
        assert pair.four.build_info()["x_ring_slots"] == slots
        assert _both_start(pair, (slots, "ends in iteration 3"), compare=two._same, tol=tol[3]) == (0, 0)
        assert _both_start(pair, (slots, "beyond 4"), compare=two._same, tol=1e-6) == (0, 0)
        assert _both_start(pair, (slots, "ends in iteration 4 again"), tol=tol[4]) == (1, 0)
    finally:
        pair.close()


def test_against_the_cpu_oracle(amd, orc, monkeypatch):
    """The CPU oracle on the device-built graph, four iterations executed: the route's error against it is at most 2.5 times
    the gathered route's (OSC_ANCHOR_AP=0)."""
    import scipy.sparse as sp

    _clean_env(monkeypatch)
    N, D, k = 20000, 256, 16
    Y, psi, _, _ = two._inputs(N, D, seed=5)
    pair = _Pair(amd, monkeypatch, Y, psi, k)
    gathered = _make(amd, monkeypatch, Y, psi, k, "0", ap="0")
    try:
        for trip in range(2):
            _both_start(pair, ("oracle", trip), compare=two._agree if trip >= 1 else two._same, tol=1e-6)
        tol4 = _tols(pair.ref.residual_history())[4]
        for trip in range(2):
            took = _both_start(pair, ("oracle, four", trip), one_less=trip == 1, tol=tol4)
            g = two._anchor_start(gathered, tol=tol4)
        assert took == (1, 0) and g[0] == 4 == pair.four.last["iters"]
        csr = pair.ref.graph_csr()[:3]
        assert all(np.array_equal(a, b) for a, b in zip(csr, pair.four.graph_csr()[:3]))
        A = sp.csr_matrix((csr[2], csr[1], csr[0]), shape=(N, N), dtype=np.float32)
        ref = oracle_solves(orc, Y, psi, A, k=k, settle_iters=4, settle_tol=tol4, ustar_iters=1)
        e_g, e_3, e_4 = (relerr(x, ref["U"]) for x in (g[3], pair.ref.U.copy(), pair.four.U.copy()))
        print(f"oracle settle: gathered {e_g:.3e} three steps {e_3:.3e} four steps {e_4:.3e} ratio to gathered {e_4 / e_g:.2f}")
        assert e_4 <= ORACLE_FACTOR * e_g, (e_g, e_3, e_4)
    finally:
        gathered.close()
        pair.close()


@pytest.mark.parametrize("name", ["per_row_gates", "chain_prior", "written_U", "auto_small"])
def test_where_the_route_must_not_run_the_handles_agree_to_the_bit(amd, name, monkeypatch):
    _clean_env(monkeypatch)
    N, D = 20000, 256
    Y, psi, _, gates = two._inputs(N, D, seed=7)
    pair = _Pair(amd, monkeypatch, Y, psi, 16, gates=gates if name == "per_row_gates" else None,
                 chain=two.CHAIN if name == "chain_prior" else None, gram4=None if name == "auto_small" else "1")
    try:
        if name == "written_U":
            for trip in range(2):
                _both_start(pair, (name, "anchor start", trip), compare=two._agree if trip == 1 else two._same, tol=1e-6)
            tol4 = _tols(pair.ref.residual_history())[4]
            U0 = (Y * np.float32(0.5)).astype(np.float32)
            for trip in range(2):
                c0 = pair.counts()
                outs = []
                for lat in pair.both:
                    lat.U = U0
                    st = lat.settle(max_iters=12, tol=tol4)
                    outs.append((st["iters"], st["res"], lat.residual_history(), lat.U.copy()))
                two._same(outs[0], outs[1], (name, trip))
                assert pair.counts() == c0 and pair.four.build_info()["anchor_gram4_last_solve"] == 0
            return
        for trip in range(2):
            assert _both_start(pair, (name, "warm", trip), compare=two._same, tol=1e-6) == (0, 0)
        tol4 = _tols(pair.ref.residual_history())[4]
        for trip in range(3):
            assert _both_start(pair, (name, trip), compare=two._same, tol=tol4) == (0, 0), (name, trip)
        assert pair.counts() == (0, 0) and pair.four.build_info()["anchor_gram4_bytes"] == 0
    finally:
        pair.close()


def test_two_runs_give_the_same_bytes(amd, monkeypatch):
    _clean_env(monkeypatch)
    Y, psi, _, _ = two._inputs(20000, 256, seed=10)
    lats = [_make(amd, monkeypatch, Y, psi, 16, "1") for _ in range(2)]
    try:
        for trip in range(2):
            outs = [two._anchor_start(lat, tol=1e-6) for lat in lats]
            two._same(outs[0], outs[1], ("repeat, warm", trip))
        tol4 = _tols(outs[0][2])[4]
        for trip in range(3):
            outs = [two._anchor_start(lat, tol=tol4) for lat in lats]
            two._same(outs[0], outs[1], ("repeat", trip))
        assert np.array_equal(lats[0].anchor_gram4(), lats[1].anchor_gram4())
        assert all(lat.build_info()["fused_four_step_solves"] == 3 for lat in lats)
    finally:
        for lat in lats:
            lat.close()


def test_everything_that_drops_the_third_steps_sums_drops_the_new_sums(amd, monkeypatch):
    """rebuild_graph, append, remove and update drop the new sums with the old ones; they are formed anew by the next solve that
    plans the route, and the results agree with the reference, which went through the same calls."""
    _clean_env(monkeypatch)
    N, D = 20000, 256
    Y, psi, _, _ = two._inputs(N, D, seed=8)
    pair = _Pair(amd, monkeypatch, Y, psi, 16)
    more = two._inputs(64, D, seed=9)[0]

    def again(what, Ynow):
        info = pair.four.build_info()
        assert info["anchor_gram4_bytes"] == 0 and info["anchor_gram3_bytes"] == 0 and info["anchor_gram_bytes"] == 0, what
        assert _both_start(pair, (what, "gathers"), compare=two._same, tol=1e-6) == (0, 0), what
        assert _both_start(pair, (what, "plans the route"), tol=1e-6) == (0, 1), what
        _check_gram4(pair.four, Ynow, what)
        tol4 = _tols(pair.ref.residual_history())[4]
        assert _both_start(pair, (what, "route"), tol=tol4) == (1, 0), what
        assert _both_start(pair, (what, "route, predicted 4"), one_less=True, tol=tol4) == (1, 0), what

    try:
        assert _both_start(pair, "first", compare=two._same, tol=1e-6) == (0, 0)
        assert _both_start(pair, "second", tol=1e-6) == (0, 1)
        for lat in pair.both:
            lat.rebuild_graph(kneighbors=12)
        again("rebuild_graph", Y)
        for lat, g4 in zip(pair.both, ("0", "1")):  # (append, remove and update may make a new handle, which reads the switches)
            monkeypatch.setenv("OSC_ANCHOR_GRAM4", g4)
            lat.append(more)
        again("append", np.concatenate([Y, more]))
        for lat, g4 in zip(pair.both, ("0", "1")):
            monkeypatch.setenv("OSC_ANCHOR_GRAM4", g4)
            lat.remove(np.arange(N, N + 64))
        again("remove", Y)
        rows = np.array([3, 777, 19999])
        Y3 = Y.copy()
        Y3[rows] = more[:3]
        for lat, g4 in zip(pair.both, ("0", "1")):
            monkeypatch.setenv("OSC_ANCHOR_GRAM4", g4)
            lat.update(rows, more[:3])
        again("update", Y3)
    finally:
        pair.close()

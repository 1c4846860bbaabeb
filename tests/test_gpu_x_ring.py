"""The ring of kept search directions: a solve that keeps its last K directions never touches x in its
p update or its x-r kernel; whole passes over the kept directions (k_update_x_ring) write it, one per solve where the solve
takes at most K iterations.  Every pass applies `x = fmaf(p, alpha, x)` in ascending iteration order, which is the sequence
of roundings the per-iteration updates perform through memory, so nothing may change a bit of any result: every comparison
here is `np.array_equal`, against the same library with OSC_X_RING=0 (read at creation: x updated every iteration).

OSC_X_RING=K forces K slots whatever the planner would say (a fresh handle has no prediction, and the planner follows the
prediction); OSC_SMALL_PATH=0 keeps the one-launch solve, which has no ring, out of the way.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SWITCHES = ("OSC_SPMM_XS", "OSC_REORDER", "OSC_SPMM_BLOCKED", "OSC_BLK_VARIANT", "OSC_BLK_INIT", "OSC_X_DEFER", "OSC_ANCHOR_SLAB",
            "OSC_ANCHOR_WY", "OSC_SMALL_PATH", "OSC_FAKE_COL_SHARD", "OSC_SHARD", "OSC_ROW_FAKE_SHARDS", "OSC_LD", "OSC_X_RING",
            "OSC_XS_NB", "OSCILLINK_RECEIPT_DYNAMICS")
CHAIN = [5, 1, 6499, 3000, 7, 2]
# how the operator apply is forced onto these sizes (tests/test_gpu_parity.py does the same on its fixtures)
LAYOUTS = {
    "blocked": {"OSC_SPMM_XS": "1", "OSC_SPMM_BLOCKED": "3", "OSC_LD": "128"},  # slab-major directions: whole 32-column slabs
    "slab": {"OSC_SPMM_XS": "1", "OSC_SPMM_BLOCKED": "0", "OSC_LD": "128"},
    "multi": {"OSC_SPMM_XS": "0", "OSC_SPMM_BLOCKED": "0"},
    "auto": {},
}


@pytest.fixture(scope="module")
def amd():
    import oscillink_amd
    from oscillink_amd import _native

    assert _native.device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return oscillink_amd


_INPUTS = {}


def _inputs(N, D, seed=3):
    """Anchors, query, gates and a second state of one shape: made once, shared, never written."""
    if (N, D, seed) not in _INPUTS:
        rng = np.random.default_rng(seed)
        Y = rng.standard_normal((N, D)).astype(np.float32)
        psi = rng.standard_normal(D).astype(np.float32)
        psi /= np.linalg.norm(psi)
        gates = rng.uniform(0.1, 1.0, N).astype(np.float32)
        V = (Y + np.float32(0.25) * rng.standard_normal((N, D))).astype(np.float32)
        for arr in (Y, psi, gates, V):
            arr.setflags(write=False)
        _INPUTS[(N, D, seed)] = (Y, psi, gates, V)
    return _INPUTS[(N, D, seed)]


def _expected(forced, max_iters, guess, iters):
    """(slots, flushes, passes) of a solve that stops in `iters` on a handle that predicted `guess` (0: nothing): the launches
    of run_cg's host loop, counted from the rule alone -- a flush goes out, with iteration `it`, when the slot direction `it`
    is written to holds one that x lacks (K pending); an ungated pass goes out behind an iteration that has no successor
    enqueued (the predicted last one, max_iters) and at the end for what is left."""
    K = min(forced, max_iters)
    if K < 2:
        return 1, 0, 0
    s = dict(applied=0, fl_iter=0, fl_upto=0, flushes=0, passes=0)

    def settle(real):
        if s["fl_iter"] and s["fl_iter"] <= real:
            s["applied"], s["fl_iter"] = s["fl_upto"], 0

    def enqueue(it):
        settle(it - 1)
        if it - 1 - s["applied"] >= K:
            s["flushes"] += 1
            s["passes"] += 1
            s["fl_iter"], s["fl_upto"] = it, it - 1

    def ungated(it):
        settle(it)
        if it > s["applied"]:
            s["passes"] += 1
            s["applied"] = it

    enq = 1
    for it in range(1, max_iters + 1):
        if it < max_iters and it != guess and enq == it:
            enq += 1
            enqueue(enq)
        else:
            ungated(it)
        if it == iters:
            break
        if it < max_iters and enq == it:
            enq += 1
            enqueue(enq)
    ungated(iters)
    return K, s["flushes"], s["passes"]


def test_the_counting_rule_at_its_fixed_points():
    for K in (2, 3, 4):
        assert _expected(K, 1, 1, 1) == (1, 0, 0)
        assert _expected(K, K, K, K) == (K, 0, 1)              # exactly full: the final pass is the only x traffic
        assert _expected(K, K + 1, K + 1, K + 1) == (K, 1, 2)  # one flush
        assert _expected(K, 2 * K + 1, 2 * K + 1, 2 * K + 1) == (K, 2, 3)
        assert _expected(K, 12, K + 1, K) == (K, 1, 2)         # a long guess: the flush of iteration K + 1 is gated off
        assert _expected(0, 12, 4, 4) == (1, 0, 0)


class _Pair:
    """Two lattices over the same inputs under the same switches: `ref` created under OSC_X_RING=0, `ring` under OSC_X_RING=K."""

    def __init__(self, amd, monkeypatch, K, N, D, k=8, layout="auto", gates=False, chain=None, env=None, seed=3):
        for v in SWITCHES:
            monkeypatch.delenv(v, raising=False)
        monkeypatch.setenv("OSC_SMALL_PATH", "0")
        for name, val in dict(LAYOUTS[layout], **(env or {})).items():
            monkeypatch.setenv(name, val)
        self.K = K
        self.Y, self.psi, g, self.V = _inputs(N, D, seed)

        def make():
            lat = amd.Oscillink(self.Y, kneighbors=k)
            lat.set_query(self.psi, gates=g if gates else None)
            if chain:
                lat.add_chain(chain, lamP=0.3)
            return lat

        monkeypatch.setenv("OSC_X_RING", "0")
        self.ref = make()
        monkeypatch.setenv("OSC_X_RING", str(K))
        self.ring = make()
        monkeypatch.delenv("OSC_X_RING")
        self.both = (self.ref, self.ring)
        self.guess = {"settle": 0, "ustar": 0}  # what the handles predict for their next solve of each kind

    def close(self):
        self.ref.close()
        self.ring.close()

    def start(self, how):
        for lat in self.both:
            if how == "anchors":  # U aliases Y: the first pass reads x0 from the anchors and writes U's buffer
                lat.reset_U(wait=False)
            elif how in ("written", "inertia", "cold"):  # in place on U / x0 handed over in the AP array / x0 = Y, state term U
                lat.U = self.V
            elif how != "as_is":
                raise ValueError(how)

    def settle(self, how, what, max_iters, tol=0.0, counters=True, **kw):
        """One settle on both lattices from the same start, compared; returns (iters, history)."""
        self.start(how)
        if how == "inertia":
            kw = dict(kw, inertia=0.3)
        if how == "cold":
            kw = dict(kw, warm_start=False)
        out = []
        for lat in self.both:
            st = lat.settle(max_iters=max_iters, tol=tol, **kw)
            out.append((st["iters"], np.float32(st["res"]), np.asarray(lat.residual_history(), dtype=np.float32), lat.U.copy()))
        self._compare(out, (what, how, max_iters, tol), "settle", max_iters, counters)
        return out[0][0], out[0][2]

    def ustar(self, what, max_iters, tol=0.0):
        out = []
        for lat in self.both:
            us = lat.solve_Ustar(tol=tol, max_iters=max_iters, use_cache=False).copy()
            hist = np.asarray(lat.residual_history(), dtype=np.float32)
            out.append((len(hist), hist[-1], hist, us))
        self._compare(out, (what, "U*", max_iters, tol), "ustar", max_iters, True)
        return out[0][0]

    def _compare(self, out, what, kind, max_iters, counters):
        (ia, ra, ha, ua), (ib, rb, hb, ub) = out
        assert ia == ib, (what, "iters", ia, ib)
        assert np.array_equal(ra, rb, equal_nan=True), (what, "res", ra, rb)
        assert np.array_equal(ha, hb, equal_nan=True), (what, "history", ha, hb)
        assert np.array_equal(ua, ub, equal_nan=True), (what, "U", float(np.nanmax(np.abs(ua - ub))))
        info_ref, info = self.ref.build_info(), self.ring.build_info()
        assert info_ref["small_solves"] == 0 and info["small_solves"] == 0, (what, info)
        assert (info_ref["x_ring_slots"], info_ref["x_ring_flushes"], info_ref["x_ring_passes"]) == (1, 0, 0), (what, info_ref)
        assert info_ref["x_ring_bytes"] == 0, (what, info_ref)
        if counters:
            want = _expected(self.K, max_iters, self.guess[kind], ia)
            got = (info["x_ring_slots"], info["x_ring_flushes"], info["x_ring_passes"])
            assert got == want, (what, "guess", self.guess[kind], "iters", ia, "slots, flushes, passes", got, want)
        self.guess[kind] = ia


STARTS = ("anchors", "written", "cold", "inertia")


def _iteration_counts(K):
    return (1, 2, K, K + 1, 2 * K + 1)  # no ring, inside it, exactly full, one flush, two flushes


@pytest.mark.parametrize("K", [2, 4])
@pytest.mark.parametrize("N,D,layout", [(20011, 96, "blocked"), (20011, 100, "blocked"), (20011, 96, "auto"), (20011, 100, "auto"),
                                        (6500, 96, "slab"), (6500, 100, "slab"), (6500, 96, "multi"), (6500, 100, "multi"),
                                        (6500, 100, "auto")])
def test_fixed_iteration_counts_from_every_start(amd, N, D, layout, K, monkeypatch):
    """tol = 0 fixes the count.  Each (start, count) runs twice: first on whatever the previous solve left as the handle's
    prediction (a wrong one, mostly), then on the right one -- x is then written by one pass up to K iterations, with one
    flush more per K iterations beyond."""
    pair = _Pair(amd, monkeypatch, K, N, D, layout=layout)
    try:
        for how in STARTS:
            for mi in _iteration_counts(K):
                for trip in ("mispredicted", "predicted"):
                    iters, _ = pair.settle(how, (layout, N, D, K, trip), mi)
                    assert iters == mi
                if mi >= 2:
                    info = pair.ring.build_info()
                    assert info["x_ring_slots"] == min(K, mi) and info["x_ring_flushes"] == (mi - 1) // K, info
                    assert info["x_ring_passes"] == info["x_ring_flushes"] + 1, info
        info = pair.ring.build_info()
        ld = 128 if "OSC_LD" in LAYOUTS[layout] else D
        assert info["x_ring_bytes"] == (K - 1) * N * ld * 4 + 4 * ld * 4, info
        if layout == "blocked":
            assert info["apply_src_blocks"] == 3, info
        elif layout == "slab":
            assert info["apply_src_blocks"] == 0 and info["apply_xs_workgroups"] > 0, info
        elif layout == "multi":
            assert info["apply_src_blocks"] == 0 and info["apply_xs_workgroups"] == 0, info
    finally:
        pair.close()


@pytest.mark.parametrize("K", [2, 4])
@pytest.mark.parametrize("name", ["chain_prior", "chain_prior_blocked", "gates", "no_preconditioner", "no_last_form", "init_finish_pass"])
def test_under_the_other_solver_inputs(amd, name, K, monkeypatch):
    spec = {
        "chain_prior": dict(N=6500, layout="multi", chain=CHAIN),
        "chain_prior_blocked": dict(N=20011, layout="blocked", chain=CHAIN),  # (the fix-up launch reads the direction's slot too)
        "gates": dict(N=20011, layout="blocked", gates=True),
        "no_preconditioner": dict(N=6500, layout="slab", settle={"precond": "none"}),
        "no_last_form": dict(N=20011, layout="blocked", env={"OSC_X_DEFER": "2"}),
        "init_finish_pass": dict(N=20011, layout="blocked", env={"OSC_BLK_INIT": "2"}),
    }[name]
    pair = _Pair(amd, monkeypatch, K, spec["N"], 100, layout=spec["layout"], gates=spec.get("gates", False), chain=spec.get("chain"),
                 env=spec.get("env"))
    try:
        for how in ("anchors", "written"):
            for mi in _iteration_counts(K):
                for trip in range(2):
                    pair.settle(how, (name, K, trip), mi, **spec.get("settle", {}))
    finally:
        pair.close()


@pytest.mark.parametrize("K", [2, 4])
@pytest.mark.parametrize("layout", ["blocked", "multi"])
def test_ustar_solve(amd, layout, K, monkeypatch):
    """x0 is the anchors, the solution goes to its own array: the first pass reads the anchors in place."""
    pair = _Pair(amd, monkeypatch, K, 20011 if layout == "blocked" else 6500, 100, layout=layout, gates=True, chain=CHAIN)
    try:
        for mi in _iteration_counts(K):
            for trip in range(2):
                assert pair.ustar((layout, K, trip), mi) == mi
        assert pair.ustar((layout, K, "tol"), 64, tol=1e-4) < 64
    finally:
        pair.close()


def _tol_for(hist, j):
    """A tolerance the solve meets in iteration j and not before: between the residuals of iterations j - 1 and j."""
    assert hist[j - 2] > hist[j - 1] > 0.0, hist
    return float(np.sqrt(np.float64(hist[j - 2]) * np.float64(hist[j - 1])))


@pytest.mark.parametrize("K", [2, 4])
@pytest.mark.parametrize("N,layout", [(20011, "blocked"), (6500, "multi")])
def test_wrong_guesses_and_stops_inside_the_ring(amd, N, layout, K, monkeypatch):
    """The two-settle recipe of bench.py's cold_and_mispredicted: a first settle leaves the handle predicting one iteration
    short (the expected-last form did not keep r: restore_r runs, then the ring goes on) or one long (the solve converges
    under a speculative iteration whose launches -- a flush among them where K directions were pending -- are gated off),
    for stops at every position of the ring."""
    pair = _Pair(amd, monkeypatch, K, N, 100, layout=layout)
    try:
        _, hist = pair.settle("anchors", "probe", 12)
        # a fresh handle predicts nothing: every iteration is enqueued ahead of its predecessor's residual
        fresh = _Pair(amd, monkeypatch, K, N, 100, layout=layout)
        try:
            assert fresh.settle("as_is", "fresh", 12, tol=_tol_for(hist, K))[0] == K
        finally:
            fresh.close()
        for how in ("anchors", "written"):
            if how == "written":
                _, hist = pair.settle(how, "probe", 12)
            for j in sorted({2, K, K + 1, K + 2, 2 * K, 2 * K + 1}):
                tol = _tol_for(hist, j)
                for name, g in (("right", j), ("short", j - 1), ("long", j + 1), ("far", 12)):
                    assert pair.settle(how, (name, "guess"), g)[0] == g  # leaves the handle predicting g
                    assert pair.settle(how, (name, j), 12, tol=tol)[0] == j
    finally:
        pair.close()


@pytest.mark.parametrize("K", [2, 4])
def test_nan_column(amd, K, monkeypatch):
    """A column that diverged stays NaN, the stop test is never met, the finite columns are untouched by it."""
    pair = _Pair(amd, monkeypatch, K, 6500, 100, layout="multi")
    try:
        bad = pair.V.copy()
        bad[7, 3] = np.nan
        for mi in (K, 2 * K + 1):
            for lat in pair.both:
                lat.U = bad
            iters, hist = pair.settle("as_is", ("nan", K), mi, tol=1e-3)
            assert iters == mi and np.isnan(hist).all()
            out = pair.ring.U
            assert np.isnan(out[:, 3]).any() and np.isfinite(np.delete(out, 3, axis=1)).all()
    finally:
        pair.close()


@pytest.mark.parametrize("K", [2, 4])
@pytest.mark.parametrize("rank", [0, 1])
@pytest.mark.parametrize("xs", ["0", "1"])
def test_fake_column_shards(amd, xs, rank, K, monkeypatch):
    """OSC_FAKE_COL_SHARD=r/2 at D = 192: a rank's 96-column window of a wider solve, at a column offset for rank 1 (the
    directions' slots, the alpha vectors and x are all addressed through the window)."""
    pair = _Pair(amd, monkeypatch, K, 6500, 192, env={"OSC_FAKE_COL_SHARD": f"{rank}/2", "OSC_SPMM_XS": xs, "OSC_SPMM_BLOCKED": "0"})
    try:
        for how in ("anchors", "written"):
            for mi in _iteration_counts(K):
                for trip in range(2):
                    pair.settle(how, ("window", rank, xs, K, trip), mi)
    finally:
        pair.close()


@pytest.mark.parametrize("D", [768, 100])
def test_the_planner_alone(amd, D, monkeypatch):
    """No OSC_X_RING: min(predicted iterations, 4) directions from the handle's second solve on (the first has no prediction).
    20 011 x 768: five arrays of the solve are beyond the cache-resident regime (200 MB), the update kernels stream with
    nontemporal accesses; 20 011 x 100: within it, ordinary accesses."""
    room = 4
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("OSC_SMALL_PATH", "0")
    N = 20011
    Y, psi, _, V = _inputs(N, D, seed=9)
    lats = []
    for off in (True, False):
        if off:
            monkeypatch.setenv("OSC_X_RING", "0")
        else:
            monkeypatch.delenv("OSC_X_RING")
        lat = amd.Oscillink(Y, kneighbors=16)
        lat.set_query(psi)
        lats.append(lat)
    ref, ring = lats
    try:
        prev = 0
        for trip, (start, kw) in enumerate([("anchors", {}), ("anchors", {}), ("written", {}), ("anchors", dict(max_iters=2, tol=0.0)),
                                            ("anchors", {}), ("anchors", dict(max_iters=9, tol=0.0)), ("anchors", {})]):
            out = []
            for lat in lats:
                if start == "anchors":
                    lat.reset_U(wait=False)
                else:
                    lat.U = V
                st = lat.settle(**dict(dict(max_iters=12, tol=1e-3), **kw))
                out.append((st["iters"], st["res"], lat.residual_history(), lat.U.copy()))
            assert out[0][:3] == out[1][:3], (trip, out[0][:3], out[1][:3])
            assert np.array_equal(out[0][3], out[1][3]), (trip, float(np.abs(out[0][3] - out[1][3]).max()))
            info = ring.build_info()
            mi = kw.get("max_iters", 12)
            want = _expected(min(prev, room), mi, prev, out[0][0])
            assert (info["x_ring_slots"], info["x_ring_flushes"], info["x_ring_passes"]) == want, (trip, prev, info, want)
            assert ref.build_info()["x_ring_slots"] == 1 and ref.build_info()["x_ring_bytes"] == 0
            prev = out[0][0]
        ld = (D + 31) // 32 * 32 if N * D >= 1 << 22 else D
        assert ring.build_info()["x_ring_bytes"] == (room - 1) * N * ld * 4 + 4 * ld * 4, ring.build_info()  # (the 9-iteration solve's)
    finally:
        ref.close()
        ring.close()

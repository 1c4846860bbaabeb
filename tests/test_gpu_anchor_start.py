"""The settle that starts from the anchors without copying them (U aliases Y until a settle writes it;
the slab-major image of the anchors is built once per lattice).  Nothing of it may change a bit of any result, so every
comparison here is `np.array_equal`, against the same library with the state materialised: `lat.U = lat.Y.copy()` uploads
through osc_set_U(ptr), which clears the alias, and OSC_ANCHOR_SLAB=0 (read at creation) restores the transpose per solve.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MAX_ITERS = (1, 2, 3, 6, 12)
SWITCHES = ("OSC_SPMM_XS", "OSC_REORDER", "OSC_SPMM_BLOCKED", "OSC_BLK_VARIANT", "OSC_BLK_INIT", "OSC_X_DEFER", "OSC_ANCHOR_SLAB",
            "OSC_SMALL_PATH", "OSC_FAKE_COL_SHARD", "OSC_SHARD", "OSC_ROW_FAKE_SHARDS", "OSC_LD", "OSCILLINK_RECEIPT_DYNAMICS")


@pytest.fixture(scope="module")
def amd():
    import oscillink_amd
    from oscillink_amd import _native

    assert _native.device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return oscillink_amd


def _inputs(N, D, seed=3, clustered=False):
    rng = np.random.default_rng(seed)
    Y = rng.standard_normal((N, D)).astype(np.float32)
    if clustered:  # tight groups of 50 rows: a clustered graph, the case the BFS row order is for
        Y = (np.repeat(rng.standard_normal((N // 50 + 1, D)), 50, axis=0)[:N] * 4.0 + Y).astype(np.float32)
        Y = Y[rng.permutation(N)]
    psi = rng.standard_normal(D).astype(np.float32)
    psi /= np.linalg.norm(psi)
    gates = rng.uniform(0.1, 1.0, N).astype(np.float32)
    return Y, psi, gates


class _Pair:
    """Two lattices over the same inputs: `a` starts its settles from the aliased state (reset_U / fresh), `m` from the same
    state materialised in U's own buffer."""

    def __init__(self, amd, Y, psi, k, gates=None, chain=None):
        self.amd, self.Y, self.psi, self.k, self.gates, self.chain = amd, Y, psi, k, gates, chain
        self.a = self.make()
        self.m = self.make()

    def make(self):
        lat = self.amd.Oscillink(self.Y, kneighbors=self.k)
        lat.set_query(self.psi, gates=self.gates)
        if self.chain:
            lat.add_chain(self.chain, lamP=0.3)
        return lat

    def close(self):
        self.a.close()
        self.m.close()


def _start(lat, aliased):
    if aliased:
        lat.reset_U(wait=False)
    else:
        lat.U = lat.Y.copy()


def _settle(lat, aliased, **kw):
    _start(lat, aliased)
    st = lat.settle(**kw)
    return st["iters"], st["res"], lat.residual_history(), lat.U.copy()


def _same(x, y, what):
    assert x[0] == y[0], (what, "iters", x[0], y[0])
    assert x[1] == y[1], (what, "res", x[1], y[1])
    assert x[2] == y[2], (what, "history", x[2], y[2])
    assert np.array_equal(x[3], y[3]), (what, "U", float(np.abs(x[3] - y[3]).max()))


def _guess(lat, aliased, g, **kw):
    """Leave the handle predicting `g` iterations for its next settle (bench.py: cold_and_mispredicted): a settle that
    takes exactly g."""
    _start(lat, aliased)
    kw = dict(kw, max_iters=g, tol=0.0)
    assert lat.settle(**kw)["iters"] == g


def _walk(pair, what, full=True, **kw):
    """max_iters x tol x predicted-iterations state, aliased against materialised.  Returns the number of comparisons."""
    a, m = pair.a, pair.m
    probe = _settle(m, False, max_iters=1, tol=0.0, **kw)
    tol_at_1 = float(probe[1]) * 1.5  # met by iteration 1's residual
    n = 0
    for mi in (MAX_ITERS if full else (1, 3, 12)):
        for tol in (0.0, 1e-3, tol_at_1):
            args = dict(kw, max_iters=mi, tol=tol)
            fa, fm = pair.make(), pair.make()  # fresh handles: no prediction, the very first solve of a lattice
            st = fa.settle(**args)  # (no reset: the state right after construction)
            ra = (st["iters"], st["res"], fa.residual_history(), fa.U.copy())
            rm = _settle(fm, False, **args)
            fa.close()
            fm.close()
            _same(ra, rm, (what, mi, tol, "fresh"))
            n += 1
            iters = rm[0]
            for name, g in (("right", iters), ("short", iters - 1), ("long", iters + 1)):
                if g < 1:
                    continue  # (a guess of 0 iterations is "no prediction": the fresh handle above)
                _guess(a, True, g, **kw)
                _guess(m, False, g, **kw)
                _same(_settle(a, True, **args), _settle(m, False, **args), (what, mi, tol, name))
                n += 1
    return n


def _clean_env(monkeypatch):
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)


@pytest.mark.parametrize("D,variant", [(768, None), (256, None), (256, "3")])
def test_aliased_start_equals_materialised_start_on_the_fused_blocked_init(amd, D, variant, monkeypatch):
    """20 000 rows take the blocked matvec with its fused INIT pass (kernel shape 0 by geometry; OSC_BLK_VARIANT forces a
    wide shape at the same size): the aliased settle gathers from the anchors' image, writes no x0 copy, and the launch
    that applies iteration 1's x update reads x0 from the anchors -- under every outcome of the speculative schedule."""
    _clean_env(monkeypatch)
    if variant is not None:
        monkeypatch.setenv("OSC_BLK_VARIANT", variant)
    Y, psi, gates = _inputs(20000, D)
    pair = _Pair(amd, Y, psi, 16)
    try:
        assert _walk(pair, f"fused D={D} variant={variant}") >= 40
        info = pair.a.build_info()
        assert info["apply_src_blocks"] > 0, info
        assert info["apply_blocked_shape"] == (0 if variant is None else int(variant)), info
        assert info["y_to_u_copies"] == 0 and info["anchor_slab_bytes"] > 0, info
    finally:
        pair.close()


FALLBACKS = {
    "slab_apply_without_blocks": dict(env={"OSC_SPMM_BLOCKED": "0"}),
    "plain_init": dict(env={"OSC_BLK_INIT": "0"}),
    "init_finish_pass": dict(env={"OSC_BLK_INIT": "2"}),
    "x_beside_r": dict(env={"OSC_X_DEFER": "0"}),
    "no_last_form": dict(env={"OSC_X_DEFER": "2"}),
    "per_solve_transpose": dict(env={"OSC_ANCHOR_SLAB": "0"}),
    "chain_prior": dict(chain=[5, 1, 19999, 9000, 7, 2]),
    "gates": dict(gates=True),
    "no_preconditioner": dict(settle={"precond": "none"}),
    "clustered_bfs_order": dict(env={"OSC_REORDER": "1"}, clustered=True),
    "inertia": dict(settle={"inertia": 0.3}),
    "cold_start": dict(settle={"warm_start": False}),
}


@pytest.mark.parametrize("name", sorted(FALLBACKS))
def test_aliased_start_equals_materialised_start_off_the_fast_path(amd, name, monkeypatch):
    """The paths that get the alias but not the deferred x0 copy, and the fast path under the other solver inputs."""
    _clean_env(monkeypatch)
    spec = FALLBACKS[name]
    for k, v in spec.get("env", {}).items():
        monkeypatch.setenv(k, v)
    Y, psi, gates = _inputs(20000, 256, clustered=spec.get("clustered", False))
    pair = _Pair(amd, Y, psi, 16, gates=gates if spec.get("gates") else None, chain=spec.get("chain"))
    try:
        assert _walk(pair, name, **spec.get("settle", {})) >= 40
        info = pair.a.build_info()
        if name == "clustered_bfs_order":  # (a re-ordered lattice gathers from nearby rows: its plan has no source blocks)
            assert info["reordered"] == 1, info
        elif name == "slab_apply_without_blocks":
            assert info["apply_src_blocks"] == 0, info
        else:
            assert info["apply_src_blocks"] > 0, info
        if name == "per_solve_transpose":
            assert info["anchor_slab_bytes"] == 0, info
    finally:
        pair.close()


@pytest.mark.parametrize("N,D", [(6000, 64), (700, 32)])
def test_aliased_start_equals_materialised_start_in_the_one_launch_solve(amd, N, D, monkeypatch):
    _clean_env(monkeypatch)
    Y, psi, gates = _inputs(N, D)
    pair = _Pair(amd, Y, psi, 8, gates=gates)
    try:
        assert _walk(pair, f"one launch N={N}") >= 40
        if N < 1000:
            assert pair.a.build_info()["small_solves"] > 0
    finally:
        pair.close()


def _receipt_terms(lat, detail):
    lat.set_receipt_detail(detail)
    rec = lat.receipt()
    keep = ("deltaH_total", "coh_drop_sum", "anchor_pen_sum", "query_term_sum", "null_points", "cg_iters")
    return {k: rec[k] for k in keep if k in rec}


@pytest.mark.parametrize("N,D", [(20000, 256), (900, 48)])
def test_readers_see_the_anchors_while_u_is_aliased(amd, N, D, monkeypatch, tmp_path):
    _clean_env(monkeypatch)
    Y, psi, gates = _inputs(N, D, seed=11)
    pair = _Pair(amd, Y, psi, 12, gates=gates)
    a, m = pair.a, pair.m
    try:
        m.U = m.Y.copy()
        rows = np.array([0, 5, N - 1, N // 2, 5], dtype=np.int32)
        for trip in range(2):  # right after construction, then after a settle and a reset
            assert np.array_equal(a.U, m.U) and np.array_equal(a.U, Y)
            assert np.array_equal(a._fetch_rows(1, rows), m._fetch_rows(1, rows))
            for detail in ("light", "full"):
                ra, rm = _receipt_terms(a, detail), _receipt_terms(m, detail)
                assert ra == rm, (detail, ra, rm)
            dh_a, dh_m = C.c_double(0.0), C.c_double(0.0)
            a._call("osc_deltaH", C.byref(dh_a))
            m._call("osc_deltaH", C.byref(dh_m))
            assert dh_a.value == dh_m.value
            assert a.bundle(k=8) == m.bundle(k=8)
            prev = (Y * np.float32(0.5)).astype(np.float32)
            assert a._compute_dynamics(prev, None, 3) == m._compute_dynamics(prev, None, 3)
            a._call("osc_dynamics_snapshot")
            m._call("osc_dynamics_snapshot")
            sa, sm = a.settle(max_iters=4, tol=0.0), m.settle(max_iters=4, tol=0.0)
            assert (sa["iters"], sa["res"]) == (sm["iters"], sm["res"]) and np.array_equal(a.U, m.U)
            assert a._compute_dynamics(None, None, 4) == m._compute_dynamics(None, None, 4)
            a.reset_U()
            m.U = m.Y.copy()
        path = str(tmp_path / "state.npz")
        a.save_state(path, format="npz")
        back = type(a).from_npz(path)
        try:
            assert np.array_equal(back.U, m.U)
            sb, sm = back.settle(max_iters=6, tol=1e-3), m.settle(max_iters=6, tol=1e-3)
            assert (sb["iters"], sb["res"]) == (sm["iters"], sm["res"]) and np.array_equal(back.U, m.U)
        finally:
            back.close()
    finally:
        pair.close()


def test_sequences_of_resets_uploads_and_settles(amd, monkeypatch):
    _clean_env(monkeypatch)
    N, D = 20000, 256
    Y, psi, gates = _inputs(N, D, seed=5)
    V = (Y + np.float32(0.25) * np.random.default_rng(6).standard_normal((N, D))).astype(np.float32)
    pair = _Pair(amd, Y, psi, 16, gates=gates)
    a, m = pair.a, pair.m
    kw = dict(max_iters=12, tol=1e-3)

    def run(lat):
        st = lat.settle(**kw)
        return st["iters"], st["res"], lat.residual_history(), lat.U.copy()

    try:
        # create -> settle -> reset_U -> settle: two fresh lattices' first settles (predictions apart, which are walked above)
        first = run(a)
        a.reset_U()
        second = run(a)
        f1, f2 = pair.make(), pair.make()
        _same(first, run(f1), "first settle")
        f2.settle(**kw)
        f2.U = f2.Y.copy()
        _same(second, run(f2), "settle after reset")
        f1.close()
        f2.close()
        # the same sequences with the alias defeated
        m.U = m.Y.copy()
        run(m)
        m.U = m.Y.copy()
        run(m)
        # reset_U -> lat.U = V -> settle
        a.reset_U()
        a.U = V
        m.U = V
        _same(run(a), run(m), "upload after reset")
        # settle -> settle: the second one is warm, not aliased
        a.reset_U()
        m.U = m.Y.copy()
        _same(run(a), run(m), "settle")
        _same(run(a), run(m), "warm settle")
        info = a.build_info()
        assert info["y_to_u_copies"] == 0, info
    finally:
        pair.close()


def test_windowed_and_multi_rank_handles_keep_the_eager_copy(amd, monkeypatch):
    _clean_env(monkeypatch)
    Y, psi, _ = _inputs(4000, 64, seed=2)
    monkeypatch.setenv("OSC_FAKE_COL_SHARD", "0/8")
    lat = amd.Oscillink(Y, kneighbors=8)
    try:
        assert lat.build_info()["y_to_u_copies"] == 1
        lat.reset_U()
        assert lat.build_info()["y_to_u_copies"] == 2
    finally:
        lat.close()
    monkeypatch.delenv("OSC_FAKE_COL_SHARD")
    from oscillink_amd.sharding import run_loopback_ranks

    def rank_fn(rank, comm):
        lt = amd.Oscillink(Y, kneighbors=8, comm=comm)
        lt.set_query(psi)
        before = lt.build_info()["y_to_u_copies"]
        st = lt.settle(max_iters=6, tol=1e-3)
        return before, st["iters"], lt.U.copy()

    out = run_loopback_ranks(2, rank_fn)
    assert all(o[0] >= 1 for o in out), [o[0] for o in out]
    one = amd.Oscillink(Y, kneighbors=8)
    try:
        one.set_query(psi)
        st = one.settle(max_iters=6, tol=1e-3)
        assert one.build_info()["y_to_u_copies"] == 0
        assert out[0][1] == st["iters"] and np.array_equal(out[0][2], out[1][2])
    finally:
        one.close()


@pytest.mark.parametrize("slab", ["1", "0"])
def test_counters_say_the_work_is_gone(amd, slab, monkeypatch):
    _clean_env(monkeypatch)
    monkeypatch.setenv("OSC_ANCHOR_SLAB", slab)
    N, D = 20000, 256
    Y, psi, _ = _inputs(N, D, seed=8)
    lat = amd.Oscillink(Y, kneighbors=16)
    try:
        lat.set_query(psi)
        for _ in range(3):
            lat.reset_U()
            lat.settle(max_iters=12, tol=1e-3)
        info = lat.build_info()
        assert info["apply_src_blocks"] > 0, info
        assert info["y_to_u_copies"] == 0, info
        ld = 256  # (N x D >= 2^22: line-aligned rows; 256 floats are 1 KB, no 4 KB multiple)
        if slab == "1":
            assert info["rows_to_slab_launches"] == 1 and info["anchor_slab_bytes"] == N * ld * 4, info
        else:
            assert info["rows_to_slab_launches"] == 3 and info["anchor_slab_bytes"] == 0, info
        lat.solve_Ustar(use_cache=False)
        lat.set_query(-psi)
        lat.solve_Ustar(use_cache=False)
        info = lat.build_info()
        assert info["rows_to_slab_launches"] == (1 if slab == "1" else 5), info
    finally:
        lat.close()

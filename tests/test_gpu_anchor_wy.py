"""The cached row sums W.Y of the anchors: the first solve that starts from the anchors on the fused
blocked INIT path leaves every row's gathered sum behind, and every later one on the same graph copy streams its INIT pass
(k_init_cached) instead of gathering.  Nothing of it may change a bit of any result, so every comparison here is
`np.array_equal`, against the same library with OSC_ANCHOR_WY=0 (read at creation: the gathering INIT pass every time).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SWITCHES = ("OSC_SPMM_XS", "OSC_REORDER", "OSC_SPMM_BLOCKED", "OSC_BLK_VARIANT", "OSC_BLK_INIT", "OSC_X_DEFER", "OSC_ANCHOR_SLAB",
            "OSC_ANCHOR_WY", "OSC_SMALL_PATH", "OSC_FAKE_COL_SHARD", "OSC_SHARD", "OSC_ROW_FAKE_SHARDS", "OSC_LD",
            "OSCILLINK_RECEIPT_DYNAMICS")
CHAIN = [5, 1, 19999, 9000, 7, 2]
KW = dict(max_iters=12, tol=1e-3)


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
    psi2 = rng.standard_normal(D).astype(np.float32)
    psi2 /= np.linalg.norm(psi2)
    gates = rng.uniform(0.1, 1.0, N).astype(np.float32)
    return Y, psi, psi2, gates


class _Pair:
    """Two lattices over the same inputs: `ref` created under OSC_ANCHOR_WY=0, `wy` without it."""

    def __init__(self, amd, monkeypatch, Y, psi, k, gates=None, chain=None):
        def make():
            lat = amd.Oscillink(Y, kneighbors=k)
            lat.set_query(psi, gates=gates)
            if chain:
                lat.add_chain(chain, lamP=0.3)
            return lat

        monkeypatch.setenv("OSC_ANCHOR_WY", "0")
        self.ref = make()
        monkeypatch.delenv("OSC_ANCHOR_WY")
        self.wy = make()
        self.both = (self.ref, self.wy)

    def close(self):
        self.ref.close()
        self.wy.close()

    def cached(self):
        assert self.ref.build_info()["cached_inits"] == 0 and self.ref.build_info()["anchor_wy_bytes"] == 0
        return self.wy.build_info()["cached_inits"]


def _anchor_start(lat, **kw):
    lat.reset_U(wait=False)
    st = lat.settle(**dict(KW, **kw))
    return st["iters"], st["res"], lat.residual_history(), lat.U.copy()


def _same(x, y, what):
    assert x[0] == y[0], (what, "iters", x[0], y[0])
    assert x[1] == y[1], (what, "res", x[1], y[1])
    assert x[2] == y[2], (what, "history", x[2], y[2])
    assert np.array_equal(x[3], y[3]), (what, "U", float(np.abs(x[3] - y[3]).max()))


def _both_start(pair, what, **kw):
    """One anchor start on both lattices, compared; returns by how much `cached_inits` grew."""
    before = pair.cached()
    _same(_anchor_start(pair.ref, **kw), _anchor_start(pair.wy, **kw), what)
    return pair.cached() - before


def _walk(pair, what, psi2, **kw):
    """Build, two cached starts, the U* solve, then another query and other lams."""
    assert _both_start(pair, (what, "build"), **kw) == 0
    assert _both_start(pair, (what, "cached 1"), **kw) == 1
    assert _both_start(pair, (what, "cached 2"), **kw) == 1
    before = pair.cached()
    us = [lat.solve_Ustar(use_cache=False).copy() for lat in pair.both]
    assert np.array_equal(us[0], us[1]), (what, "U*", float(np.abs(us[0] - us[1]).max()))
    assert pair.ref.residual_history() == pair.wy.residual_history(), (what, "U* history")
    assert pair.cached() == before + 1, (what, "the U* solve starts from the anchors too")
    for lat in pair.both:
        lat.set_query(psi2, gates=None)
        lat.lamC, lat.lamQ = 0.8, 2.5
    assert _both_start(pair, (what, "other query and lams"), **kw) == 1
    us = [lat.solve_Ustar(use_cache=False).copy() for lat in pair.both]
    assert np.array_equal(us[0], us[1]), (what, "U* 2", float(np.abs(us[0] - us[1]).max()))


def _clean_env(monkeypatch):
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)


@pytest.mark.parametrize("N,D,variant,shape", [(20000, 256, None, 0), (20000, 256, "3", 3), (20000, 768, None, None),
                                               (20000, 768, "3", 3), (30011, 200, None, None), (30011, 200, "3", 3)])
def test_cached_init_equals_gathering_init(amd, N, D, variant, shape, monkeypatch):
    """Kernel shape 0 by geometry and a forced wide shape; D = 200 leaves the last slab 8 of its 32 columns (`cok` cuts lanes
    off) and 30 011 rows are no multiple of any deal of groups (`row < rhi` does)."""
    _clean_env(monkeypatch)
    if variant is not None:
        monkeypatch.setenv("OSC_BLK_VARIANT", variant)
    Y, psi, psi2, _ = _inputs(N, D)
    pair = _Pair(amd, monkeypatch, Y, psi, 16)
    try:
        _walk(pair, f"N={N} D={D} variant={variant}", psi2)
        info = pair.wy.build_info()
        assert info["apply_src_blocks"] > 0, info
        if shape is not None:
            assert info["apply_blocked_shape"] == shape, info
        ld = (D + 31) // 32 * 32
        assert info["anchor_wy_bytes"] == N * ld * 4 == info["anchor_slab_bytes"], info
    finally:
        pair.close()


SOLVER_INPUTS = {
    "gates": dict(gates=True),
    "no_preconditioner": dict(settle={"precond": "none"}),
    "chain_prior": dict(chain=CHAIN),
    "chain_prior_and_gates_wide": dict(chain=CHAIN, gates=True, env={"OSC_BLK_VARIANT": "3"}),
}


@pytest.mark.parametrize("name", sorted(SOLVER_INPUTS))
def test_cached_init_under_the_other_solver_inputs(amd, name, monkeypatch):
    _clean_env(monkeypatch)
    spec = SOLVER_INPUTS[name]
    for k, v in spec.get("env", {}).items():
        monkeypatch.setenv(k, v)
    Y, psi, psi2, gates = _inputs(20000, 256)
    pair = _Pair(amd, monkeypatch, Y, psi, 16, gates=gates if spec.get("gates") else None, chain=spec.get("chain"))
    try:
        _walk(pair, name, psi2, **spec.get("settle", {}))
        assert pair.wy.build_info()["apply_src_blocks"] > 0
    finally:
        pair.close()


def test_graph_changes_drop_the_cached_sums(amd, monkeypatch):
    """A rebuilt or injected graph has other row sums, and a plan with another block count forms them in another order: the
    next anchor start gathers again (and equals the reference lattice's), the one after it is served from the new sums."""
    _clean_env(monkeypatch)
    N, D = 20000, 256
    Y, psi, _, gates = _inputs(N, D, seed=7)
    pair = _Pair(amd, monkeypatch, Y, psi, 16, gates=gates)
    donor = amd.Oscillink(Y, kneighbors=9)
    try:
        assert _both_start(pair, "build") == 0
        assert _both_start(pair, "cached") == 1
        for lat in pair.both:
            lat.rebuild_graph(kneighbors=12)
        assert pair.wy.build_info()["anchor_wy_bytes"] == 0
        assert _both_start(pair, "after rebuild_graph") == 0
        assert _both_start(pair, "cached after rebuild_graph") == 1
        rowptr, col, a = donor._host_csr()[:3]
        for lat in pair.both:
            lat.set_graph_csr(rowptr, col, a)
        assert pair.wy.build_info()["anchor_wy_bytes"] == 0
        assert _both_start(pair, "after set_graph_csr") == 0
        assert _both_start(pair, "cached after set_graph_csr") == 1
        # the chain prior leaves W alone: the sums stay valid unless the plan with the chain asks for another block count
        blocks = pair.wy.build_info()["apply_src_blocks"]
        for lat in pair.both:
            lat.add_chain(CHAIN, lamP=0.3)
        grew = _both_start(pair, "after add_chain")
        assert grew == (1 if pair.wy.build_info()["apply_src_blocks"] == blocks else 0)
        assert _both_start(pair, "cached after add_chain") == 1
        blocks = pair.wy.build_info()["apply_src_blocks"]
        for lat in pair.both:
            lat.clear_chain()
        grew = _both_start(pair, "after clear_chain")
        assert grew == (1 if pair.wy.build_info()["apply_src_blocks"] == blocks else 0)
        assert _both_start(pair, "cached after clear_chain") == 1
        assert pair.wy.build_info()["anchor_wy_bytes"] == N * 256 * 4
    finally:
        donor.close()
        pair.close()


def test_reordered_lattice_keeps_its_own_init(amd, monkeypatch):
    """A re-ordered lattice gathers from nearby rows: its plan has no source blocks, so nothing is cached for it."""
    _clean_env(monkeypatch)
    monkeypatch.setenv("OSC_REORDER", "1")
    Y, psi, _, _ = _inputs(20000, 256, clustered=True)
    pair = _Pair(amd, monkeypatch, Y, psi, 16)
    try:
        for trip in range(3):
            assert _both_start(pair, ("reordered", trip)) == 0
        info = pair.wy.build_info()
        assert info["reordered"] == 1 and info["cached_inits"] == 0 and info["anchor_wy_bytes"] == 0, info
    finally:
        pair.close()


@pytest.mark.parametrize("switch", [None, "OSC_ANCHOR_SLAB", "OSC_ANCHOR_WY"])
def test_counters(amd, switch, monkeypatch):
    _clean_env(monkeypatch)
    if switch is not None:
        monkeypatch.setenv(switch, "0")
    N, D = 20000, 256
    Y, psi, _, _ = _inputs(N, D, seed=8)
    lat = amd.Oscillink(Y, kneighbors=16)
    try:
        lat.set_query(psi)
        for _ in range(3):
            lat.reset_U()
            lat.settle(**KW)
        info = lat.build_info()
        assert info["apply_src_blocks"] > 0, info
        ld = 256  # (N x D >= 2^22: line-aligned rows; 256 floats are 1 KB, no 4 KB multiple)
        if switch is None:
            assert info["cached_inits"] == 2 and info["rows_to_slab_launches"] == 1, info
            assert info["anchor_wy_bytes"] == N * ld * 4, info
        else:
            assert info["cached_inits"] == 0 and info["anchor_wy_bytes"] == 0, info
            assert info["rows_to_slab_launches"] == (3 if switch == "OSC_ANCHOR_SLAB" else 1), info
    finally:
        lat.close()


def test_joining_a_communicator_drops_the_image_and_the_sums(amd, monkeypatch):
    """`osc_comm_init` gives the handle another column window, and `Ys` / `WYs` are laid out over the window.  Per rank of a
    two-rank loopback group: handle A solves on the full window first and joins then, handle B joins before it has solved
    anything.  A's image and sums are gone after the call, and its next solve equals B's to the bit."""
    from oscillink_amd import _native as nat
    from oscillink_amd import sharding

    _clean_env(monkeypatch)
    N, D, ld = 20000, 256, 256
    Y, psi, _, _ = _inputs(N, D, seed=11)
    uid_b = sharding.loopback_id()

    def join(lat, uid, rank, world):
        nat.check(nat.lib().osc_comm_init(lat._h, bytes(uid), int(rank), int(world)), lat._h, "osc_comm_init")

    def rank_fn(rank, comm):
        uid_a, _, world = comm
        a, b = amd.Oscillink(Y, kneighbors=16), amd.Oscillink(Y, kneighbors=16)
        try:
            for lat in (a, b):
                lat.set_query(psi)
            a.solve_Ustar(use_cache=False)
            info = a.build_info()
            assert info["anchor_slab_bytes"] == N * ld * 4 == info["anchor_wy_bytes"], info
            join(a, uid_a, rank, world)
            info = a.build_info()
            assert info["anchor_slab_bytes"] == 0 and info["anchor_wy_bytes"] == 0, info
            join(b, uid_b, rank, world)
            out = []
            for lat in (a, b):
                us = lat.solve_Ustar(use_cache=False).copy()
                info = lat.build_info()
                assert info["apply_src_blocks"] > 0 and info["anchor_slab_bytes"] > 0, info
                out.append((us, lat.residual_history()))
            return out
        finally:
            a.close()
            b.close()

    for rank, ((ua, ha), (ub, hb)) in enumerate(sharding.run_loopback_ranks(2, rank_fn, timeout_s=120.0)):
        assert np.array_equal(ua, ub), (rank, float(np.abs(ua - ub).max()))
        assert ha == hb, (rank, ha, hb)

"""The device BFS row order (csrc/bfs_order.hip), the clustering sample (k_clustering_sample), the state move (k_permute_ell,
k_move_rows, k_move_1d) and the decision in maybe_reorder, on hand-made graphs injected with set_graph_csr.

The expected order and the expected clustering count come from tests/_order_reference.py (a queue BFS and a set lookup in
plain Python, themselves checked against SciPy in tests/test_order_reference_host.py); `bfs_on_device` proves which path gave
the order.  What each graph reaches -- sort passes, depth, tile seams -- is asserted there through the same makers."""
import time

import numpy as np
import pytest

from tests import _order_reference as ref
from tests import _small_reference as sr
from tests._cases import relerr

pytestmark = pytest.mark.gpu


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


def _anchors(N, D, seed=0):
    return np.random.default_rng(seed).standard_normal((N, D)).astype(np.float32)


def _row_order(lat):
    from oscillink_amd import _native as nat

    perm = np.full(lat.N, -1, dtype=np.int32)
    lat._call("osc_get_row_order", nat.i32(perm))
    return perm


def _inject(amd, Y, g):
    lat = amd.Oscillink(Y, _build_graph=False)
    lat.set_graph_csr(*g)
    return lat


def _check_order(lat, g, on_device):
    want, depth = ref.bfs_order(g[0], g[1])
    N = lat.N
    print(f"\nN {N}: depth {depth}, sort passes {ref.sort_passes(N, depth)}, declines {ref.declines(depth)}")
    assert ref.declines(depth) == (on_device == 0)
    info = lat.build_info()
    assert info["reordered"] == 1 and info["order_kind"] == "bfs", info
    assert info["bfs_on_device"] == on_device, info
    got = _row_order(lat)
    assert np.array_equal(got, want), f"first difference at position {int(np.flatnonzero(got != want)[0])}"
    return depth


@pytest.mark.parametrize("name", list(ref.ORDER_CASES))
def test_injected_graph_order_equals_the_reference_walk(amd, name, monkeypatch):
    monkeypatch.setenv("OSC_REORDER", "1")
    monkeypatch.setenv("OSC_BALANCE", "0")
    monkeypatch.delenv("OSC_BFS_HOST", raising=False)
    make, on_device = ref.ORDER_CASES[name]
    g = make()
    lat = _inject(amd, _anchors(g[0].shape[0] - 1, 4), g)
    _check_order(lat, g, on_device)
    lat.close()


def test_order_of_a_million_rows_crosses_the_scan_carry(amd, monkeypatch):
    """N = 1 050 000, D = 1: 1026 scan tiles over N and 1026 sort tiles -- the second 1024-tile chunk of k_scan_sums with its
    carry -- and 6 sort passes.  The time of the injection (host packing, upload, device BFS, state move) is printed: 0.03 s on
    an MI355X, 1.1 s for the whole case with the graph build and the reference walk."""
    monkeypatch.setenv("OSC_REORDER", "1")
    monkeypatch.setenv("OSC_BALANCE", "0")
    monkeypatch.delenv("OSC_BFS_HOST", raising=False)
    g = ref.big_paths()
    lat = amd.Oscillink(_anchors(ref.BIG_N, 1), _build_graph=False)
    t0 = time.perf_counter()
    lat.set_graph_csr(*g)
    t1 = time.perf_counter()
    depth = _check_order(lat, g, 1)
    print(f"set_graph_csr {t1 - t0:.2f} s, reference walk and comparison {time.perf_counter() - t1:.2f} s")
    assert ref.sort_passes(ref.BIG_N, depth) == 6
    lat.close()


@pytest.mark.parametrize("small_path", ["default", "general"])
@pytest.mark.parametrize("name", ref.STATE_MOVE_CASES)
def test_state_moves_with_the_order(amd, orc, name, small_path, monkeypatch):
    """A reordered handle answers every API read exactly as a handle in API order does, and solves the injected system:
    U* against a float64 direct solve, by the yardstick of test_gpu_small_solve.py (at most twice the float32 oracle's own
    distance, which must itself lie at the float32 floor).  Gates and an explicit U are set BEFORE the graph arrives on the
    reordered handle, so the state move carries them (k_move_1d, k_move_rows)."""
    monkeypatch.setenv("OSC_BALANCE", "0")
    monkeypatch.delenv("OSC_BFS_HOST", raising=False)
    if small_path == "general":
        monkeypatch.setenv("OSC_SMALL_PATH", "0")
    g = ref.ORDER_CASES[name][0]()
    N, D = g[0].shape[0] - 1, 4
    Y, psi = sr.inputs(N, D)
    U0 = _anchors(N, D, seed=5)
    gates = sr.gates_with_exact_ends(N)
    lats = {}
    for reorder in ("1", "0"):
        monkeypatch.setenv("OSC_REORDER", reorder)
        lat = amd.Oscillink(Y, _build_graph=False)
        lat.U = U0
        if reorder == "1":
            lat.set_query(psi, gates=gates)
        lat.set_graph_csr(*g)
        if reorder == "0":
            lat.set_query(psi, gates=gates)
        lat._U_host = lat._Y_host = None  # read both back from the device
        lats[reorder] = lat
    moved, plain = lats["1"], lats["0"]
    assert moved.build_info()["reordered"] == 1 and moved.build_info()["bfs_on_device"] == 1
    assert plain.build_info()["reordered"] == 0 and plain.build_info()["bfs_on_device"] == 0
    assert not np.array_equal(_row_order(moved), np.arange(N)) and np.array_equal(_row_order(plain), np.arange(N))
    # (the few rows osc_edge_prefix reads, before graph_csr() fills the host cache that would answer instead)
    pm, pp = moved._edge_prefix(), plain._edge_prefix()
    assert pm.shape == pp.shape and pm.shape[0] == min(2048, g[1].size) and np.array_equal(pm, pp)
    rows = np.repeat(np.arange(N), np.diff(g[0]))
    assert np.array_equal(pm, np.stack([rows, g[1]], axis=1)[:2048])
    cm, cp = moved.graph_csr(), plain.graph_csr()
    for got in (cm, cp):
        assert np.array_equal(got[0], g[0]) and np.array_equal(got[1], g[1]) and np.array_equal(got[2], g[2])
    assert np.array_equal(cm[3], cp[3]) and np.array_equal(cm[4], cp[4])  # w, sqrt_deg
    assert np.array_equal(moved.Y, Y) and np.array_equal(plain.Y, Y)
    assert np.array_equal(moved.U, U0) and np.array_equal(plain.U, U0)
    assert np.array_equal(moved.B_diag, gates) and np.array_equal(plain.B_diag, gates)
    moved.reset_U()  # U aliases Y again: read through the order
    assert np.array_equal(moved.U, Y)
    # the solve on the moved state
    chain = sr.chain_for(N)
    moved.add_chain(chain, lamP=sr.CHAIN_LAMP)
    A = sr.adjacency(moved)
    oracle = orc.OracleLattice(Y, kneighbors=6, deterministic_k=True, dense=False, graph=A)
    sr.configure(oracle, psi, gates, chain)
    x64, direct_res = sr.ustar_fp64(orc, A, Y, psi, gates, chain)
    assert direct_res < 1e-10
    want = oracle.solve_Ustar(tol=1e-6, max_iters=64)
    got = moved.solve_Ustar(tol=1e-6, max_iters=64)
    d_ref, d_dev = relerr(want, x64), relerr(got, x64)
    small = moved.build_info()["small_solves"]
    print(f"\n{name} {small_path}: one-launch solves {small}, iterations oracle {oracle.last_ustar['iters']} / device "
          f"{moved.last_ustar['iters']}, distance oracle {d_ref:.4e} / device {d_dev:.4e}, ratio {d_dev / d_ref:.3f}")
    if small_path == "general":
        assert small == 0
    assert 1e-8 < d_ref < 2e-6
    assert d_dev <= 2.0 * d_ref
    for lat in lats.values():
        lat.close()


def test_clustering_sample_counts_exactly_and_decides(amd, monkeypatch):
    """Automatic mode at N = 9000 (the sample stride 9000 / 1024 is not constant): the sampled clustering coefficient is
    hits / pairs of the reference, the same two integers divided in double, on a graph that reaches every path of the kernel
    (tests/test_order_reference_host.py prints the table), and on a sparse graph that must stay in API order."""
    monkeypatch.delenv("OSC_REORDER", raising=False)
    monkeypatch.delenv("OSC_BFS_HOST", raising=False)
    monkeypatch.setenv("OSC_BALANCE", "0")
    Y = _anchors(9000, 4)
    g = ref.clustering_graph()
    hits, pairs, value = ref.clustering(g[0], g[1])
    lat = _inject(amd, Y, g)
    got = lat.build_info()["clustering"]
    print(f"\nclustered graph: reference {hits} / {pairs} = {value!r}, device {got!r} (x pairs = {got * pairs!r})")
    assert value >= 0.05 and got == value
    _check_order(lat, g, 1)
    lat.close()
    g = ref.sparse_remainder()
    hits, pairs, value = ref.clustering(g[0], g[1])
    lat = _inject(amd, Y, g)
    info = lat.build_info()
    print(f"sparse graph: reference {hits} / {pairs} = {value!r}, device {info['clustering']!r}")
    assert 0.0 < value < 0.05 and info["clustering"] == value
    assert info["reordered"] == 0 and info["bfs_on_device"] == 0 and info["order_kind"] == "none", info
    assert np.array_equal(_row_order(lat), np.arange(9000))
    lat.close()

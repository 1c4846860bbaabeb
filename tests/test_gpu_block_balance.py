"""Balanced source blocks (oscillink_amd/csrc/block_balance.hpp, balance_kernels.hip): an unstructured
lattice's rows stored in an order under which every row's neighbours spread over the source blocks of the blocked CG
matvec.  The order is internal: every call speaks the caller's row ids, and every result equals, to rounding, that of a
handle created under OSC_BALANCE=0 on the same data (a row's edges are summed in another order, so not to the bit).

OSC_BALANCE=1 with the switches that force the blocked plan at small sizes (OSC_SMALL_PATH=0, OSC_SPMM_XS=1,
OSC_SPMM_BLOCKED=nb, and OSC_LD for the 128-byte row pitch the slab mode needs, which small lattices do not get by
themselves), as tests/test_gpu_anchor_wy.py and tests/test_gpu_parity.py force it.  Shapes: 3001 x 72 at k = 32 over 8
blocks (3001 is no multiple of 8: the last block is 7 rows short; 72 columns are no multiple of 32; a fifth of the rows is
at full degree 32 = 8 blocks x 4 slots) and 2050 x 40 at k = 12 over 3 blocks (2050 = 3 x 684 - 2); the communicator case
1203 x 128 over 3 blocks (two ranks' windows of 64 columns).  Tolerance on U and U*: 2e-5 relative, what the parity tests
hold a settle to against the oracle."""
import numpy as np
import pytest

from tests._cases import relerr

pytestmark = pytest.mark.gpu

SWITCHES = ("OSC_SPMM_XS", "OSC_REORDER", "OSC_SPMM_BLOCKED", "OSC_BLK_VARIANT", "OSC_BLK_INIT", "OSC_SMALL_PATH", "OSC_BALANCE",
            "OSC_BALANCE_HOST", "OSC_FAKE_COL_SHARD", "OSC_SHARD", "OSC_ROW_FAKE_SHARDS", "OSC_LD")
SHAPES = [(3001, 72, 32, 8), (2050, 40, 12, 3)]
KW = dict(max_iters=12, tol=1e-4)
SLOTS = 4
TOL = 2e-5


@pytest.fixture(scope="module")
def amd():
    import oscillink_amd
    from oscillink_amd import _native

    assert _native.device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return oscillink_amd


def _env(monkeypatch, nb, **extra):
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("OSC_SMALL_PATH", "0")
    monkeypatch.setenv("OSC_SPMM_XS", "1")
    monkeypatch.setenv("OSC_SPMM_BLOCKED", str(nb))
    monkeypatch.setenv("OSC_LD", "128")  # (one pitch for every shape here: D <= 128)
    for name, val in extra.items():
        monkeypatch.setenv(name, val)


_INPUTS = {}


def _inputs(N, D):
    if (N, D) not in _INPUTS:
        rng = np.random.default_rng(11)
        Y = rng.standard_normal((N, D)).astype(np.float32)
        psi = rng.standard_normal(D).astype(np.float32)
        psi /= np.linalg.norm(psi)
        gates = rng.uniform(0.1, 1.0, N).astype(np.float32)
        for a in (Y, psi, gates):
            a.setflags(write=False)
        _INPUTS[(N, D)] = (Y, psi, gates)
    return _INPUTS[(N, D)]


def _row_order(lat):
    from oscillink_amd import _native as nat

    perm = np.zeros(lat.N, dtype=np.int32)
    lat._call("osc_get_row_order", nat.i32(perm))
    return perm


def _displaced(lat, perm, nb):
    """Edges beyond SLOTS per (row, source block) when API row perm[p] is stored at position p: a NumPy count."""
    rp, col = lat.graph_csr()[:2]
    N = lat.N
    inv = np.empty(N, dtype=np.int64)
    inv[perm] = np.arange(N)
    rpb = (N + nb - 1) // nb
    rows = np.repeat(np.arange(N), np.diff(rp))
    blk = np.minimum(nb - 1, inv[col] // rpb)
    cnt = np.bincount(rows * nb + blk, minlength=N * nb)
    return int(np.maximum(0, cnt - SLOTS).sum())


def _pair(amd, monkeypatch, N, D, k, nb, **extra):
    """(OSC_BALANCE=0, OSC_BALANCE=1) over the same inputs; the switches are read at creation."""
    Y, psi, gates = _inputs(N, D)
    lats = []
    for bal in ("0", "1"):
        _env(monkeypatch, nb, OSC_BALANCE=bal, **extra)
        lat = amd.Oscillink(Y, kneighbors=k)
        lat.set_query(psi)
        lats.append(lat)
    return lats


@pytest.mark.parametrize("N,D,k,nb", SHAPES)
def test_device_order_equals_the_host_reference_and_counts_its_displaced_edges(amd, N, D, k, nb, monkeypatch):
    """(a) the permutation of the device rounds equals the host reference's to the element (OSC_BALANCE_HOST=1 runs
    block_balance.hpp inside the library on the same graph); (f) the reported displaced edges equal a NumPy count over
    graph_csr() and the returned permutation; two builds give the same order."""
    Y, psi, _ = _inputs(N, D)
    _env(monkeypatch, nb, OSC_BALANCE="1")
    dev = amd.Oscillink(Y, kneighbors=k)
    dev2 = amd.Oscillink(Y, kneighbors=k)
    _env(monkeypatch, nb, OSC_BALANCE="1", OSC_BALANCE_HOST="1")
    host = amd.Oscillink(Y, kneighbors=k)
    try:
        info, hinfo = dev.build_info(), host.build_info()
        assert info["order_kind"] == "balanced" and hinfo["order_kind"] == "balanced", (info, hinfo)
        assert info["reordered"] == 0 and info["balance_src_blocks"] == nb, info
        assert info["balance_on_device"] == 1 and dev2.build_info()["balance_on_device"] == 1, info  # the kernels ran, not the fall-back
        assert hinfo["balance_on_device"] == 0, hinfo
        perm = _row_order(dev)
        assert np.array_equal(np.sort(perm), np.arange(N))
        assert np.array_equal(perm, _row_order(host))
        assert np.array_equal(perm, _row_order(dev2))
        for key in ("displaced_edges_before", "displaced_edges_after", "balance_rounds"):
            assert info[key] == hinfo[key], (key, info[key], hinfo[key])
        deg = np.diff(dev.graph_csr()[0])
        assert (deg == k).any() and deg.max() == k  # a row at full degree
        assert info["displaced_edges_before"] == _displaced(dev, np.arange(N), nb)
        assert info["displaced_edges_after"] == _displaced(dev, perm, nb)
        assert info["displaced_edges_after"] < info["displaced_edges_before"], info
        rpb = (N + nb - 1) // nb
        for b in range(nb):  # block-major, ascending API id inside a block
            assert np.all(np.diff(perm[b * rpb:(b + 1) * rpb]) > 0), b
    finally:
        for lat in (dev, dev2, host):
            lat.close()


@pytest.mark.parametrize("N,D,k,nb", SHAPES)
def test_results_equal_the_api_order_s_to_rounding(amd, N, D, k, nb, monkeypatch):
    """(b) settle from the anchors and warm, U*, the light receipt and bundle against a handle in API order: same iteration
    counts, U and U* within 2e-5, the same graph in API labels, U in API order; (c) then gates set through the API."""
    ref, bal = _pair(amd, monkeypatch, N, D, k, nb)
    _, psi, gates = _inputs(N, D)
    try:
        assert ref.build_info()["order_kind"] == "none" and bal.build_info()["order_kind"] == "balanced"
        for x, y in zip(ref.graph_csr(), bal.graph_csr()):
            assert np.array_equal(x, y)
        for step in ("anchor start", "warm start", "gates"):
            if step == "gates":
                for lat in (ref, bal):
                    lat.set_gates(gates)
                    lat.reset_U()
            sts = [lat.settle(**KW) for lat in (ref, bal)]
            assert sts[0]["iters"] == sts[1]["iters"] and sts[0]["iters"] >= 1, (step, sts)
            assert sts[0]["res"] == pytest.approx(sts[1]["res"], rel=2e-2, abs=1e-7), (step, sts)
            e = relerr(bal.U, ref.U)
            print(f"N={N} nb={nb} {step}: iters {sts[1]['iters']} relerr U {e:.3e}")
            assert e < TOL, (step, e)
            us = [lat.solve_Ustar(use_cache=False).copy() for lat in (ref, bal)]
            assert ref.last_ustar["iters"] == bal.last_ustar["iters"], step
            e = relerr(us[1], us[0])
            print(f"N={N} nb={nb} {step}: relerr U* {e:.3e}")
            assert e < TOL, (step, e)
            assert bal.build_info()["apply_src_blocks"] == nb and ref.build_info()["apply_src_blocks"] == nb
        for lat in (ref, bal):
            lat.set_receipt_detail("light")
        r0, r1 = ref.receipt(), bal.receipt()
        assert r1["deltaH_total"] == pytest.approx(r0["deltaH_total"], rel=1e-4)
        b0, b1 = ref.bundle(k=6), bal.bundle(k=6)
        assert [b["id"] for b in b0] == [b["id"] for b in b1]
        assert np.allclose([b["score"] for b in b1], [b["score"] for b in b0], rtol=1e-3, atol=1e-4)
        # U speaks the caller's row ids: row i of a fresh state is anchor i
        bal.reset_U()
        assert np.array_equal(bal.U, np.asarray(bal.Y))
    finally:
        ref.close()
        bal.close()


def test_chain_prior_under_the_balanced_order(amd, monkeypatch):
    """(c) a chain prior in the caller's ids, installed under the balanced order (the fix-up launch behind the blocked
    matvec), and its chain receipt."""
    N, D, k, nb = SHAPES[0]
    ref, bal = _pair(amd, monkeypatch, N, D, k, nb)
    chain = [5, 1, N - 1, 1500, 7, 2]
    try:
        for lat in (ref, bal):
            lat.add_chain(chain, lamP=0.3)
        assert bal.build_info()["order_kind"] == "balanced"
        sts = [lat.settle(**KW) for lat in (ref, bal)]
        assert sts[0]["iters"] == sts[1]["iters"], sts
        assert relerr(bal.U, ref.U) < TOL, relerr(bal.U, ref.U)
        c0, c1 = ref.chain_receipt(chain), bal.chain_receipt(chain)
        assert c0["verdict"] == c1["verdict"]
        assert np.allclose([e["z_struct"] for e in c1["edges"]], [e["z_struct"] for e in c0["edges"]], rtol=1e-3, atol=1e-4)
    finally:
        ref.close()
        bal.close()


def test_rebuilds_and_switches(amd, monkeypatch):
    """(d) rebuild_graph and an injected adjacency drop the order and derive it again for the new graph; OSC_REORDER=0 and
    OSC_BALANCE=0 leave the API order."""
    N, D, k, nb = SHAPES[0]
    Y, psi, _ = _inputs(N, D)
    ref, bal = _pair(amd, monkeypatch, N, D, k, nb)
    try:
        first = _row_order(bal)
        for lat, switch in ((ref, "0"), (bal, "1")):
            monkeypatch.setenv("OSC_BALANCE", switch)  # (a rebuild reads the build switches again)
            lat.rebuild_graph(kneighbors=20)
        info = bal.build_info()
        assert info["order_kind"] == "balanced" and ref.build_info()["order_kind"] == "none", info
        second = _row_order(bal)
        assert not np.array_equal(first, second)
        assert info["displaced_edges_after"] == _displaced(bal, second, nb)
        for x, y in zip(ref.graph_csr(), bal.graph_csr()):
            assert np.array_equal(x, y)
        sts = [lat.settle(**KW) for lat in (ref, bal)]
        assert sts[0]["iters"] == sts[1]["iters"] and relerr(bal.U, ref.U) < TOL
        rp, col, a = ref.graph_csr()[:3]
        rows = np.repeat(np.arange(N), np.diff(rp))
        keep = (rows + col) % 3 != 0  # a thinner graph, symmetric by construction
        rows = rows[keep]
        rp2 = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=N))]).astype(np.int64)
        for lat in (ref, bal):
            lat.set_graph_csr(rp2, col[keep], a[keep])
            lat.reset_U()
        # (the host reference on this graph, the oracle's k = 20 lists thinned the same way: 363 -> 150 displaced in 7 rounds)
        info = bal.build_info()
        assert info["order_kind"] == "balanced" and ref.build_info()["order_kind"] == "none", info
        assert info["balance_on_device"] == 1, info
        third = _row_order(bal)
        assert np.array_equal(np.sort(third), np.arange(N)) and not np.array_equal(third, np.arange(N))
        assert not np.array_equal(third, second)
        assert 0 < info["displaced_edges_before"] == _displaced(bal, np.arange(N), nb)
        assert info["displaced_edges_after"] == _displaced(bal, third, nb) < info["displaced_edges_before"], info
        for x, y in zip(ref.graph_csr(), bal.graph_csr()):
            assert np.array_equal(x, y)
        sts = [lat.settle(**KW) for lat in (ref, bal)]
        assert sts[0]["iters"] == sts[1]["iters"] and relerr(bal.U, ref.U) < TOL
    finally:
        ref.close()
        bal.close()
    for extra in ({"OSC_REORDER": "0", "OSC_BALANCE": "1"}, {"OSC_BALANCE": "0"}):
        _env(monkeypatch, nb, **extra)
        lat = amd.Oscillink(Y, kneighbors=k)
        try:
            assert lat.build_info()["order_kind"] == "none", extra
            assert np.array_equal(_row_order(lat), np.arange(N)), extra
        finally:
            lat.close()


def test_a_communicator_keeps_the_api_order(amd, monkeypatch):
    """(e) two loopback ranks under OSC_BALANCE=1: the order kind stays none, the sharded settle equals the one-process
    balanced handle's to rounding."""
    from oscillink_amd.sharding import run_loopback_ranks

    N, D, k, nb = 1203, 128, 12, 3
    Y, psi, _ = _inputs(N, D)
    _env(monkeypatch, nb, OSC_BALANCE="1")

    def rank_fn(rank, comm):
        lat = amd.Oscillink(Y, kneighbors=k, comm=comm)
        lat.set_query(psi)
        st = dict(lat.settle(**KW))
        return lat.build_info()["order_kind"], _row_order(lat), st, lat.U.copy()

    out = run_loopback_ranks(2, rank_fn)
    one = amd.Oscillink(Y, kneighbors=k)
    try:
        one.set_query(psi)
        st = one.settle(**KW)
        assert one.build_info()["order_kind"] == "balanced"
        for kind, perm, rst, U in out:
            assert kind == "none" and np.array_equal(perm, np.arange(N))
            assert rst["iters"] == st["iters"] and relerr(U, one.U) < TOL
    finally:
        one.close()

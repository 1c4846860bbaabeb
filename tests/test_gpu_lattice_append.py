"""OscillinkLattice.append: a lattice grown from its kept kNN lists answers like a lattice built from
the concatenated anchors.

The rule, for mode="incremental": per-row kNN lists equal as (id, value bits) sets, graph_csr() equal array by array, equal
settle iteration counts and residual history lengths, U within the route-parity tolerance 2e-5, equal state signature,
bundle ids and chain verdict, append_info()["route"] == 1.  Anchors come from default_rng(N0 + D + k)."""
import numpy as np
import pytest

from tests._fullsize import device_knn_lists
from tests._knn_reference import check_lists, lists_f64

pytestmark = pytest.mark.gpu


def _lat(Y, k, **kw):
    from oscillink_amd import OscillinkLattice

    return OscillinkLattice(Y, kneighbors=k, **kw)


def _anchors(N0, M, D, k):
    rng = np.random.default_rng(N0 + D + k)
    Y = rng.standard_normal((N0 + M, D)).astype(np.float32)
    return Y, rng.standard_normal(D).astype(np.float32)


def _sorted_lists(lat):
    idx, val = device_knn_lists(lat, lat.N, lat._kneighbors)
    order = np.argsort(idx, axis=1, kind="stable")  # in-row order is not part of the contract
    return np.take_along_axis(idx, order, axis=1), np.take_along_axis(val, order, axis=1).view(np.uint32)


def _assert_rule(app, fresh, psi, chain=None, route=1):
    assert app.N == fresh.N and app._kneighbors == fresh._kneighbors
    assert app.append_info()["route"] == route
    ia, va = _sorted_lists(app)
    jf, vf = _sorted_lists(fresh)
    rows = np.nonzero((ia != jf).any(axis=1) | (va != vf).any(axis=1))[0]
    assert rows.size == 0, ("kNN lists differ", rows[:8].tolist(), ia[rows[:2]].tolist(), jf[rows[:2]].tolist())
    for name, a, f in zip(("rowptr", "col", "A", "W", "sqrt_deg"), app.graph_csr(), fresh.graph_csr()):
        assert np.array_equal(a, f, equal_nan=True), name
    for lat in (app, fresh):
        lat.set_query(psi)
    sa, sf = app.settle(), fresh.settle()
    assert sa["iters"] == sf["iters"]
    assert len(app.residual_history()) == len(fresh.residual_history())
    Ua, Uf = app.U, fresh.U
    print("U byte-equal:", bool(np.array_equal(Ua, Uf, equal_nan=True)))
    np.testing.assert_allclose(Ua, Uf, rtol=0, atol=2e-5)
    assert app.receipt()["meta"]["state_sig"] == fresh.receipt()["meta"]["state_sig"]
    assert [b["id"] for b in app.bundle(k=6)] == [b["id"] for b in fresh.bundle(k=6)]
    chain = [0, 1, app.N - 1] if chain is None else chain
    assert app.chain_receipt(chain)["verdict"] == fresh.chain_receipt(chain)["verdict"]


# ---- mfma family: the dense route ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("N0", [1000, 1024])
@pytest.mark.parametrize("M", [1, 37, 200])
def test_dense_route_append_matches_a_fresh_build(N0, M):
    Y, psi = _anchors(N0, M, 64, 16)
    app = _lat(Y[:N0], 16)
    ids = app.append(Y[N0:], mode="incremental")
    assert ids.tolist() == list(range(N0, N0 + M))
    info = app.append_info()
    assert info["score_family"] == "mfma" and info["new_rows"] == M and info["merged_rows"] + info["redo_rows"] == N0
    _assert_rule(app, _lat(Y, 16), psi)


def test_two_appends_in_a_row_an_appended_handle_seeds_the_next():
    N0, D, k = 1000, 64, 16
    Y, psi = _anchors(N0, 237, D, k)
    app = _lat(Y[:N0], k)
    app.append(Y[N0:N0 + 37], mode="incremental")
    ids = app.append(Y[N0 + 37:], mode="incremental")
    assert ids[0] == N0 + 37 and ids[-1] == N0 + 236
    _assert_rule(app, _lat(Y, k), psi)


# ---- butterfly family ----------------------------------------------------------------------------------------------------
def test_butterfly_family_at_the_smallest_size(monkeypatch):
    monkeypatch.setenv("OSC_KNN_MODE", "prefilter")
    N0, M, D, k = 1000, 150, 64, 16
    Y, psi = _anchors(N0, M, D, k)
    app = _lat(Y[:N0], k)
    assert app.append_info()["score_family"] == "butterfly"
    app.append(Y[N0:], mode="incremental")
    fresh = _lat(Y, k)
    assert fresh.build_info()["fallback_rows"] == 0
    assert app.append_info()["score_family"] == "butterfly"
    _assert_rule(app, fresh, psi)


def test_default_planner_panel_route():
    N0, M, D, k = 20000, 300, 128, 16
    Y, psi = _anchors(N0, M, D, k)
    app = _lat(Y[:N0], k)
    assert app.build_info()["prefilter"] == 2
    app.append(Y[N0:], mode="incremental")
    fresh = _lat(Y, k)
    assert fresh.build_info()["prefilter"] == 2
    _assert_rule(app, fresh, psi)


def test_row_pitch_changes_with_the_row_count():
    N0, M, D, k = 8300, 200, 500, 16  # N D crosses 2^22: the row pitch goes 500 -> 512
    assert N0 * D < 2 ** 22 <= (N0 + M) * D
    Y, psi = _anchors(N0, M, D, k)
    app = _lat(Y[:N0], k)
    app.append(Y[N0:], mode="incremental")
    np.testing.assert_array_equal(app.Y, Y)
    _assert_rule(app, _lat(Y, k), psi)


def test_several_chunks_with_the_redo_set_across_a_chunk_edge(monkeypatch):
    """OSC_APPEND_SCRATCH_MB=1 leaves one 128-row tile per chunk at 1960 columns: 160 redo rows + 300 new rows are four
    chunks, the redo set ends inside the second, and every chunk's new columns are merged before the next is scored."""
    monkeypatch.setenv("OSC_APPEND_SCRATCH_MB", "1")
    D, k, M = 8, 120, 300
    rng = np.random.default_rng(1660 + D + k)
    main = rng.standard_normal((1800, D)).astype(np.float32)
    main[:, 0] = np.abs(main[:, 0]) + 3.0  # one half-space: every pair of them has a positive cosine
    lone = rng.standard_normal((100, D)).astype(np.float32)
    lone[:, 0] = -np.abs(lone[:, 0]) - 3.0  # 99 mates with a positive cosine < k: their k-th member is clipped
    Y = np.concatenate([main[:1500], lone, np.zeros((60, D), dtype=np.float32), main[1500:]])
    order = np.concatenate([rng.permutation(1660), 1660 + np.arange(M)])  # the redo rows scattered over the old rows
    Y = np.ascontiguousarray(Y[order])
    N0 = 1660
    app = _lat(Y[:N0], k)
    app.append(Y[N0:], mode="incremental")
    info = app.append_info()
    assert info["redo_rows"] == 160 and info["merged_rows"] == 1500 and info["merge_hits"] > 0
    _assert_rule(app, _lat(Y, k), rng.standard_normal(D).astype(np.float32))


# ---- ties ------------------------------------------------------------------------------------------------------------------
def test_a_copy_of_an_old_row_loses_every_tie_to_it():
    N0, D, k = 1000, 64, 16
    Y, psi = _anchors(N0, 1, D, k)
    Y[N0] = Y[5]
    app = _lat(Y[:N0], k)
    app.append(Y[N0:], mode="incremental")
    _assert_rule(app, _lat(Y, k), psi)
    idx, _ = device_knn_lists(app, N0 + 1, k)
    for r in range(N0):  # wherever the copy is a member, so is row 5 (equal score, smaller index)
        if r != 5 and N0 in idx[r]:
            assert 5 in idx[r]


def test_new_rows_that_are_near_copies_of_one_another():
    N0, D, k = 1000, 64, 16
    Y, psi = _anchors(N0, 8, D, k)
    rng = np.random.default_rng(3)
    centre = np.zeros(D, dtype=np.float32)
    centre[0] = 40.0  # far from the i.i.d. rows
    Y[:N0, 0] = -np.abs(Y[:N0, 0])
    Y[N0:] = centre + 1e-3 * rng.standard_normal((8, D)).astype(np.float32)
    app = _lat(Y[:N0], k)
    app.append(Y[N0:], mode="incremental")
    _assert_rule(app, _lat(Y, k), psi)
    idx, _ = device_knn_lists(app, N0 + 8, k)
    for r in range(N0, N0 + 8):  # the new x new block: each new row lists the seven others
        assert set(range(N0, N0 + 8)) - {r} <= set(idx[r].tolist())


def test_all_equal_anchors():
    Y = np.ones((320, 6), dtype=np.float32)
    psi = np.ones(6, dtype=np.float32)
    app = _lat(Y[:300], 5)
    app.append(Y[300:], mode="incremental")
    _assert_rule(app, _lat(Y, 5), psi)


# ---- redo set, non-finite rows --------------------------------------------------------------------------------------------
def test_rows_with_clipped_members_are_redone():
    N0, M, D, k = 40, 5, 2, 30  # the k-th cosines are negative and stored as 0
    Y, psi = _anchors(N0, M, D, k)
    app = _lat(Y[:N0], k)
    app.append(Y[N0:], mode="incremental")
    assert app.append_info()["redo_rows"] > 0
    _assert_rule(app, _lat(Y, k), psi)


def test_zero_nan_and_inf_rows_old_and_new():
    """The whole rule against the fresh build.  `_assert_rule` compares U with NaN == NaN (assert_allclose's default), so
    the non-finite part of the state must sit in the same places; most of the state must be finite, so that the comparison
    is one of numbers."""
    N0, M, D, k = 1000, 40, 64, 16
    Y, psi = _anchors(N0, M, D, k)
    for base in (100, N0 + 10):
        Y[base] = 0.0
        Y[base + 1, 3] = np.nan
        Y[base + 2, 7] = np.inf
    app = _lat(Y[:N0], k)
    app.append(Y[N0:], mode="incremental")
    assert app.append_info()["redo_rows"] >= 3
    fresh = _lat(Y, k)
    idx, _ = device_knn_lists(app, N0 + M, k)
    for r in (101, 102, N0 + 11, N0 + 12):  # a non-finite row has an empty list and stands in nobody's
        assert (idx[r] == -1).all() and not (idx == r).any()
    _assert_rule(app, fresh, psi, chain=[0, 1, 2])
    finite = np.isfinite(fresh.U)
    print("finite entries of U:", int(finite.sum()), "of", finite.size)
    assert np.array_equal(finite, np.isfinite(app.U))
    # (a non-finite row has no edge and every solve here is column-wise with per-row updates, so most of the state stays
    # finite -- 64 480 of 66 560 entries on an MI355X -- and the comparison above is over real numbers)
    assert finite.mean() > 0.9


# ---- planner fallbacks ----------------------------------------------------------------------------------------------------
def test_auto_mode_rebuilds_when_the_effective_k_changes():
    N0, M, D, k = 10, 12, 8, 16
    Y, psi = _anchors(N0, M, D, k)
    app = _lat(Y[:N0], k)
    assert app._kneighbors == 9
    app.append(Y[N0:])
    assert app._kneighbors == 16
    _assert_rule(app, _lat(Y, k), psi, route=2)


def test_auto_mode_rebuilds_on_the_device_when_the_new_rows_are_too_many():
    N0, M, D, k = 1000, 200, 64, 16  # M above N / 32: the planner expects the rebuild to be no slower
    Y, psi = _anchors(N0, M, D, k)
    app = _lat(Y[:N0], k)
    app.append(Y[N0:])
    info = app.append_info()
    assert info["route"] == 2 and info["denied"] == 8 and info["new_rows"] == M
    np.testing.assert_array_equal(app.Y, Y)  # (the old rows came device to device)
    _assert_rule(app, _lat(Y, k), psi, route=2)


def test_a_lattice_never_built_gets_a_graph_over_all_rows():
    N0, M, D, k = 300, 20, 16, 6
    Y, psi = _anchors(N0, M, D, k)
    lat = _lat(Y[:N0], k, _build_graph=False)
    with pytest.raises(NotImplementedError, match="no kNN lists"):
        lat.append(Y[N0:], mode="incremental")
    lat.append(Y[N0:])
    _assert_rule(lat, _lat(Y, k), psi, route=2)


def test_an_injected_graph_cannot_grow():
    Y, _ = _anchors(50, 3, 8, 4)
    lat = _lat(Y[:50], 4)
    rowptr, col, a, _, _ = lat.graph_csr()
    lat.set_graph_csr(rowptr, col, a)
    with pytest.raises(NotImplementedError, match="no kNN lists"):
        lat.append(Y[50:])
    assert lat.N == 50


def test_forced_incremental_on_an_ineligible_lattice_raises_and_changes_nothing():
    N0, M, D, k = 10, 12, 8, 16
    Y, psi = _anchors(N0, M, D, k)
    lat, twin = _lat(Y[:N0], k), _lat(Y[:N0], k)
    before = [x.copy() for x in lat.graph_csr()]
    with pytest.raises(NotImplementedError, match="effective k"):
        lat.append(Y[N0:], mode="incremental")
    assert lat.N == N0 and lat.append_info()["route"] == 0
    for a, b in zip(lat.graph_csr(), before):
        assert np.array_equal(a, b)
    for x in (lat, twin):
        x.set_query(psi)
    assert lat.settle()["iters"] == twin.settle()["iters"]
    assert np.array_equal(lat.U, twin.U)


def test_wrong_width_raises_and_an_empty_append_is_a_no_op():
    Y, psi = _anchors(200, 4, 16, 6)
    lat = _lat(Y[:200], 6)
    version = lat._state_version
    with pytest.raises(ValueError):
        lat.append(np.zeros((3, 15), dtype=np.float32))
    with pytest.raises(ValueError):
        lat.append(np.zeros(16, dtype=np.float32))
    with pytest.raises(ValueError):
        lat.append(Y[200:], gates=np.ones(3, dtype=np.float32))
    ids = lat.append(np.zeros((0, 16), dtype=np.float32))
    assert ids.shape == (0,) and lat.N == 200 and lat._state_version == version and lat.append_info()["route"] == 0
    _assert_rule(lat, _lat(Y[:200], 6), psi, route=0)


# ---- carried state ---------------------------------------------------------------------------------------------------------
def test_settings_survive_and_the_query_basis_is_invalidated():
    N0, M, D, k = 1000, 60, 64, 16
    Y, psi = _anchors(N0, M, D, k)
    rng = np.random.default_rng(11)
    gates_old = rng.uniform(0.2, 1.0, N0).astype(np.float32)
    gates_new = rng.uniform(0.2, 1.0, M).astype(np.float32)
    chain, psis = [3, 17, 250, 999], rng.standard_normal((5, D)).astype(np.float32)
    events = []

    def dress(lat, gates):
        lat.lamC, lat.lamQ = 0.7, 3.0
        lat.set_query(psi, gates)
        lat.add_chain(chain, lamP=0.3, weights=[1.0, 0.5, 2.0])
        lat.set_receipt_secret(b"secret")

    app = _lat(Y[:N0], k)
    dress(app, gates_old)
    app.set_logger(lambda ev, payload: events.append(ev))
    app.bundle_many(psis, k=5)  # a query basis of the OLD lattice is cached now
    app.append(Y[N0:], gates_new, mode="incremental")
    assert "append" in events
    fresh = _lat(Y, k)
    dress(fresh, np.concatenate([gates_old, gates_new]))
    np.testing.assert_array_equal(app.B_diag, fresh.B_diag)
    assert app.lamP == fresh.lamP == 0.3 and app.verify_current_receipt(b"secret")
    # psi on the NEW handle is the one re-applied by append (nothing has called set_query since)
    np.testing.assert_array_equal(app.psi, psi)
    assert app.bundle(k=6) == fresh.bundle(k=6)
    assert app.receipt()["meta"]["state_sig"] == fresh.receipt()["meta"]["state_sig"]
    assert app.receipt()["deltaH_total"] == fresh.receipt()["deltaH_total"]
    ba, bf = app.bundle_many(psis, k=5, as_arrays=True), fresh.bundle_many(psis, k=5, as_arrays=True)
    for a, f in zip(ba, bf):  # ids, score, align
        np.testing.assert_array_equal(a, f)
    ra, rf = app.receipt_many(psis, as_arrays=True), fresh.receipt_many(psis, as_arrays=True)
    assert set(ra) == set(rf)
    for name in ra:
        np.testing.assert_array_equal(ra[name], rf[name], err_msg=name)
    _assert_rule(app, fresh, psi, chain=chain)


# ---- across families -------------------------------------------------------------------------------------------------------
def test_mfma_lists_kept_where_a_fresh_build_would_take_the_panel_route():
    N0, M, D, k = 8100, 200, 64, 16
    Y, _ = _anchors(N0, M, D, k)
    app = _lat(Y[:N0], k)
    assert app.build_info()["prefilter"] == 0 and app.append_info()["score_family"] == "mfma"
    app.append(Y[N0:], mode="incremental")
    info = app.append_info()
    assert info["route"] == 1 and info["score_family"] == "mfma"
    fresh = _lat(Y, k)
    assert fresh.build_info()["prefilter"] == 2 and fresh.append_info()["score_family"] == "butterfly"
    ref = lists_f64(Y, k)
    idx, val = device_knn_lists(app, N0 + M, k)
    differing = check_lists(Y, idx, val, k, gap_tol=1e-6, ref=ref)
    print("rows whose member sets differ from the float64 yardstick:", differing)
    (rp_a, col_a, *_), (rp_f, col_f, *_) = app.graph_csr(), fresh.graph_csr()
    clear = np.nonzero(ref[2] >= 1e-6)[0]
    bad = [int(r) for r in clear if set(col_a[rp_a[r]:rp_a[r + 1]].tolist()) != set(col_f[rp_f[r]:rp_f[r + 1]].tolist())]
    assert not bad, bad[:8]

"""OscillinkLattice.update: a lattice with rows replaced in place answers like a lattice built from
the changed anchors.

The rule, for mode="incremental" against fresh = OscillinkLattice(Y2, same settings) with Y2 = Y.copy(); Y2[ids] = Ynew:
update_info()["route"] == 1, per-row kNN lists equal as (id, value bits) sets, graph_csr() equal array by array, equal settle
iteration counts and residual history lengths, U within the route-parity tolerance 2e-5, equal state signature, bundle ids and
chain verdict, lat.Y array-equal to Y2, the returned ids equal to the given ones as int64.  Anchors come from
default_rng(N0 + D + k), ids and new rows from the same generator."""
import numpy as np
import pytest

from tests._fullsize import device_knn_lists

pytestmark = pytest.mark.gpu


def _lat(Y, k, **kw):
    from oscillink_amd import OscillinkLattice

    return OscillinkLattice(Y, kneighbors=k, **kw)


def _anchors(N0, M, D, k):
    """Anchors, a query, M distinct ids and M new rows, all from one generator."""
    rng = np.random.default_rng(N0 + D + k)
    Y = rng.standard_normal((N0, D)).astype(np.float32)
    psi = rng.standard_normal(D).astype(np.float32)
    ids = rng.choice(N0, size=M, replace=False)
    return Y, psi, ids, rng.standard_normal((M, D)).astype(np.float32)


def _changed(Y, ids, Ynew):
    Y2 = Y.copy()
    Y2[np.asarray(ids, dtype=np.int64)] = Ynew
    return Y2


def _sorted_lists(lat):
    idx, val = device_knn_lists(lat, lat.N, lat._kneighbors)
    order = np.argsort(idx, axis=1, kind="stable")  # in-row order is not part of the contract
    return np.take_along_axis(idx, order, axis=1), np.take_along_axis(val, order, axis=1).view(np.uint32)


def _rows_naming(lat, ids):
    """Rows of a built lattice, other than `ids` themselves, whose list names one of `ids`."""
    idx, _ = device_knn_lists(lat, lat.N, lat._kneighbors)
    hit = np.isin(idx, np.asarray(ids)).any(axis=1)
    hit[np.asarray(ids)] = False
    return int(hit.sum())


def _assert_rule(upd, fresh, psi, chain=None, route=1):
    assert upd.N == fresh.N and upd._kneighbors == fresh._kneighbors
    assert upd.update_info()["route"] == route
    ia, va = _sorted_lists(upd)
    jf, vf = _sorted_lists(fresh)
    rows = np.nonzero((ia != jf).any(axis=1) | (va != vf).any(axis=1))[0]
    assert rows.size == 0, ("kNN lists differ", rows[:8].tolist(), ia[rows[:2]].tolist(), jf[rows[:2]].tolist())
    for name, a, f in zip(("rowptr", "col", "A", "W", "sqrt_deg"), upd.graph_csr(), fresh.graph_csr()):
        assert np.array_equal(a, f, equal_nan=True), name
    for lat in (upd, fresh):
        lat.set_query(psi)
    sa, sf = upd.settle(), fresh.settle()
    assert sa["iters"] == sf["iters"]
    assert len(upd.residual_history()) == len(fresh.residual_history())
    Ua, Uf = upd.U, fresh.U
    print("U byte-equal:", bool(np.array_equal(Ua, Uf, equal_nan=True)))
    np.testing.assert_allclose(Ua, Uf, rtol=0, atol=2e-5, equal_nan=True)
    assert upd.receipt()["meta"]["state_sig"] == fresh.receipt()["meta"]["state_sig"]
    assert [b["id"] for b in upd.bundle(k=6)] == [b["id"] for b in fresh.bundle(k=6)]
    chain = [0, 1, upd.N - 1] if chain is None else chain
    assert upd.chain_receipt(chain)["verdict"] == fresh.chain_receipt(chain)["verdict"]


def _update_and_check(Y, psi, ids, Ynew, k, mode="incremental", route=1, dense=False):
    """Replaces rows `ids` of a lattice over Y and holds it to the fresh build of the changed anchors; returns the lattice."""
    lat = _lat(Y, k)
    N0, k_eff = lat.N, lat._kneighbors
    naming = _rows_naming(lat, ids)
    out = lat.update(ids, Ynew, mode=mode)
    Y2 = _changed(Y, ids, Ynew)
    assert out.dtype == np.int64 and np.array_equal(out, np.asarray(ids, dtype=np.int64))
    assert lat.N == N0 and lat._kneighbors == k_eff
    assert np.array_equal(lat.Y, Y2, equal_nan=True)
    info = lat.update_info()
    assert info["replaced_rows"] == len(ids)
    if route == 1:
        assert info["merged_rows"] + info["redo_rows"] + info["replaced_rows"] == N0
        print("redo rows:", info["redo_rows"], "rows naming a replaced id:", naming, "merge hits:", info["merge_hits"])
        if dense:
            assert info["redo_rows"] >= naming
    _assert_rule(lat, _lat(Y2, k), psi, route=route)
    return lat


# ---- mfma family: the dense route ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("N0", [1000, 1024])
@pytest.mark.parametrize("M", [1, 37, 200])
def test_dense_route_update_matches_a_fresh_build(N0, M):
    Y, psi, ids, Ynew = _anchors(N0, M, 64, 16)
    lat = _update_and_check(Y, psi, ids, Ynew, 16, dense=True)
    assert lat.update_info()["score_family"] == "mfma"


@pytest.mark.parametrize("ids", [[0], [999], list(range(120, 136)), [900, 5, 17, 3, 640, 128, 127]],
                         ids=["first", "last", "across_a_tile_edge", "unsorted"])
def test_shaped_id_sets(ids):
    Y, psi, _, _ = _anchors(1000, 1, 64, 16)
    Ynew = np.random.default_rng(len(ids)).standard_normal((len(ids), 64)).astype(np.float32)
    _update_and_check(Y, psi, ids, Ynew, 16, dense=True)


# ---- ties: a replaced column's index may lie below a member's ------------------------------------------------------------
def _all_v_but_one(odd):
    """320 x 64: every row is one vector v, except row `odd`, whose cosine to v is about 0.5."""
    rng = np.random.default_rng(320 + 64 + 16)
    v = rng.standard_normal(64).astype(np.float32)
    u = rng.standard_normal(64)
    u -= (u @ v) / (v @ v) * v
    other = (0.5 * v / np.linalg.norm(v) + np.sqrt(0.75) * u / np.linalg.norm(u)).astype(np.float32)
    Y = np.tile(v, (320, 1))
    Y[odd] = other
    cos = float(other @ v / (np.linalg.norm(other) * np.linalg.norm(v)))
    assert abs(cos - 0.5) < 1e-3
    return Y, v, rng.standard_normal(64).astype(np.float32)


def test_equal_score_lower_index_wins():
    """Row 2 stands in no list.  As a copy of v its score equals every member's bit for bit and its index is below the
    highest-index member's, which it must evict in every other row: the tie an appended column always loses."""
    Y, v, psi = _all_v_but_one(2)
    k = 16
    lat = _lat(Y, k)
    idx, val = device_knn_lists(lat, 320, k)
    assert not (np.delete(idx, 2, axis=0) == 2).any()
    assert np.unique(np.delete(val, 2, axis=0).view(np.uint32)).size == 1  # one score, bit for bit
    lat.update([2], v[None, :], mode="incremental")
    info = lat.update_info()
    print("merge hits:", info["merge_hits"], "redo rows:", info["redo_rows"])
    assert info["route"] == 1 and info["redo_rows"] == 0 and info["merge_hits"] == 319
    after, _ = device_knn_lists(lat, 320, k)
    for i in range(320):
        if i == 2:
            continue
        evicted = max(idx[i].tolist())
        assert set(after[i].tolist()) == (set(idx[i].tolist()) - {evicted}) | {2}, i
    _assert_rule(lat, _lat(_changed(Y, [2], v[None, :]), k), psi)


def test_equal_score_higher_index_loses():
    Y, v, psi = _all_v_but_one(300)
    k = 16
    lat = _lat(Y, k)
    idx, val = device_knn_lists(lat, 320, k)
    assert not (np.delete(idx, 300, axis=0) == 300).any()
    lat.update([300], v[None, :], mode="incremental")
    info = lat.update_info()
    assert info["route"] == 1 and info["redo_rows"] == 0 and info["merge_hits"] == 0
    after, after_val = device_knn_lists(lat, 320, k)
    keep = np.arange(320) != 300
    assert np.array_equal(np.sort(after[keep], axis=1), np.sort(idx[keep], axis=1))  # nothing but row 300's own list changes
    assert np.array_equal(after_val[keep].view(np.uint32), val[keep].view(np.uint32))
    assert set(after[300].tolist()) == set(range(16))
    _assert_rule(lat, _lat(_changed(Y, [300], v[None, :]), k), psi)


def test_copy_of_a_listed_row_enters_below_it():
    N0, D, k = 1000, 64, 16
    Y, psi, _, _ = _anchors(N0, 1, D, k)
    lat = _lat(Y, k)
    idx, val = device_knn_lists(lat, N0, k)
    found = None
    for i in range(150, N0):
        worst_v = val[i].min()
        w = int(idx[i][val[i] == worst_v].max())  # lowest value, highest index among equal values
        if w > 3 and 3 not in idx[i]:
            found = (i, w)
            break
    assert found is not None
    i, w = found
    Ynew = Y[w][None, :].copy()
    lat.update([3], Ynew, mode="incremental")
    info = lat.update_info()
    assert info["route"] == 1 and info["merge_hits"] > 0
    after, after_val = device_knn_lists(lat, N0, k)
    # score(i, 3) == score(i, w) bit for bit and 3 < w: 3 enters row i's list and evicts w
    assert 3 in after[i] and w not in after[i]
    assert after_val[i][after[i] == 3].view(np.uint32)[0] == val[i][idx[i] == w].view(np.uint32)[0]
    _assert_rule(lat, _lat(_changed(Y, [3], Ynew), k), psi)


def test_eight_near_copies_among_the_replaced_rows():
    N0, D, k = 1000, 64, 16
    Y, psi, _, _ = _anchors(N0, 1, D, k)
    rng = np.random.default_rng(3)
    centre = np.zeros(D, dtype=np.float32)
    centre[0] = 40.0  # far from the i.i.d. rows
    Y[:, 0] = -np.abs(Y[:, 0])
    copies = [100, 7, 640, 641, 999, 128, 127, 333]
    ids = copies + [5, 500, 870]
    Ynew = rng.standard_normal((len(ids), D)).astype(np.float32)
    Ynew[:, 0] = -np.abs(Ynew[:, 0])
    Ynew[:8] = centre + 1e-3 * rng.standard_normal((8, D)).astype(np.float32)
    lat = _update_and_check(Y, psi, ids, Ynew, k, dense=True)
    idx, _ = device_knn_lists(lat, N0, k)
    for r in copies:  # each of the eight lists the seven others
        assert set(copies) - {r} <= set(idx[r].tolist())


@pytest.mark.parametrize("ids", [[3, 150], [150, 319]], ids=["a_listed_and_an_unlisted_row", "rows_in_no_list"])
def test_all_equal_anchors(ids):
    """Every list is the five lowest other ids, every score one value.  Row 3 stands in every list, so every row is redone;
    rows 150 and 319 stand in none, and as replaced columns they tie with every worst member at a higher index: no hit."""
    Y = np.ones((320, 6), dtype=np.float32)
    lat = _update_and_check(Y, np.ones(6, dtype=np.float32), ids, np.ones((2, 6), dtype=np.float32), 5, dense=True)
    if ids == [150, 319]:
        info = lat.update_info()
        assert info["redo_rows"] == 0 and info["merge_hits"] == 0


# ---- redo set, non-finite rows --------------------------------------------------------------------------------------------
def test_rows_with_clipped_members():
    N0, M, D, k = 40, 3, 2, 30  # the k-th cosines are negative and stored as 0
    Y, psi, ids, Ynew = _anchors(N0, M, D, k)
    lat = _update_and_check(Y, psi, ids, Ynew, k, dense=True)
    assert lat.update_info()["redo_rows"] > 0


def test_zero_nan_and_inf_rows_old_and_new():
    """Such rows among the old rows (100..102 stay), among the new rows (500..502 get them), a NaN row replaced by a finite
    one (201) and a finite row replaced by a NaN one (501).  `_assert_rule` compares U with NaN == NaN, so the non-finite part
    of the state must sit in the same places; most of the state must be finite, so that the comparison is one of numbers."""
    N0, M, D, k = 1000, 40, 64, 16
    Y, psi, ids, Ynew = _anchors(N0, M, D, k)
    ids = np.setdiff1d(ids, [100, 101, 102, 200, 201, 202, 500, 501, 502])[:30]
    ids = np.concatenate([ids, [500, 501, 502, 200, 201, 202]])
    Ynew = Ynew[:ids.size].copy()
    for base in (100, 200):
        Y[base] = 0.0
        Y[base + 1, 3] = np.nan
        Y[base + 2, 7] = np.inf
    at = {int(r): j for j, r in enumerate(ids)}
    Ynew[at[500]] = 0.0
    Ynew[at[501], 5] = np.nan
    Ynew[at[502], 9] = -np.inf
    assert np.isfinite(Ynew[[at[200], at[201], at[202]]]).all()
    lat = _lat(Y, k)
    lat.update(ids, Ynew, mode="incremental")
    Y2 = _changed(Y, ids, Ynew)
    assert np.array_equal(lat.Y, Y2, equal_nan=True)
    fresh = _lat(Y2, k)
    idx, _ = device_knn_lists(lat, N0, k)
    for r in (101, 102, 501, 502):  # a non-finite row has an empty list and stands in nobody's
        assert (idx[r] == -1).all() and not (idx == r).any()
    for r in (201, 202):  # finite now: a list of its own
        assert (idx[r] >= 0).all()
    _assert_rule(lat, fresh, psi, chain=[0, 1, 2])
    finite = np.isfinite(fresh.U)
    print("finite entries of U:", int(finite.sum()), "of", finite.size)
    assert np.array_equal(finite, np.isfinite(lat.U))
    assert finite.mean() > 0.9


# ---- chunks ----------------------------------------------------------------------------------------------------------------
def test_several_chunks_with_the_replaced_rows_starting_inside_one(monkeypatch):
    """OSC_APPEND_SCRATCH_MB=1 leaves one 128-row tile per chunk at 2000 columns; with k = 120 most rows name one of the 20
    replaced ones, so the chunk loop runs many times, and the replaced rows' part of the query list starts where the redo
    rows end: inside a chunk unless their number is a multiple of 128."""
    monkeypatch.setenv("OSC_APPEND_SCRATCH_MB", "1")
    N0, M, D, k = 2000, 20, 8, 120
    Y, psi, ids, Ynew = _anchors(N0, M, D, k)
    lat = _update_and_check(Y, psi, ids, Ynew, k, dense=True)
    info = lat.update_info()
    assert info["redo_rows"] > 128 and info["redo_rows"] % 128 != 0 and info["merged_rows"] > 0


# ---- butterfly family ----------------------------------------------------------------------------------------------------
def test_butterfly_family_at_the_smallest_size(monkeypatch):
    monkeypatch.setenv("OSC_KNN_MODE", "prefilter")
    N0, M, D, k = 1000, 50, 64, 16
    Y, psi, ids, Ynew = _anchors(N0, M, D, k)
    lat = _lat(Y, k)
    assert lat.append_info()["score_family"] == "butterfly"
    lat.update(ids, Ynew, mode="incremental")
    fresh = _lat(_changed(Y, ids, Ynew), k)
    assert fresh.build_info()["fallback_rows"] <= 32  # (its lists are butterfly-scored throughout)
    assert lat.update_info()["score_family"] == "butterfly"
    _assert_rule(lat, fresh, psi)


def test_default_planner_panel_route():
    N0, M, D, k = 20000, 30, 128, 16
    Y, psi, ids, Ynew = _anchors(N0, M, D, k)
    lat = _lat(Y, k)
    assert lat.build_info()["prefilter"] == 2
    lat.update(ids, Ynew, mode="incremental")
    info = lat.update_info()
    assert info["score_family"] == "butterfly" and info["replaced_rows"] == M
    fresh = _lat(_changed(Y, ids, Ynew), k)
    assert fresh.build_info()["prefilter"] == 2
    _assert_rule(lat, fresh, psi)


# ---- compositions on the dense route ---------------------------------------------------------------------------------------
def test_two_updates_in_a_row_an_updated_handle_seeds_the_next():
    N0, D, k = 1000, 64, 16
    Y, psi, ids, Ynew = _anchors(N0, 37, D, k)
    rng = np.random.default_rng(5)
    second = np.concatenate([ids[:5], rng.choice(np.setdiff1d(np.arange(N0), ids), size=18, replace=False)])
    Ysecond = rng.standard_normal((second.size, D)).astype(np.float32)
    lat = _lat(Y, k)
    lat.update(ids, Ynew, mode="incremental")
    lat.update(second, Ysecond, mode="incremental")
    _assert_rule(lat, _lat(_changed(_changed(Y, ids, Ynew), second, Ysecond), k), psi)


def test_append_then_update():
    N0, D, k = 1000, 64, 16
    Y, psi, _, _ = _anchors(N0, 1, D, k)
    rng = np.random.default_rng(6)
    Yapp = rng.standard_normal((20, D)).astype(np.float32)
    ids = np.array([N0 + 19, 3, 500, N0 + 4])  # old rows and appended ones
    Ynew = rng.standard_normal((ids.size, D)).astype(np.float32)
    lat = _lat(Y, k)
    lat.append(Yapp, mode="incremental")
    lat.update(ids, Ynew, mode="incremental")
    assert lat.append_info()["route"] == 0
    _assert_rule(lat, _lat(_changed(np.concatenate([Y, Yapp]), ids, Ynew), k), psi)


def test_remove_then_update():
    N0, D, k = 1000, 64, 16
    Y, psi, gone, _ = _anchors(N0, 37, D, k)
    rng = np.random.default_rng(7)
    ids = rng.choice(N0 - 37, size=12, replace=False)
    Ynew = rng.standard_normal((ids.size, D)).astype(np.float32)
    lat = _lat(Y, k)
    lat.remove(gone, mode="incremental")
    lat.update(ids, Ynew, mode="incremental")
    assert lat.remove_info()["route"] == 0
    _assert_rule(lat, _lat(_changed(np.delete(Y, gone, axis=0), ids, Ynew), k), psi)


def test_update_then_append():
    N0, D, k = 1000, 64, 16
    Y, psi, ids, Ynew = _anchors(N0, 37, D, k)
    Yapp = np.random.default_rng(8).standard_normal((20, D)).astype(np.float32)
    lat = _lat(Y, k)
    lat.update(ids, Ynew, mode="incremental")
    lat.append(Yapp, mode="incremental")
    assert lat.append_info()["route"] == 1
    _assert_rule(lat, _lat(np.concatenate([_changed(Y, ids, Ynew), Yapp]), k), psi, route=0)  # (the handle came from append)


def test_update_then_remove():
    N0, D, k = 1000, 64, 16
    Y, psi, ids, Ynew = _anchors(N0, 37, D, k)
    gone = np.concatenate([ids[:4], [0, 998]])  # replaced rows and others
    lat = _lat(Y, k)
    lat.update(ids, Ynew, mode="incremental")
    lat.remove(gone, mode="incremental")
    assert lat.remove_info()["route"] == 1
    _assert_rule(lat, _lat(np.delete(_changed(Y, ids, Ynew), gone, axis=0), k), psi, route=0)


# ---- planner and errors ---------------------------------------------------------------------------------------------------
def test_auto_mode_takes_the_incremental_route_for_one_row():
    Y, psi, ids, Ynew = _anchors(1000, 1, 64, 16)
    _update_and_check(Y, psi, ids, Ynew, 16, mode="auto", route=1, dense=True)


def test_auto_mode_rebuilds_on_the_device_when_the_query_rows_are_too_many():
    N0, D, k = 1000, 64, 16
    Y, psi, ids, Ynew = _anchors(N0, N0 // 4, D, k)
    lat = _update_and_check(Y, psi, ids, Ynew, k, mode="auto", route=2)
    assert lat.update_info()["denied"] == 8


def test_mode_rebuild():
    Y, psi, ids, Ynew = _anchors(1000, 1, 64, 16)
    lat = _update_and_check(Y, psi, ids, Ynew, 16, mode="rebuild", route=2)
    assert lat.update_info()["denied"] == 0


def test_a_lattice_never_built_gets_a_graph_over_the_changed_rows():
    N0, M, D, k = 300, 20, 16, 6
    Y, psi, ids, Ynew = _anchors(N0, M, D, k)
    lat = _lat(Y, k, _build_graph=False)
    with pytest.raises(NotImplementedError, match="no kNN lists"):
        lat.update(ids, Ynew, mode="incremental")
    assert lat.update_info()["route"] == 0
    lat.update(ids, Ynew)
    _assert_rule(lat, _lat(_changed(Y, ids, Ynew), k), psi, route=2)


@pytest.mark.parametrize("mode", ["auto", "incremental", "rebuild"])
def test_an_injected_graph_cannot_be_updated(mode):
    Y, _, ids, Ynew = _anchors(50, 3, 8, 4)
    lat = _lat(Y, 4)
    rowptr, col, a, _, _ = lat.graph_csr()
    lat.set_graph_csr(rowptr, col, a)
    with pytest.raises(NotImplementedError, match="no kNN lists"):
        lat.update(ids, Ynew, mode=mode)
    assert lat.N == 50 and np.array_equal(lat.Y, Y)


def test_bad_arguments_raise_and_change_nothing():
    from oscillink_amd import _native as nat

    N0, D, k = 200, 16, 6
    Y, psi, _, _ = _anchors(N0, 1, D, k)
    rows = np.random.default_rng(9).standard_normal((2, D)).astype(np.float32)
    lat, twin = _lat(Y, k), _lat(Y, k)
    for x in (lat, twin):
        x.add_chain([3, 17, 150], lamP=0.3)
    before = [x.copy() for x in lat.graph_csr()]
    version = lat._state_version
    with pytest.raises(ValueError, match="mode"):
        lat.update([1, 2], rows, mode="fast")
    with pytest.raises(ValueError, match="integers"):
        lat.update(np.array([1.0, 2.0]), rows)
    with pytest.raises(ValueError, match="out of bounds"):
        lat.update([0, N0], rows)
    with pytest.raises(ValueError, match="out of bounds"):
        lat.update([-1, 0], rows)
    with pytest.raises(ValueError, match="twice"):
        lat.update([5, 5], rows)
    with pytest.raises(ValueError, match="2D"):
        lat.update([1], rows[0])
    with pytest.raises(ValueError, match="column count"):
        lat.update([1, 2], rows[:, :D - 1])
    with pytest.raises(ValueError, match="length mismatch"):
        lat.update([1, 2, 3], rows)
    with pytest.raises(ValueError, match="gates length"):
        lat.update([1, 2], rows, gates=np.ones(3, dtype=np.float32))
    lat._has_comm = True
    try:
        with pytest.raises(nat.NativeError, match="communicator"):
            lat.update([1, 2], rows)
    finally:
        lat._has_comm = False
    assert lat.N == N0 and lat._state_version == version and lat.update_info()["route"] == 0
    assert np.array_equal(lat.Y, Y)
    for a, b in zip(lat.graph_csr(), before):
        assert np.array_equal(a, b)
    for x in (lat, twin):
        x.set_query(psi)
    assert lat.settle()["iters"] == twin.settle()["iters"]
    assert np.array_equal(lat.U, twin.U)


def test_empty_ids_is_a_no_op():
    Y, psi, _, _ = _anchors(200, 1, 16, 6)
    lat = _lat(Y, 6)
    version = lat._state_version
    for ids in ([], np.empty(0, dtype=np.int32)):
        out = lat.update(ids, np.empty((0, 16), dtype=np.float32))
        assert out.dtype == np.int64 and out.size == 0
    assert lat.N == 200 and lat._state_version == version
    _assert_rule(lat, _lat(Y, 6), psi, route=0)


# ---- carried state ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_gates", [False, True], ids=["gates_kept", "gates_given"])
def test_settings_survive_and_the_query_basis_is_invalidated(with_gates):
    N0, M, D, k = 1000, 60, 64, 16
    Y, psi, ids, Ynew = _anchors(N0, M, D, k)
    rng = np.random.default_rng(11)
    gates = rng.uniform(0.2, 1.0, N0).astype(np.float32)
    g_new = rng.uniform(0.2, 1.0, M).astype(np.float32) if with_gates else None
    gates2 = gates.copy()
    if with_gates:
        gates2[ids] = g_new
    others = np.setdiff1d(np.arange(N0), ids)
    chain = [int(others[3]), int(ids[0]), int(others[250]), int(ids[7])]  # through two replaced nodes
    psis = rng.standard_normal((5, D)).astype(np.float32)
    events = []

    def dress(lat, gates):
        lat.lamC, lat.lamQ = 0.7, 3.0
        lat.set_query(psi, gates)
        lat.add_chain(chain, lamP=0.3, weights=[1.0, 0.5, 2.0])
        lat.set_receipt_secret(b"secret")

    lat = _lat(Y, k)
    dress(lat, gates)
    lat.set_logger(lambda ev, payload: events.append((ev, payload)))
    lat.bundle_many(psis, k=5)  # a query basis of the OLD lattice is cached now
    lat.update(ids, Ynew, g_new, mode="incremental")
    logged = [p for ev, p in events if ev == "update"]
    assert len(logged) == 1 and logged[0]["rows"] == M and logged[0]["N"] == N0 and logged[0]["route"] == 1
    fresh = _lat(_changed(Y, ids, Ynew), k)
    dress(fresh, gates2)
    np.testing.assert_array_equal(lat.B_diag, fresh.B_diag)
    np.testing.assert_array_equal(lat.B_diag, gates2)
    assert lat.lamP == fresh.lamP == 0.3 and lat.verify_current_receipt(b"secret")
    assert lat._chain_nodes == chain
    np.testing.assert_array_equal(lat.psi, psi)  # psi on the NEW handle is the one re-applied by update
    assert lat.bundle(k=6) == fresh.bundle(k=6)
    assert lat.receipt()["meta"]["state_sig"] == fresh.receipt()["meta"]["state_sig"]
    assert lat.receipt()["deltaH_total"] == fresh.receipt()["deltaH_total"]
    ba, bf = lat.bundle_many(psis, k=5, as_arrays=True), fresh.bundle_many(psis, k=5, as_arrays=True)
    for a, f in zip(ba, bf):  # ids, score, align
        np.testing.assert_array_equal(a, f)
    ra, rf = lat.receipt_many(psis, as_arrays=True), fresh.receipt_many(psis, as_arrays=True)
    assert set(ra) == set(rf)
    for name in ra:
        np.testing.assert_array_equal(ra[name], rf[name], err_msg=name)
    _assert_rule(lat, fresh, psi, chain=chain)

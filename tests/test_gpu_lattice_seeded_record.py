"""append, remove and update share one seeded kNN build and one record of how a handle came to be.
What that sharing could break: each of append_info() / remove_info() / update_info() reports its own operation and zeros for
the other two; a refused call leaves all three as they were; `denied` lands under the operation that was denied; and an
append's merge gets the first column id of a chunk's fresh part right where the new rows start inside a chunk.

Shapes: 320 x 16, k 6 (dense route, mfma family) and 1000 x 64, k 16 under OSC_KNN_MODE=prefilter, the smallest butterfly
lattice of the append, remove and update tests."""
import numpy as np
import pytest

from tests._fullsize import device_knn_lists

pytestmark = pytest.mark.gpu

SHAPES = [pytest.param(320, 16, 6, None, "mfma", id="mfma"), pytest.param(1000, 64, 16, "prefilter", "butterfly", id="butterfly")]


def _lat(Y, k):
    from oscillink_amd import OscillinkLattice

    return OscillinkLattice(Y, kneighbors=k)


def _infos(lat):
    return {"append": lat.append_info(), "remove": lat.remove_info(), "update": lat.update_info()}


def _assert_only(lat, op, family):
    """`op`'s record says route 1, the other two say nothing happened: route 0, every count and every time zero."""
    infos = _infos(lat)
    for name, info in infos.items():
        assert info["score_family"] == family, name  # (the lists' family is the handle's, whoever asks)
        if name == op:
            assert info["route"] == 1 and info["denied"] == 0, (name, info)
        else:
            assert all(v == 0 for key, v in info.items() if key != "score_family"), (name, info)
    return infos[op]


@pytest.mark.parametrize("N,D,k,knn_mode,family", SHAPES)
def test_each_operation_reports_under_its_own_name_only(monkeypatch, N, D, k, knn_mode, family):
    if knn_mode:
        monkeypatch.setenv("OSC_KNN_MODE", knn_mode)
    rng = np.random.default_rng(N + D + k)
    Y = rng.standard_normal((N + 5, D)).astype(np.float32)
    lat = _lat(Y[:N], k)
    for name, info in _infos(lat).items():  # a created lattice: made by none of the three
        assert all(v == 0 for key, v in info.items() if key != "score_family"), (name, info)
    lat.append(Y[N:], mode="incremental")
    info = _assert_only(lat, "append", family)
    assert info["new_rows"] == 5 and info["merged_rows"] + info["redo_rows"] == N
    lat.remove([3, N + 1, 17], mode="incremental")
    info = _assert_only(lat, "remove", family)
    assert info["removed_rows"] == 3 and info["kept_rows"] + info["redo_rows"] == N + 2
    lat.update([0, N + 1, 9, 40], rng.standard_normal((4, D)).astype(np.float32), mode="incremental")
    info = _assert_only(lat, "update", family)
    assert info["replaced_rows"] == 4 and info["merged_rows"] + info["redo_rows"] + info["replaced_rows"] == N + 2


@pytest.mark.parametrize("N,D,k,knn_mode,family", SHAPES)
def test_a_refused_forced_call_leaves_all_three_records(monkeypatch, N, D, k, knn_mode, family):
    if knn_mode:
        monkeypatch.setenv("OSC_KNN_MODE", knn_mode)
    rng = np.random.default_rng(N + D + k + 1)
    Y = rng.standard_normal((N, D)).astype(np.float32)
    lat = _lat(Y, k)
    lat.remove([5, 6], mode="incremental")
    _assert_only(lat, "remove", family)
    rowptr, col, a, _, _ = lat.graph_csr()
    lat.set_graph_csr(rowptr, col, a)  # an injected graph keeps no kNN lists: nothing can seed a build
    before = _infos(lat)
    Ynew = rng.standard_normal((2, D)).astype(np.float32)
    for call in (lambda: lat.append(Ynew, mode="incremental"), lambda: lat.remove([1], mode="incremental"),
                 lambda: lat.update([1, 2], Ynew, mode="incremental")):
        with pytest.raises(NotImplementedError, match="no kNN lists"):
            call()
        assert lat.N == N - 2 and _infos(lat) == before


def test_denied_by_an_effective_k_change_is_reported_under_append_or_remove():
    """k changes with the row count only where N - 1 < k: lattices of a few rows (the check runs on the host before the
    score family matters, so there is no butterfly form of it)."""
    rng = np.random.default_rng(11)
    Y = rng.standard_normal((12, 8)).astype(np.float32)
    lat = _lat(Y[:6], 6)
    assert lat._kneighbors == 5
    lat.append(Y[6:9])  # auto
    infos = _infos(lat)
    assert lat._kneighbors == 6 and infos["append"]["route"] == 2 and infos["append"]["denied"] == 3
    assert infos["remove"]["denied"] == 0 and infos["update"]["denied"] == 0 and infos["remove"]["route"] == 0
    lat = _lat(Y[:8], 6)
    assert lat._kneighbors == 6
    lat.remove([0, 7])  # auto
    infos = _infos(lat)
    assert lat._kneighbors == 5 and infos["remove"]["route"] == 2 and infos["remove"]["denied"] == 3
    assert infos["append"]["denied"] == 0 and infos["update"]["denied"] == 0 and infos["append"]["route"] == 0


@pytest.mark.parametrize("N,D,k,knn_mode,family", SHAPES)
def test_denied_by_too_many_query_rows_is_reported_under_update(monkeypatch, N, D, k, knn_mode, family):
    if knn_mode:
        monkeypatch.setenv("OSC_KNN_MODE", knn_mode)
    rng = np.random.default_rng(N + D + k + 2)
    Y = rng.standard_normal((N, D)).astype(np.float32)
    M = N // 4  # above both families' cap of max(32, N / 32) and max(32, N / 256) query rows
    lat = _lat(Y, k)
    lat.update(rng.choice(N, size=M, replace=False), rng.standard_normal((M, D)).astype(np.float32))  # auto
    infos = _infos(lat)
    assert infos["update"]["route"] == 2 and infos["update"]["denied"] == 8 and infos["update"]["replaced_rows"] == M
    assert infos["append"]["denied"] == 0 and infos["remove"]["denied"] == 0
    assert infos["append"]["route"] == 0 and infos["remove"]["route"] == 0


def _sorted_lists(lat):
    idx, val = device_knn_lists(lat, lat.N, lat._kneighbors)
    order = np.argsort(idx, axis=1, kind="stable")  # in-row order is not part of the contract
    return np.take_along_axis(idx, order, axis=1), np.take_along_axis(val, order, axis=1).view(np.uint32)


def test_appended_rows_that_start_inside_a_chunk_and_a_tie_that_must_lose(monkeypatch):
    """OSC_APPEND_SCRATCH_MB=1 leaves one 128-row tile per chunk at 1200 columns.  60 all-zero old rows (every score 0: their
    lists are redone) and 200 new rows are three chunks; the new rows start at entry 60 of the first, so each chunk's merge
    starts at a column id worked out from where the chunk stands in the query list.  New row N0 + 7 is a copy of old row 5: wherever both
    could enter a list with equal scores the old row's lower index wins, as in the fresh build."""
    monkeypatch.setenv("OSC_APPEND_SCRATCH_MB", "1")
    N0, M, D, k = 1000, 200, 64, 16
    rng = np.random.default_rng(N0 + M + D + k)
    Y = rng.standard_normal((N0 + M, D)).astype(np.float32)
    zero_rows = rng.choice(np.arange(10, N0), size=60, replace=False)
    Y[zero_rows] = 0.0
    Y[N0 + 7] = Y[5]
    app = _lat(Y[:N0], k)
    app.append(Y[N0:], mode="incremental")
    info = app.append_info()
    assert info["route"] == 1 and info["new_rows"] == M and info["redo_rows"] == 60 and info["merged_rows"] == N0 - 60
    assert info["merge_hits"] > 0
    fresh = _lat(Y, k)
    ia, va = _sorted_lists(app)
    jf, vf = _sorted_lists(fresh)
    rows = np.nonzero((ia != jf).any(axis=1) | (va != vf).any(axis=1))[0]
    assert rows.size == 0, ("kNN lists differ", rows[:8].tolist(), ia[rows[:2]].tolist(), jf[rows[:2]].tolist())
    for name, a, f in zip(("rowptr", "col", "A", "W", "sqrt_deg"), app.graph_csr(), fresh.graph_csr()):
        assert np.array_equal(a, f), name
    idx, _ = device_knn_lists(app, N0 + M, k)
    holds_copy = [r for r in range(N0) if r != 5 and (N0 + 7) in idx[r]]
    assert holds_copy, "the copy entered no old row's list: the tie was never at stake"
    for r in holds_copy:
        assert 5 in idx[r]

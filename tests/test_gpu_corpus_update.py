"""Corpus.update: a corpus whose rows were replaced in place against a fresh Corpus over the changed
rows.  Search ids and cosines and every array refine_many returns must be the same bytes: the replaced rows are normalised
with append's arithmetic, k_cq_gemm sums every output in one fixed order, and everything behind the select reads only the
gathered rows."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ID_KEYS = ("ids", "candidates")
REFINES = ({}, {"gates": "diffusion"}, {"receipts": "full"})
N, Q, TOP_K = 3000, 5, 40
# the first and the last row, both sides of a bitmap word, of a GEMM row tile and of the 1024-row mark, and scattered ones
IDS = np.array([2999, 0, 31, 32, 127, 128, 1023, 1024, 2000, 5, 1500, 777, 2047, 2048, 64, 63], dtype=np.int64)


@pytest.fixture(scope="module")
def amd():
    import oscillink_amd

    return oscillink_amd


def _rows(D, seed=0):
    """Anchors with tied pairs, their replacements (one a copy of a row that stays, one a copy of another new row, one zero
    row) and queries (psi = 0: every cosine ties; a replaced row's new vector; an old vector that is gone)."""
    rng = np.random.default_rng(seed + D)
    Y = rng.standard_normal((N, D)).astype(np.float32)
    Y[1::7] = Y[0::7][: Y[1::7].shape[0]]
    Ynew = rng.standard_normal((IDS.size, D)).astype(np.float32)
    Ynew[2] = Y[10]
    Ynew[4] = Ynew[3]
    Ynew[6] = 0.0
    P = rng.standard_normal((Q, D)).astype(np.float32)
    P[0] = 0.0
    P[1] = Ynew[0]
    P[2] = Y[IDS[1]]
    return Y, Ynew, P


def _changed(Y, ids, Ynew):
    Y2 = Y.copy()
    Y2[ids] = Ynew
    return Y2


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(got, want) and got.tobytes() == want.tobytes(), what


def _same_dict(got, want, idmap, what):
    assert set(got) == set(want), what
    for key, w in want.items():
        _same(got[key], idmap[w].astype(w.dtype) if key in ID_KEYS else w, f"{what}: {key}")


def _check_against_fresh(amd, c, Yc, P, *, allow=None):
    """c (whose rows are Yc) against a fresh Corpus of its live rows, and under `allow` against one of the allowed live rows."""
    for mask in (None,) if allow is None else (None, allow):
        visible = c.alive() if mask is None else mask & c.alive()
        idmap = np.flatnonzero(visible)
        kw = {} if mask is None else {"allow": mask}
        with amd.Corpus(Yc[visible]) as f:
            for top_k in (1, TOP_K):
                ids, cos = c.search(P, top_k, **kw)
                fids, fcos = f.search(P, top_k)
                _same(ids, idmap[fids].astype(np.int32), f"search ids top_k={top_k} {kw.keys()}")
                _same(cos, fcos, f"search cos top_k={top_k} {kw.keys()}")
            for extra in REFINES:
                got = c.refine_many(P, TOP_K, as_arrays=True, **extra, **kw)
                want = f.refine_many(P, TOP_K, as_arrays=True, **extra)
                _same_dict(got, want, idmap, f"refine_many {extra} {kw.keys()}")


@pytest.mark.parametrize("D", [64, 70], ids=["D64", "D70_pitch_not_a_multiple_of_32"])
def test_updated_corpus_answers_like_a_fresh_one(amd, D):
    Y, Ynew, P = _rows(D)
    allow = np.random.default_rng(1).random(N) < 0.5
    allow[IDS[:8]] = True
    with amd.Corpus(Y) as c:
        before = (c.N, c.n_live, c.capacity)
        assert c.update(IDS, Ynew) is None
        assert (c.N, c.n_live, c.capacity) == before and c.alive().all()
        Y2 = _changed(Y, IDS, Ynew)
        ids, _ = c.search(P, TOP_K)
        assert ids[1, 0] == IDS[0]  # psi = the new vector of row 2999
        assert ids[2, 0] == 1  # psi = the old vector of row 0, which is gone: its twin, row 1, comes first
        _check_against_fresh(amd, c, Y2, P, allow=allow)
        c.update([], np.zeros((0, D), dtype=np.float32))  # nothing
        c.update(IDS[:3], Y[IDS[:3]])  # and back again, for three of them
        _check_against_fresh(amd, c, _changed(Y2, IDS[:3], Y[IDS[:3]]), P)


def test_update_on_a_corpus_with_tombstones(amd):
    Y, Ynew, P = _rows(64, seed=2)
    gone = np.array([1, 30, 33, 126, 129, 1022, 2998, *range(400, 440)])
    assert not np.isin(gone, IDS).any()
    allow = np.random.default_rng(2).random(N) < 0.5
    with amd.Corpus(Y) as c:
        c.remove(gone)
        c.update(IDS, Ynew)
        assert (c.N, c.n_live) == (N, N - gone.size) and not c.alive()[gone].any() and c.alive().sum() == N - gone.size
        _check_against_fresh(amd, c, _changed(Y, IDS, Ynew), P, allow=allow)


def test_update_after_compact(amd):
    Y, Ynew, P = _rows(64, seed=3)
    gone = np.array([0, 31, 127, 2999, *range(400, 440)])
    with amd.Corpus(Y) as c:
        c.remove(gone)
        new_id = c.compact()
        Yc = np.delete(Y, gone, axis=0)
        ids = np.array([c.N - 1, 0, 31, 32, 127, 128, 1023, 1024, 2000, 5, 1500, 777, 2047, 2048, 64, 63])
        assert c.N == N - gone.size == Yc.shape[0] and new_id[2998] == c.N - 1
        c.update(ids, Ynew)
        assert c.N == c.n_live == Yc.shape[0]
        _check_against_fresh(amd, c, _changed(Yc, ids, Ynew), P)


def test_errors_change_nothing(amd):
    Y, Ynew, P = _rows(64, seed=4)
    with amd.Corpus(Y) as c:
        c.remove([7, 1500])
        before = c.search(P, TOP_K), (c.N, c.n_live, c.capacity)
        bad_rows = Ynew[:2].copy()
        bad_rows[1, 3] = np.nan
        inf_rows = Ynew[:2].copy()
        inf_rows[0, 0] = np.inf
        with pytest.raises(ValueError, match="outside"):
            c.update([5, N], Ynew[:2])
        with pytest.raises(ValueError, match="outside"):
            c.update([-1, 5], Ynew[:2])
        with pytest.raises(ValueError, match="removed row"):
            c.update([5, 1500], Ynew[:2])
        with pytest.raises(ValueError, match="twice"):
            c.update([5, 5], Ynew[:2])
        with pytest.raises(ValueError, match="finite"):
            c.update([5, 6], bad_rows)
        with pytest.raises(ValueError, match="finite"):
            c.update([5, 6], inf_rows)
        with pytest.raises(ValueError, match="array"):
            c.update([5, 6], Ynew[:3])
        with pytest.raises(ValueError, match="array"):
            c.update([5, 6], Ynew[:2, :63])
        with pytest.raises(ValueError, match="array"):
            c.update([5], Ynew[0])
        with pytest.raises(ValueError, match="integers"):
            c.update(np.array([5.0, 6.0]), Ynew[:2])
        after = c.search(P, TOP_K), (c.N, c.n_live, c.capacity)
        assert after[1] == before[1]
        _same(after[0][0], before[0][0], "ids after the rejected calls")
        _same(after[0][1], before[0][1], "cos after the rejected calls")
        alive = c.alive()
        assert not alive[[7, 1500]].any() and alive.sum() == N - 2

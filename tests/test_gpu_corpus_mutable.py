"""A Corpus that has been appended to, pruned, filtered and compacted against the yardstick of
the whole feature: a fresh Corpus built from the rows that should be visible, ids mapped through np.flatnonzero.  Search ids
and cosines and every array refine_many returns must be the same bytes -- k_cq_gemm sums every output in one fixed order,
and everything behind the select reads only the gathered rows."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D = 64
ID_KEYS = ("ids", "candidates")
REFINES = ({}, {"gates": "diffusion"}, {"receipts": "full"})


@pytest.fixture(scope="module")
def amd():
    import oscillink_amd

    return oscillink_amd


def _corpora(D=D, N=600, seed=0):  # tests/test_gpu_refine_many.py's recipe
    rng = np.random.default_rng(seed)
    gauss = rng.standard_normal((N, D)).astype(np.float32)
    centers = rng.standard_normal((8, D)).astype(np.float32) * 3
    clustered = (centers[rng.integers(0, 8, N)] + 0.3 * rng.standard_normal((N, D))).astype(np.float32)
    dup = gauss.copy()
    dup[1::7] = dup[0::7][: dup[1::7].shape[0]]
    zero = gauss.copy()
    zero[::11] = 0.0
    return {"gauss": gauss, "clustered": clustered, "dup": dup, "zero": zero}


CORPORA = _corpora()
BIG = _corpora(N=1100, seed=3)["dup"]


def _queries(Y, Q=6, seed=1):
    """psi = 0 (every cosine ties), psi = corpus rows 5 and 0, and random ones."""
    rng = np.random.default_rng(seed)
    P = rng.standard_normal((Q, Y.shape[1])).astype(np.float32)
    P[0] = 0.0
    P[1] = Y[5]
    P[2] = Y[0]
    return P


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(got, want) and got.tobytes() == want.tobytes(), what


def _same_dict(got, want, idmap, what):
    assert set(got) == set(want), what
    for key, w in want.items():
        _same(got[key], idmap[w].astype(w.dtype) if key in ID_KEYS else w, f"{what}: {key}")


def _check_against_fresh(amd, c, Yc, P, top_ks, *, visible=None, allow=None, refine_top_k=100, refines=REFINES):
    """c (whose rows are Yc) under `allow` against a fresh Corpus of Yc[visible], for all queries at once."""
    visible = c.alive() if visible is None else visible
    idmap = np.flatnonzero(visible)
    kw = {} if allow is None else {"allow": allow}
    with amd.Corpus(Yc[visible]) as f:
        for top_k in top_ks:
            ids, cos = c.search(P, top_k, **kw)
            fids, fcos = f.search(P, top_k)
            _same(ids, idmap[fids].astype(np.int32), f"search ids top_k={top_k}")
            _same(cos, fcos, f"search cos top_k={top_k}")
        for extra in refines:
            got = c.refine_many(P, refine_top_k, as_arrays=True, **extra, **kw)
            want = f.refine_many(P, refine_top_k, as_arrays=True, **extra)
            _same_dict(got, want, idmap, f"refine_many {extra}")


# ---------------------------------------------------------------------------------------------------------------- append
@pytest.mark.parametrize("kind", sorted(CORPORA))
def test_appended_corpus_answers_like_a_fresh_one(amd, kind):
    Y = CORPORA[kind]
    P = _queries(Y)
    with amd.Corpus(Y[:333]) as c, amd.Corpus(Y) as f:
        assert (c.N, c.n_live, c.capacity) == (333, 333, 333)
        ids = c.append(Y[333:428])  # crosses the word 416 and the GEMM tile 384, and has to grow
        assert ids.dtype == np.int64 and np.array_equal(ids, np.arange(333, 428))
        cap = c.capacity
        assert cap >= 428 and cap > 333 and cap % 128 == 0
        assert np.array_equal(c.append(Y[428:]), np.arange(428, 600))  # crosses the tile 512
        assert np.array_equal(c.append(np.zeros((0, D), dtype=np.float32)), np.zeros(0, dtype=np.int64))
        assert (c.N, c.n_live) == (600, 600) and c.capacity >= 600 and c.alive().all() and c.alive().shape == (600,)
        idmap = np.arange(600)
        for top_k in (1, 100, 600):
            got, want = c.search(P, top_k), f.search(P, top_k)
            _same(got[0], want[0], f"search ids top_k={top_k}")
            _same(got[1], want[1], f"search cos top_k={top_k}")
        for extra in REFINES:
            _same_dict(c.refine_many(P, 100, as_arrays=True, **extra), f.refine_many(P, 100, as_arrays=True, **extra), idmap,
                       f"refine_many {extra}")
        _same_dict(c.diffusion_gates_many(P, 100), f.diffusion_gates_many(P, 100), idmap, "diffusion_gates_many")
        for top_k in (1, 100, 600):
            assert c.info(top_k) == f.info(top_k)


# ---------------------------------------------------------------------------------------------------------------- remove
DUP_REMOVED = np.array([0, 599, *range(64, 96), 7, 15, 21, 358])  # 7, 15, 21, 358: one row of a tied pair each


def test_removed_rows_leave_the_search_and_ties_keep_their_order(amd):
    Y = CORPORA["dup"]
    assert np.array_equal(Y[0], Y[1]) and np.array_equal(Y[7], Y[8]) and np.array_equal(Y[14], Y[15])
    assert np.array_equal(Y[21], Y[22]) and np.array_equal(Y[357], Y[358])
    P = _queries(Y)
    with amd.Corpus(Y) as c:
        assert c.remove(DUP_REMOVED) == DUP_REMOVED.size
        alive = c.alive()
        assert (c.N, c.n_live) == (600, 600 - DUP_REMOVED.size) and not alive[DUP_REMOVED].any()
        assert alive.sum() == c.n_live
        live_ids = np.flatnonzero(alive)
        for top_k in (1, 100, 600):
            ids, cos = c.search(P, top_k)
            K = min(top_k, c.n_live)
            assert ids.shape == (P.shape[0], K) and alive[ids].all()
            assert ids[2, 0] == 1  # psi = Y[0]: row 0 is gone, its twin comes first
            # psi = 0: every cosine ties, so the answer is the K smallest live ids -- a masked row that still advanced the
            # position inside the tie class would push live rows out
            assert np.array_equal(ids[0], live_ids[:K]) and not cos[0].any()
        _check_against_fresh(amd, c, Y, P, (1, 100, 600))
        before = c.search(P, 100)
        assert c.remove(DUP_REMOVED) == 0 and c.remove([]) == 0 and c.n_live == 600 - DUP_REMOVED.size
        after = c.search(P, 100)
        _same(after[0], before[0], "ids after removing again")
        _same(after[1], before[1], "cos after removing again")


def test_top_k_is_clamped_to_the_live_rows(amd):
    Y = CORPORA["gauss"]
    P = _queries(Y)
    with amd.Corpus(Y[:40]) as c:
        assert c.remove(np.arange(3, 33, 2)) == 15
        out = c.refine_many(P, 100, as_arrays=True)
        assert out["candidates"].shape == (P.shape[0], 25) and c.search(P, 100)[0].shape == (P.shape[0], 25)
        _check_against_fresh(amd, c, Y[:40], P, (1, 25, 100))
    with amd.Corpus(Y[:5]) as c:
        assert c.remove([1, 4]) == 2
        assert c.search(P, 100)[0].shape == (P.shape[0], 3) and c.info(100) == c.info(3)
        _check_against_fresh(amd, c, Y[:5], P, (1, 3, 5))


def test_removed_rows_across_both_strides_of_the_select(amd):
    P = _queries(BIG)
    with amd.Corpus(BIG) as c:  # 1100 rows: a second, partial round of the 1024 threads
        assert c.remove([1023, 1024, 1099]) == 3
        ids, _ = c.search(P, 1024)
        assert ids.shape == (P.shape[0], 1024) and np.array_equal(ids[0], np.flatnonzero(c.alive())[:1024])
        _check_against_fresh(amd, c, BIG, P, (1, 100, 1024), refines=({},))


# ----------------------------------------------------------------------------------------------------------------- allow
def test_shared_filter_with_and_without_tombstones(amd):
    Y = CORPORA["clustered"]
    P = _queries(Y)
    rng = np.random.default_rng(5)
    allow = rng.random(600) < 0.5
    with amd.Corpus(Y) as c:
        assert allow.sum() >= 250  # K = min(top_k, n_live) rows must be eligible: no top_k beyond them
        _check_against_fresh(amd, c, Y, P, (1, 100, 250), visible=allow, allow=allow)
        got, want = c.diffusion_gates_many(P, 100, allow=allow), None
        with amd.Corpus(Y[allow]) as f:
            want = f.diffusion_gates_many(P, 100)
        _same_dict(got, want, np.flatnonzero(allow), "diffusion_gates_many")
        assert c.remove(np.flatnonzero(rng.random(600) < 0.2)) > 0
        assert (allow & c.alive()).sum() >= 200
        _check_against_fresh(amd, c, Y, P, (1, 100, 200), visible=allow & c.alive(), allow=allow)


def test_per_query_filter_each_query_against_its_own_fresh_corpus(amd):
    Y = CORPORA["zero"]
    P = _queries(Y)
    Q = P.shape[0]
    rng = np.random.default_rng(6)
    allow = rng.random((Q, 600)) < 0.4
    assert allow.sum(axis=1).min() >= 150
    with amd.Corpus(Y) as c:
        assert c.remove([0, 5, 31, 32, 599]) == 5
        res = {top_k: c.search(P, top_k, allow=allow) for top_k in (1, 100)}
        plain = c.refine_many(P, 100, as_arrays=True, allow=allow)
        gated = c.refine_many(P, 100, as_arrays=True, gates="diffusion", allow=allow)
        for q in range(Q):
            vis = allow[q] & c.alive()
            idmap = np.flatnonzero(vis)
            with amd.Corpus(Y[vis]) as f:
                for top_k, (ids, cos) in res.items():
                    fids, fcos = f.search(P[q:q + 1], top_k)
                    _same(ids[q], idmap[fids[0]].astype(np.int32), f"query {q} ids top_k={top_k}")
                    _same(cos[q], fcos[0], f"query {q} cos top_k={top_k}")
                for got, extra in ((plain, {}), (gated, {"gates": "diffusion"})):
                    want = f.refine_many(P[q:q + 1], 100, as_arrays=True, **extra)
                    _same_dict({k: v[q:q + 1] for k, v in got.items()}, want, idmap, f"query {q} refine_many {extra}")


def test_filter_with_exactly_k_rows_and_with_one_fewer(amd):
    Y = CORPORA["gauss"]
    P = _queries(Y)
    Q = P.shape[0]
    with amd.Corpus(Y) as c:
        assert c.remove([10, 20, 30]) == 3
        rows = np.flatnonzero(c.alive())[::5][:100]
        allow = np.zeros(600, dtype=bool)
        allow[rows] = True
        allow[[10, 20]] = True  # allowed but removed: they do not count
        ids, _ = c.search(P, 100, allow=allow)
        assert np.array_equal(np.sort(ids, axis=1), np.tile(rows, (Q, 1)))
        _check_against_fresh(amd, c, Y, P, (1, 100), visible=allow & c.alive(), allow=allow)
        short = allow.copy()
        short[rows[0]] = False
        for call in (lambda a: c.search(P, 100, allow=a), lambda a: c.refine_many(P, 100, allow=a),
                     lambda a: c.diffusion_gates_many(P, 100, allow=a)):
            with pytest.raises(ValueError, match=r"query 0 has 99 eligible"):
                call(short)
            per_query = np.tile(allow, (Q, 1))
            per_query[3] = short
            with pytest.raises(ValueError, match=r"query 3 has 99 eligible"):
                call(per_query)
        _same(c.search(P, 100, allow=allow)[0], ids, "the call after a rejected filter")
        _same(c.search(P, 99, allow=short)[0].shape, (Q, 99), "K - 1 rows serve top_k = K - 1")


@pytest.mark.parametrize("tombstones", [False, True])
def test_filter_of_all_true_returns_the_bytes_of_no_filter(amd, tombstones):
    Y = CORPORA["dup"]
    P = _queries(Y)
    with amd.Corpus(Y) as c:
        if tombstones:
            c.remove(DUP_REMOVED)
        for allow in (np.ones(600, dtype=bool), np.ones((P.shape[0], 600), dtype=bool)):
            for top_k in (1, 100, 600):
                got, want = c.search(P, top_k, allow=allow), c.search(P, top_k)
                _same(got[0], want[0], f"ids top_k={top_k}")
                _same(got[1], want[1], f"cos top_k={top_k}")
            for extra in REFINES:
                _same_dict(c.refine_many(P, 100, as_arrays=True, allow=allow, **extra),
                           c.refine_many(P, 100, as_arrays=True, **extra), np.arange(600), f"refine_many {extra}")


def test_filter_masking_a_row_promotes_its_twin(amd):
    Y = CORPORA["dup"]
    P = _queries(Y)
    allow = np.ones(600, dtype=bool)
    allow[0] = False
    with amd.Corpus(Y) as c:
        assert c.search(P, 10)[0][2, 0] == 0
        ids, cos = c.search(P, 10, allow=allow)
        assert ids[2, 0] == 1 and np.array_equal(ids[0], np.arange(1, 11))
        _check_against_fresh(amd, c, Y, P, (1, 100, 599), visible=allow, allow=allow, refines=({},))
        with pytest.raises(ValueError, match=r"query 0 has 599 eligible"):
            c.search(P, 600, allow=allow)


# --------------------------------------------------------------------------------------------------------------- compact
def test_compact_renumbers_and_changes_no_answer(amd):
    Y = CORPORA["dup"]
    P = _queries(Y)
    with amd.Corpus(Y) as c:
        assert np.array_equal(c.compact(), np.arange(600)) and c.N == 600  # nothing to drop
        c.remove(DUP_REMOVED)
        alive = c.alive()
        before_s = {top_k: c.search(P, top_k) for top_k in (1, 100, 600)}
        before_r = [c.refine_many(P, 100, as_arrays=True, **extra) for extra in REFINES]
        new_id = c.compact()
        n = int(alive.sum())
        assert new_id.dtype == np.int64 and new_id.shape == (600,)
        assert np.array_equal(new_id[alive], np.arange(n)) and np.all(new_id[~alive] == -1)
        assert c.N == n and c.n_live == n and c.alive().all() and c.capacity == (n + 127) // 128 * 128
        for top_k, (ids, cos) in before_s.items():
            got = c.search(P, top_k)
            _same(got[0], new_id[ids].astype(np.int32), f"ids top_k={top_k}")
            _same(got[1], cos, f"cos top_k={top_k}")
        for extra, want in zip(REFINES, before_r):
            _same_dict(c.refine_many(P, 100, as_arrays=True, **extra), want, new_id, f"refine_many {extra}")
        Yc = Y[alive]
        _check_against_fresh(amd, c, Yc, P, (1, 100, 600))
        assert np.array_equal(c.append(Y[DUP_REMOVED]), np.arange(n, 600))  # append after compact
        Yc = np.vstack([Yc, Y[DUP_REMOVED]])
        assert c.remove([n + 1]) == 1
        _check_against_fresh(amd, c, Yc, P, (1, 100, 600))


# ---------------------------------------------------------------------------------------------------------------- errors
def test_errors_leave_the_corpus_as_it_was(amd):
    Y = CORPORA["gauss"]
    P = _queries(Y)
    Q = P.shape[0]
    with amd.Corpus(Y[:100]) as c:
        want = c.search(P, 10)
        with pytest.raises(ValueError, match="Ynew"):
            c.append(np.zeros((3, D + 1), dtype=np.float32))
        with pytest.raises(ValueError, match="Ynew"):
            c.append(np.zeros(D, dtype=np.float32))
        bad = Y[100:103].copy()
        bad[1, 7] = np.inf
        with pytest.raises(ValueError, match="finite"):
            c.append(bad)
        bad[1, 7] = np.nan
        with pytest.raises(ValueError, match="finite"):
            c.append(bad)
        for ids in ([100], [-1], [3, 4, 100]):
            with pytest.raises(ValueError, match=r"outside \[0, 100\)"):
                c.remove(ids)
        assert (c.N, c.n_live) == (100, 100)  # [3, 4, 100] removed nothing
        with pytest.raises(ValueError, match="integers"):
            c.remove([1.5])
        allow = np.ones(100, dtype=bool)
        cand = np.tile(np.arange(10), (Q, 1))
        with pytest.raises(ValueError, match="allow cannot be combined with candidates"):
            c.refine_many(P, 10, candidates=cand, allow=allow)
        with pytest.raises(ValueError, match="allow cannot be combined with candidates"):
            c.diffusion_gates_many(P, 10, candidates=cand, allow=allow)
        for wrong in (np.ones(99, dtype=bool), np.ones((Q + 1, 100), dtype=bool), np.ones((Q, 101), dtype=bool),
                      np.ones((1, Q, 100), dtype=bool)):
            with pytest.raises(ValueError, match="allow must have shape"):
                c.search(P, 10, allow=wrong)
        for wrong in (np.ones(100, dtype=np.uint8), np.ones(100, dtype=np.float32), np.ones((Q, 100), dtype=np.int64)):
            with pytest.raises(ValueError, match="bool"):
                c.search(P, 10, allow=wrong)
        assert c.remove([4]) == 1
        ok = cand.copy()
        ok[:, 4] = 77
        with pytest.raises(ValueError, match=r"query 2 names removed id 4"):
            cand2 = ok.copy()
            cand2[2, 7] = 4
            c.refine_many(P, 10, candidates=cand2)
        assert np.array_equal(c.refine_many(P, 10, candidates=ok, as_arrays=True)["candidates"], ok)
        got = c.search(P, 10)
        live_map = np.flatnonzero(c.alive())
        with amd.Corpus(Y[:100][c.alive()]) as f:
            _same(got[0], live_map[f.search(P, 10)[0]].astype(np.int32), "search after the rejected calls")
        assert not np.array_equal(got[0], want[0]) or not (want[0] == 4).any()


def test_a_corpus_without_live_rows_and_a_closed_one(amd):
    Y = CORPORA["gauss"]
    P = _queries(Y)
    c = amd.Corpus(Y[:40])
    assert c.remove(np.arange(40)) == 40 and c.n_live == 0 and c.N == 40 and not c.alive().any()
    for call in (lambda: c.search(P, 5), lambda: c.refine_many(P, 5), lambda: c.diffusion_gates_many(P, 5), c.compact):
        with pytest.raises(ValueError, match="no live rows"):
            call()
    assert np.array_equal(c.append(Y[40:50]), np.arange(40, 50)) and c.n_live == 10  # ids are not reused
    ids, _ = c.search(P, 100)
    assert ids.shape == (P.shape[0], 10) and np.array_equal(ids[0], np.arange(40, 50))
    c.close()
    for call in (lambda: c.search(P, 5), lambda: c.append(Y[:2]), lambda: c.remove([0]), c.compact, c.alive,
                 lambda: c.n_live, lambda: c.capacity):
        with pytest.raises(ValueError, match="closed"):
            call()

"""Candidate lattices of different sizes in one batch (`ragged=True`) against section 13.6's
yardstick: for query q with eligible set E_q, a fresh Corpus(Y[E_q]) called with that one query and the same top_k computes
the n_q-row lattice (K is clamped to its rows).  Every array the ragged batch returns for q, cut to n_q, must be the same
bytes (ids mapped through np.flatnonzero), and everything behind n_q must be the documented fill: -1 in ids, local and
candidates, 0 in score, align, gates and cos.  No key and no query is left out of the comparison."""
import numpy as np
import pytest

from tests.test_gpu_corpus_mutable import _corpora, _queries, _same, _same_dict

pytestmark = pytest.mark.gpu

TOP_K, KN, KPICK = 300, 6, 8
# the seams: the list-length clamp (1, 2, kneighbors, kneighbors + 1), the lanes of the select and of k_mutual_ell (63 .. 65),
# the dense tile (127 .. 129), the 256-thread row ownership (255 .. 257), K itself, and more eligible rows than K
ELIGIBLE = (1, 2, KN, KN + 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 500)
PER_K = ("ids", "local", "score", "align")           # (Q, min(k, K)), cut to min(k, n_q)
PER_ROW = ("candidates", "gates")                    # (Q, K), cut to n_q
FLAT = {"null_offsets": ("null_i", "null_j", "null_z", "null_r"),
        "chain_offsets": ("chain_z_struct", "chain_z_path", "chain_r_struct", "chain_r_path")}
FILL = {"ids": -1, "local": -1, "candidates": -1, "score": 0, "align": 0, "gates": 0}


@pytest.fixture(scope="module")
def amd():
    import oscillink_amd

    return oscillink_amd


def _allow_rows(N, counts, seed):
    rng = np.random.default_rng(seed)
    allow = np.zeros((len(counts), N), dtype=bool)
    for q, e in enumerate(counts):
        allow[q, rng.choice(N, size=e, replace=False)] = True
    return allow


def _chains_for(rows):
    """A chain per query inside its own n_q rows (None where the lattice has a single row), and weights for them."""
    chains, weights = [], []
    for n in rows:
        ch = None if n < 2 else ([0, 1] if n < 8 else [0, n - 1, 3, 1, n // 2])
        chains.append(ch)
        weights.append(None if ch is None else [0.5 + 0.25 * t for t in range(len(ch) - 1)])
    return chains, weights


def _cut(got, q, n):
    """Query q of a ragged result as a one-query result of an n-row lattice; checks the fill behind n on the way."""
    out = {}
    for key, v in got.items():
        if key == "rows":
            assert v.dtype == np.int32 and int(v[q]) == n, (key, q, int(v[q]), n)
        elif key in PER_K or key in PER_ROW:
            m = min(v.shape[1], n)
            assert np.all(v[q, m:] == FILL[key]), (key, q, v[q, m:])
            out[key] = v[q:q + 1, :m]
        elif key in FLAT:
            out[key] = v[q:q + 2] - v[q]
            for flat in FLAT[key]:
                out[flat] = got[flat][int(v[q]):int(v[q + 1])]
        elif not any(key in flats for flats in FLAT.values()):
            assert v.shape[0] == len(got["rows"]), key
            out[key] = v[q:q + 1]
    return out


def _mode_kwargs(name, rows, q=None):
    """refine_many's arguments for a mode: the whole batch's (q None) or the yardstick's one-query call."""
    pick = (lambda lst: lst) if q is None else (lambda lst: lst[q:q + 1])
    chains, weights = _chains_for(rows)
    if name == "gates_array":
        g = np.random.default_rng(17).random((len(rows), TOP_K)).astype(np.float32)
        g[:, ::5] = 1.0
        if q is None:
            g[np.arange(TOP_K)[None, :] >= np.asarray(rows)[:, None]] = np.nan  # never read behind n_q
            return {"gates": g}
        return {"gates": g[q:q + 1, :rows[q]]}
    return {"plain": {}, "diffusion": {"gates": "diffusion"}, "full": {"receipts": "full"}, "light": {"receipts": "light"},
            "chains": {"chains": pick(chains)},
            "chains_weights_full": {"chains": pick(chains), "chain_weights": pick(weights), "receipts": "full",
                                    "gates": "diffusion"}}[name]


MODES = ("plain", "diffusion", "gates_array", "full", "light", "chains", "chains_weights_full")


class _Batch:
    """A corpus, a per-query filter, and per query the fresh corpus over its eligible rows (the yardstick)."""

    def __init__(self, amd, Y, P, allow, removed=()):
        self.P, self.allow = P, allow
        self.c = amd.Corpus(Y)
        if len(removed):
            self.c.remove(list(removed))
        alive = self.c.alive()
        self.vis = [(allow if allow.ndim == 1 else allow[q]) & alive for q in range(P.shape[0])]
        self.idmap = [np.flatnonzero(v) for v in self.vis]
        self.rows = [min(TOP_K, int(v.sum())) for v in self.vis]
        self.fresh = [amd.Corpus(Y[v]) for v in self.vis]

    def close(self):
        for f in self.fresh:
            f.close()
        self.c.close()

    def check_refine(self, mode):
        got = self.c.refine_many(self.P, TOP_K, KPICK, as_arrays=True, kneighbors=KN, allow=self.allow, ragged=True,
                                 **_mode_kwargs(mode, self.rows))
        for q, f in enumerate(self.fresh):
            want = f.refine_many(self.P[q:q + 1], TOP_K, KPICK, as_arrays=True, kneighbors=KN,
                                 **_mode_kwargs(mode, self.rows, q))
            _same_dict(_cut(got, q, self.rows[q]), want, self.idmap[q], f"{mode}: query {q} (n = {self.rows[q]})")
        return got

    def check_dicts(self, mode):
        got = self.c.refine_many(self.P, TOP_K, KPICK, kneighbors=KN, allow=self.allow, ragged=True,
                                 **_mode_kwargs(mode, self.rows))
        for q, f in enumerate(self.fresh):
            want = f.refine_many(self.P[q:q + 1], TOP_K, KPICK, kneighbors=KN, **_mode_kwargs(mode, self.rows, q))[0]
            for b in want["bundle"]:
                b["id"] = int(self.idmap[q][b["id"]])
            assert len(got[q]["bundle"]) == min(KPICK, self.rows[q])
            assert got[q] == want, f"{mode}: dict form of query {q} (n = {self.rows[q]})"

    def check_gates_and_search(self):
        got = self.c.diffusion_gates_many(self.P, TOP_K, kneighbors=KN, allow=self.allow, ragged=True)
        ids, cos, rows = self.c.search(self.P, TOP_K, allow=self.allow, ragged=True)
        _same(rows, np.asarray(self.rows, dtype=np.int32), "search rows")
        for q, f in enumerate(self.fresh):
            n = self.rows[q]
            want = f.diffusion_gates_many(self.P[q:q + 1], TOP_K, kneighbors=KN)
            _same_dict(_cut(got, q, n), want, self.idmap[q], f"diffusion_gates_many: query {q} (n = {n})")
            fids, fcos = f.search(self.P[q:q + 1], TOP_K)
            _same(ids[q:q + 1, :n], self.idmap[q][fids].astype(np.int32), f"search ids: query {q}")
            _same(cos[q:q + 1, :n], fcos, f"search cos: query {q}")
            assert np.all(ids[q, n:] == -1) and np.all(cos[q, n:] == 0), q


BIG = _corpora(N=1100, seed=3)["dup"]


@pytest.fixture(scope="module")
def seams(amd):
    b = _Batch(amd, BIG, _queries(BIG, Q=len(ELIGIBLE)), _allow_rows(1100, ELIGIBLE, seed=11))
    assert b.rows == [min(TOP_K, e) for e in ELIGIBLE]
    yield b
    b.close()


@pytest.mark.parametrize("mode", MODES)
def test_sizes_at_every_seam_in_one_batch(seams, mode):
    seams.check_refine(mode)


@pytest.mark.parametrize("mode", ["full", "chains_weights_full"])
def test_dict_form_at_every_seam(seams, mode):
    seams.check_dicts(mode)


def test_gates_many_and_search_at_every_seam(seams):
    seams.check_gates_and_search()


def test_wide_rows(amd):
    Y = _corpora(D=300, N=1100, seed=3)["dup"]
    counts = (1, 2, 65, 129, 257, 300)
    b = _Batch(amd, Y, _queries(Y, Q=len(counts)), _allow_rows(1100, counts, seed=12))
    try:
        for mode in ("plain", "chains_weights_full"):
            b.check_refine(mode)
        b.check_gates_and_search()
    finally:
        b.close()


def test_shared_filter_with_fewer_than_k_rows(amd):
    allow = _allow_rows(1100, (40,), seed=13)[0]
    b = _Batch(amd, BIG, _queries(BIG, Q=5), allow)
    try:
        assert b.rows == [40] * 5
        for mode in ("plain", "full"):
            b.check_refine(mode)
        b.check_gates_and_search()
    finally:
        b.close()


def test_filter_with_tombstones(amd):
    counts = (3, 70, 130, 290, 600)
    allow = _allow_rows(1100, counts, seed=14)
    removed = np.concatenate([np.flatnonzero(allow[q])[:2] for q in range(len(counts))] + [np.arange(400, 440)])
    b = _Batch(amd, BIG, _queries(BIG, Q=len(counts)), allow, removed=removed)
    try:
        assert b.rows[0] == 1 and all(r < e for r, e in zip(b.rows[:4], counts)) and b.rows[4] == TOP_K
        for mode in ("plain", "diffusion", "full"):
            b.check_refine(mode)
        b.check_gates_and_search()
    finally:
        b.close()


def test_ragged_candidates(amd):
    sizes = (1, 2, 65, 300)
    rng = np.random.default_rng(15)
    lists = [rng.choice(1100, size=n, replace=False).tolist() for n in sizes]
    padded = np.full((len(sizes), TOP_K), -1, dtype=np.int64)
    for q, row in enumerate(lists):
        padded[q, :len(row)] = row
    P = _queries(BIG, Q=len(sizes))
    ident = np.arange(1100)
    with amd.Corpus(BIG) as c:
        for extra in ({}, {"gates": "diffusion", "receipts": "full"}):
            a = c.refine_many(P, TOP_K, KPICK, as_arrays=True, candidates=lists, ragged=True, **extra)
            b = c.refine_many(P, TOP_K, KPICK, as_arrays=True, candidates=padded, ragged=True, **extra)
            assert set(a) == set(b)
            for key in a:
                _same(a[key], b[key], f"lists against the padded array: {key}")
            for q, row in enumerate(lists):
                want = c.refine_many(P[q:q + 1], len(row), KPICK, as_arrays=True, candidates=[row], **extra)
                _same_dict(_cut(a, q, len(row)), want, ident, f"candidates {extra}: query {q}")
        ga = c.diffusion_gates_many(P, TOP_K, candidates=lists, ragged=True)
        for q, row in enumerate(lists):
            want = c.diffusion_gates_many(P[q:q + 1], len(row), candidates=[row])
            _same_dict(_cut(ga, q, len(row)), want, ident, f"gates of given candidates: query {q}")


def test_a_query_does_not_see_its_batch(amd, monkeypatch):
    counts = (65, 1, 300, 129, 7)
    allow = _allow_rows(1100, counts, seed=16)
    P = _queries(BIG, Q=len(counts))
    kw = dict(as_arrays=True, receipts="full", gates="diffusion", ragged=True)

    def row(c, order):
        """query 0 at position order.index(0) of the batch `order`"""
        got = c.refine_many(P[list(order)], TOP_K, KPICK, allow=allow[list(order)], **kw)
        return _cut(got, list(order).index(0), counts[0])

    with amd.Corpus(BIG) as c:
        alone = row(c, (0,))
        batches = {"first": (0, 3, 4), "last": (3, 4, 0), "between a 1-row and a K-row lattice": (1, 0, 2),
                   "all": (4, 3, 2, 0, 1)}
        for name, order in batches.items():
            got = row(c, order)
            for key in alone:
                _same(got[key], alone[key], f"{name}: {key}")
    monkeypatch.setenv("OSC_CORPUS_CHUNK", "2")
    with amd.Corpus(BIG) as c:
        assert c.info(TOP_K)["chunk"] == 2
        got = row(c, (4, 3, 2, 0, 1))
        for key in alone:
            _same(got[key], alone[key], f"chunks of 2: {key}")


def test_ragged_with_nothing_short_is_the_plain_call(amd):
    P = _queries(BIG)
    allow = _allow_rows(1100, (400,) * P.shape[0], seed=18)
    with amd.Corpus(BIG) as c:
        for kw in ({}, {"allow": allow}, {"allow": allow[0]}):
            for extra in ({}, {"gates": "diffusion", "receipts": "full"}):
                plain = c.refine_many(P, 100, as_arrays=True, **kw, **extra)
                got = c.refine_many(P, 100, as_arrays=True, ragged=True, **kw, **extra)
                _same(got.pop("rows"), np.full(P.shape[0], 100, dtype=np.int32), "rows")
                assert set(got) == set(plain)
                for key in plain:
                    _same(got[key], plain[key], f"{sorted(kw)} {sorted(extra)}: {key}")
            ids, cos = c.search(P, 100, **kw)
            rids, rcos, rows = c.search(P, 100, ragged=True, **kw)
            _same(rids, ids, "search ids")
            _same(rcos, cos, "search cos")
            assert np.all(rows == 100)


@pytest.mark.parametrize("n", [2, 65, 129])
def test_against_the_loop_itself(amd, n):
    """Oscillink(Y[cand_q], kneighbors=min(6, n_q - 1)) -> set_query -> settle -> receipt -> bundle, under the tolerances of
    the uniform case: tests/test_gpu_refine_receipts.py's check_query (1e-4 relative, equal iteration counts unless the
    deciding residual sits at its tolerance, the near-tie rule for null points, its rounding floor for a solve that ends
    exactly) and tests/test_gpu_refine_many.py's _compare (picks equal up to a near tie, score 1e-4, align 1e-5).  state_sig
    is compared as a string by check_query."""
    from tests.test_gpu_refine_many import _compare
    from tests.test_gpu_refine_receipts import check_query, loop, rounding_floor

    P = _queries(BIG, Q=3, seed=n)[1:]  # a corpus row and a random query
    allow = _allow_rows(1100, (n, 40), seed=n)
    kw = {"kneighbors": min(KN, n - 1)}
    with amd.Corpus(BIG) as c:
        arr = c.refine_many(P, TOP_K, KPICK, as_arrays=True, receipts="full", kneighbors=KN, allow=allow, ragged=True)
        dct = c.refine_many(P, TOP_K, KPICK, receipts="full", kneighbors=KN, allow=allow, ragged=True)
    one = _cut(arr, 0, n)
    cand = one["candidates"][0]
    lp = loop(amd, BIG[cand], P[0], KPICK, 0.5, kw)
    assert dct[0]["receipt"]["meta"]["state_sig"] == lp["receipt"]["meta"]["state_sig"]
    check_query(f"ragged{n}", 0, one, dct[0], lp, allow_iter_exception=True, sum_floor=n == 2,
                res_floor=rounding_floor(BIG[cand], P[0], kw) if n == 2 else 1e-7)
    _compare(amd, BIG, P[:1], one, n, KPICK, 0.5, kw)


def test_errors_come_before_any_device_work(amd):
    P = _queries(BIG, Q=3)
    allow = _allow_rows(1100, (5, 0, 300), seed=19)
    lists = [[1, 2, 3], [4, 5], [6]]
    with amd.Corpus(BIG) as c:
        before = c.refine_many(P, 100, as_arrays=True)
        for call in (lambda **kw: c.refine_many(P, 100, **kw), lambda **kw: c.search(P, 100, **kw),
                     lambda **kw: c.diffusion_gates_many(P, 100, **kw)):
            with pytest.raises(ValueError, match=r"query 1 has 0 eligible"):
                call(allow=allow, ragged=True)
        ok = _allow_rows(1100, (5, 9, 300), seed=19)
        with pytest.raises(ValueError, match=r"query 0: chain indices out of bounds"):
            c.refine_many(P, 100, allow=ok, ragged=True, chains=[[0, 5], None, [0, 99]])
        with pytest.raises(ValueError, match=r"query 1: chain indices out of bounds"):
            c.refine_many(P, 100, candidates=lists, ragged=True, chains=[[0, 2], [0, 2], None])
        with pytest.raises(ValueError, match=r"query 1 has an id behind a -1"):
            c.refine_many(P, 4, candidates=np.array([[1, 2, 3, -1], [4, -1, 5, -1], [6, -1, -1, -1]]), ragged=True)
        with pytest.raises(ValueError, match=r"query 0 has an id behind a -1"):
            c.refine_many(P, 4, candidates=[[1, -1, 3], [4, 5], [6]], ragged=True)
        with pytest.raises(ValueError, match=r"query 2 has 5 ids, need 1 .. K = 4"):
            c.refine_many(P, 4, candidates=[[1, 2, 3], [4, 5], [6, 7, 8, 9, 10]], ragged=True)
        with pytest.raises(ValueError, match=r"query 1 has 0 ids"):
            c.refine_many(P, 4, candidates=[[1, 2, 3], [], [6]], ragged=True)
        with pytest.raises(ValueError, match=r"repeated id"):
            c.refine_many(P, 4, candidates=np.array([[1, 2, 3, 4], [4, 5, 6, 5], [6, 7, 8, 9]]), ragged=True)
        with pytest.raises(ValueError, match=r"query 0 has 5 eligible rows"):
            c.refine_many(P, 100, allow=ok)
        after = c.refine_many(P, 100, as_arrays=True)
        for key in before:
            _same(after[key], before[key], f"the call after the rejected ones: {key}")
        assert c.N == 1100 and c.n_live == 1100

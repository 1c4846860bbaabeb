"""Per-query settings of Corpus.refine_many and diffusion_gates_many: lamG, lamC, lamQ, lamP,
kneighbors, k, alpha, settle_dt, settle_max_iters and settle_tol as length-Q arrays.  The yardstick is the call itself: what
the batch returns for query q, cut at its picks and rows with the fill checked behind them, must be the same bytes as the
one-query call with q's settings as scalars -- every key, every query, every mode.  Q = 12 in chunks of 5 (OSC_CORPUS_CHUNK),
so the settings change inside chunks and across their seams; top_k = 130 is two 128-row dense tiles.

The values and the seams they reach: kneighbors {1, 2, 6, 16, 64, 128} (the list length inside the 128-wide list, one and
two 64-lane passes of k_mutual_ell), k {0, 1, 8, 130, 500} (no pick, one, fewer than K, K, more than K), alpha {0, 0.5, 1},
lamG {0.5, 1, 2}, lamC {0, 0.5, 1.5} and lamQ {4, 0, 0.5} (exact zeros), lamP {0, 0.2, 1.5} (a chain that is present but
inactive), settle_dt {0.5, 1, 2}, settle_max_iters {1, 12, 40}, settle_tol {1e-3, 1e-6, 0} (0 is never met: the settle runs
to max_iters)."""
import numpy as np
import pytest

from tests.test_gpu_corpus_mutable import _corpora, _queries, _same, _same_dict
from tests.test_gpu_refine_ragged import FILL, FLAT, MODES, PER_K, PER_ROW, _chains_for

pytestmark = pytest.mark.gpu

N, TOP_K, Q, CHUNK = 1500, 130, 12, 5
TEN = ("lamG", "lamC", "lamQ", "lamP", "kneighbors", "k", "alpha", "settle_dt", "settle_max_iters", "settle_tol")
INTS = ("kneighbors", "k", "settle_max_iters")
SCALARS = dict(lamG=2.0, lamC=0.5, lamQ=0.5, lamP=1.5, kneighbors=16, k=8, alpha=1.0, settle_dt=2.0, settle_max_iters=40,
               settle_tol=1e-6)
RAGGED_ROWS = (1, 2, 7, 64, 129, 130)


def _cycle(values, shift=0):
    return [values[(q + shift) % len(values)] for q in range(Q)]


# cycles of different lengths and offsets: no two queries share a settings tuple, and neighbours differ in every field
MIXED = {"kneighbors": np.array(_cycle((1, 2, 6, 16, 64, 128))), "k": np.array(_cycle((0, 1, 8, 130, 500))),
         "alpha": np.array(_cycle((0.0, 0.5, 1.0), 1)), "lamG": np.array(_cycle((0.5, 1.0, 2.0), 2)),
         "lamC": np.array(_cycle((0.0, 0.5, 1.5, 0.5))), "lamQ": np.array(_cycle((4.0, 0.0, 0.5, 4.0, 0.5), 1)),
         "lamP": np.array(_cycle((0.0, 0.2, 1.5), 1)), "settle_dt": np.array(_cycle((0.5, 1.0, 2.0, 1.0), 3)),
         "settle_max_iters": np.array(_cycle((1, 12, 40), 2)), "settle_tol": np.array(_cycle((1e-3, 1e-6, 0.0, 1e-3, 1e-6), 2))}


def _one(settings, q):
    """query q's settings as Python scalars"""
    return {n: (int(v[q]) if n in INTS else float(v[q])) for n, v in settings.items()}


@pytest.fixture(scope="module")
def amd():
    import oscillink_amd

    return oscillink_amd


class _Case:
    def __init__(self, amd, D):
        self.Y = _corpora(D=D, N=N, seed=3)["dup"]
        self.P = _queries(self.Y, Q=Q)
        self.c = amd.Corpus(self.Y)
        assert self.c.info(TOP_K)["chunk"] == CHUNK
        rng = np.random.default_rng(21)
        self.gates = rng.random((Q, TOP_K)).astype(np.float32)
        self.gates[:, ::5] = 1.0
        self.lists = [rng.choice(N, size=RAGGED_ROWS[q % len(RAGGED_ROWS)], replace=False).tolist() for q in range(Q)]

    def rows(self, ragged):
        return [len(r) for r in self.lists] if ragged else [TOP_K] * Q

    def mode_kwargs(self, mode, ragged, qs):
        """refine_many's arguments of a mode (tests/test_gpu_refine_ragged.py's MODES) for the queries `qs`, in that order"""
        rows = self.rows(ragged)
        chains, weights = _chains_for(rows)
        pick = lambda lst: [lst[q] for q in qs]  # noqa: E731
        kw = {"plain": {}, "diffusion": {"gates": "diffusion"}, "gates_array": {"gates": self.gates[list(qs)]},
              "full": {"receipts": "full"}, "light": {"receipts": "light"}, "chains": {"chains": pick(chains)},
              "chains_weights_full": {"chains": pick(chains), "chain_weights": pick(weights), "receipts": "full",
                                      "gates": "diffusion"}}[mode]
        if ragged:
            kw = dict(kw, ragged=True, candidates=pick(self.lists))
        return kw

    def call(self, mode, settings, qs=None, ragged=False, **kw):
        qs = list(range(Q)) if qs is None else list(qs)
        return self.c.refine_many(self.P[qs], TOP_K, **settings, **self.mode_kwargs(mode, ragged, qs), **kw)


@pytest.fixture(scope="module", params=[20, 300])
def case(request, amd):
    mp = pytest.MonkeyPatch()
    mp.setenv("OSC_CORPUS_CHUNK", str(CHUNK))
    try:
        cs = _Case(amd, request.param)
    finally:
        mp.undo()
    yield cs
    cs.c.close()


def _cut(got, q, n, p):
    """Query q of a result as a one-query result of an n-row lattice with p picks; the fill behind them is checked on the way,
    and `picks` / `rows`, where the result has them, must say p / n."""
    out = {}
    for key, v in got.items():
        if key == "rows":
            assert v.dtype == np.int32 and int(v[q]) == n, (key, q, int(v[q]), n)
            out[key] = v[q:q + 1]
        elif key == "picks":
            assert v.dtype == np.int32 and int(v[q]) == p, (key, q, int(v[q]), p)
        elif key in PER_K or key in PER_ROW:
            m = min(v.shape[1], p if key in PER_K else n)
            assert np.all(v[q, m:] == FILL[key]), (key, q, v[q, m:])
            out[key] = v[q:q + 1, :m]
        elif key in FLAT:
            out[key] = v[q:q + 2] - v[q]
            for flat in FLAT[key]:
                out[flat] = got[flat][int(v[q]):int(v[q + 1])]
        elif not any(key in flats for flats in FLAT.values()):
            assert v.shape[0] == len(got["candidates"]), key
            out[key] = v[q:q + 1]
    return out


def _picks(settings, rows):
    return [min(max(int(settings["k"][q]), 0), rows[q]) for q in range(len(rows))]


def _check_each_query(cs, mode, settings, ragged):
    rows = cs.rows(ragged)
    picks = _picks(settings, rows)
    got = cs.call(mode, settings, ragged=ragged, as_arrays=True)
    assert got["picks"].tolist() == picks and got["ids"].shape == (Q, min(max(settings["k"]), TOP_K))
    lst = cs.call(mode, settings, ragged=ragged)
    ident = np.arange(N)
    for q in range(Q):
        one = _one(settings, q)
        want = cs.call(mode, one, qs=[q], ragged=ragged, as_arrays=True)
        what = f"{mode}{' ragged' if ragged else ''}: query {q} {one}"
        _same_dict(_cut(got, q, rows[q], picks[q]), _cut(want, 0, rows[q], picks[q]), ident, what)
        want_lst = cs.call(mode, one, qs=[q], ragged=ragged)
        assert lst[q] == want_lst[0], f"list / dict form, {what}"
        bundle = lst[q]["bundle"] if isinstance(lst[q], dict) else lst[q]
        assert len(bundle) == picks[q], what


# ---- 1. equal records equal the scalar call: the per-lattice reads against the launch's arguments
@pytest.mark.parametrize("mode", MODES)
def test_equal_records_equal_the_scalar_call(case, mode):
    arrays = {n: np.full(Q, v) for n, v in SCALARS.items()}
    want = case.call(mode, SCALARS, as_arrays=True)
    got = case.call(mode, arrays, as_arrays=True)
    _same(got.pop("picks"), np.full(Q, SCALARS["k"], dtype=np.int32), "picks")
    assert set(got) == set(want)
    for key in want:
        _same(got[key], want[key], f"{mode}: {key}")
    assert case.call(mode, arrays) == case.call(mode, SCALARS), f"{mode}: list / dict form"
    one = dict(SCALARS, lamC=np.full(Q, SCALARS["lamC"], dtype=np.float32))  # one array arms the call; k stays a scalar
    got = case.call(mode, one, as_arrays=True)
    assert set(got) == set(want)
    for key in want:
        _same(got[key], want[key], f"{mode}, one array: {key}")


# ---- 2. each query against its own scalar call
@pytest.mark.parametrize("mode", MODES)
def test_each_query_against_its_own_scalar_call(case, mode):
    _check_each_query(case, mode, MIXED, ragged=False)


@pytest.mark.parametrize("mode", MODES)
def test_each_query_against_its_own_scalar_call_ragged(case, mode):
    _check_each_query(case, mode, MIXED, ragged=True)


def test_six_columns_per_thread(amd, monkeypatch):
    monkeypatch.setenv("OSC_CORPUS_CHUNK", str(CHUNK))
    cs = _Case(amd, 1290)
    try:
        for mode in ("plain", "full"):
            _check_each_query(cs, mode, MIXED, ragged=False)
    finally:
        cs.c.close()


# ---- 3. order independence
@pytest.mark.parametrize("mode,ragged", [("plain", False), ("chains_weights_full", False), ("chains_weights_full", True)])
def test_permuting_queries_and_settings_permutes_the_results(case, mode, ragged):
    perm = np.random.default_rng(5).permutation(Q)
    assert not np.array_equal(perm, np.arange(Q))
    rows = case.rows(ragged)
    picks = _picks(MIXED, rows)
    base = case.call(mode, MIXED, ragged=ragged, as_arrays=True)
    got = case.call(mode, {n: v[perm] for n, v in MIXED.items()}, qs=perm, ragged=ragged, as_arrays=True)
    ident = np.arange(N)
    for at, q in enumerate(perm):
        _same_dict(_cut(got, at, rows[q], picks[q]), _cut(base, q, rows[q], picks[q]), ident, f"{mode}: query {q} at {at}")


# ---- 4. against the loop itself
def test_plain_mode_against_the_loop(case, amd):
    from tests.test_gpu_refine_many import _compare

    got = case.call("plain", MIXED, as_arrays=True)
    picks = _picks(MIXED, case.rows(False))
    for q in range(Q):
        one = _one(MIXED, q)
        kw = {n: one[n] for n in ("kneighbors", "lamG", "lamC", "lamQ")}
        _compare(amd, case.Y, case.P[q:q + 1], _cut(got, q, TOP_K, picks[q]), TOP_K, one["k"], one["alpha"], kw)


def test_full_receipts_with_chains_against_the_loop(case, amd):
    mode = "chains_weights_full"
    kw = {k: v for k, v in case.mode_kwargs(mode, False, range(Q)).items() if k != "gates"}
    arr = case.c.refine_many(case.P, TOP_K, **MIXED, **kw, as_arrays=True)
    dct = case.c.refine_many(case.P, TOP_K, **MIXED, **kw)
    for q in range(Q):
        one = _one(MIXED, q)
        lat = amd.Oscillink(case.Y[arr["candidates"][q]], kneighbors=one["kneighbors"], lamG=one["lamG"], lamC=one["lamC"],
                            lamQ=one["lamQ"])
        lat.add_chain(kw["chains"][q], lamP=one["lamP"], weights=kw["chain_weights"][q])
        lat.set_receipt_detail("full")
        lat.set_query(case.P[q])
        s = lat.settle(dt=one["settle_dt"], max_iters=one["settle_max_iters"], tol=one["settle_tol"])
        hist = lat.residual_history()
        rec = lat.receipt()
        lat.close()
        assert dct[q]["receipt"]["meta"]["state_sig"] == rec["meta"]["state_sig"], (q, one)
        gi, wi = int(arr["settle_iters"][q]), int(s["iters"])
        print(f"query {q}: settle {gi}/{wi} res {float(arr['settle_res'][q]):.6e}/{s['res']:.6e} {one}")
        if gi != wi:  # tests/test_gpu_refine_many.py's rule: only where the loop's deciding residual sits at its tolerance
            deciding = hist[min(gi, wi) - 1]
            assert abs(deciding - one["settle_tol"]) <= 1e-3 * one["settle_tol"], (q, gi, wi, deciding, one)
        assert dct[q]["settle"]["iters"] == gi


# ---- 5. diffusion_gates_many with per-query kneighbors
@pytest.mark.parametrize("ragged", [False, True])
def test_gates_many_with_per_query_kneighbors(case, ragged):
    kn = MIXED["kneighbors"]
    rows = case.rows(ragged)
    extra = dict(ragged=True, candidates=case.lists) if ragged else {}
    got = case.c.diffusion_gates_many(case.P, TOP_K, kneighbors=kn, **extra)
    ident = np.arange(N)
    for q in range(Q):
        one = dict(ragged=True, candidates=[case.lists[q]]) if ragged else {}
        want = case.c.diffusion_gates_many(case.P[q:q + 1], TOP_K, kneighbors=int(kn[q]), **one)
        _same_dict(_cut(got, q, rows[q], 0), _cut(want, 0, rows[q], 0), ident, f"gates: query {q} kneighbors {int(kn[q])}")
    same = case.c.diffusion_gates_many(case.P, TOP_K, kneighbors=np.full(Q, 6), **extra)
    want = case.c.diffusion_gates_many(case.P, TOP_K, kneighbors=6, **extra)
    for key in want:
        _same(same[key], want[key], f"equal records: {key}")


# ---- 6. arming
def test_arming_is_spent_by_the_next_call_whatever_it_returns(case):
    import ctypes as C

    from oscillink_amd import _native as nat

    c, P = case.c, case.P
    never = c.refine_many(P, TOP_K, as_arrays=True, receipts="full")
    rec = np.zeros(Q, dtype=nat.SETTING_DTYPE)
    for name in TEN:
        rec[name] = MIXED[name]
    ptr = rec.ctypes.data_as(C.c_void_p)

    def scalar_call_is_untouched(what):
        again = c.refine_many(P, TOP_K, as_arrays=True, receipts="full")
        for key in never:
            _same(again[key], never[key], f"{what}: {key}")

    # a failed armed call (top_k = 0) spends the arming
    c._call("osc_corpus_settings", ptr, Q)
    with pytest.raises(ValueError, match="top_k"):
        c._call("osc_corpus_refine", nat.f32(P), Q, 0, None, 6, 1.0, 1.0, 0.5, 4.0, 1e-4, 64, 8, 0.5, None, None, None, None,
                None, None)
    scalar_call_is_untouched("after a failed armed call")
    # an armed call with another Q is refused, and spends the arming too
    c._call("osc_corpus_settings", ptr, Q)
    with pytest.raises(ValueError, match="another Q"):
        c.refine_many(P[:5], TOP_K, as_arrays=True)
    scalar_call_is_untouched("after an armed call with another Q")
    # Q = 0 and NULL clear it
    for args in ((ptr, 0), (None, Q)):
        c._call("osc_corpus_settings", ptr, Q)
        c._call("osc_corpus_settings", *args)
        scalar_call_is_untouched(f"after clearing with {args[1]}")
    # bad records are refused with the query's index, and arm nothing
    bad = rec.copy()
    bad["lamG"][7] = 0.0
    with pytest.raises(ValueError, match="query 7: lamG"):
        c._call("osc_corpus_settings", bad.ctypes.data_as(C.c_void_p), Q)
    scalar_call_is_untouched("after refused records")
    assert nat.lib().osc_corpus_settings(nat.Handle(), ptr, Q) == nat.OSC_E_INVALID
    # and an armed call does differ from the scalar one (the arming is not a no-op)
    rec["k"] = 8  # (the scalar call's output width: the caller of the C entry point sizes the outputs by the records)
    c._call("osc_corpus_settings", ptr, Q)
    armed = c.refine_many(P, TOP_K, as_arrays=True, receipts="full")
    assert not np.array_equal(armed["deltaH"], never["deltaH"])

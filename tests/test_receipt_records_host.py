"""The receipt records of `receipt()`, `receipt_many()` and `Corpus.refine_many(receipts=...)`, byte for byte, without a
device.  The objects are stubs (`__new__`, attributes set by hand); `_call` is a function that
writes a fixed pattern through the ctypes pointers it receives, so everything the host side does with the device's
numbers -- key order, rounding, the null cap, the signature block, the `as_arrays` layout -- ends up in the result.
Each case is serialised with `json.dumps` WITHOUT `sort_keys` (key order counts) and compared as a string with
tests/golden/receipt_records_parent.json.

The fixture was recorded by running this file's case builder on the commit BEFORE the receipt assembly moved into
`oscillink_amd/_receipts.py` (`PYTHONPATH=<a checkout of that commit> python tests/test_receipt_records_host.py
--record`), so `cases()` uses only names that exist on both sides of that change.  Re-record it only for a change that is
meant to alter a receipt, and say so.
"""
import contextlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "receipt_records_parent.json")
ENV_KEYS = ("OSCILLINK_RECEIPT_NULL_CAP", "OSCILLINK_RECEIPT_DYNAMICS")
DYNAMICS = {"temperature": 0.125, "step_deltaH": -1.5, "top_flows": [{"edge": [0, 1], "flow": 0.25}], "radius": 2}


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.pop(k, None) for k in ENV_KEYS}
    os.environ.update({f"OSCILLINK_RECEIPT_{k}": v for k, v in kv.items()})
    try:
        yield
    finally:
        for k in ENV_KEYS:
            os.environ.pop(k, None)
            if old[k] is not None:
                os.environ[k] = old[k]


def _plain(x):
    """JSON-able, order kept; arrays with their dtype so that a changed dtype shows."""
    if isinstance(x, dict):
        return {k: _plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    if isinstance(x, np.ndarray):
        return {"dtype": str(x.dtype), "shape": list(x.shape), "data": x.tolist()}
    if isinstance(x, np.generic):
        return {"numpy_scalar": str(x.dtype), "value": x.item()}
    return x


def _scalars(args):
    return [a for a in args if isinstance(a, (int, float))]


def _fill(ptr, values):
    if ptr is not None:
        for t, v in enumerate(values):
            ptr[t] = v


# ---------------------------------------------------------------------------------------------------------------- lattice
def fake_lattice(N=6, D=4, *, detail="full", secret=None, mode="minimal", gates=None, chain=None, rows_nulls=2,
                 many_totals=(2, 1), basis_solves=False, dynamics=None, cls=None):
    """An OscillinkLattice with no device behind it.  `_call` serves osc_deltaH and osc_receipt_many: query q gets the sums
    (0.1 + q, 0.2 + q, 0.3 + q, 0.4 + q) / 3 (not float32 numbers), `many_totals[q % len]` null points before the cap."""
    if cls is None:
        from oscillink_amd.lattice import OscillinkLattice as cls
    lat = cls.__new__(cls)
    lat._h = None
    lat.N, lat.D, lat._has_comm = N, D, False
    lat._B = np.ones(N, np.float32) if gates is None else np.asarray(gates, np.float32)
    lat._psi = np.linspace(-1.0, 1.0, D).astype(np.float32)
    lat.lamG, lat.lamC, lat.lamQ, lat.lamP = 1.0, 0.5, 4.0, 0.0 if chain is None else 0.2
    lat._chain_nodes, lat._chain_weights = chain, None
    lat._kneighbors, lat._deterministic_k, lat._neighbor_seed = 3, True, 7
    lat.stats = {"ustar_solves": 2, "ustar_cache_hits": 5, "query_basis_solves": 1}
    lat.last = {"iters": 4, "res": 0.00025, "t_ms": 1.5}
    lat.last_ustar = {"iters": 9, "res": 3e-05, "converged": True, "solve_ms": 2.25}
    lat.last_query_basis = {"iters": {"X": 11, "x": 7}, "res": {"X": 2e-05, "x": 1e-05}, "converged": True,
                            "solve_ms": 3.5, "psi_inf": 1.0, "x_only": False}
    lat._graph_build_ms = 12.5
    lat._Ustar_sig = "state-signature"
    lat._receipt_secret = secret
    lat._signature_mode, lat._receipt_detail, lat._last_dynamics = mode, detail, dynamics
    lat.events = []

    def ensure_query_basis(tol, max_iters, psi_inf, extend=True):
        if basis_solves:
            lat.stats["query_basis_solves"] += 1

    def receipt_rows(z_th):
        n = rows_nulls
        f = np.arange(1, N + 1, dtype=np.float32)
        z = np.zeros(N, np.float32)
        z[:4] = [4.5, 9.0, 4.5, 4.5]  # a three-way tie behind the maximum: the cap must keep row 1, then row 0
        return f / 3, f / 7, f / 11, (np.arange(N, dtype=np.int32), np.arange(N, dtype=np.int32)[::-1].copy(), z, f / 13, n)

    def call(name, *args):
        if name == "osc_deltaH":
            args[0]._obj.value = 1.0 / 3.0
            return
        assert name == "osc_receipt_many", name
        lat.events.append([name, _scalars(args)])
        q_n, full, cap = args[1], args[2], args[4]
        at = 0
        for q in range(q_n):
            for t in range(4):
                args[5 + t][q] = (0.1 * (t + 1) + q) / 3.0
            tot = many_totals[q % len(many_totals)] if full else 0
            kept = min(tot, cap) if cap > 0 else tot
            args[9][q] = tot
            for e in range(kept):
                assert at < args[15]
                args[11][at], args[12][at] = q + e, N - 1 - e
                args[13][at], args[14][at] = 3.25 + e + q / 3.0, (1 + e) / 7.0
                at += 1
            args[10][q + 1] = at

    lat._ensure_query_basis = ensure_query_basis
    lat._ensure_device_ustar = lambda: None
    lat.graph_stats = lambda: (14, 3, 0.5)
    lat._edge_prefix = lambda limit=2048: np.array([[0, 1], [1, 0], [2, 3], [3, 2]], np.int64)
    lat._signature = lambda: "state-signature"
    lat._receipt_rows = receipt_rows
    lat._log = lambda ev, payload: lat.events.append([ev, _plain(payload)])
    lat._call = call
    return lat


def queries(Q, D):
    return (np.arange(Q * D, dtype=np.float32).reshape(Q, D) / 7.0 - 1.0).astype(np.float32)


def _lattice_cases(out):
    def one(name, env=None, many=None, **kw):
        with _env(**(env or {})):
            lat = fake_lattice(**kw)
            res = lat.receipt() if many is None else lat.receipt_many(queries(2, lat.D), **many)
            out[name] = {"result": _plain(res), "events": lat.events}

    one("receipt light", detail="light")
    one("receipt full minimal signature", secret=b"k3y")
    one("receipt full extended signature dynamics", env={"DYNAMICS": "1"}, secret=b"k3y", mode="extended", dynamics=DYNAMICS)
    one("receipt dynamics off", secret=b"k3y", dynamics=DYNAMICS)
    one("receipt null cap 2 of 4", env={"NULL_CAP": "2"}, rows_nulls=4)
    one("receipt null cap not reached", env={"NULL_CAP": "4"}, rows_nulls=4)
    one("receipt_many arrays full", many={"as_arrays": True})
    one("receipt_many arrays light", many={"as_arrays": True}, detail="light")
    one("receipt_many light", many={}, detail="light")
    one("receipt_many full", many={})
    one("receipt_many full basis solved", many={"tol": 1e-5}, basis_solves=True)
    one("receipt_many minimal signature", many={}, secret=b"k3y")
    one("receipt_many extended signature dynamics", env={"DYNAMICS": "true"}, many={}, secret=b"k3y", mode="extended",
        dynamics=DYNAMICS, detail="light")
    one("receipt_many gates", many={}, gates=[1.0, 0.5, 0.25, 1.0, 0.0, 0.75])
    one("receipt_many chain", many={}, chain=[0, 2, 4])
    one("receipt_many null cap 1", env={"NULL_CAP": "1"}, many={})
    one("receipt_many null cap 1 arrays", env={"NULL_CAP": "1"}, many={"as_arrays": True})
    for raw in ("", "abc", "-3", " 7 "):
        one(f"receipt_many null cap {raw!r}", env={"NULL_CAP": raw}, many={"as_arrays": True})
    lat = fake_lattice()
    out["receipt_many no queries"] = _plain([lat.receipt_many(np.zeros((0, 4), np.float32)),
                                             lat.receipt_many(np.zeros((0, 4), np.float32), as_arrays=True)])

    def bundle_call(name, *args):  # osc_bundle_many: ids, score, align behind (P, Q, kk, alpha, lambda)
        q_n, kk = args[1], args[2]
        _fill(args[5], [(5 * t) % 6 for t in range(q_n * kk)])
        _fill(args[6], [(t + 1) / 3.0 for t in range(q_n * kk)])
        _fill(args[7], [-(t + 1) / 7.0 for t in range(q_n * kk)])

    lat = fake_lattice()
    lat._call = bundle_call
    out["bundle_many lists"] = _plain(lat.bundle_many(queries(2, 4), k=3))
    out["bundle_many arrays"] = _plain(lat.bundle_many(queries(2, 4), k=3, as_arrays=True))
    out["bundle_many no queries"] = _plain(lat.bundle_many(np.zeros((0, 4), np.float32), k=3))


# ----------------------------------------------------------------------------------------------------------------- corpus
def fake_corpus(K=5, kk=3, totals=(4, 1)):
    """A Corpus with no device behind it (N = 50, D = 8) whose `_call` serves the four refine entry points."""
    from oscillink_amd.corpus import Corpus

    c = Corpus.__new__(Corpus)
    c._h, c.N, c.D = object(), 50, 8
    c.events = []

    def call(name, *args):
        c.events.append([name, _scalars(args)])
        q_n = args[1]
        gated = name != "osc_corpus_refine"
        first = {"osc_corpus_refine": 13, "osc_corpus_refine_gated": 19, "osc_corpus_refine_receipts": 26,
                 "osc_corpus_refine_chains": 31}[name]
        o = list(args[first:])
        cand = o.pop(0)
        gates = o.pop(0) if gated else None
        local, score, align, iters, res = o[:5]
        o = o[5:]
        _fill(cand, [(7 * t + 3) % 50 for t in range(q_n * K)])
        _fill(gates, [((3 * t) % 5) / 4.0 for t in range(q_n * K)])
        _fill(local, [(2 * t + 1) % K for t in range(q_n * kk)])
        _fill(score, [(t + 1) / 3.0 for t in range(q_n * kk)])
        _fill(align, [-(t + 1) / 7.0 for t in range(q_n * kk)])
        _fill(iters, [5 + q for q in range(q_n)])
        _fill(res, [(q + 1) / 15000.0 for q in range(q_n)])  # the second query misses the 1e-4 of ustar_converged
        if gated:
            _fill(o.pop(0), [3 + q for q in range(q_n)])
            _fill(o.pop(0), [(q + 1) / 70000.0 for q in range(q_n)])
        if name in ("osc_corpus_refine", "osc_corpus_refine_gated"):
            return
        detail, cap = args[23], args[25]
        (s_iters, s_res, s0, s1, s2, s3, total, offsets, ni, nj, nz, nr, capacity, nnz, pairs, pairs_n,
         prefix_cap), o = o[:17], o[17:]
        if detail >= 0:
            _fill(s_iters, [2 + q for q in range(q_n)])
            _fill(s_res, [(q + 1) / 9000.0 for q in range(q_n)])
            at = 0
            for q in range(q_n):
                for t, s in enumerate((s0, s1, s2, s3)):
                    s[q] = (0.1 * (t + 1) + q) / 3.0 if (t == 0 or detail == 1) else 0.0
                tot = totals[q % len(totals)] if detail == 1 else 0
                kept = min(tot, cap) if cap > 0 else tot
                total[q] = tot
                for e in range(kept):
                    assert at < capacity
                    ni[at], nj[at], nz[at], nr[at] = e, K - 1 - e, 9.5 - e - q / 3.0, (1 + e) / 7.0
                    at += 1
                offsets[q + 1] = at
                if nnz is not None:
                    nnz[q] = 8 + 2 * q
                    pairs_n[q] = 3 + q
                    for e in range(3 + q):
                        pairs[(q * prefix_cap + e) * 2], pairs[(q * prefix_cap + e) * 2 + 1] = e, (e + 1 + q) % K
        if name == "osc_corpus_refine_chains":
            z_s, z_p, r_s, r_p, gain, verdict, weak_k, weak_z = o
            off = args[26]
            for q in range(q_n):
                n_e = max(int(off[q + 1] - off[q]) - 1, 0)
                e0 = sum(max(int(off[t + 1] - off[t]) - 1, 0) for t in range(q))
                for e in range(n_e):
                    z_s[e0 + e], z_p[e0 + e] = (e + 1) / 3.0, -(e + 1) / 3.0
                    r_s[e0 + e], r_p[e0 + e] = (e + 1) / 7.0, (e + 2) / 7.0
                if n_e:
                    gain[q], verdict[q], weak_k[q], weak_z[q] = 1.0 / 3.0, 1, n_e - 1, 2.0 / 3.0

    c._call = call
    return c


def _corpus_cases(out):
    K = 5
    given = (np.arange(2 * K, dtype=np.float32).reshape(2, K) % 4) / 4.0

    def one(name, env=None, **kw):
        with _env(**(env or {})):
            c = fake_corpus()
            try:
                out[name] = {"result": _plain(c.refine_many(queries(2, 8), K, k=3, **kw)), "events": c.events}
            finally:
                c._h = None

    one("refine_many lists")
    one("refine_many arrays")
    one("refine_many lists diffusion gates", gates="diffusion")
    one("refine_many arrays given gates", gates=given, as_arrays=True)
    one("refine_many receipts light", receipts="light")
    one("refine_many receipts full", receipts="full")
    one("refine_many receipts full arrays", receipts="full", as_arrays=True)
    one("refine_many receipts light arrays", receipts="light", as_arrays=True)
    one("refine_many receipts full given gates", receipts="full", gates=given)
    one("refine_many receipts light diffusion gates", receipts="light", gates="diffusion", deterministic_k=True)
    one("refine_many chains receipts full", receipts="full", chains=[[0, 1, 2], None])
    one("refine_many chains receipts light gates", receipts="light", chains=[[0, 1, 2], None], gates=given, lamP=0.3)
    one("refine_many chains receipts full arrays", receipts="full", chains=[[0, 1, 2], None], as_arrays=True)
    one("refine_many chains lists", chains=[[0, 1, 2], None])
    one("refine_many chains arrays", chains=[[0, 1, 2], None], as_arrays=True)
    one("refine_many receipts full null cap 3", env={"NULL_CAP": "3"}, receipts="full")
    one("refine_many receipts full null cap 3 arrays", env={"NULL_CAP": "3"}, receipts="full", as_arrays=True)
    for raw in ("", "abc", "-3", " 7 "):
        one(f"refine_many null cap {raw!r}", env={"NULL_CAP": raw}, receipts="full", as_arrays=True)
    c = fake_corpus()
    out["refine_many no queries"] = _plain([c.refine_many(np.zeros((0, 8), np.float32), K, receipts="full"),
                                            c.refine_many(np.zeros((0, 8), np.float32), K, receipts="full", as_arrays=True)])
    c._h = None


def psis_errors():
    """The two psis messages from each of the three callers."""
    lat, c = fake_lattice(D=8), fake_corpus()
    bad = queries(3, 8)
    bad[1, 2] = np.inf
    out = {}
    for who, fn in (("bundle_many", lat.bundle_many), ("receipt_many", lat.receipt_many),
                    ("refine_many", lambda p: c.refine_many(p, 5)), ("search", lambda p: c.search(p, 5))):
        got = []
        for p in (np.zeros((2, 7), np.float32), np.zeros(8, np.float32), bad):
            with pytest.raises(ValueError) as e:
                fn(p)
            got.append(str(e.value))
        out[who] = got
    c._h = None
    return out


def cases():
    out = {}
    _lattice_cases(out)
    _corpus_cases(out)
    out["psis errors"] = psis_errors()
    return {k: json.dumps(v) for k, v in out.items()}


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def built():
    return cases()


def test_every_case_is_recorded(recorded, built):
    assert list(built) == list(recorded)


def test_records_equal_the_parents_byte_for_byte(recorded, built):
    for name, text in built.items():
        assert text == recorded[name], name


def test_cases_exercise_what_they_claim(built):
    """The stubs do reach the interesting branches: the cap drops points, the stable sort keeps row 1 then row 0, the sums
    are rounded to float32, a signature and dynamics are present, a query fails ustar_converged."""
    r = json.loads(built["receipt null cap 2 of 4"])["result"]
    assert [p["edge"][0] for p in r["null_points"]] == [1, 0]
    assert r["meta"]["null_points_summary"] == {"total_null_points": 4, "returned_null_points": 2, "null_cap_applied": True}
    many = json.loads(built["receipt_many full"])["result"]
    assert [len(m["null_points"]) for m in many] == [2, 1]
    assert many[1]["coh_drop_sum"] == float(np.float32((0.2 + 1) / 3.0)) != (0.2 + 1) / 3.0
    assert many[0]["meta"]["ustar_source"] == "query_basis" and "ustar_source" not in r["meta"]
    ext = json.loads(built["receipt_many extended signature dynamics"])["result"][0]["meta"]
    assert ext["signature"]["payload"]["mode"] == "extended" and ext["dynamics"] == DYNAMICS
    assert list(ext)[-2:] == ["signature", "dynamics"]
    ref = json.loads(built["refine_many chains receipts full"])["result"]
    assert [x["receipt"]["meta"]["ustar_converged"] for x in ref] == [True, False]
    assert ref[0]["chain_receipt"]["edges"][1]["edge"] == [1, 2] and ref[1]["chain_receipt"] is None
    capped = json.loads(built["refine_many receipts full null cap 3"])["result"]
    assert capped[0]["receipt"]["meta"]["null_points_summary"]["null_cap_applied"] is True
    assert len(capped[0]["receipt"]["null_points"]) == 3


def test_null_cap_reaches_the_native_calls_as_0_0_0_7(built):
    for raw, want in (("", 0), ("abc", 0), ("-3", 0), (" 7 ", 7)):
        ev = json.loads(built[f"receipt_many null cap {raw!r}"])["events"]
        assert [e[1][3] for e in ev if e[0] == "osc_receipt_many"] == [want]  # (Q, full, z_th, cap, capacity)
        ev = json.loads(built[f"refine_many null cap {raw!r}"])["events"]
        assert [e[1][-3] for e in ev] == [want]  # (.., detail, z_th, cap, capacity, prefix cap)


def test_null_cap_parse():
    from oscillink_amd import _receipts as rc

    for raw, want in (("", 0), ("abc", 0), ("-3", 0), (" 7 ", 7)):
        with _env(NULL_CAP=raw):
            assert rc.null_cap() == want
    with _env():
        assert rc.null_cap() == 0


def test_psis_errors_are_the_same_text_from_every_caller(built):
    got = json.loads(built["psis errors"])
    assert got["bundle_many"] == got["receipt_many"] == got["refine_many"] == got["search"]
    assert got["search"][0] == "psis must be a (Q, 8) array, got shape (2, 7)"
    assert got["search"][2] == "psis row 1 is not finite"


if __name__ == "__main__":  # --record: write the fixture from whichever oscillink_amd comes first on the path
    sys.path.append(ROOT)
    if "--record" in sys.argv:
        with open(FIXTURE, "w") as f:
            json.dump(cases(), f, indent=0)
            f.write("\n")

"""`bundle_many`, `receipt_many` and `_mmr_many` (csrc/query_kernels.hip, csrc/receipt_many_kernels.hip, csrc/osc_query.hip)
at the seams of their kernels -- column widths beyond one 256-column trip, masked4 tails, the GEMM's K padding, more
than 64 / 128 / 256 queries, rows with more than 64 neighbours, row counts around the 128-row tile -- against two
float64 references that share no code with the kernels (tests/_query_seams.py, whose tables name what each entry reaches).

Gates.  Reference A (dense float64 solve of the lattice's own operator, end to end): ids equal up to the first MMR step
whose float64 margin is below NEAR_TIE = 1e-4, score and align within 2e-4 up to that step, the three sums within 1e-4 by
the relative rule of test_gpu_receipt_many.test_fixtures_against_yardstick_and_loop, deltaH_total within 1e-4 relative,
null points different only on rows whose float64 margin is below NEAR = 1e-3.  Reference B (float64 from the device's
own float32 basis: the CG solve drops out): the same id and null-point rules with margins from float64, and
`qs.B_TOL` on score, align, the sums and deltaH -- twice the distance of a plain float32 numpy evaluation from float64,
measured on the CPU (tests/test_query_seams_host.py).  In every batch at most one query in four is compared over fewer
than all k steps and at least one in full, per reference.

MEASURED below holds what the tests printed on an MI355X (a record, no assertion reads it)."""
import hashlib

import numpy as np
import pytest

from tests import _query_seams as qs
from tests import _queries as yq
from tests import _receipt_yardstick as yr

pytestmark = pytest.mark.gpu

# case id -> the largest distances the tests printed on an MI355X, over the states run:
#   (score from A, align from A, score from B, align from B, sums from A, deltaH from A, sums from B, deltaH from B)
# score / align absolute, sums by the relative rule, deltaH relative.  Bounds: A 2e-4 / 2e-4 / 1e-4 / 1e-4, B qs.B_TOL =
# 5.86e-6 / 5.7e-7 / 4.58e-7 / 4.84e-7.
MEASURED = {
    "width-d3-plain": (9.8e-07, 5.2e-07, 4.6e-07, 6.9e-08, 5.5e-08, 3.6e-08, 4.9e-08, 4.0e-08),
    "width-d5-plain": (8.1e-07, 1.2e-07, 7.5e-07, 3.1e-08, 1.5e-07, 8.7e-08, 4.9e-08, 5.2e-08),
    "width-d33-plain": (3.4e-07, 4.4e-08, 3.6e-07, 3.0e-08, 2.4e-07, 1.2e-07, 3.5e-08, 4.7e-08),
    "width-d255-plain": (6.1e-07, 5.1e-08, 6.0e-07, 2.7e-08, 3.2e-07, 1.3e-07, 3.9e-08, 5.6e-08),
    "width-d257-plain": (6.4e-07, 3.6e-08, 4.5e-07, 3.0e-08, 1.2e-07, 5.3e-08, 4.8e-08, 5.0e-08),
    "width-d261-plain": (2.8e-07, 3.4e-08, 2.9e-07, 3.0e-08, 1.0e-07, 8.0e-08, 4.8e-08, 4.4e-08),
    "width-d261-gates_chain": (4.0e-07, 4.0e-08, 4.4e-07, 2.9e-08, 1.1e-07, 1.1e-07, 5.4e-08, 6.4e-08),
    "width-d515-plain": (5.1e-07, 3.1e-08, 5.0e-07, 2.9e-08, 2.0e-07, 6.8e-08, 5.0e-08, 4.3e-08),
    "width-d768-plain": (4.4e-07, 4.4e-08, 4.0e-07, 2.9e-08, 4.4e-07, 1.4e-07, 5.1e-08, 3.5e-08),
    "width-d772-plain": (3.3e-07, 3.7e-08, 3.4e-07, 3.0e-08, 1.5e-07, 5.9e-08, 4.8e-08, 3.5e-08),
    "width-d772-gates_chain": (7.8e-07, 1.6e-07, 4.2e-07, 3.2e-08, 8.5e-08, 6.7e-08, 3.3e-08, 4.7e-08),
    "queries-gates_chain_n333_d50_k7-q1": (1.7e-06, 9.5e-08, 3.6e-07, 2.8e-08, 1.8e-08, 1.8e-08, 2.0e-08, 2.2e-08),
    "queries-gates_chain_n333_d50_k7-q2": (1.7e-06, 1.3e-07, 4.2e-07, 3.0e-08, 1.1e-07, 7.7e-08, 4.2e-08, 1.8e-08),
    "queries-gates_chain_n333_d50_k7-q63": (2.1e-06, 2.1e-07, 5.0e-07, 3.7e-08, 2.6e-07, 1.3e-07, 5.4e-08, 6.1e-08),
    "queries-gates_chain_n333_d50_k7-q64": (1.7e-06, 2.2e-07, 5.0e-07, 3.7e-08, 7.9e-08, 2.9e-08, 5.4e-08, 6.1e-08),
    "queries-gates_chain_n333_d50_k7-q65": (2.0e-06, 2.2e-07, 5.0e-07, 3.7e-08, 7.9e-08, 2.9e-08, 5.4e-08, 6.1e-08),
    "queries-gates_chain_n333_d50_k7-q127": (2.0e-06, 3.3e-07, 5.4e-07, 4.0e-08, 7.9e-08, 2.9e-08, 5.4e-08, 6.1e-08),
    "queries-gates_chain_n333_d50_k7-q128": (2.0e-06, 2.2e-07, 5.4e-07, 4.0e-08, 1.8e-07, 9.3e-08, 5.4e-08, 6.1e-08),
    "queries-gates_chain_n333_d50_k7-q129": (2.0e-06, 2.2e-07, 5.4e-07, 4.0e-08, 1.8e-07, 9.3e-08, 5.4e-08, 6.1e-08),
    "queries-gates_chain_n333_d50_k7-q255": (2.0e-06, 2.2e-07, 5.4e-07, 4.0e-08, 1.8e-07, 9.3e-08, 5.4e-08, 6.1e-08),
    "queries-gates_chain_n333_d50_k7-q256": (2.0e-06, 3.2e-07, 5.4e-07, 4.0e-08, 4.4e-07, 1.6e-07, 5.4e-08, 6.1e-08),
    "queries-gates_chain_n333_d50_k7-q257": (2.0e-06, 3.3e-07, 5.4e-07, 4.0e-08, 4.4e-07, 1.6e-07, 5.4e-08, 6.1e-08),
    "queries-gates_chain_n333_d50_k7-q300": (2.0e-06, 3.3e-07, 5.6e-07, 4.0e-08, 4.4e-07, 1.6e-07, 5.4e-08, 6.1e-08),
    "queries-n333_d261-q1": (3.3e-07, 2.9e-08, 3.1e-07, 2.8e-08, 1.7e-07, 8.2e-08, 5.2e-08, 4.3e-08),
    "queries-n333_d261-q2": (3.3e-07, 3.1e-08, 3.4e-07, 2.9e-08, 6.2e-08, 4.1e-08, 5.2e-08, 3.2e-08),
    "queries-n333_d261-q63": (4.0e-07, 3.1e-08, 5.5e-07, 3.0e-08, 5.2e-08, 4.1e-08, 5.5e-08, 5.0e-08),
    "queries-n333_d261-q64": (3.3e-07, 3.1e-08, 5.5e-07, 3.0e-08, 5.2e-08, 3.8e-08, 5.5e-08, 5.0e-08),
    "queries-n333_d261-q65": (3.8e-07, 3.1e-08, 5.5e-07, 3.0e-08, 5.2e-08, 4.8e-08, 5.5e-08, 5.0e-08),
    "queries-n333_d261-q127": (3.8e-07, 3.1e-08, 5.8e-07, 3.0e-08, 5.4e-08, 5.4e-08, 5.7e-08, 5.5e-08),
    "queries-n333_d261-q128": (3.8e-07, 3.1e-08, 5.8e-07, 3.0e-08, 5.2e-08, 4.8e-08, 5.7e-08, 5.5e-08),
    "queries-n333_d261-q129": (5.2e-07, 3.1e-08, 5.8e-07, 3.0e-08, 5.2e-08, 5.2e-08, 5.7e-08, 5.5e-08),
    "queries-n333_d261-q255": (5.2e-07, 3.1e-08, 5.9e-07, 3.1e-08, 5.2e-08, 5.2e-08, 5.8e-08, 5.5e-08),
    "queries-n333_d261-q256": (5.2e-07, 3.1e-08, 5.9e-07, 3.1e-08, 5.2e-08, 5.2e-08, 5.8e-08, 5.5e-08),
    "queries-n333_d261-q257": (5.2e-07, 3.7e-08, 5.9e-07, 3.1e-08, 5.2e-08, 5.2e-08, 5.8e-08, 5.5e-08),
    "queries-n333_d261-q300": (5.2e-07, 3.7e-08, 5.9e-07, 3.1e-08, 5.2e-08, 5.2e-08, 5.8e-08, 5.5e-08),
    "rows-n127": (4.8e-07, 7.4e-08, 4.5e-07, 3.0e-08, 7.4e-08, 5.5e-08, 4.8e-08, 5.0e-08),
    "rows-n128": (3.5e-07, 5.3e-08, 3.1e-07, 2.8e-08, 6.4e-07, 1.7e-07, 4.7e-08, 4.5e-08),
    "rows-n129": (3.4e-07, 5.1e-08, 3.1e-07, 3.2e-08, 4.7e-07, 1.6e-07, 5.3e-08, 4.8e-08),
    "rows-n130": (3.0e-07, 4.4e-08, 2.8e-07, 3.0e-08, 3.5e-07, 1.1e-07, 5.3e-08, 4.3e-08),
    "rows-n257": (4.4e-07, 4.0e-08, 4.6e-07, 3.0e-08, 4.0e-07, 1.1e-07, 5.4e-08, 4.8e-08),
    "rows-n513": (3.4e-07, 6.5e-08, 3.3e-07, 2.9e-08, 1.3e-07, 5.3e-08, 5.8e-08, 4.9e-08),
    "degree-built-k70": (5.1e-07, 1.6e-07, 5.8e-07, 3.3e-08, 1.7e-07, 6.8e-08, 5.5e-08, 5.4e-08),
    "degree-built-k140": (5.8e-07, 7.0e-08, 5.8e-07, 3.2e-08, 1.8e-07, 8.0e-08, 4.8e-08, 5.5e-08),
    "degree-hub64-d32": (9.1e-07, 8.8e-08, 3.5e-07, 3.0e-08, 7.5e-07, 6.0e-08, 1.6e-07, 5.1e-08),
    "degree-hub64-d261": (4.7e-07, 5.6e-08, 3.9e-07, 3.0e-08, 5.9e-08, 5.7e-08, 5.6e-08, 5.5e-08),
    "degree-hub65-d32": (6.3e-07, 9.5e-08, 2.9e-07, 3.2e-08, 3.8e-07, 1.3e-07, 6.3e-08, 5.7e-08),
    "degree-hub65-d261": (5.8e-07, 5.7e-08, 3.8e-07, 3.0e-08, 1.7e-07, 7.6e-08, 6.2e-08, 5.5e-08),
    "degree-hub120-d32": (5.3e-07, 1.3e-07, 5.2e-07, 3.0e-08, 1.1e-07, 5.7e-08, 5.7e-08, 5.7e-08),
    "degree-hub120-d261": (5.0e-07, 6.6e-08, 5.0e-07, 3.0e-08, 8.7e-08, 5.1e-08, 6.0e-08, 5.2e-08),
    "degree-hub128-d32": (4.8e-07, 6.0e-08, 4.7e-07, 3.0e-08, 2.0e-07, 6.0e-08, 5.3e-08, 4.4e-08),
    "degree-hub128-d261": (5.3e-07, 5.8e-08, 5.3e-07, 3.0e-08, 2.0e-07, 7.1e-08, 5.8e-08, 5.6e-08),
    "degree-empty_rows-d32": (4.0e-07, 6.6e-08, 3.7e-07, 3.1e-08, 1.0e-06, 6.1e-08, 5.6e-08, 4.8e-08),
    "degree-empty_rows-d261": (3.3e-07, 5.4e-08, 3.4e-07, 3.0e-08, 5.2e-07, 2.2e-07, 5.9e-08, 5.6e-08),
}

A_TOL = (qs.A_ATOL, qs.A_ATOL)
B_TOL = (qs.B_TOL["score"], qs.B_TOL["align"])


@pytest.fixture(scope="module")
def amd():
    import oscillink_amd
    from oscillink_amd import _native

    assert _native.device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return oscillink_amd


@pytest.fixture(autouse=True)
def _plain_env(monkeypatch):
    for k in ("OSCILLINK_RECEIPT_NULL_CAP", "OSCILLINK_RECEIPT_DYNAMICS"):
        monkeypatch.delenv(k, raising=False)


# ------------------------------------------------------------------------------------------------------------ references
class _Refs:
    """float64 answers per query of one lattice and one basis, computed on first use and kept"""

    def __init__(self, s, X, x, P):
        self.s, self.X, self.x, self.P = s, np.asarray(X, np.float64), np.asarray(x, np.float64), P
        self._bundle, self._receipt = {}, {}

    def bundle(self, q):
        if q not in self._bundle:
            self._bundle[q] = qs.bundle64(self.s, qs.ustar(self.X, self.x, self.P[q]), self.P[q])
        return self._bundle[q]

    def receipt(self, q, state, U):
        if (q, state) not in self._receipt:
            self._receipt[(q, state)] = qs.receipt(self.s, U, qs.ustar(self.X, self.x, self.P[q]), self.P[q])
        return self._receipt[(q, state)]


def _check_bundles(got, refs, queries, atol, what):
    """ids up to the first near tie, score and align up to there (atol: one bound each); returns the largest
    (score, align) distances and what missed (asserted by the caller once the figures are printed).  Asserts the cap."""
    ids, score, align = got
    truncated, dist, missed = 0, (0.0, 0.0), []
    for q in queries:
        w_ids, w_score, w_align, margins = refs.bundle(q)
        n = qs.full_steps(margins)
        truncated += int(n < len(w_ids))
        assert ids.shape[1] == len(w_ids), (what, q)
        assert ids[q, :n].tolist() == w_ids[:n], (what, q, ids[q].tolist(), w_ids, margins)
        if n:
            d = (float(np.max(np.abs(score[q, :n] - w_score[:n]))), float(np.max(np.abs(align[q, :n] - w_align[:n]))))
            if not (d[0] <= atol[0] and d[1] <= atol[1]):
                missed.append((what, q, d, atol))
            dist = (max(dist[0], d[0]), max(dist[1], d[1]))
    assert qs.cap_holds(truncated, len(queries)), (what, truncated, len(queries))
    return dist, missed


def _check_receipts(got, refs, queries, state, U, tol_sums, tol_dH, what, nulls=True):
    """the three sums, deltaH_total and (nulls=True) the null points; returns the largest (sums, deltaH) distances and
    what missed its bound (asserted by the caller once the figures are printed)"""
    d_sums = d_dH = 0.0
    missed = []
    for q in queries:
        want = refs.receipt(q, state, U)
        ds = qs.sums_distance(got[q], want)
        dh = abs(got[q]["deltaH_total"] - want["deltaH"]) / abs(want["deltaH"])
        if not ds <= tol_sums:
            missed.append((what, q, ds, tol_sums, {k: (got[q][k], want[k]) for k in qs.SUMS}))
        if not dh <= tol_dH:
            missed.append((what, q, dh, tol_dH, got[q]["deltaH_total"], want["deltaH"]))
        d_sums, d_dH = max(d_sums, ds), max(d_dH, dh)
        if nulls:
            g = yr.null_edges(got[q]["null_points"])
            bad = [i for i in set(g) | set(want["nulls"]) if g.get(i) != want["nulls"].get(i) and want["margin"][i] >= qs.NEAR]
            assert not bad, (what, q, bad[:5])
            assert got[q]["meta"]["null_points_summary"]["total_null_points"] == len(got[q]["null_points"])
    return (d_sums, d_dH), missed


def _report(case_id, call, a, b):
    print(f"\nseams {case_id} {call}: from A " + " ".join(f"{v:.3e}" for v in a) + " | from B " + " ".join(f"{v:.3e}" for v in b))


def _both_references(lat, Y, P):
    s = qs.setup_of_lattice(lat, Y)
    return s, _Refs(s, *s.basis64(), P)


def _run_case(amd, c, states=("fresh", "settled")):
    """bundle_many(k = 8) and receipt_many of one table entry in the given states against both references"""
    lat, Y, P = qs.lattice_of(amd, c)
    s, ref_a = _both_references(lat, Y, P)
    every = range(P.shape[0])
    ref_b = None
    for state in states:
        if state == "settled":
            lat.settle(max_iters=12, tol=1e-3)
        U = lat.U.astype(np.float64)
        got = lat.bundle_many(P, k=qs.K, alpha=qs.ALPHA, as_arrays=True)
        assert lat.last_query_basis["converged"]
        if ref_b is None:
            ref_b = _Refs(s, *lat.query_basis(), P)
        a, miss_a = _check_bundles(got, ref_a, every, A_TOL, (c["id"], state, "A"))
        b, miss_b = _check_bundles(got, ref_b, every, B_TOL, (c["id"], state, "B"))
        _report(c["id"], f"bundle_many {state}", a, b)
        assert not miss_a + miss_b, (miss_a + miss_b)[:3]
        rec = lat.receipt_many(P)
        assert len(rec) == P.shape[0]
        ra, miss_a = _check_receipts(rec, ref_a, every, state, U, qs.A_RTOL, qs.A_RTOL, (c["id"], state, "A"))
        rb, miss_b = _check_receipts(rec, ref_b, every, state, U, qs.B_TOL["sums"], qs.B_TOL["deltaH"], (c["id"], state, "B"))
        _report(c["id"], f"receipt_many {state}", ra, rb)
        assert not miss_a + miss_b, (miss_a + miss_b)[:3]
    return lat


# ----------------------------------------------------------------------------------------------------------- 1. widths
@pytest.mark.parametrize("D,variant", [(D, v) for D, v, _, _ in qs.WIDTHS], ids=lambda v: str(v))
def test_column_widths(amd, D, variant):
    _run_case(amd, qs.case(f"width-d{D}-{variant}"))


# ------------------------------------------------------------------------------------------------------ 2. query counts
_QUERY_LATTICES = {}


def _query_lattice(amd, name):
    """one lattice per name for the whole module, with reference A and (per state of the basis' x) reference B"""
    if name not in _QUERY_LATTICES:
        lat, Y, P = qs.lattice_of(amd, qs.case(f"queries-{name}"))
        s, ref_a = _both_references(lat, Y, P)
        _QUERY_LATTICES[name] = (lat, s, P, ref_a, {})
    return _QUERY_LATTICES[name]


def _reference_b(lat, s, P, cache):
    """reference B of the resident basis (a batch with a larger |psi|_inf solves x again: one reference per x)"""
    X, x = lat.query_basis()
    key = hashlib.sha256(X.tobytes() + x.tobytes()).hexdigest()
    if key not in cache:
        cache[key] = _Refs(s, X, x, P)
    return cache[key]


@pytest.mark.parametrize("Q", [n for n, _ in qs.QUERY_COUNTS])
@pytest.mark.parametrize("name", list(qs.QUERY_LATTICES))
def test_query_counts(amd, name, Q):
    """Every query of the batch against reference B, queries 0, 63, 64, 127, 128, 255, 256 and Q - 1 against reference A;
    at Q = 65, 129 and 257 the null points of every query (lane slots u >= 1), otherwise those of the A queries."""
    lat, s, Pall, ref_a, cache = _query_lattice(amd, name)
    P = Pall[:Q]
    U = lat.U.astype(np.float64)
    got = lat.bundle_many(P, k=qs.K, alpha=qs.ALPHA, as_arrays=True)
    assert lat.last_query_basis["converged"]
    ref_b = _reference_b(lat, s, Pall, cache)
    sel, every = qs.a_queries(Q), range(Q)
    cid = f"queries-{name}-q{Q}"
    a, miss_a = _check_bundles(got, ref_a, sel, A_TOL, (cid, "A"))
    b, miss_b = _check_bundles(got, ref_b, every, B_TOL, (cid, "B"))
    _report(cid, "bundle_many", a, b)
    assert not miss_a + miss_b, (miss_a + miss_b)[:3]
    rec = lat.receipt_many(P)
    assert len(rec) == Q and _reference_b(lat, s, Pall, cache) is ref_b
    ra, miss_a = _check_receipts(rec, ref_a, sel, "fresh", U, qs.A_RTOL, qs.A_RTOL, (cid, "A"))
    rb, miss_b = _check_receipts(rec, ref_b, every, "fresh", U, qs.B_TOL["sums"], qs.B_TOL["deltaH"], (cid, "B"), nulls=False)
    _report(cid, "receipt_many", ra, rb)
    assert not miss_a + miss_b, (miss_a + miss_b)[:3]
    _check_receipts(rec, ref_b, every if Q in qs.EXTENDED_Q else sel, "fresh", U, qs.B_TOL["sums"], qs.B_TOL["deltaH"],
                    (cid, "B nulls"))


# -------------------------------------------------------------------------------------------------------- 3. row counts
@pytest.mark.parametrize("N", [n for n, _, _ in qs.ROWS])
def test_row_counts(amd, N):
    _run_case(amd, qs.case(f"rows-n{N}"))


# ----------------------------------------------------------------------------------------------------------- 4. degrees
@pytest.mark.parametrize("knn,more_than", [(k, m) for k, m, _, _ in qs.DEG_BUILT])
def test_degrees_above_64_on_the_built_graph(amd, knn, more_than):
    lat = _run_case(amd, qs.case(f"degree-built-k{knn}"), states=("fresh",))
    assert int(np.diff(lat.graph_csr()[0]).max()) > more_than


@pytest.mark.parametrize("kind,D", [(k, D) for k, D, _ in qs.DEG_INJECTED])
def test_degrees_on_injected_graphs(amd, kind, D):
    """A hub row of exactly 64, 65, 120 and 128 neighbours and a graph of mostly empty rows, through `set_graph_csr`.

    [hub64-32] found the one defect of this module: with the row constant s_i = x_i / (sqrt_deg_i + 1e-12) rounded to
    float32 (k_query_basis_stats), coh_drop_sum of query 1 (the one scaled by 3) was 117.875084 against 117.875203 in
    float64 from the same device basis: 1.006e-6 by the relative rule where reference B allows 4.58e-7.  (s_i - s_j)^2
    |psi|^2 carries that one rounding through all D columns of the row, where a plain float32 evaluation rounds column by
    column; rounding s alone in an otherwise float64 evaluation on the CPU gave 1.20e-6, rounding p alone 8.6e-9.  This
    graph has rows whose single edge weighs about 0.05 (s about 4) next to |psi|^2 = 288.  s is fp64 now: 1.6e-7."""
    lat = _run_case(amd, qs.case(f"degree-{kind}-d{D}"), states=("fresh",))
    deg = np.diff(lat.graph_csr()[0])
    if kind.startswith("hub"):
        assert int(deg[qs.HUB]) == int(kind[3:]) == int(deg.max())
    else:
        assert np.count_nonzero(deg == 0) > lat.N // 2


# ---------------------------------------------------------------------------------------------------------- 5. _mmr_many
@pytest.mark.parametrize("Q", qs.MMR_Q)
@pytest.mark.parametrize("N,D,seed", qs.MMR_SHAPES, ids=lambda v: str(v))
def test_mmr_many_at_the_seams(amd, N, D, seed, Q):
    Y = qs.anchors(N, D, seed)
    lat = amd.Oscillink(Y, kneighbors=6, deterministic_k=True)
    S = qs.mmr_scores(N, Q, seed)
    k = qs.MMR_K
    got = lat._mmr_many(S, k, 0.5)
    assert got.shape == (Q, k)
    truncated = 0
    for q in range(Q):
        ids = got[q].tolist()
        assert len(set(ids)) == k and min(ids) >= 0 and max(ids) < N, (q, ids)
        assert ids[0] == int(np.argmax(S[:, q])), (q, ids)  # no similarity yet: the first maximum, smaller id on a tie
        want, margins = yq.mmr(Y, S[:, q], k, 0.5)
        ok, cut = yq.same_until_near_tie(ids, want, margins, 1e-6)
        assert ok, (q, ids, want, margins)
        truncated += int(cut)
        ok, _ = yq.same_until_near_tie(ids, lat._mmr(S[:, q], k, 0.5), margins, 1e-6)
        assert ok, (q, "per-column _mmr")
    # Equal scores: the first pick is row 0; after it the similarity term decides (checked against float64 above).  Without
    # that term (lambda_div = 0) ties alone decide and every list is the stable descending order: 0 ... 9 in those columns.
    flat = lat._mmr_many(S, k, 0.0)
    for q in range(Q):
        assert flat[q].tolist() == np.argsort(-S[:, q], kind="stable")[:k].tolist(), q
    for q in qs.equal_columns(Q):
        assert got[q, 0] == 0 and flat[q].tolist() == list(range(k)), q
    for c0 in range(0, Q, 64):
        if c0 + 4 < Q:
            assert got[c0 + 4, 0] == 7, c0  # rows 7 and 47 tie for the largest score
    print(f"\nseams mmr_many N {N} D {D} Q {Q}: {truncated} of {Q} id lists compared up to a near tie")


def test_mmr_many_picks_every_row_once(amd):
    N, D, seed = qs.MMR_SHAPES[2]
    Y = qs.anchors(N, D, seed)
    lat = amd.Oscillink(Y, kneighbors=6, deterministic_k=True)
    S = qs.mmr_scores(N, 65, seed)
    got = lat._mmr_many(S, N + 71, 0.5)
    assert got.shape == (65, N)
    for q in range(65):
        assert sorted(got[q].tolist()) == list(range(N)), q
    for q in qs.equal_columns(65):  # equal scores: the similarity term alone decides after the first pick
        want, margins = yq.mmr(Y, S[:, q], N, 0.5)
        assert yq.same_until_near_tie(got[q].tolist(), want, margins, 1e-6)[0], q


# -------------------------------------------------------------------------------------------------------- 6. independence
def _receipt_fields(r):
    return ([r["deltaH_total"]] + [r[k] for k in qs.SUMS],
            [(p["edge"], p["z"], p["residual"]) for p in r["null_points"]])


def test_independence_at_the_new_seams(amd):
    """Queries 0, 64, 128, 256 and Q - 1 of the 257-query batch at D = 261 give, run alone, the bytes they gave inside the
    batch; the batch run twice gives the same bytes."""
    lat, s, Pall, _, _ = _query_lattice(amd, "n333_d261")
    P = Pall[:257]
    big = lat.bundle_many(P, k=qs.K, as_arrays=True)
    rec = lat.receipt_many(P)
    again = lat.bundle_many(P, k=qs.K, as_arrays=True)
    rec2 = lat.receipt_many(P)
    for a, b in zip(big, again):
        assert np.array_equal(a, b)
    for q in range(257):
        assert _receipt_fields(rec[q]) == _receipt_fields(rec2[q]), q
    for q in (0, 64, 128, 256, 257 - 1):
        alone = lat.bundle_many(P[q:q + 1], k=qs.K, as_arrays=True)
        for a, b in zip(alone, big):
            assert np.array_equal(a[0], b[q]), q
        assert _receipt_fields(lat.receipt_many(P[q:q + 1])[0]) == _receipt_fields(rec[q]), q

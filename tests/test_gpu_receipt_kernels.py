"""The receipt kernels (receipt_kernels.hip: k_receipt_rows<NCH>, k_receipt_pairs<NCH>, k_receipt_finish) against the float64
yardstick of tests/_receipt_reference.py, at the shapes where launch_receipt_rows and receipt_rows() (osc_api.hip) branch.

Every lattice is created without a kNN build; `set_graph_csr` injects the case's graph, random gates in [0.1, 1] and a random
query follow, and a loose solve (tol 1e-3, at most 16 iterations) leaves a U* on the device.  The yardstick is evaluated on
THAT U* (fetched), so the CG is outside the comparison.  z_th is the median of the yardstick's z over the rows with an edge:
both outcomes of `z > z_th` occur, half and half.

Bounds (TOL = 1e-4: test_gpu_parity.py / test_gpu_dynamics.py; 1e-3 on z and R: _check_solves):
  |coh_dev - coh_ref| <= 1e-4 mag_i;  anchor, query: 1e-4 relative per row;  the three sums of receipt(): 1e-4 relative;
  a compared row has the yardstick's decision and column, its z and R to 1e-3 relative.  A row is left out of the null
  comparison only when its yardstick margin is below 1e-3, at most 2 % of the rows with an edge per case.
tests/test_receipt_reference_host.py shows float32 arithmetic to stay within a quarter of each bound on every case.

  case                 N     D     ld    chunks  kernel(s)
  row_d7 .. row_d2100  300   7..   8, 256, 260, 516, 772, 1024, 1028, 1536, 1540, 2100
                                         1 1 2 3 4 4 5 6 7 9   k_receipt_rows <1> <1> <2> <3> <4> <4> <6> (dead sixth chunk)
                                                               <6> <0> <0> (7 and 9 trips of 256 columns)
  row_d50_ld64         300   50    64    1       <1>, 14 pad columns
  row_d250_ld288       300   250   288   2       <2>, 38 pad columns that reach into the second chunk
  row_isolated         309   64    64    1       <1>, nine rows of degree 0
  row_hub              400   64    64    1       <1>, degrees 300 / 130 / 100 / 65
  pair_d7 .. d1536     4096  7..   8, 260, 516, 772, 1056, 1536
                                         1 2 3 4 5 6           k_receipt_pairs <1> <2> <3> <4> <6> <6> + k_receipt_finish
  pair_hub (_reversed) 4096  64    64    1       k_receipt_finish: mirror slots in c0 / c1 / the tail loop, up to 64 lower
                                                 neighbours per chunk, a last row of 300 lower neighbours (five e0 chunks)
The chunk count is ceil(ld / 256) with ld from the pitch rule documented in osc_create (osc_api.hip, "Row pitch"), restated in
_receipt_reference.pitch(); build_info() does not expose the pitch.  The pair form is receipt_rows()'s choice from N >= 4096
on (OSC_RECEIPT_PAIR unset).  Nothing reports which form ran: when k_receipt_finish misses a mirror slot it raises a flag and
receipt_rows() runs the one-launch kernel over the result, so a lookup that finds nothing shows in no output (a lookup that
finds the WRONG slot does, on the hub graphs).

Measured on an MI355X, the largest error of each kind over all cases as a fraction of its bound: coh 0.0026 (row_hub), anchor
0.0019, query 0.0019, the three sums 0.00083, z 0.00016, R 0.00034; at most 1.0 % of the rows with an edge left out (cap 2 %),
no compared row with another decision or column.  Slips tried on scratch builds: coh without its 0.5 -> all 22 tolerance
cases fail; `R >= rmax` -> the four exact-tie cases; s2 / deg for s2 / N -> every case; a c1 match placed at 0 + pos for
64 + pos -> both hub cases; c1 matches ignored -> nothing fails (the flag, then the one-launch kernel: see above)."""
import numpy as np
import pytest

from tests import _receipt_reference as RR

pytestmark = pytest.mark.gpu

SWITCHES = ("OSC_SPMM_XS", "OSC_REORDER", "OSC_SPMM_BLOCKED", "OSC_BLK_VARIANT", "OSC_BLK_INIT", "OSC_SMALL_PATH", "OSC_BALANCE",
            "OSC_BALANCE_HOST", "OSC_FAKE_COL_SHARD", "OSC_SHARD", "OSC_ROW_FAKE_SHARDS", "OSC_LD", "OSC_RECEIPT_PAIR")


@pytest.fixture(scope="module")
def amd():
    import oscillink_amd
    from oscillink_amd import _native

    assert _native.device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return oscillink_amd


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)


def _settled(amd, case, env=None):
    """(lattice, fetched U*) for a case; the switches are read when the lattice is created and when a graph is injected."""
    with pytest.MonkeyPatch.context() as mp:
        for v in SWITCHES:
            mp.delenv(v, raising=False)
        if case.osc_ld is not None:
            mp.setenv("OSC_LD", str(case.osc_ld))
        for k, v in (env or {}).items():
            mp.setenv(k, v)
        lamG, lamC, lamQ = RR.LAMS
        lat = amd.Oscillink(case.Y, kneighbors=4, lamG=lamG, lamC=lamC, lamQ=lamQ, _build_graph=False)
        lat.set_graph_csr(*case.graph)
    lat.set_query(case.psi, gates=case.B)
    Us = lat.solve_Ustar(tol=1e-3, max_iters=16).copy()
    assert np.all(np.isfinite(Us))
    return lat, Us


def _device_rows(lat, z_th):
    coh, anc, qry, (i, j, z, r, n) = lat._receipt_rows(z_th)
    return coh, anc, qry, i[:n].copy(), j[:n].copy(), z[:n].copy(), r[:n].copy()


def _check(amd, case, env=None):
    """One case against the yardstick; returns what the device gave, for the tests that compare two runs."""
    lat, Us = _settled(amd, case, env)
    rowptr, col, a, _, sd = lat.graph_csr()
    assert np.array_equal(rowptr, case.rowptr) and np.array_equal(col, case.col) and np.array_equal(a, case.a)
    ref = RR.receipt_reference(case.Y, Us, case.psi, case.B, rowptr, col, a, sd, *RR.LAMS)
    z_th = ref.median_z()
    coh, anc, qry, i, j, z, r = _device_rows(lat, z_th)
    lat.set_receipt_detail("full")
    rec = lat.receipt()
    res = RR.compare((coh, anc, qry, rec), ref, z_th, i, j, z, r)
    print(f"RECEIPT {case.name} N={case.N} D={case.D} ld={case.ld} chunks={case.nch} pair={case.pair} env={env} z_th={z_th:.4f}",
          {k: (float(f"{v:.3g}") if isinstance(v, float) else v) for k, v in res.items()})
    assert RR.within_bounds(res) == []
    n_edge = int(np.count_nonzero(ref.null_col >= 0))
    assert res["nulls_among_compared"] > 0.4 * n_edge and res["non_nulls_among_compared"] > 0.4 * n_edge
    lat.close()
    return Us, (coh, anc, qry, i, j, z, r), ref


@pytest.mark.parametrize("name", [n for n in RR.ROW_CASES if n.startswith("row_d")])
def test_row_kernel_at_every_width(amd, name):
    """N = 300 < 4096: always the one-launch form.  Degree 5 (odd: the EU = 2 loop's tail), random weights."""
    case = RR.build_case(name)
    assert not case.pair and case.nch == RR.CASES[name][2]
    _check(amd, case)


def test_row_kernel_rows_without_edges(amd):
    """Nine rows of degree 0 behind the circulant: coh = 0 and no null point, at the median z_th and at z_th = -1 (their z is
    0, which is above -1: only the missing argmax keeps them out of the list)."""
    case = RR.build_case("row_isolated")
    _check(amd, case)  # (within_bounds: coh == 0.0 and no null point on the rows without edges)
    lat, Us = _settled(amd, case)
    coh, anc, qry, i, j, z, r = _device_rows(lat, -1.0)
    assert np.all(coh[300:] == 0.0) and np.array_equal(i, np.arange(300))  # every row with an edge, none of the others
    ref = RR.receipt_reference(case.Y, Us, case.psi, case.B, case.rowptr, case.col, case.a, case.sqrt_deg(), *RR.LAMS)
    assert np.all(ref.null_z[300:] == 0.0) and np.all(ref.null_col[300:] == -1)
    # at z_th = -1 every row with an edge reports its z and R: all 300 against the yardstick (gap margin as in the tier)
    _, margin = ref.decide(-1.0)
    ok = margin[:300] >= RR.MARGIN
    assert np.count_nonzero(~ok) <= RR.LEFT_OUT_CAP * 300 and np.array_equal(j[ok], ref.null_col[:300][ok])
    assert np.allclose(z[ok], ref.null_z[:300][ok], rtol=RR.Z_RTOL, atol=0.0)
    assert np.allclose(r[ok], ref.null_R[:300][ok], rtol=RR.Z_RTOL, atol=0.0)


def test_row_kernel_on_the_hub_graph(amd):
    """ELL width 300 at N = 400: rows of 300, 130, 100 and 65 edges through the one-launch kernel (dense-row z statistics in
    double over long rows, the float32 coh sum over 300 edges in order)."""
    _check(amd, RR.build_case("row_hub"))


@pytest.mark.parametrize("name", [n for n in RR.PAIR_CASES if n.startswith("pair_d")])
def test_pair_form_at_every_width(amd, name):
    """N = 4096: the smallest lattice that takes the pair form; one case per k_receipt_pairs instantiation."""
    case = RR.build_case(name)
    assert case.pair and case.nch == RR.CASES[name][2]
    _check(amd, case)


@pytest.mark.parametrize("name", RR.HUB_CASES)
def test_pair_form_on_hub_graphs_and_against_the_one_launch_form(amd, name):
    """k_receipt_finish where its lookups branch (tests/test_receipt_reference_host.py counts them per graph): mirror slots
    found in c0, in c1 (positions 64..127) and by the tail loop (>= 128), 64 lower neighbours in one chunk (sixteen rounds of
    the four-in-flight loop) and, reversed, a last row whose 300 neighbours are all lower (five e0 chunks).  Both forms against
    the yardstick, and equal to each other with `==`."""
    case = RR.build_case(name)
    fb = RR.finish_branches(case.rowptr, case.col)
    assert case.pair and fb["c1"] > 0 and fb["tail"] > 0 and fb["max_lower_in_chunk"] == 64
    us_pair, pair, _ = _check(amd, case)
    us_rows, rows, _ = _check(amd, case, {"OSC_RECEIPT_PAIR": "0"})
    assert np.array_equal(us_pair, us_rows)  # (the same U* under both forms: the precondition of the comparison)
    for x, y in zip(pair, rows):
        assert np.array_equal(x, y)


# ------------------------------------------------------------------------------------------------------------- exact ties
def _row_order(lat):
    from oscillink_amd import _native as nat

    perm = np.zeros(lat.N, dtype=np.int32)
    lat._call("osc_get_row_order", nat.i32(perm))
    return perm


# (the switches that balance the source blocks of a blocked plan leave lattices of these sizes in API order)
ORDERS = {"api": ({}, "none"), "bfs": ({"OSC_REORDER": "1"}, "bfs")}


@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("stars", [40, 600])
def test_exact_tie_goes_to_the_smaller_api_id(amd, stars, order):
    """Disjoint stars, each centre with three twin pairs of leaves (same anchor row, edge weight and gate); the far pair carries
    the centre's largest R twice, bit for bit.  The centre's null point must be the twin with the smaller API id -- the
    reference's first argmax -- in the row form (40 stars, N = 280) and the pair form (600 stars, N = 4200), in API order and
    in the breadth-first stored order (OSC_REORDER=1), where k_receipt_rows / k_receipt_finish meet the twins in stored order and
    decide by `api_id`.  (The breadth-first order visits a centre's leaves in ascending id, so it stores no twin pair reversed
    -- the count is printed; the rule is pinned all the same: `>=` for `>`, or the api_id comparison turned round, fails here.)"""
    case, centres, twins = RR.stars_case(stars, 16, 21)
    assert case.pair == (stars == 600)
    lat, Us = _settled(amd, case, ORDERS[order][0])
    kind = lat.build_info()["order_kind"]
    assert kind == ORDERS[order][1]
    # the precondition: a twin's row has one neighbour (no summation order) and every CG update is elementwise
    a, b = twins[:, :, 0], twins[:, :, 1]
    assert np.array_equal(Us[a], Us[b]), "the twins' U* rows are not bit-identical: the case does not apply"
    perm = _row_order(lat)
    stored = np.empty(case.N, dtype=np.int64)
    stored[perm] = np.arange(case.N)
    print(f"TIES stars={stars} order={order} (stored: {kind}): {int(np.count_nonzero(stored[a] > stored[b]))} of {a.size} twin pairs stored "
          f"reversed, {int(np.count_nonzero(stored[a[:, 0]] > stored[b[:, 0]]))} of {stars} far pairs")
    coh, anc, qry, i, j, z, r = _device_rows(lat, 0.0)
    got = dict(zip(i.tolist(), j.tolist()))
    ref = RR.receipt_reference(case.Y, Us, case.psi, case.B, case.rowptr, case.col, case.a, case.sqrt_deg(), *RR.LAMS)
    assert np.all(ref.null_z[centres] > 1.0)
    for s, c in enumerate(centres):
        assert got[int(c)] == int(a[s, 0]) == int(ref.null_col[c]), (s, int(c), got[int(c)], twins[s, 0])
    for leaf, c in zip(twins.reshape(stars, 6).T, np.tile(centres, (6, 1))):
        assert all(got.get(int(x), int(y)) == int(y) for x, y in zip(leaf, c))  # a leaf's only candidate is its centre
    ri = {int(x): t for t, x in enumerate(i)}
    at = np.array([ri[int(c)] for c in centres])
    assert np.allclose(r[at], ref.null_R[centres], rtol=RR.Z_RTOL, atol=0.0)
    assert np.allclose(z[at], ref.null_z[centres], rtol=RR.Z_RTOL, atol=0.0)
    # the twins themselves: equal inputs, equal outputs
    assert np.array_equal(coh[a], coh[b]) and np.array_equal(anc[a], anc[b]) and np.array_equal(qry[a], qry[b])
    lat.close()

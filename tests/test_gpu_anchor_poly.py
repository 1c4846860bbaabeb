"""The polynomial last form of an anchor start that ends in iteration 4 ("Polynomial last form"): under the
four-step route's conditions every CG vector of a column is a combination of W^k Y and psi W^k 1, so x4 = sum a_k W^k Y + sum q_k
W^k 1 with nine coefficients a column (anchor_gram.hpp: poly4_coeffs, formed by k_anchor_gram_scalars), and a solve predicted and
shown to end in iteration 4 is that kernel and one elementwise pass over the lattice's held row sums (k_settle_poly): no matvec.
The reference everywhere is a second handle on the same inputs under OSC_ANCHOR_POLY=0, which keeps the folded form; the handle
under test runs with OSC_ANCHOR_POLY=1; both run under OSC_ANCHOR_GRAM4=1 and get the same calls.

Where the solve is predicted to end in iteration 4 and does: every scalar comes from the same kernel on the same sums, so iteration
counts and residual histories are EQUAL; U agrees within 2e-6 relative (U_TOL, the suite's bound between routes);
`poly_four_step_solves` advances by one on the handle under test alone, `blocked_applies` by 0 there and by 1 on the reference;
every other counter is equal.  Wherever the form is declined -- stops in 1, 2, 3 or beyond 4, max_iters = 3, a prediction other than
4, a new query before its prediction, non-uniform gates, a chain prior, the windowed handle, a warm start from a written U, the
memory rule denying W^4 Y -- the handles agree to the bit.  A predicted 4 that does not come true (the pass was gated off by the
device's own word) costs one counted redo and gives the reference's bytes.  Against float64 (the CPU oracle on the device-built
graph, four iterations executed) the new form's error is no larger than the reference handle's.

Shapes: those of tests/test_gpu_anchor_gram.py, one per class of the pass's launch shape (16 and 32 lanes a row; one, two and
three float4 chunks a lane; two column tiles) and a row count that is no multiple of the rows per trip; k = 16."""
import numpy as np
import pytest

from tests import test_gpu_anchor_gram as two
from tests import test_gpu_anchor_gram4 as four
from tests._cases import relerr
from tests._fullsize import oracle_solves

pytestmark = pytest.mark.gpu

# (the counters under test, the matvec count they explain, a wall-clock time)
UNEQUAL = ("poly_four_step_solves", "anchor_poly_bytes", "anchor_poly_last_solve", "anchor_poly_builds", "anchor_poly_redos",
           "blocked_applies", "balance_ms")

XS = {"OSC_SPMM_XS": "1"}  # (the slab mode, and with it the route, at every width)
SHAPES = dict(two.SHAPES)
SHAPES.update({
    "lanes16_partial_trip": dict(N=20011, D=64, env=XS),       # 16 lanes a row, 16 rows a trip: 20011 = 1250 * 16 + 11
    "lanes32": dict(N=20000, D=128, env=XS),                   # 32 lanes a row
    "chunks2": dict(N=20000, D=512, env=XS),                   # 64 lanes, two chunks
    "chunks3_partial_trip": dict(N=20003, D=768, env=XS),      # 64 lanes, three chunks: the benchmark's shape; 4 rows a trip
    "two_tiles_ragged": dict(N=20000, D=772, env=dict(XS, OSC_LD="800")),  # two column tiles of 400 and 372, the last chunk partial
})


@pytest.fixture(scope="module")
def amd():
    import oscillink_amd
    from oscillink_amd import _native

    assert _native.device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return oscillink_amd


@pytest.fixture(scope="module")
def orc():
    from oracle import oscillink_oracle

    return oscillink_oracle


def _clean_env(monkeypatch):
    four._clean_env(monkeypatch)
    for v in ("OSC_GRAM4_FOLD", "OSC_ANCHOR_POLY", "OSC_ANCHOR_POLY_MAX_MB", "OSC_TWO_STEPS"):
        monkeypatch.delenv(v, raising=False)


def _make(amd, monkeypatch, Y, psi, k, poly, gates=None, chain=None):
    monkeypatch.setenv("OSC_ANCHOR_POLY", "1" if poly else "0")
    return four._make(amd, monkeypatch, Y, psi, k, "1", gates, chain)


class _Pair:
    """`ref` under OSC_ANCHOR_POLY=0, `poly` under OSC_ANCHOR_POLY=1; both on the four-step route (OSC_ANCHOR_GRAM4=1)."""

    def __init__(self, amd, monkeypatch, Y, psi, k, gates=None, chain=None):
        self.ref = _make(amd, monkeypatch, Y, psi, k, False, gates, chain)
        self.poly = _make(amd, monkeypatch, Y, psi, k, True, gates, chain)
        self.both = (self.ref, self.poly)

    def close(self):
        self.ref.close()
        self.poly.close()


def _counters(lat):
    return {key: v for key, v in lat.build_info().items() if key not in UNEQUAL}


def _both_start(pair, what, redo=0, start=two._anchor_start, **kw):
    """One anchor start on both lattices.  Whether the solve took the four-step route is read off the reference's counter; it takes
    the polynomial form exactly if it was also predicted to end in iteration 4 and the handle holds W^4 Y (formed, at the latest, by
    this very solve: the start that forms the fourth step's sums keeps it).  Then the handle under
    test counts it (+1 / 0) and launches no matvec where the reference launches one, iterations and histories are equal and U
    agrees within U_TOL.  Otherwise the handles agree to the bit and launch the same matvecs; `redo`: the redos the handle under
    test must count (a predicted 4 that did not come true).  All other counters are equal either way.  Returns (route, poly)."""
    i0 = [lat.build_info() for lat in pair.both]
    predicted = pair.poly.last["iters"]
    x, y = start(pair.ref, **kw), start(pair.poly, **kw)
    i1 = [lat.build_info() for lat in pair.both]
    d = [{key: i1[j][key] - i0[j][key] for key in ("poly_four_step_solves", "anchor_poly_redos", "blocked_applies", "fused_four_step_solves")}
         for j in range(2)]
    assert _counters(pair.ref) == _counters(pair.poly), (what, _counters(pair.ref), _counters(pair.poly))
    took = d[0]["fused_four_step_solves"]
    poly = int(took == 1 and predicted == 4 and i1[1]["anchor_poly_bytes"] > 0)
    assert (d[0]["poly_four_step_solves"], d[1]["poly_four_step_solves"]) == (0, poly), (what, d, took, predicted)
    assert (d[0]["anchor_poly_redos"], d[1]["anchor_poly_redos"]) == (0, redo), (what, d)
    assert i1[1]["anchor_poly_last_solve"] == poly and i1[0]["anchor_poly_last_solve"] == 0, (what, i1[1])
    assert (i1[0]["anchor_poly_bytes"], i1[0]["anchor_poly_builds"]) == (0, 0), (what, i1[0])
    if poly:
        assert (d[0]["blocked_applies"], d[1]["blocked_applies"]) == (1, 0), (what, d)
        assert x[0] == y[0] == 4, (what, x[0], y[0])
        assert np.array_equal(x[2], y[2]), (what, "history", x[2], y[2])
        assert x[1] == y[1], (what, "residual", x[1], y[1])
        e = relerr(y[3], x[3])
        print(f"{what}: polynomial against folded U rel {e:.3e}")
        assert e < two.U_TOL, (what, "U", e)
    else:
        assert d[0]["blocked_applies"] == d[1]["blocked_applies"], (what, d)
        two._same(x, y, what)
    return took, poly


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_polynomial_and_folded_last_forms_agree(amd, name, monkeypatch):
    _clean_env(monkeypatch)
    spec = SHAPES[name]
    for k, v in spec.get("env", {}).items():
        monkeypatch.setenv(k, v)
    N, D = spec["N"], spec["D"]
    Y, psi, psi2, _ = two._inputs(N, D)
    pair = _Pair(amd, monkeypatch, Y, psi, 16)
    try:
        if spec.get("window"):  # (settles start from U's own copy, the U* solves take 5 iterations: declined, the same bytes)
            for trip in range(2):
                assert _both_start(pair, (name, "settle", trip)) == (0, 0)
            for trip in range(3):
                us = [lat.solve_Ustar(use_cache=False).copy() for lat in pair.both]
                hs = [lat.residual_history() for lat in pair.both]
                assert np.array_equal(hs[0], hs[1]) and np.array_equal(us[0], us[1]), (name, "U*", trip)
                assert _counters(pair.ref) == _counters(pair.poly), (name, "U*", trip)
            assert [lat.build_info()["poly_four_step_solves"] for lat in pair.both] == [0, 0]
            return
        assert _both_start(pair, (name, "first")) == (0, 0)
        polys = _both_start(pair, (name, "second"))[1]  # (forms the sums and W^4 Y; polynomial already if the first start took 4 iterations)
        assert polys == int(pair.poly.last["iters"] == 4), (name, polys, pair.poly.last)
        assert _both_start(pair, (name, "to convergence"), redo=polys, tol=1e-6) == (0, 0)
        info = pair.poly.build_info()
        # (W^4 Y is kept by the start that forms the fourth step's sums: N x ld floats)
        assert info["anchor_poly_builds"] == 1 and info["anchor_poly_bytes"] >= 4 * N * D and info["anchor_poly_bytes"] % (4 * N) == 0, info
        tol = four._tols(pair.ref.residual_history())
        assert _both_start(pair, (name, "predicted longer, ends in iteration 4"), tol=tol[4]) == (1, 0)
        assert _both_start(pair, (name, "again, predicted 4"), tol=tol[4]) == (1, 1)
        assert _both_start(pair, (name, "and again"), tol=tol[4]) == (1, 1)
        # a predicted 4 that does not come true: the pass was gated off, one redo, the reference's bytes
        assert _both_start(pair, (name, "predicted 4, ends in iteration 3"), redo=1, tol=tol[3]) == (0, 0)
        assert pair.poly.last["iters"] == 3
        assert _both_start(pair, (name, "predicted 3, ends in 4"), tol=tol[4]) == (1, 0)
        assert _both_start(pair, (name, "predicted 4, the tolerance tightened"), redo=1, tol=1e-6) == (0, 0)
        assert len(pair.poly.residual_history()) > 4
        assert _both_start(pair, (name, "predicted longer, ends in 4"), tol=tol[4]) == (1, 0)
        assert _both_start(pair, (name, "predicted 4, max_iters 3"), max_iters=3, tol=tol[4]) == (0, 0)
        assert _both_start(pair, (name, "ends in iteration 2"), tol=tol[2]) == (0, 0)
        assert pair.poly.last["iters"] == 2
        assert _both_start(pair, (name, "ends in iteration 1"), tol=tol[1]) == (0, 0)
        assert pair.poly.last["iters"] == 1
        for lat in pair.both:
            lat.set_query(psi2, gates=None)
            lat.lamC, lat.lamQ = 0.8, 2.5
        assert _both_start(pair, (name, "other query and lams, before their prediction"), tol=1e-6) == (0, 0)
        tol = four._tols(pair.ref.residual_history())
        assert _both_start(pair, (name, "other query and lams"), tol=tol[4]) == (1, 0)
        assert _both_start(pair, (name, "other query and lams, predicted 4"), tol=tol[4]) == (1, 1)
        info = pair.poly.build_info()
        assert info["poly_four_step_solves"] == 3 + polys and info["anchor_poly_redos"] == 2 + polys and info["anchor_poly_builds"] == 1, info
        if "shape" in spec:
            assert info["apply_blocked_shape"] == spec["shape"], info
        if "order" in spec:
            assert info["order_kind"] == spec["order"], info
    finally:
        pair.close()


def test_against_float64(amd, orc, monkeypatch):
    """The CPU oracle on the device-built graph, four iterations executed: the polynomial form's error against it is no larger
    than the reference handle's (tests/host_logic/sweep_poly4.cpp: its fp32 model gives 0.5 of the gathered route's)."""
    import scipy.sparse as sp

    _clean_env(monkeypatch)
    N, D, k = 20000, 256, 16
    Y, psi, _, _ = two._inputs(N, D, seed=5)
    pair = _Pair(amd, monkeypatch, Y, psi, k)
    try:
        for trip in range(2):
            _both_start(pair, ("oracle", trip), tol=1e-6)
        tol4 = four._tols(pair.ref.residual_history())[4]
        for trip in range(2):
            took = _both_start(pair, ("oracle, four", trip), tol=tol4)
        assert took == (1, 1) and pair.poly.last["iters"] == 4
        csr = pair.ref.graph_csr()[:3]
        assert all(np.array_equal(a, b) for a, b in zip(csr, pair.poly.graph_csr()[:3]))
        A = sp.csr_matrix((csr[2], csr[1], csr[0]), shape=(N, N), dtype=np.float32)
        ref = oracle_solves(orc, Y, psi, A, k=k, settle_iters=4, settle_tol=tol4, ustar_iters=1)
        e_r, e_p = (relerr(x, ref["U"]) for x in (pair.ref.U.copy(), pair.poly.U.copy()))
        print(f"float64 settle: folded (reference handle) {e_r:.3e} polynomial {e_p:.3e} ratio {e_p / e_r:.2f}")
        assert e_p <= e_r, (e_r, e_p)
    finally:
        pair.close()


@pytest.mark.parametrize("case", ["gates", "chain", "denied"])
def test_declined_lattices_agree_to_the_bit(amd, case, monkeypatch):
    """Non-uniform gates and a chain prior keep the solve off the Gram route altogether; under a memory rule that denies W^4 Y
    (OSC_ANCHOR_POLY_MAX_MB=0: nothing may be kept) the four-step route runs as ever, folded where predicted."""
    _clean_env(monkeypatch)
    N, D = 20000, 256
    Y, psi, _, gates = two._inputs(N, D, seed=6)
    if case == "denied":
        monkeypatch.setenv("OSC_ANCHOR_POLY_MAX_MB", "0")
    pair = _Pair(amd, monkeypatch, Y, psi, 16, gates=gates if case == "gates" else None, chain=two.CHAIN if case == "chain" else None)
    try:
        for trip in range(2):
            _both_start(pair, (case, "plan", trip), tol=1e-6)
        hist = pair.ref.residual_history()
        tol4 = four._tols(hist)[4] if len(hist) >= 4 else 1e-3
        for trip in range(3):
            took = _both_start(pair, (case, trip), tol=tol4)
            assert took[1] == 0 and took[0] == (1 if case == "denied" else 0), (case, trip, took)
        info = pair.poly.build_info()
        assert (info["poly_four_step_solves"], info["anchor_poly_bytes"], info["anchor_poly_builds"], info["anchor_poly_redos"]) == (0, 0, 0, 0), info
        if case == "denied":
            assert info["folded_four_step_solves"] == 2, info
    finally:
        pair.close()


def _warm(lat, **kw):
    st = lat.settle(**dict(two.KW, **kw))  # (no reset_U: the start is the written U)
    return st["iters"], st["res"], lat.residual_history(), lat.U.copy()


def test_what_runs_behind_a_polynomial_solve(amd, monkeypatch):
    """A polynomial solve leaves nothing defined in R, P and AP.  Every solve forms its own residual first, so what follows is held
    to the reference handle within U_TOL: a warm-started settle (declined: it starts from a written U, and its U differs by what the
    starts differed by), a light receipt's deltaH, and the U* solve, which does not depend on U at all."""
    _clean_env(monkeypatch)
    Y, psi, _, _ = two._inputs(20000, 256, seed=12)
    pair = _Pair(amd, monkeypatch, Y, psi, 16)
    try:
        for lat in pair.both:
            lat.set_receipt_detail("light")
        for trip in range(2):
            _both_start(pair, ("behind", "plan", trip), tol=1e-6)
        tol4 = four._tols(pair.ref.residual_history())[4]
        assert _both_start(pair, ("behind", "predicted longer"), tol=tol4) == (1, 0)
        assert _both_start(pair, ("behind", "polynomial"), tol=tol4) == (1, 1)
        i0 = [lat.build_info() for lat in pair.both]
        outs = [_warm(lat, tol=1e-5) for lat in pair.both]
        i1 = [lat.build_info() for lat in pair.both]
        assert outs[0][0] == outs[1][0], ("warm start", outs[0][0], outs[1][0])
        e = relerr(outs[1][3], outs[0][3])
        print(f"warm start behind a polynomial solve: iters {outs[0][0]} U rel {e:.3e}")
        assert e < two.U_TOL, e
        assert i1[1]["poly_four_step_solves"] == i0[1]["poly_four_step_solves"] and i1[1]["anchor_poly_redos"] == i0[1]["anchor_poly_redos"]
        assert i1[0]["blocked_applies"] - i0[0]["blocked_applies"] == i1[1]["blocked_applies"] - i0[1]["blocked_applies"]
        assert _both_start(pair, ("behind", "predicted by the warm start"), tol=tol4)[0] == 1
        assert _both_start(pair, ("behind", "polynomial again"), tol=tol4) == (1, 1)
        us = [lat.solve_Ustar(use_cache=False).copy() for lat in pair.both]
        e = relerr(us[1], us[0])
        print(f"U* behind a polynomial solve: rel {e:.3e}")
        assert e < two.U_TOL and np.array_equal(pair.ref.residual_history(), pair.poly.residual_history())
        assert _both_start(pair, ("behind", "polynomial, behind U*"), tol=tol4) == (1, 1)
        dh = [float(lat.receipt()["deltaH_total"]) for lat in pair.both]
        e = abs(dh[1] - dh[0]) / abs(dh[0])
        print(f"light receipts behind a polynomial solve: deltaH {dh[0]:.9g} / {dh[1]:.9g}, rel {e:.3e}")
        assert e < two.U_TOL, (dh, e)
        assert _counters(pair.ref) == _counters(pair.poly)
    finally:
        pair.close()


@pytest.mark.parametrize("keep_state", [False, True], ids=["plain", "keep_state"])
def test_append_remove_and_update_drop_the_kept_row_sums(amd, keep_state, monkeypatch):
    """append, remove and update drop W^4 Y with W^3 Y; the next two anchor starts -- the first gathers, the second forms the row
    sums anew -- agree with the reference handle, which went through the same calls, and `anchor_poly_builds` shows that W^4 Y was
    formed again; the start after them takes the polynomial form again."""
    _clean_env(monkeypatch)
    N, D = 20000, 256
    Y, psi, _, _ = two._inputs(N, D, seed=8)
    pair = _Pair(amd, monkeypatch, Y, psi, 16)
    more = two._inputs(64, D, seed=9)[0]
    state = {"builds": 0}

    def builds():
        # (append, remove and update may make a new handle, whose counters start at 0: only a change is looked for)
        return pair.poly.build_info()["anchor_poly_builds"], pair.poly.build_info()["anchor_poly_bytes"]

    def again(what):
        assert builds()[1] == 0, what
        b0 = builds()[0]
        _both_start(pair, (what, "first"), tol=1e-6)
        _both_start(pair, (what, "second"), tol=1e-6)
        assert builds()[0] == b0 + 1 and builds()[1] > 0, (what, b0, builds())
        tol4 = four._tols(pair.ref.residual_history())[4]
        assert _both_start(pair, (what, "predicted longer, ends in 4"), tol=tol4) == (1, 0)
        assert _both_start(pair, (what, "polynomial"), tol=tol4) == (1, 1)
        state["builds"] += 1

    def both(call):
        for lat, poly in zip(pair.both, ("0", "1")):  # (a new handle reads the switches)
            monkeypatch.setenv("OSC_ANCHOR_POLY", poly)
            call(lat)

    try:
        again("fresh")
        both(lambda lat: lat.append(more, keep_state=keep_state))
        again("append")
        both(lambda lat: lat.remove(np.arange(N, N + 64), keep_state=keep_state))
        again("remove")
        rows = np.array([3, 777, 19999])
        both(lambda lat: lat.update(rows, more[:3], keep_state=keep_state))
        again("update")
        assert state["builds"] == 4
    finally:
        pair.close()

"""The folded last form of an anchor start that ends in iteration 4 ("Four steps"): x4 is affine in the
gathered row sum of p3, so the INIT pass -- which runs behind alpha3, beta3 and alpha4 -- stores e, x4 with a zero row sum, in
x's place and no r2 (two_steps_elem under go[2], the device's copy of the host's decision), and iteration 3's matvec reads the
row of e, does one fmaf per element and stores x4 over it (k_apply_blocked, FMODE 3): one row stream where FUSED_LAST has three.
The reference everywhere is a second handle on the same inputs under OSC_GRAM4_FOLD=0, which keeps the unfolded arithmetic;
both run under OSC_ANCHOR_GRAM4=1 and get the same calls.

Where the solve ends in iteration 4 (the tolerance is the geometric mean of the reference's residuals 3 and 4, as in
tests/test_gpu_anchor_gram4.py): every scalar comes from the same kernel on the same sums, so iteration counts and residual
histories are EQUAL; U agrees within 2e-6 relative (the suite's bound between routes; the CPU model of
tests/host_logic/sweep_gram4_fold.cpp gives 5.0e-8 in that norm); `folded_four_step_solves` advances by one on the one handle and
stays 0 on the other; every other counter is equal.  A solve that ends in iteration 4 behind another prediction keeps the
unfolded form on both handles (the INIT pass is launched in its foldable form only behind a prediction of 4): the same bytes.
Wherever the route is declined -- stops in 1, 2, 3, beyond 4, max_iters = 3,
a prediction that ends elsewhere, another query and other lams before their prediction, the windowed handle's settles and U*
solves -- the handles agree to the bit.  Against the CPU oracle the folded route may be at most the siblings' 2.5 x of the
gathered route.  After a folded solve the R array holds nothing defined: a warm-started settle, a receipt and a U* solve behind
one are held to the reference handle.

Shapes: those of tests/test_gpu_anchor_gram.py."""
import numpy as np
import pytest

from tests import test_gpu_anchor_gram as two
from tests import test_gpu_anchor_gram4 as four
from tests._cases import relerr
from tests._fullsize import oracle_solves

pytestmark = pytest.mark.gpu

ORACLE_FACTOR = 2.5
UNEQUAL = ("folded_four_step_solves", "balance_ms")  # (the counter under test; a wall-clock time)


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
    monkeypatch.delenv("OSC_GRAM4_FOLD", raising=False)


def _make(amd, monkeypatch, Y, psi, k, fold, ap="1"):
    if fold:
        monkeypatch.delenv("OSC_GRAM4_FOLD", raising=False)
    else:
        monkeypatch.setenv("OSC_GRAM4_FOLD", "0")
    return four._make(amd, monkeypatch, Y, psi, k, "1", ap=ap)


class _Pair:
    """`ref` under OSC_GRAM4_FOLD=0, `fold` with the switch unset; both on the four-step route (OSC_ANCHOR_GRAM4=1)."""

    def __init__(self, amd, monkeypatch, Y, psi, k):
        self.ref = _make(amd, monkeypatch, Y, psi, k, False)
        self.fold = _make(amd, monkeypatch, Y, psi, k, True)
        self.both = (self.ref, self.fold)

    def close(self):
        self.ref.close()
        self.fold.close()


def _counters(lat):
    return {key: v for key, v in lat.build_info().items() if key not in UNEQUAL}


def _both_start(pair, what, **kw):
    """One anchor start on both lattices.  Whether the solve took the four-step route is read off the reference's counter.  It is
    folded exactly if it was also predicted to end in iteration 4 (the handle's previous settle took 4 iterations: only then is the
    INIT pass launched in its foldable form): then the fold handle counts it (+1 / 0), iterations and histories are equal and U
    agrees within U_TOL.  Otherwise the handles agree to the bit and nobody folded.  All other counters are equal either way.
    Returns (route taken, folded)."""
    f0 = [lat.build_info()["folded_four_step_solves"] for lat in pair.both]
    t0 = pair.ref.build_info()["fused_four_step_solves"]
    predicted = pair.fold.last["iters"]
    x, y = two._anchor_start(pair.ref, **kw), two._anchor_start(pair.fold, **kw)
    took = pair.ref.build_info()["fused_four_step_solves"] - t0
    f1 = [lat.build_info()["folded_four_step_solves"] for lat in pair.both]
    assert _counters(pair.ref) == _counters(pair.fold), (what, _counters(pair.ref), _counters(pair.fold))
    folded = int(took == 1 and predicted == 4)
    assert (f1[0] - f0[0], f1[1] - f0[1]) == (0, folded), (what, f0, f1, took, predicted)
    if folded:
        assert x[0] == y[0] == 4, (what, x[0], y[0])
        assert np.array_equal(x[2], y[2]), (what, "history", x[2], y[2])
        e = relerr(y[3], x[3])
        print(f"{what}: folded against unfolded U rel {e:.3e}")
        assert e < two.U_TOL, (what, "U", e)
    else:
        two._same(x, y, what)
    return took, folded


@pytest.mark.parametrize("name", sorted(two.SHAPES))
def test_folded_and_unfolded_last_forms_agree(amd, name, monkeypatch):
    _clean_env(monkeypatch)
    spec = two.SHAPES[name]
    for k, v in spec.get("env", {}).items():
        monkeypatch.setenv(k, v)
    N, D = spec["N"], spec["D"]
    Y, psi, psi2, _ = two._inputs(N, D)
    pair = _Pair(amd, monkeypatch, Y, psi, 16)
    try:
        if spec.get("window"):  # (settles start from U's own copy, the U* solves take 5 iterations: nothing folds, the same bytes)
            for trip in range(2):
                assert _both_start(pair, (name, "settle", trip)) == (0, 0)
            for trip in range(3):
                us = [lat.solve_Ustar(use_cache=False).copy() for lat in pair.both]
                hs = [lat.residual_history() for lat in pair.both]
                assert np.array_equal(hs[0], hs[1]) and np.array_equal(us[0], us[1]), (name, "U*", trip)
                assert _counters(pair.ref) == _counters(pair.fold), (name, "U*", trip)
            assert [lat.build_info()["folded_four_step_solves"] for lat in pair.both] == [0, 0]
            return
        assert _both_start(pair, (name, "first")) == (0, 0)
        _both_start(pair, (name, "second"))
        tol = four._tols(pair.ref.residual_history())
        assert _both_start(pair, (name, "ends in iteration 4"), tol=tol[4])[0] == 1
        assert _both_start(pair, (name, "again, predicted 4"), tol=tol[4]) == (1, 1)
        assert _both_start(pair, (name, "and again"), tol=tol[4]) == (1, 1)
        assert _both_start(pair, (name, "predicted 4, ends in iteration 3"), tol=tol[3]) == (0, 0)  # (the foldable pass, go[2] = 0)
        assert pair.fold.last["iters"] == 3
        assert _both_start(pair, (name, "predicted 3, ends in 4"), tol=tol[4]) == (1, 0)
        assert _both_start(pair, (name, "predicted 4, runs beyond 4"), tol=1e-6) == (0, 0)  # (the foldable pass, go[2] = 0)
        assert len(pair.fold.residual_history()) > 4
        assert _both_start(pair, (name, "predicted longer, ends in 4"), tol=tol[4]) == (1, 0)
        assert _both_start(pair, (name, "predicted 4, max_iters 3"), max_iters=3, tol=tol[4]) == (0, 0)
        assert _both_start(pair, (name, "ends in iteration 2"), tol=tol[2]) == (0, 0)
        assert pair.fold.last["iters"] == 2
        assert _both_start(pair, (name, "ends in iteration 1"), tol=tol[1]) == (0, 0)
        assert pair.fold.last["iters"] == 1
        for lat in pair.both:
            lat.set_query(psi2, gates=None)
            lat.lamC, lat.lamQ = 0.8, 2.5
        assert _both_start(pair, (name, "other query and lams, prediction"), tol=1e-6) == (0, 0)
        tol = four._tols(pair.ref.residual_history())
        assert _both_start(pair, (name, "other query and lams"), tol=tol[4]) == (1, 0)
        assert _both_start(pair, (name, "other query and lams, predicted 4"), tol=tol[4]) == (1, 1)
        info = pair.fold.build_info()
        assert 3 <= info["folded_four_step_solves"] < info["fused_four_step_solves"], info
        assert pair.ref.build_info()["folded_four_step_solves"] == 0
        if "shape" in spec:
            assert info["apply_blocked_shape"] == spec["shape"], info
        if "order" in spec:
            assert info["order_kind"] == spec["order"], info
    finally:
        pair.close()


def test_against_the_cpu_oracle(amd, orc, monkeypatch):
    """The CPU oracle on the device-built graph, four iterations executed: the folded route's error against it is at most 2.5
    times the gathered route's (OSC_ANCHOR_AP=0)."""
    import scipy.sparse as sp

    _clean_env(monkeypatch)
    N, D, k = 20000, 256, 16
    Y, psi, _, _ = two._inputs(N, D, seed=5)
    pair = _Pair(amd, monkeypatch, Y, psi, k)
    gathered = _make(amd, monkeypatch, Y, psi, k, True, ap="0")
    try:
        for trip in range(2):
            _both_start(pair, ("oracle", trip), tol=1e-6)
        tol4 = four._tols(pair.ref.residual_history())[4]
        for trip in range(2):
            took = _both_start(pair, ("oracle, four", trip), tol=tol4)
            g = two._anchor_start(gathered, tol=tol4)
        assert took == (1, 1) and g[0] == 4 == pair.fold.last["iters"]
        csr = pair.ref.graph_csr()[:3]
        assert all(np.array_equal(a, b) for a, b in zip(csr, pair.fold.graph_csr()[:3]))
        A = sp.csr_matrix((csr[2], csr[1], csr[0]), shape=(N, N), dtype=np.float32)
        ref = oracle_solves(orc, Y, psi, A, k=k, settle_iters=4, settle_tol=tol4, ustar_iters=1)
        e_g, e_u, e_f = (relerr(x, ref["U"]) for x in (g[3], pair.ref.U.copy(), pair.fold.U.copy()))
        print(f"oracle settle: gathered {e_g:.3e} unfolded {e_u:.3e} folded {e_f:.3e} ratio to gathered {e_f / e_g:.2f}")
        assert e_f <= ORACLE_FACTOR * e_g, (e_g, e_u, e_f)
    finally:
        gathered.close()
        pair.close()


def test_two_runs_of_the_folded_route_give_the_same_bytes(amd, monkeypatch):
    _clean_env(monkeypatch)
    Y, psi, _, _ = two._inputs(20000, 256, seed=10)
    lats = [_make(amd, monkeypatch, Y, psi, 16, True) for _ in range(2)]
    try:
        for trip in range(2):
            outs = [two._anchor_start(lat, tol=1e-6) for lat in lats]
            two._same(outs[0], outs[1], ("repeat, warm", trip))
        tol4 = four._tols(outs[0][2])[4]
        first = None
        for trip in range(4):  # (the first one behind a longer prediction: unfolded)
            outs = [two._anchor_start(lat, tol=tol4) for lat in lats]
            two._same(outs[0], outs[1], ("repeat", trip))
            if trip >= 1:
                first = outs[0] if first is None else first
                two._same(first, outs[0], ("repeat, same handle", trip))
        assert all(lat.build_info()["folded_four_step_solves"] == 3 for lat in lats)
    finally:
        for lat in lats:
            lat.close()


def test_what_runs_behind_a_folded_solve_does_not_miss_r(amd, monkeypatch):
    """A folded solve leaves nothing defined in the R array (the unfolded form left r2 there).  Every solve forms its own residual
    first, so what follows is the reference handle's: a warm-started settle, a receipt, and the U* solve, which does not depend on
    U at all (equal bytes).  The warm start is an implicit Euler step from the two handles' U: (I + dt M)^-1 does not enlarge their
    difference (M is positive semidefinite), each solve misses its exact solution by at most its residual (A's eigenvalues are
    at least 1; the residual is the largest column norm, hence sqrt(D) for the Frobenius norm), and U is rounded to float32.  deltaH is quadratic in d = U - U*: a perturbation of U of relative size e changes it by
    2 e |U| / |d| relative to first order, bounded here with e = U_TOL, the factor 2 of slack and float32's rounding of the
    returned value, from the reference handle's own U and U*."""
    _clean_env(monkeypatch)
    Y, psi, _, _ = two._inputs(20000, 256, seed=12)
    pair = _Pair(amd, monkeypatch, Y, psi, 16)
    try:
        for trip in range(2):
            _both_start(pair, ("behind", "plan", trip), tol=1e-6)
        tol4 = four._tols(pair.ref.residual_history())[4]
        assert _both_start(pair, ("behind", "predicted longer"), tol=tol4) == (1, 0)
        assert _both_start(pair, ("behind", "folded"), tol=tol4) == (1, 1)
        u0 = [lat.U.astype(np.float64) for lat in pair.both]
        outs = []
        for lat in pair.both:  # warm start: no reset_U
            st = lat.settle(max_iters=12, tol=1e-5)
            outs.append((st["res"], lat.U.astype(np.float64)))
        gap = np.linalg.norm(outs[1][1] - outs[0][1])
        bound = np.linalg.norm(u0[1] - u0[0]) + np.sqrt(Y.shape[1]) * (outs[0][0] + outs[1][0]) + 2.0 ** -22 * np.linalg.norm(outs[0][1])
        print(f"warm start behind a folded solve: |dU| {gap:.3e}, bound {bound:.3e}, rel {gap / np.linalg.norm(outs[0][1]):.3e}")
        assert max(outs[0][0], outs[1][0]) <= 1e-5 and gap <= bound, (gap, bound, outs[0][0], outs[1][0])
        assert _both_start(pair, ("behind", "predicted by the warm start"), tol=tol4)[0] == 1
        assert _both_start(pair, ("behind", "folded again"), tol=tol4) == (1, 1)
        us = [lat.solve_Ustar(use_cache=False).copy() for lat in pair.both]
        assert np.array_equal(us[0], us[1]) and np.array_equal(pair.ref.residual_history(), pair.fold.residual_history())
        assert _both_start(pair, ("behind", "folded, behind U*"), tol=tol4) == (1, 1)
        rs = [lat.receipt() for lat in pair.both]
        U = pair.ref.U.astype(np.float64)
        d = U - us[0].astype(np.float64)
        bound = 2.0 * 2.0 * two.U_TOL * np.linalg.norm(U) / np.linalg.norm(d) + 2.0 ** -23
        dh = [float(r["deltaH_total"]) for r in rs]
        print(f"receipts behind a folded solve: deltaH {dh[0]:.9g} / {dh[1]:.9g}, rel {abs(dh[1] - dh[0]) / abs(dh[0]):.3e}, bound {bound:.3e}")
        assert abs(dh[1] - dh[0]) <= bound * abs(dh[0]), (dh, bound)
        assert _counters(pair.ref) == _counters(pair.fold)
    finally:
        pair.close()


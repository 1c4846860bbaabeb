"""CPU checks of the multi-query receipt algebra in float64 against the oracle's receipt formulas
(receipts.py:10-83) at the exact U*(psi), and of the float64 yardstick the GPU tests use (tests/_receipt_yardstick.py)."""
import numpy as np
import pytest

from tests import _queries as yq
from tests import _receipt_yardstick as yr
from tests._cases import PARAM_CASES, ctor_kwargs, load_case, make_inputs, random_gates

CASES = ["c1_n80_d128_k8", "g1_n400_d64_k6_chain8", "gates_chain_n333_d50_k7", "c5mini_n600_d96_k12"] + PARAM_CASES


def _oracle(name):
    from oracle import oscillink_oracle as orc

    case = load_case(name)
    rc = case["recipe"]
    Y, psi = make_inputs(rc)
    N = Y.shape[0]
    A = np.zeros((N, N), dtype=np.float32)
    A[np.repeat(np.arange(N), np.diff(case["indptr"])), case["indices"]] = case["A_data"]
    kw = {k: v for k, v in ctor_kwargs(rc).items() if k != "row_cap_val"}
    ref = orc.OracleLattice(Y, kneighbors=rc["k"], deterministic_k=True, graph=A, **kw)
    gates = random_gates(rc) if rc["gates"] == "random" else case["gates"] if rc["gates"] == "diffusion" else None
    ref.set_query(psi, gates=gates)
    if rc["chain"]:
        ref.add_chain(rc["chain"], lamP=rc["lamP"])
    M = yq.dense_M(A, ref.sqrt_deg, ref.B_diag, ref.lamG, ref.lamC, ref.lamQ, ref.lamP, ref.L_path)
    return ref, Y, psi, A, M


def _queries(Y, psi):
    rng = np.random.default_rng(11)
    D = Y.shape[1]
    return [psi.astype(np.float64), rng.standard_normal(D), 3.0 * rng.standard_normal(D), Y[3].astype(np.float64),
            np.zeros(D)]


def _terms(ref, Y, A, M):
    """The per-basis terms of section 12 in float64."""
    B = ref.B_diag.astype(np.float64)
    X, x = yq.basis(M, Y, B, ref.lamG, ref.lamQ)
    Yd = Y.astype(np.float64)
    sd = ref.sqrt_deg.astype(np.float64) + 1e-12
    Mx = M @ x
    t = {"X": X, "x": x, "Mx": Mx, "h2": float(x @ Mx),
         "a0": float(np.sum((X - Yd) ** 2)), "a1": (x[:, None] * (X - Yd)).sum(axis=0), "a2": float(x @ x),
         "b0": float(np.sum(B[:, None] * X * X)), "b1": ((B * (x - 1.0))[:, None] * X).sum(axis=0),
         "b2": float(np.sum(B * (x - 1.0) ** 2)), "P": X / sd[:, None], "s": x / sd}
    r, c = np.nonzero(A > 0)
    t["r"], t["c"], t["w"] = r, c, A[r, c].astype(np.float64)
    t["d"] = np.sum((t["P"][r] - t["P"][c]) ** 2, axis=1)
    return t


def _states(ref, Y, psi, M):
    """U = Y, U after one settle, U = U*(psi0)"""
    U_settled = ref.U.copy()
    ref.settle(max_iters=12, tol=1e-3)
    U_settled, ref.U = ref.U.astype(np.float64), U_settled
    return {"fresh": Y.astype(np.float64), "settled": U_settled,
            "stationary": yq.ustar(M, Y, ref.B_diag, psi, ref.lamG, ref.lamQ)}


@pytest.mark.parametrize("name", CASES)
def test_energy_sums_are_quadratic_in_psi(name):
    from oracle import oscillink_oracle as orc

    ref, Y, psi, A, M = _oracle(name)
    t = _terms(ref, Y, A, M)
    Yd, B = Y.astype(np.float64), ref.B_diag.astype(np.float64)
    for q in _queries(Y, psi):
        U = t["X"] + np.outer(t["x"], q)
        pp = float(q @ q)
        anchor = ref.lamG * (t["a0"] + 2 * q @ t["a1"] + pp * t["a2"])
        query = ref.lamQ * (t["b0"] + 2 * q @ t["b1"] + pp * t["b2"])
        assert anchor == pytest.approx(ref.lamG * np.sum((U - Yd) ** 2), rel=1e-9, abs=1e-9)
        assert query == pytest.approx(ref.lamQ * np.sum(B[:, None] * (U - q[None, :]) ** 2), rel=1e-9, abs=1e-9)
        # the oracle's per-node components (float32 rows) on the same U*
        _, anc, qry = orc.per_node_components(Yd, U, A.astype(np.float64), ref.sqrt_deg.astype(np.float64), ref.lamG,
                                              ref.lamC, ref.lamQ, B, q)
        assert anchor == pytest.approx(float(np.sum(anc, dtype=np.float64)), rel=1e-5, abs=1e-5)
        assert query == pytest.approx(float(np.sum(qry, dtype=np.float64)), rel=1e-5, abs=1e-5)


@pytest.mark.parametrize("name", CASES)
def test_centred_deltaH(name):
    from oracle import oscillink_oracle as orc

    ref, Y, psi, A, M = _oracle(name)
    t = _terms(ref, Y, A, M)
    psi0 = psi.astype(np.float64)
    for state, U in _states(ref, Y, psi, M).items():
        E0 = U - t["X"] - np.outer(t["x"], psi0)
        h0 = float(np.sum(E0 * (M @ E0)))
        h1 = E0.T @ t["Mx"]
        for q in _queries(Y, psi):
            dl = q - psi0
            dH = h0 - 2 * dl @ h1 + (dl @ dl) * t["h2"]
            E = U - (t["X"] + np.outer(t["x"], q))
            want = float(np.sum(E * (M @ E)))
            scale = max(abs(want), float(np.sum((U - Y) * (M @ (U - Y)))) * 1e-12, 1e-30)
            assert abs(dH - want) <= 1e-9 * scale + 1e-12, (state, dH, want)
            if state != "stationary" or np.any(dl):
                assert dH == pytest.approx(orc.deltaH_trace(U, t["X"] + np.outer(t["x"], q), lambda V: M @ V), rel=1e-5)
        # at U = U*(psi0) the centred form is exactly h0 = 0 at psi0: no cancellation between large terms
        if state == "stationary":
            assert abs(h0) < 1e-18 * max(1.0, float(np.sum(Y.astype(np.float64) ** 2)))


@pytest.mark.parametrize("name", CASES)
def test_coherence_and_null_points_from_the_basis(name):
    ref, Y, psi, A, M = _oracle(name)
    t = _terms(ref, Y, A, M)
    r, c, w = t["r"], t["c"], t["w"]
    N = Y.shape[0]
    lamC = ref.lamC
    sd = ref.sqrt_deg.astype(np.float64)
    for q in _queries(Y, psi):
        U = t["X"] + np.outer(t["x"], q)
        p = t["P"] @ q
        ds, dp = t["s"][r] - t["s"][c], p[r] - p[c]
        # R_ij(psi) = lamC A_ij (d_ij + 2 (s_i - s_j)(p_i - p_j) + (s_i - s_j)^2 |psi|^2)
        R = lamC * w * (t["d"] + 2 * ds * dp + ds * ds * float(q @ q))
        _, _, want_R = yr.edge_residuals(U, A, sd, lamC)
        assert np.allclose(R, want_R, rtol=1e-9, atol=1e-12 * max(1.0, float(np.max(want_R, initial=0.0))))
        # coherence drop: the section-11 per-row form summed
        Yn = Y.astype(np.float64) / (sd[:, None] + 1e-12)
        c0 = np.bincount(r, weights=0.5 * lamC * w * (np.sum((Yn[r] - Yn[c]) ** 2, axis=1) - t["d"]), minlength=N)
        c2 = np.bincount(r, weights=0.5 * lamC * w * ds * ds, minlength=N)
        cross = np.bincount(r, weights=lamC * w * ds * dp, minlength=N)
        coh = c0 - float(q @ q) * c2 - cross
        assert float(np.sum(coh)) == pytest.approx(float(np.sum(yq.coherence_drop(Y, U, A, sd, lamC))), rel=1e-9, abs=1e-9)
        # the dense-row rule from S1 / S2 / first argmax reproduces the oracle's list except on near-tie rows
        s1 = np.bincount(r, weights=R, minlength=N)
        s2 = np.bincount(r, weights=R * R, minlength=N)
        mu = s1 / N
        sigma = np.sqrt(np.maximum(s2 / N - mu * mu, 0.0)) + 1e-12
        got = []
        for i in range(N):
            sel = np.nonzero(r == i)[0]
            if sel.size == 0:
                continue
            e = sel[int(np.argmax(R[sel]))]  # first maximum: columns ascend within a row
            z = (R[e] - mu[i]) / sigma[i]
            if R[e] > 0 and z > yr.Z_TH:
                got.append({"edge": [i, int(c[e])], "z": float(z), "residual": float(R[e])})
        want = yr.receipt(Y, U, q, A, sd, ref.B_diag, ref.lamG, lamC, ref.lamQ, M)
        margin = want["margin"]
        bad = [i for i in yr.differing_rows(got, want["null_points"]) if margin[i] >= 1e-3]
        assert not bad, (bad[:5], [margin[i] for i in bad[:5]])
        if lamC == 0:
            assert got == [] and want["null_points"] == []


def test_yardstick_receipt_matches_oracle_lattice():
    """the yardstick at psi0 is the oracle lattice's own receipt quantities at its (tight) U* solve"""
    ref, Y, psi, A, M = _oracle("g1_n400_d64_k6_chain8")
    want = yr.receipt(Y, ref.U, psi, A, ref.sqrt_deg, ref.B_diag, ref.lamG, ref.lamC, ref.lamQ, M)
    Us = ref.solve_Ustar(tol=1e-7, max_iters=800)
    coh, anc, qry = ref.components(Us)
    assert float(np.sum(anc, dtype=np.float64)) == pytest.approx(want["anchor_pen_sum"], rel=1e-4)
    assert float(np.sum(qry, dtype=np.float64)) == pytest.approx(want["query_term_sum"], rel=1e-4)
    assert float(np.sum(coh, dtype=np.float64)) == pytest.approx(want["coh_drop_sum"], rel=1e-4, abs=1e-4)
    assert ref.deltaH(Us) == pytest.approx(want["deltaH"], rel=1e-4)
    got = ref.nulls(Us)
    bad = [i for i in yr.differing_rows(got, want["null_points"]) if want["margin"][i] >= 1e-3]
    assert not bad

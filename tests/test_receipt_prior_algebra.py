"""The algebra behind receipt_many(chains=..., lamP=...) in float64, without a device: deltaH by the
identity G^T M' = S^T, the anchor and query sums from the moments of the Green's columns, the coherence drop and the null-point
residuals R_ij by the per-(row, query) expansion (tests/_receipt_prior.py), against tests/_receipt_yardstick.py on the dense
M_q = M + lamP L_path,q.

Required: relative 1e-10 on deltaH and the three sums against the float64 value on the yardstick's own U*_q, floored as
tests/test_receipt_algebra.py floors deltaH; R_ij absolute 1e-12 x max R.  The yardstick's deltaH and sums themselves go
through the oracle's float32 rows (oscillink_oracle.deltaH_trace, per_node_components), so against those numbers the bound is
test_receipt_algebra.py's 1e-5."""
import numpy as np
import pytest

from oracle import oscillink_oracle as orc
from tests import _receipt_prior as rp
from tests import _queries as yq
from tests.test_gpu_receipt_many import _batch

cm, yr = rp.cm, rp.yr
LAMPS = (0.2, 0.5)
REL = 1e-10


def _cases(inp):
    rowptr, col, _ = inp["csr"]
    ch = cm.chains(inp)
    a = ch["walk"][2]
    c64 = rp.spread(rowptr, col, 64, start=7)
    return {"walk": (ch["walk"], None), "walk weighted": (ch["walk"], [1.0, 0.5, 2.0, 0.7, 0.3]),
            "mixed": (ch["mixed"], None), "mixed weighted": (ch["mixed"], cm.OWN_WEIGHTS), "[a, a]: m = 1": ([a, a], None),
            "m = 8": (rp.spread(rowptr, col, 8), None),
            "m = 64": (c64 + [c64[0]], [0.25 + (t % 5) * 0.5 for t in range(64)])}


def _states(inp, Y, M, B, lamG, lamQ):
    """U = Y, U after one oracle settle, U = U*(psi0) of the lattice without a chain"""
    kw = {k: v for k, v in inp["kw"].items() if k != "row_cap_val"}
    N = Y.shape[0]
    ref = orc.OracleLattice(inp["Y"], graph=cm.dense_adj(inp["csr"], N).astype(np.float32), **kw)
    ref.set_query(inp["psi"], gates=inp["gates"])
    ref.settle(max_iters=12, tol=1e-3)
    return {"fresh": Y.copy(), "settled": ref.U.astype(np.float64),
            "stationary": yq.ustar(M, Y, B, inp["psi"].astype(np.float64), lamG, lamQ)}


@pytest.mark.parametrize("name", cm.FIXTURES)
def test_identity_moments_and_expansion_against_the_dense_yardstick(name):
    inp = cm.inputs(name)
    Y, A, sd, B, lamG, lamC, lamQ, M = rp.lattice_terms(inp)
    N = Y.shape[0]
    assert N <= yq.DENSE_LIMIT
    psi0 = inp["psi"].astype(np.float64)
    P = _batch(inp["Y"], inp["psi"]).astype(np.float64)
    states = _states(inp, Y, M, B, lamG, lamQ)
    h_fresh = float(np.sum((states["stationary"] - Y) * (M @ (states["stationary"] - Y))))
    worst = {"dH": 0.0, "sums": 0.0, "R": 0.0}
    for lamP in LAMPS:
        Ms = M + lamP * np.eye(N)
        for cname, (chain, weights) in _cases(inp).items():
            Lp, Wp = rp.path_terms(N, chain, weights)
            Mq = M + lamP * Lp
            for q in (0, 2, 5):  # psi0, a large random query, psi = 0
                psi = P[q]
                want = yr.receipt(inp["Y"], states["settled"], psi, A, sd, B, lamG, lamC, lamQ, Mq)
                Uq = want["Ustar"]
                Xs, xs, G, C, nodes = rp.pieces(Ms, Y, B, lamG, lamQ, lamP, Wp, chain, psi)
                assert len(nodes) == len(set(chain))
                K = lamP * Wp[np.ix_(nodes, nodes)]
                for state, U in states.items():
                    got = rp.deltaH_identity(U, Ms, Xs, xs, G, C, nodes, K, psi0, psi)
                    ref = float(np.sum((U - Uq) * (Mq @ (U - Uq))))
                    scale = max(abs(ref), 1e-12 * h_fresh, 1e-30)
                    worst["dH"] = max(worst["dH"], abs(got - ref) / scale)
                    assert abs(got - ref) <= REL * scale + 1e-12, (name, lamP, cname, q, state, got, ref)
                    if state == "settled":
                        assert got == pytest.approx(want["deltaH"], rel=1e-5), (name, lamP, cname, q)
                anchor, query = rp.sums(Y, B, Xs, xs, G, C, psi, lamG, lamQ)
                r, c, R, coh = rp.edges(Y, A, sd, lamC, Xs, xs, G, C, psi)
                ref_a = lamG * float(np.sum((Uq - Y) ** 2))
                ref_q = lamQ * float(np.sum(B[:, None] * (Uq - psi[None, :]) ** 2))
                di = sd.astype(np.float64)[:, None] + 1e-12
                wr, wc, wR = yr.edge_residuals(Uq, A, sd, lamC)
                ref_c = float(np.sum(0.5 * np.asarray(A, np.float64)[wr, wc] * lamC
                                     * np.sum(((Y / di)[wr] - (Y / di)[wc]) ** 2, axis=1)) - 0.5 * np.sum(wR))
                floor = 1e-3 * max(abs(ref_a) + abs(ref_q), 1e-12)
                for key, g, w in (("anchor_pen_sum", anchor, ref_a), ("query_term_sum", query, ref_q),
                                  ("coh_drop_sum", coh, ref_c)):
                    dev = abs(g - w) / max(abs(w), floor)
                    worst["sums"] = max(worst["sums"], dev)
                    assert dev <= REL, (name, lamP, cname, q, key, g, w)
                    assert g == pytest.approx(want[key], rel=1e-5, abs=1e-5 * floor * 1e3), (name, lamP, cname, q, key)
                assert np.array_equal(r, wr) and np.array_equal(c, wc)
                rmax = float(np.max(wR, initial=0.0))
                worst["R"] = max(worst["R"], float(np.max(np.abs(R - wR), initial=0.0)) / max(rmax, 1e-300))
                assert np.all(np.abs(R - wR) <= 1e-12 * rmax), (name, lamP, cname, q)
    print(f"{name}: worst relative deviation: deltaH {worst['dH']:.3g}, sums {worst['sums']:.3g}; R_ij / max R {worst['R']:.3g}")


@pytest.mark.parametrize("name", ["gates_chain_n333_d50_k7", "lam_g03_c0_q0_n240_d40_k6"])
def test_identity_with_inexact_green_columns_and_basis(name):
    """With Green's columns of residual R_G = S - M' G and a perturbed basis, deltaH by the identity differs from the deltaH of
    the implied U*_q = X' + x' psi^T + G C by exactly -<R_G C, (U - U'0) + (U - U*_q)>, within section 12.3's bound
    |R_G C|_F (|U - U'0|_F + |U - U*_q|_F); the basis's own residual does not enter (h0', h1', h2' are quadratic forms of the
    stored basis)."""
    inp = cm.inputs(name)
    Y, A, sd, B, lamG, lamC, lamQ, M = rp.lattice_terms(inp)
    N = Y.shape[0]
    lamP = 0.5
    Ms = M + lamP * np.eye(N)
    rng = np.random.default_rng(11)
    psi0 = inp["psi"].astype(np.float64)
    psi = _batch(inp["Y"], inp["psi"])[2].astype(np.float64)
    U = Y + 0.1 * rng.standard_normal(Y.shape)
    for chain, weights in (cm.chains(inp)["mixed"], cm.OWN_WEIGHTS), (cm.chains(inp)["walk"], None):
        Lp, Wp = rp.path_terms(N, chain, weights)
        Mq = M + lamP * Lp
        Xs, xs, G, _, nodes = rp.pieces(Ms, Y, B, lamG, lamQ, lamP, Wp, chain, psi)
        G = G + 1e-5 * rng.standard_normal(G.shape)
        Xs = Xs + 1e-5 * rng.standard_normal(Xs.shape)
        xs = xs + 1e-5 * rng.standard_normal(xs.shape)
        K = lamP * Wp[np.ix_(nodes, nodes)]
        m = len(nodes)
        C = np.linalg.solve(np.eye(m) - K @ G[nodes], K) @ (Xs[nodes] + xs[nodes, None] * psi[None, :])
        U0 = Xs + np.outer(xs, psi)
        Uq = U0 + G @ C
        got = rp.deltaH_identity(U, Ms, Xs, xs, G, C, nodes, K, psi0, psi)
        implied = float(np.sum((U - Uq) * (Mq @ (U - Uq))))
        exact, bound = rp.identity_bound(Ms, G, C, nodes, U, U0, Uq)
        print(f"{name}: identity - implied = {got - implied:.3e} (exact form {exact:.3e}, bound {bound:.3e}, deltaH {implied:.3e})")
        assert abs((got - implied) - exact) <= 1e-10 * max(abs(implied), 1.0)
        assert abs(got - implied) <= bound * (1 + 1e-12)
        assert abs(got - implied) > 0

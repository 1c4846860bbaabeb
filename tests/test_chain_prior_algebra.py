"""The algebra behind chain_receipt_many(lamP=...) in float64, without a device: for a lattice with no
chain of its own, M + lamP L_path,q = M' - S_q K_q S_q^T with M' = M + lamP I, so by Woodbury
    U*_q = U'0 + G T_q (S_q^T U'0),  T_q = (I - K_q Ghat)^-1 K_q,  G = M'^-1 S_q,  Ghat = S_q^T G,  U'0 = X' + x' psi_q^T,
where M' X' = lamG Y and M' x' = lamQ B -- the basis of the operator with lamG + lamP in lamG's place, X scaled by
lamG / (lamG + lamP).  Checked against the dense solve of M + lamP L_path on the fixtures of tests/_chain_many.py, with the
residual identity the contract rests on: r_c = r0_c + sum_e R_e (T_q V_q)[e, c] for inexact G and U'0."""
import numpy as np
import pytest

from oracle import oscillink_oracle as orc
from tests import _chain_many as cm
from tests import _queries as yq
from tests import _refine_chains as rc

LAMPS = (0.2, 0.5)


def _setup(name):
    inp = cm.inputs(name)
    Y = inp["Y"]
    N = Y.shape[0]
    kw = inp["kw"]
    A = cm.dense_adj(inp["csr"], N)
    sd = orc.normalized_laplacian(A.astype(np.float32))[1]
    lam = (kw.get("lamG", 1.0), kw.get("lamC", 0.5), kw.get("lamQ", 4.0))
    B = np.ones(N, np.float32) if inp["gates"] is None else inp["gates"]
    ch = cm.chains(inp)
    a = ch["walk"][2]
    cases = {"walk": (ch["walk"], None), "walk weighted": (ch["walk"], [1.0, 0.5, 2.0, 0.7, 0.3]),
             "mixed": (ch["mixed"], cm.OWN_WEIGHTS), "aa": ([a, a], None), "aa weighted": ([a, a], [0.25])}
    return inp, Y.astype(np.float64), A, sd, lam, np.asarray(B, np.float64), cases


def _path(N, chain, weights):
    Ap = rc.path_adjacency(N, chain, weights).astype(np.float64)
    dm = 1.0 / np.sqrt(np.maximum(Ap.sum(axis=1), 1e-12))
    Wp = (Ap * dm[:, None]) * dm[None, :]
    return np.eye(N) - Wp, Wp


def _woodbury(Ms, Y, B, lamG, lamQ, lamP, Wp, chain, psi, G=None, U0=None):
    N = Y.shape[0]
    nodes = sorted(set(chain))
    m = len(nodes)
    K = lamP * Wp[np.ix_(nodes, nodes)]
    if G is None:
        E = np.zeros((N, m))
        E[nodes, range(m)] = 1.0
        G = np.linalg.solve(Ms, E)
    if U0 is None:
        Xs, xs = yq.basis(Ms, Y, B, lamG, lamQ)
        U0 = Xs + xs[:, None] * psi[None, :]
    T = np.linalg.solve(np.eye(m) - K @ G[nodes], K)
    TV = T @ U0[nodes]
    return U0 + G @ TV, TV, K, G, nodes


@pytest.mark.parametrize("name", cm.FIXTURES)
def test_woodbury_form_against_the_dense_solve(name):
    inp, Y, A, sd, (lamG, lamC, lamQ), B, cases = _setup(name)
    N = Y.shape[0]
    M = yq.dense_M(A, sd, B, lamG, lamC, lamQ)
    P = cm.queries(inp).astype(np.float64)
    worst = 0.0
    for lamP in LAMPS:
        Ms = M + lamP * np.eye(N)
        # the shifted basis is the basis of the operator with lamG + lamP, X scaled
        Xs, xs = yq.basis(Ms, Y, B, lamG, lamQ)
        Xp, xp = yq.basis(yq.dense_M(A, sd, B, lamG + lamP, lamC, lamQ), Y, B, lamG + lamP, lamQ)
        assert np.max(np.abs(Xs - lamG / (lamG + lamP) * Xp)) <= 1e-12 * max(1.0, np.max(np.abs(Xs)))
        assert np.max(np.abs(xs - xp)) <= 1e-12 * max(1.0, np.max(np.abs(xs)))
        for cname, (chain, weights) in cases.items():
            Lp, Wp = _path(N, chain, weights)
            # L_path is the identity outside the chain's nodes: the update touches those rows and columns alone
            nodes = sorted(set(chain))
            rest = np.setdiff1d(np.arange(N), nodes)
            assert np.count_nonzero(Wp[rest]) == 0 and np.count_nonzero(Wp[:, rest]) == 0
            K = lamP * Wp[np.ix_(nodes, nodes)]
            assert np.linalg.norm(K, 2) <= lamP * (1 + 1e-12)
            for q in (0, 2, 5):
                Uref = yq.ustar(M + lamP * Lp, Y, B, P[q], lamG, lamQ)
                U, _, _, G, _ = _woodbury(Ms, Y, B, lamG, lamQ, lamP, Wp, chain, P[q])
                err = float(np.max(np.abs(U - Uref)))
                worst = max(worst, err)
                assert err <= 1e-10, (name, lamP, cname, q, err)
            # I - K Ghat is far from singular: rho(K Ghat) <= lamP / (lamG + lamP)
            Gh = G[nodes]
            assert np.max(np.abs(np.linalg.eigvals(K @ Gh))) <= lamP / (lamG + lamP) * (1 + 1e-9)
            assert np.linalg.norm(Gh, 2) <= 1.0 / (lamG + lamP) * (1 + 1e-9)
    print(f"{name}: max |U_woodbury - U_dense| = {worst:.3g}")


@pytest.mark.parametrize("name", ["gates_chain_n333_d50_k7", "lam_g03_c0_q0_n240_d40_k6"])
def test_residual_identity_with_perturbed_columns(name):
    """With Green's columns of residual R_e = S e_e - M' G_e and a basis of residual r0 = rhs - M' U'0, the implied U*_q has
    residual r0 + R (T_q V_q) against M_q exactly -- whatever the perturbation -- so |r_c| <= |r0_c| + sum_e |R_e| |(T_q V_q)[e, c]|."""
    inp, Y, A, sd, (lamG, lamC, lamQ), B, cases = _setup(name)
    N = Y.shape[0]
    lamP = 0.5
    M = yq.dense_M(A, sd, B, lamG, lamC, lamQ)
    Ms = M + lamP * np.eye(N)
    rng = np.random.default_rng(4)
    psi = cm.queries(inp)[1].astype(np.float64)
    rhs = lamG * Y + lamQ * B[:, None] * psi[None, :]
    for cname in ("mixed", "walk weighted", "aa"):
        chain, weights = cases[cname]
        Lp, Wp = _path(N, chain, weights)
        nodes = sorted(set(chain))
        m = len(nodes)
        E = np.zeros((N, m))
        E[nodes, range(m)] = 1.0
        G = np.linalg.solve(Ms, E) + 1e-5 * rng.standard_normal((N, m))
        Xs, xs = yq.basis(Ms, Y, B, lamG, lamQ)
        U0 = Xs + xs[:, None] * psi[None, :] + 1e-5 * rng.standard_normal(Y.shape)
        U, TV, K, _, _ = _woodbury(Ms, Y, B, lamG, lamQ, lamP, Wp, chain, psi, G=G, U0=U0)
        R = E - Ms @ G
        r0 = rhs - Ms @ U0
        r = rhs - (M + lamP * Lp) @ U
        scale = max(1.0, float(np.max(np.abs(rhs))))
        assert np.max(np.abs(r - (r0 + R @ TV))) <= 1e-11 * scale, (name, cname)
        bound = np.linalg.norm(r0, axis=0) + np.linalg.norm(R, axis=0) @ np.abs(TV)
        assert np.all(np.linalg.norm(r, axis=0) <= bound * (1 + 1e-9)), (name, cname)
        # the a-priori size of T_q: |T|_2 <= tau = lamP (lamG + lamP) / lamG
        T = np.linalg.solve(np.eye(m) - K @ G[nodes], K)
        assert np.linalg.norm(T, 2) <= lamP * (lamG + lamP) / lamG * (1 + 1e-3), (name, cname)

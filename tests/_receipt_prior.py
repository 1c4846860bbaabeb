"""Float64 restatement of the algebra behind receipt_many(chains=..., lamP=...), checked by
tests/test_receipt_prior_algebra.py against tests/_receipt_yardstick.py on the dense M_q = M + lamP L_path,q.  The device is
never compared with these lines: tests/test_gpu_receipt_prior_many.py takes the fixtures, the chains and the dense yardstick.

U*_q = X' + x' psi^T + G C with (X', x') the basis of M' = M + lamP I, G the Green's columns of M' at the chain's m distinct
nodes, Ghat = G[nodes], K = lamP W_path[nodes, nodes] and C = T_q V_q.  Nothing below forms U*_q."""
import numpy as np

from tests import _chain_many as cm  # noqa: F401  (the fixtures and chains of the tests that import this module)
from tests import _queries as yq
from tests import _receipt_yardstick as yr  # noqa: F401
from tests._bundle_prior import path_terms, pieces, spread  # noqa: F401


def lattice_terms(inp):
    """(Y, A, sd, B, lamG, lamC, lamQ, M) of a fixture without a chain of its own, float64."""
    from oracle import oscillink_oracle as orc

    Y = inp["Y"].astype(np.float64)
    N = Y.shape[0]
    kw = inp["kw"]
    A = cm.dense_adj(inp["csr"], N)
    sd = orc.normalized_laplacian(A.astype(np.float32))[1]
    lamG, lamC, lamQ = kw.get("lamG", 1.0), kw.get("lamC", 0.5), kw.get("lamQ", 4.0)
    B = np.asarray(np.ones(N, np.float32) if inp["gates"] is None else inp["gates"], np.float64)
    return Y, A, sd, B, lamG, lamC, lamQ, yq.dense_M(A, sd, B, lamG, lamC, lamQ)


def deltaH_identity(U, Ms, Xs, xs, G, C, nodes, K, psi0, psi):
    """deltaH under M_q = M' - S K S^T by the identity G^T M' = S^T: m rows of U, X', x' and m x m work per query."""
    E0 = U - Xs - np.outer(xs, psi0)
    Mx = Ms @ xs
    h0 = float(np.sum(E0 * (Ms @ E0)))
    h1 = E0.T @ Mx
    h2 = float(xs @ Mx)
    dl = psi - psi0
    F0 = (E0 - np.outer(xs, dl))[nodes]
    Gh = G[nodes]
    F = F0 - Gh @ C
    return (h0 - 2.0 * dl @ h1 + float(dl @ dl) * h2 - 2.0 * float(np.sum(C * F0)) + float(np.sum(C * (Gh @ C)))
            - float(np.sum(F * (K @ F))))


def sums(Y, B, Xs, xs, G, C, psi, lamG, lamQ):
    """(anchor_pen_sum, query_term_sum) from section 12's sums on (X', x') and the moments of the Green's columns."""
    n2 = float(psi @ psi)
    e, H = C @ psi, C @ C.T
    dxy = Xs - Y
    a0, a1, a2 = float(np.sum(dxy * dxy)), (xs[:, None] * dxy).sum(axis=0), float(xs @ xs)
    b0, b1 = float(np.sum(B[:, None] * Xs * Xs)), ((B * (xs - 1.0))[:, None] * Xs).sum(axis=0)
    b2 = float(np.sum(B * (xs - 1.0) ** 2))
    PA, PB = G.T @ dxy, G.T @ (B[:, None] * Xs)
    ga, gb = G.T @ xs, G.T @ (B * (xs - 1.0))
    GA, GB = G.T @ G, G.T @ (B[:, None] * G)
    anchor = a0 + 2.0 * psi @ a1 + n2 * a2 + 2.0 * float(np.sum(C * PA)) + 2.0 * float(e @ ga) + float(np.sum(H * GA))
    query = b0 + 2.0 * psi @ b1 + n2 * b2 + 2.0 * float(np.sum(C * PB)) + 2.0 * float(e @ gb) + float(np.sum(H * GB))
    return lamG * anchor, lamQ * query


def edges(Y, A, sd, lamC, Xs, xs, G, C, psi):
    """(r, c, R_ij, coh_drop_sum): the null-point residual of every graph edge by the expansion (split quadratic term) and
    the coherence drop's sum by section 11.1's line."""
    n2 = float(psi @ psi)
    e, H = C @ psi, C @ C.T
    di = np.asarray(sd, np.float64) + 1e-12
    s, p = xs / di, (Xs @ psi) / di
    gam, kap = G / di[:, None], (Xs @ C.T) / di[:, None]
    Pn, Yn = Xs / di[:, None], Y / di[:, None]
    r, c = np.nonzero(np.asarray(A) > 0)
    w = np.asarray(A, np.float64)[r, c]
    ds, dp = s[r] - s[c], p[r] - p[c]
    dg, dk = gam[r] - gam[c], kap[r] - kap[c]
    d = np.einsum("ij,ij->i", Pn[r] - Pn[c], Pn[r] - Pn[c])
    nu = np.einsum("ib,bc,ic->i", gam, H, gam)
    x = 2.0 * np.einsum("ib,ib->i", dg, dk + ds[:, None] * e[None, :]) + nu[r] + nu[c] \
        - 2.0 * np.einsum("ib,ib->i", gam[c], gam[r] @ H)
    u2 = d + 2.0 * ds * dp + ds * ds * n2 + x
    yd = Yn[r] - Yn[c]
    coh = float(np.sum(0.5 * lamC * w * (np.einsum("ij,ij->i", yd, yd) - u2)))
    return r, c, lamC * w * u2, coh


def identity_bound(Ms, G, C, nodes, U, U0, Uq):
    """Section 12.3's bound on |deltaH by the identity - deltaH of the implied U*_q|: |R_G C|_F (|U - U'0|_F + |U - U*_q|_F) with
    R_G = S - M' G the Green's columns' residuals; and the exact difference -<R_G C, (U - U'0) + (U - U*_q)>."""
    S = np.zeros_like(G)
    S[nodes, range(len(nodes))] = 1.0
    RC = (S - Ms @ G) @ C
    exact = -float(np.sum(RC * ((U - U0) + (U - Uq))))
    return exact, float(np.linalg.norm(RC)) * (float(np.linalg.norm(U - U0)) + float(np.linalg.norm(U - Uq)))

"""Float64 restatement of the expansion behind bundle_many(chains=..., lamP=...), checked by
tests/test_bundle_prior_algebra.py against bundle() on the dense solve.  The device is never compared with this expansion:
tests/test_gpu_bundle_prior_many.py takes only `path_terms` (the chain's L_path for its dense yardstick) and `spread` (chains
of a given size) from here, and its yardstick is the dense solve of M + lamP L_path itself.

U*_q,i = X'_i + x'_i psi + sum_b G_ib C_b with (X', x') the basis of M' = M + lamP I, G the Green's columns of M' at the
chain's m distinct nodes and C = T_q V_q.  Nothing below forms U*."""
import numpy as np

from oracle import oscillink_oracle as orc
from tests import _queries as yq


def path_terms(N, chain, weights):
    """(L_path, W_path) of a chain as add_chain builds them: normalized_laplacian of path_adjacency, float64."""
    Ap = orc.path_adjacency(N, chain, weights).astype(np.float64)
    dm = 1.0 / np.sqrt(np.maximum(Ap.sum(axis=1), 1e-12))
    Wp = (Ap * dm[:, None]) * dm[None, :]
    return np.eye(N) - Wp, Wp


def pieces(Ms, Y, B, lamG, lamQ, lamP, Wp, chain, psi):
    """(X', x', G, C, nodes) of one (query, chain) pair from the dense M'."""
    N = Y.shape[0]
    nodes = sorted(set(int(c) for c in chain))
    m = len(nodes)
    E = np.zeros((N, m))
    E[nodes, range(m)] = 1.0
    G = np.linalg.solve(Ms, E)
    Xs, xs = yq.basis(Ms, Y, B, lamG, lamQ)
    K = lamP * Wp[np.ix_(nodes, nodes)]
    T = np.linalg.solve(np.eye(m) - K @ G[nodes], K)
    C = T @ (Xs[nodes] + xs[nodes, None] * psi[None, :])
    return Xs, xs, G, C, nodes


def expansion(Y, A, sd, lamC, Xs, xs, G, C, psi, split=True):
    """(align, coh) per row by the lines of DESIGN.md section 11.1; `split` picks the form of dgamma^T H dgamma."""
    psi = np.asarray(psi, np.float64)
    n2 = float(psi @ psi)
    e = C @ psi
    H = C @ C.T
    g = Xs @ psi
    k = Xs @ C.T
    dot = g + xs * n2 + G @ e
    un2 = (np.einsum("ij,ij->i", Xs, Xs) + 2 * xs * g + xs * xs * n2 + 2 * np.einsum("ib,ib->i", G, k + xs[:, None] * e[None, :])
           + np.einsum("ib,bc,ic->i", G, H, G))
    align = dot / (np.sqrt(np.maximum(un2, 0.0)) + 1e-12) / (np.sqrt(n2) + 1e-12)
    di = np.asarray(sd, np.float64) + 1e-12
    s, p, gam, kap = xs / di, g / di, G / di[:, None], k / di[:, None]
    Yn, Pn = Y / di[:, None], Xs / di[:, None]
    r, c = np.nonzero(np.asarray(A) > 0)
    w = np.asarray(A, np.float64)[r, c]
    hw = 0.5 * lamC * w
    yd, pd = Yn[r] - Yn[c], Pn[r] - Pn[c]
    N = Y.shape[0]
    c0, c2, cross, extra = np.zeros(N), np.zeros(N), np.zeros(N), np.zeros(N)
    np.add.at(c0, r, hw * (np.einsum("ij,ij->i", yd, yd) - np.einsum("ij,ij->i", pd, pd)))
    ds, dp = s[r] - s[c], p[r] - p[c]
    np.add.at(c2, r, hw * ds * ds)
    np.add.at(cross, r, lamC * w * ds * dp)
    dg, dk = gam[r] - gam[c], kap[r] - kap[c]
    lin = 2 * np.einsum("ib,ib->i", dg, dk + ds[:, None] * e[None, :])
    if split:
        nu = np.einsum("ib,bc,ic->i", gam, H, gam)
        quad = nu[r] + nu[c] - 2 * np.einsum("ib,ib->i", gam[c], gam[r] @ H)
    else:
        quad = np.einsum("ib,bc,ic->i", dg, H, dg)
    np.add.at(extra, r, hw * (lin + quad))
    return align, c0 - n2 * c2 - cross - extra


def score_of(align, coh, alpha=0.5):
    mu, sigma = coh.mean(), coh.std() + 1e-12
    return alpha * (coh - mu) / sigma + (1 - alpha) * align


def spread(rowptr, col, m, start=0):
    """m distinct nodes: a walk along the graph's edges from `start`, then the rows after it that are not on it."""
    from tests._chain_many import walk

    w = walk(rowptr, col, start, m)
    on = set(w)
    rest = [i for i in range(len(rowptr) - 1) if i not in on]
    return (w + rest)[:m]

"""Float64 yardstick for gated candidate lattices (Corpus.refine_many(gates=...)): the diffusion
gates by a dense solve of L_sym + gamma I (reference preprocess/diffusion.py:35-124 in float64), and the test corpus and
settings the gated tests share.  The gated bundle itself goes through tests/_queries (dense_M with B = gates)."""
import numpy as np

# (top_k, k, refine settings, beta, gamma): test_refine_many_against_loop's corpus and settings
SETTINGS = [
    (100, 8, {}, 1.0, 0.15),
    (64, 8, {"kneighbors": 16}, 1.2, 0.1),
    (30, 40, {"lamG": 2.0, "lamC": 1.5, "lamQ": 0.5, "row_cap_val": 0.3}, 1.0, 0.5),
    (7, 8, {"kneighbors": 2000}, 1.0, 0.15),
]


def corpus(top_k, k):
    """2000 x 96, six clusters, 5 queries; query 1 sits inside a cluster (Y[5] + 0.1 noise)."""
    rng = np.random.default_rng(top_k + k)
    centers = rng.standard_normal((6, 96)).astype(np.float32) * 2
    Y = (centers[rng.integers(0, 6, 2000)] + 0.5 * rng.standard_normal((2000, 96))).astype(np.float32)
    P = rng.standard_normal((5, 96)).astype(np.float32)
    P[1] = Y[5] + 0.1 * rng.standard_normal(96).astype(np.float32)
    return Y, P


def lattice_kw(kw):
    return dict(kneighbors=kw.get("kneighbors", 6), row_cap_val=kw.get("row_cap_val", 1.0), lamG=kw.get("lamG", 1.0),
                lamC=kw.get("lamC", 0.5), lamQ=kw.get("lamQ", 4.0))


def host_cos(Y, P):
    Yd = Y.astype(np.float64)
    Yn = Yd / (np.linalg.norm(Yd, axis=1, keepdims=True) + 1e-12)
    Pd = np.atleast_2d(P).astype(np.float64)
    return (Yn @ Pd.T).T / (np.linalg.norm(Pd, axis=1, keepdims=True) + 1e-12)


def dense_adj(csr, n):
    """Dense capped adjacency from (rowptr, col, a, ...)."""
    rowptr, col, a = csr[0], csr[1], csr[2]
    A = np.zeros((n, n))
    A[np.repeat(np.arange(n), np.diff(rowptr)), col] = a
    return A


def laplacian64(A, sqrt_deg):
    """L_sym as tests/_queries.dense_M builds it."""
    A = np.asarray(A, np.float64)
    dm = 1.0 / np.asarray(sqrt_deg, np.float64)
    return np.eye(A.shape[0]) - (A * dm[:, None]) * dm[None, :]


def source64(Yc, psi, beta):
    Yd = np.asarray(Yc, np.float64)
    Yn = Yd / (np.linalg.norm(Yd, axis=1, keepdims=True) + 1e-12)
    p = np.asarray(psi, np.float64)
    return beta * np.maximum(0.0, Yn @ (p / (np.linalg.norm(p) + 1e-12)))


def gates64(A, sqrt_deg, Yc, psi, beta, gamma):
    """(gates, raw h, s): (L_sym + gamma I) h = s = beta max(0, cos(Yc_i, psi)) solved densely in float64, then the
    reference's min-max normalisation (ones when max h - min h < 1e-12) and clip."""
    n = np.asarray(A).shape[0]
    s = source64(Yc, psi, beta)
    raw = np.linalg.solve(laplacian64(A, sqrt_deg) + gamma * np.eye(n), s)
    lo, hi = raw.min(), raw.max()
    g = np.ones(n) if hi - lo < 1e-12 else (raw - lo) / (hi - lo)
    return np.clip(g, 0.0, 1.0), raw, s


def oracle_cg(orc, A, sqrt_deg, s, gamma, tol, max_iters):
    """oracle.cg_solve of (L_sym + gamma I) h = s in float32 on the given graph: (h, iters, residual history)."""
    L = laplacian64(A, sqrt_deg).astype(np.float32)
    g32 = np.float32(gamma)
    hist = []
    h, it, _ = orc.cg_solve(lambda x: (L @ x) + g32 * x, np.asarray(s, np.float32), x0=None,
                            M_diag=np.diag(L).astype(np.float32) + g32, tol=tol, max_iters=max_iters, history=hist)
    return np.asarray(h), it, hist

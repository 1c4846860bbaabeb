"""Float64 yardstick for multi-query bundles: U*(psi) solved exactly (dense, N <= 2000) and bundle() from it with the
reference's formulas (lattice.py:530-568, receipts.py:28-38) and MMR tie rule (graph.py:114-133: first maximum)."""
import numpy as np

DENSE_LIMIT = 2000


def dense_M(A, sqrt_deg, B, lamG, lamC, lamQ, lamP=0.0, L_path=None):
    """M = lamG I + lamC L_sym + lamQ diag(B) (+ lamP L_path), float64; A the capped adjacency."""
    A = np.asarray(A, dtype=np.float64)
    N = A.shape[0]
    assert N <= DENSE_LIMIT
    dm = 1.0 / np.asarray(sqrt_deg, dtype=np.float64)
    L = np.eye(N) - (A * dm[:, None]) * dm[None, :]
    M = lamG * np.eye(N) + lamC * L + lamQ * np.diag(np.asarray(B, dtype=np.float64))
    if L_path is not None and lamP > 0:
        M = M + lamP * np.asarray(L_path, dtype=np.float64)
    return M


def basis(M, Y, B, lamG, lamQ):
    """(X, x) with M X = lamG Y, M x = lamQ B: U*(psi) = X + x psi^T."""
    rhs = np.concatenate([lamG * np.asarray(Y, dtype=np.float64), lamQ * np.asarray(B, dtype=np.float64)[:, None]], axis=1)
    S = np.linalg.solve(M, rhs)
    return S[:, :-1], S[:, -1]


def ustar(M, Y, B, psi, lamG, lamQ):
    rhs = lamG * np.asarray(Y, np.float64) + lamQ * np.asarray(B, np.float64)[:, None] * np.asarray(psi, np.float64)[None, :]
    return np.linalg.solve(M, rhs)


def coherence_drop(Y, U, A, sqrt_deg, lamC):
    """coh_drop per node (receipts.py:28-38); A dense or a CSR tuple (rowptr, col, a)."""
    di = np.asarray(sqrt_deg, dtype=np.float64)[:, None] + 1e-12
    Yn = np.asarray(Y, np.float64) / di
    Un = np.asarray(U, np.float64) / di
    if isinstance(A, tuple):  # CSR (rowptr, col, a) of the capped adjacency
        rowptr, c, w = A
        r = np.repeat(np.arange(Y.shape[0]), np.diff(rowptr))
        keep = w > 0
        r, c, w = r[keep], c[keep], w[keep].astype(np.float64)
    else:
        r, c = np.nonzero(np.asarray(A) > 0)
        w = np.asarray(A, dtype=np.float64)[r, c]
    yd = Yn[r] - Yn[c]
    ud = Un[r] - Un[c]
    coh = np.zeros(Y.shape[0])
    np.add.at(coh, r, 0.5 * lamC * w * (np.einsum("ij,ij->i", yd, yd) - np.einsum("ij,ij->i", ud, ud)))
    return coh


def mmr(Y, scores, k, lambda_div=0.5):
    """mmr_diversify in float64; also the margin of each step (best value - runner-up value)."""
    Yd = np.asarray(Y, np.float64)
    Yn = Yd / (np.linalg.norm(Yd, axis=1, keepdims=True) + 1e-12)
    N = Yd.shape[0]
    base = (1.0 - lambda_div) * np.asarray(scores, np.float64)
    maxsim = np.zeros(N)
    alive = np.ones(N, dtype=bool)
    chosen, margins = [], []
    for step in range(min(k, N)):
        val = np.where(alive, base - (lambda_div * maxsim if step else 0.0), -np.inf)
        i = int(np.argmax(val))  # first maximum
        rest = np.delete(val, i)
        margins.append(float(val[i] - rest.max()) if rest.size and np.isfinite(rest.max()) else np.inf)
        chosen.append(i)
        alive[i] = False
        sim = Yn @ Yn[i]
        maxsim = sim if step == 0 else np.maximum(maxsim, sim)
    return chosen, margins


def bundle(Y, U, psi, A, sqrt_deg, lamC, k=8, alpha=0.5):
    """(ids, score, align, margins) of bundle(k, alpha) for the stationary state U."""
    U = np.asarray(U, np.float64)
    psi = np.asarray(psi, np.float64)
    align = (U / (np.linalg.norm(U, axis=1, keepdims=True) + 1e-12)) @ (psi / (np.linalg.norm(psi) + 1e-12))
    coh = coherence_drop(Y, U, A, sqrt_deg, lamC)
    mu, sigma = coh.mean(), coh.std() + 1e-12
    score = alpha * (coh - mu) / sigma + (1 - alpha) * align
    ids, margins = mmr(Y, score, k)
    return ids, score[ids], align[ids], margins


def same_until_near_tie(got, want, margins, eps):
    """True iff the id lists agree up to the first step whose margin is below eps; second value: truncated or not."""
    for t, (g, w) in enumerate(zip(got, want)):
        if margins[t] < eps:
            return True, True
        if g != w:
            return False, False
    return len(got) == len(want), False

"""Float64 yardstick for multi-query receipts: U*(psi) from a dense solve (N <= 2000), then the
oracle's per_node_components / deltaH_trace / null_points on it, plus the margin of every row's null-point decision."""
import numpy as np

from tests import _queries as yq

Z_TH = 3.0


def edge_residuals(Ustar, A, sqrt_deg, lamC):
    """(r, c, R) with R_ij = lamC A_ij |Un_i - Un_j|^2 in float64 over the positive entries of A (row-major)."""
    A = np.asarray(A, dtype=np.float64)
    r, c = np.nonzero(A > 0)
    Un = np.asarray(Ustar, np.float64) / (np.asarray(sqrt_deg, np.float64)[:, None] + 1e-12)
    d = Un[r] - Un[c]
    return r, c, lamC * A[r, c] * np.einsum("ij,ij->i", d, d)


def null_margins(r, R, N, z_th=Z_TH):
    """Per row: min(top-two R gap relative to the largest, |z - z_th|) of the dense-row rule (inf for rows without edges)."""
    s1 = np.bincount(r, weights=R, minlength=N)
    s2 = np.bincount(r, weights=R * R, minlength=N)
    mu = s1 / N
    sigma = np.sqrt(np.maximum(s2 / N - mu * mu, 0.0)) + 1e-12
    margin = np.full(N, np.inf)
    if r.size == 0:
        return margin
    order = np.lexsort((-R, r))
    rs, Rs = r[order], R[order]
    starts = np.r_[0, np.nonzero(rs[1:] != rs[:-1])[0] + 1]
    for t, s in enumerate(starts):
        i = int(rs[s])
        e = starts[t + 1] if t + 1 < len(starts) else rs.size
        top = Rs[s]
        gap = (top - Rs[s + 1]) / max(abs(top), 1e-30) if e - s > 1 else np.inf
        z = (top - mu[i]) / sigma[i]
        margin[i] = min(gap, abs(z - z_th))
    return margin


def receipt(Y, U, psi, A, sqrt_deg, B, lamG, lamC, lamQ, M, z_th=Z_TH):
    """dict of deltaH / the three sums / null points (oracle formulas at the exact U*(psi)) and the per-row margins."""
    from oracle import oscillink_oracle as orc

    Y = np.asarray(Y, np.float32)
    psi = np.asarray(psi, np.float32)
    Us = yq.ustar(M, Y, B, psi, lamG, lamQ)
    coh, anc, qry = orc.per_node_components(Y.astype(np.float64), Us, np.asarray(A, np.float64),
                                            np.asarray(sqrt_deg, np.float64), lamG, lamC, lamQ,
                                            np.asarray(B, np.float64), psi.astype(np.float64))
    dH = orc.deltaH_trace(np.asarray(U, np.float64), Us, lambda V: M @ V)
    nulls = orc.null_points(Us.astype(np.float32), np.asarray(A, np.float32), np.asarray(sqrt_deg, np.float32), lamC, z_th)
    r, _, R = edge_residuals(Us, A, sqrt_deg, lamC)
    return {"deltaH": float(dH), "coh_drop_sum": float(np.sum(coh, dtype=np.float64)),
            "anchor_pen_sum": float(np.sum(anc, dtype=np.float64)), "query_term_sum": float(np.sum(qry, dtype=np.float64)),
            "null_points": nulls, "margin": null_margins(r, R, Y.shape[0], z_th), "Ustar": Us}


def null_edges(nulls):
    """{row: col} of a null-point list."""
    return {int(p["edge"][0]): int(p["edge"][1]) for p in nulls}


def differing_rows(got, want):
    """Rows whose null point differs (present in one list only, or a different edge)."""
    g, w = null_edges(got), null_edges(want)
    return sorted(i for i in set(g) | set(w) if g.get(i) != w.get(i))

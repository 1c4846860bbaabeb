"""Inputs and float64 yardstick shared by tests/test_gpu_bundle_gated_many.py and tests/test_bundle_gated_host.py
(bundle_gated_many): the seeded shapes of the seams, the five (query, gates) pairs of a case,
and the per-query comparison against tests/_queries."""
import numpy as np

from tests import _gated as yg
from tests import _queries as yq

NEAR_TIE = 1e-4
GATE_BETA, GATE_GAMMA = 1.0, 0.1
TOL = 1e-4
LOOP_ITERS = 64  # the reference loop's solve_Ustar(): tol 1e-4, 64 iterations at most

# name: (N, D, kneighbors, bundle k, seed, clustered)
CASES = {
    "seam_n97_d40": (97, 40, 6, 6, 11, False),     # three full 32-row steps and one row; two slabs, the second 8 wide
    "d64": (97, 64, 6, 6, 12, False),               # exactly two slabs
    "d1": (97, 1, 6, 6, 13, False),
    "d33": (97, 33, 6, 6, 14, False),
    "n2": (2, 40, 1, 1, 15, False),
    "n33": (33, 40, 6, 6, 16, False),
    "reordered_n1500_d33": (1500, 33, 8, 6, 7, True),
}
ITERS_CASE = "seam_n97_d40"  # case 7 (iteration counts) runs on the first case's inputs


def anchors(name):
    N, D, _, _, seed, clustered = CASES[name]
    rng = np.random.default_rng(seed)
    if clustered:  # test_routes_against_per_query_path's recipe
        centers = rng.standard_normal((N // 100, D)).astype(np.float32)
        Y = centers[np.arange(N) % centers.shape[0]] + 0.15 * rng.standard_normal((N, D)).astype(np.float32)
        Y = Y[rng.permutation(N)]
    else:
        Y = rng.standard_normal((N, D)).astype(np.float32)
    return np.ascontiguousarray(Y, dtype=np.float32)


def queries(name, Y):
    """random, an anchor row, 3 x scale, psi = 0, 1 / sqrt(D) scale"""
    N, D = Y.shape
    rng = np.random.default_rng(CASES[name][4] + 1000)
    rows = [rng.standard_normal(D), Y[min(5, N - 1)], 3.0 * rng.standard_normal(D), np.zeros(D),
            rng.standard_normal(D) / np.sqrt(D)]
    return np.stack(rows).astype(np.float32)


def given_gates(name, N):
    """uniform [0, 1), all ones, all zeros, a 0/1 mask; the fifth row (the query's diffusion gates) is the caller's"""
    rng = np.random.default_rng(CASES[name][4] + 2000)
    G = np.zeros((5, N), dtype=np.float32)
    G[0] = rng.uniform(0.0, 1.0, N)
    G[1] = 1.0
    G[3] = (rng.uniform(0.0, 1.0, N) < 0.5)
    return G


def dense_graph(csr, N):
    """(A dense float64, sqrt_deg) from graph_csr()'s tuple"""
    return yg.dense_adj(csr, N), np.asarray(csr[4], np.float64)


def yardstick(Y, A, sd, psi, g, lams, k):
    """float64 (U*, ids, score, align, margins) of set_query(psi, gates=g); bundle(k, 0.5)"""
    lamG, lamC, lamQ = lams
    M = yq.dense_M(A, sd, g, lamG, lamC, lamQ)
    U = yq.ustar(M, Y, g, psi, lamG, lamQ)
    ids, score, align, margins = yq.bundle(Y, U, psi, A, sd, lamC, k=k)
    return M, U, ids, score, align, margins


def first_near_tie(margins):
    """index of the first pick whose margin is below NEAR_TIE, or None"""
    return next((t for t, m in enumerate(margins) if m < NEAR_TIE), None)


def cut_before_last(margins):
    t = first_near_tie(margins)
    return t is not None and t < len(margins) - 1


def history_clear_of_tol(hist, tol=TOL, band=0.05):
    """the 5 % condition of the iteration-count case: a converged history ends at least 5 % below tol, one step after a
    residual at least 5 % above it; an unconverged one stays 5 % above throughout"""
    if hist[-1] <= tol:
        return hist[-1] <= (1 - band) * tol and (len(hist) < 2 or hist[-2] >= (1 + band) * tol)
    return min(hist) >= (1 + band) * tol

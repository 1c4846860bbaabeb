"""Shared pieces of tests/test_gpu_small_solve.py: seeded inputs, the oracle on a device-built graph, and a float64
solution of the stationary system M U* = rhs on that same graph.

M is what `OracleLattice.M_mul` states -- lamG I + lamC (I - W) + lamQ diag(B) (+ lamP (I - W_path) iff a chain is present
and lamP > 0), W = D^-1/2 A D^-1/2 with sqrt_deg = sqrt(max(row sum, 1e-12)) -- assembled in float64 from the float32
adjacency the device reports, and solved by a sparse direct factorisation (SuperLU through scipy.sparse.linalg)."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from tests._cases import make_inputs

CHAIN_LAMP = 0.2


def inputs(N, D, seed=0):
    """Seeded standard_normal anchors and a unit-norm query, as tests/_cases.make_inputs draws them."""
    return make_inputs({"N": N, "D": D, "seed": seed, "gen": "default_rng", "psi_mode": "random"})


def gates_with_exact_ends(N, seed=1):
    """Gates in [0, 1] with entries exactly 0.0 (an anchor-only row) and exactly 1.0."""
    g = np.random.default_rng(seed).uniform(0.0, 1.0, size=N).astype(np.float32)
    g[[0, 3, N // 3, N - 1]] = 0.0
    g[[1, 4, N // 2, N - 2]] = 1.0
    return g


def chain_for(N):
    return [5, 1, N - 1, N // 2, 7, 2]


def adjacency(lat):
    """The lattice's capped adjacency as SciPy CSR (float32), from graph_csr()."""
    rp, col, a, _, _ = lat.graph_csr()
    A = sp.csr_matrix((a.astype(np.float32), col.astype(np.int32), rp.astype(np.int64)), shape=(lat.N, lat.N))
    A.sort_indices()
    return A


def oracle_on(orc, lat, Y, kneighbors):
    """The sparse oracle on the graph the device built: kNN ties play no part in what follows."""
    return orc.OracleLattice(Y, kneighbors=kneighbors, deterministic_k=True, dense=False, graph=adjacency(lat))


def configure(L, psi, gates=None, chain=None):
    L.set_query(psi, gates=gates)
    if chain is not None:
        L.add_chain(chain, lamP=CHAIN_LAMP)


def _laplacian64(A):
    A = sp.csr_matrix(A, dtype=np.float64)
    d = np.asarray(A.sum(axis=1)).ravel()
    inv = 1.0 / np.sqrt(np.maximum(d, 1e-12))
    return sp.identity(A.shape[0], dtype=np.float64, format="csr") - sp.diags(inv) @ A @ sp.diags(inv)


def ustar_fp64(orc, A, Y, psi, gates=None, chain=None, lamG=1.0, lamC=0.5, lamQ=4.0, lamP=CHAIN_LAMP):
    """(U* float64 (N, D), the largest column residual ||M x - rhs||_2 of the direct solve)."""
    N = Y.shape[0]
    B = np.ones(N) if gates is None else gates.astype(np.float64)
    M = lamG * sp.identity(N, dtype=np.float64, format="csr") + lamC * _laplacian64(A) + lamQ * sp.diags(B)
    if chain is not None and lamP > 0.0:
        M = M + lamP * _laplacian64(orc.path_adjacency(N, chain, None, dense=False))
    rhs = lamG * Y.astype(np.float64) + lamQ * B[:, None] * psi.astype(np.float64)[None, :]
    M = sp.csc_matrix(M)
    # (minimum degree on the pattern of M + M^T: a third of COLAMD's fill on these symmetric graphs, 3.6 s against 14 s at
    # N = 6000)
    X = spla.splu(M, permc_spec="MMD_AT_PLUS_A").solve(rhs)
    return X, float(np.linalg.norm(M @ X - rhs, axis=0).max())

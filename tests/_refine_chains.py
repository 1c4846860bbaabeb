"""Cases and float64 yardstick of Corpus.refine_many(chains=...), shared by
tests/test_refine_chains_host.py (the CPU proof that the cases do not rest on a knife edge) and
tests/test_gpu_refine_chains.py.

The lattices are the smallest that reach every place the path term can go wrong -- the row / slot indexing and the column
groups: a plain chain, a chain with a self-step, a revisited edge (max weight) and a node with three path neighbours that
ends on the last row, a lattice whose every row is on the chain, chain rows on both sides of the 256-row stride, and NC = 2
with one live column in the second group."""
import numpy as np

from tests import _refine_shapes as rs

KNEIGHBORS = 6
K_BUNDLE = 8
ALPHA = 0.5
Z_TH = 2.5
N_QUERIES = 5

# (name, top_k, chain, weights, lamP)
CASES = [
    ("plain100", 100, list(range(8)), None, 0.2),
    ("weights64", 64, [0, 3, 3, 9, 0, 3, 63], [1, .5, 2, .7, .3, 1.5], 0.5),
    ("all7", 7, [6, 0, 1, 2, 3, 4, 5], None, 0.2),
    ("stride300", 300, [0, 299, 256, 1, 257, 255], None, 1.0),
    ("nc2", 100, list(range(8)), None, 0.2),
]
CASE = {c[0]: c for c in CASES}


def clustered(top_k, k):
    """test_refine_many_against_loop's corpus: 2000 x 96, six clusters, seed = top_k + k, five queries."""
    rng = np.random.default_rng(top_k + k)
    centers = rng.standard_normal((6, 96)).astype(np.float32) * 2
    Y = (centers[rng.integers(0, 6, 2000)] + 0.5 * rng.standard_normal((2000, 96))).astype(np.float32)
    P = rng.standard_normal((5, 96)).astype(np.float32)
    return Y, P


_CORPORA = {}


def corpus(name):
    """(Y, P) of a case, five queries, built once per process and read-only.  "nc2" runs on _refine_shapes' (257, 100)
    corpus; its three queries are followed by two more from a generator of their own."""
    if name not in _CORPORA:
        if name == "nc2":
            Y, P3 = rs.cached_corpus(257, 100)
            P = np.concatenate([P3, np.random.default_rng(257 + 100 + 1).standard_normal((2, 257)).astype(np.float32)])
        else:
            Y, P = clustered(CASE[name][1], K_BUNDLE)
        Y.setflags(write=False)
        P.setflags(write=False)
        _CORPORA[name] = (Y, P)
    return _CORPORA[name]


def path_adjacency(K, chain, weights=None):
    """build_path_laplacian's A (graph.py:96-111), float32."""
    A = np.zeros((K, K), dtype=np.float32)
    w = [1.0] * (len(chain) - 1) if weights is None else weights
    for t in range(len(chain) - 1):
        i, j = int(chain[t]), int(chain[t + 1])
        A[i, j] = max(A[i, j], float(w[t]))
        A[j, i] = max(A[j, i], float(w[t]))
    return A


def chain_yardstick(Us, Yc, A, sqrt_deg, lamC, Ap, chain):
    """chain_receipt (lattice.py:466-528) in float64 on a given U*: per chain edge z, R, and the row's mu and sigma for the
    structural and the path residuals, the gain's terms and the sum of the magnitudes of what the gain adds up."""
    di = np.asarray(sqrt_deg, np.float64) + 1e-12
    Un = np.asarray(Us, np.float64) / di[:, None]
    Yn = np.asarray(Yc, np.float64) / di[:, None]
    A = np.asarray(A, np.float64)
    Ap = np.asarray(Ap, np.float64)
    out = {k: [] for k in ("z_struct", "z_path", "r_struct", "r_path", "bound_struct", "bound_path", "term")}
    mag = 0.0
    for t in range(len(chain) - 1):
        i, j = int(chain[t]), int(chain[t + 1])
        d2 = np.sum((Un[i][None, :] - Un) ** 2, axis=1)
        for name, R in (("struct", lamC * A[i] * d2), ("path", max(lamC, 1e-6) * Ap[i] * d2)):
            mu, sig = float(R.mean()), float(R.std()) + 1e-12
            out["z_" + name].append((float(R[j]) - mu) / sig)
            out["r_" + name].append(float(R[j]))
            out["bound_" + name].append((abs(float(R[j])) + abs(mu)) / sig)  # the rounding of R - mu, in units of z
        dy, du = float(np.sum((Yn[i] - Yn[j]) ** 2)), float(d2[j])
        w = max(float(A[i, j]), 0.0)
        out["term"].append(0.5 * lamC * w * (dy - du))
        mag += 0.5 * lamC * w * (dy + du)
    out = {k: np.asarray(v) for k, v in out.items()}
    out["gain"] = float(np.sum(out["term"]))
    out["gain_magnitude"] = mag
    out["zmax"] = np.maximum(out["z_struct"], out["z_path"])
    return out

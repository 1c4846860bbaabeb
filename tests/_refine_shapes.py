"""The (D, top_k) shapes that take Corpus.refine_many's per-lattice kernels past 256 columns and
256 rows, and the corpus they run on.  Shared by tests/test_refine_shapes_host.py (the CPU proof of the yardstick's
margins) and tests/test_gpu_refine_shapes.py.

One workgroup of 256 threads runs a lattice.  The columns per thread are compiled in: cq_with_nc dispatches on
ceil(ldn / 256) to NC in {1, 2, 3, 4, 6} (5 falls through to 6), ldn = D rounded up to 32.  Rows beyond 256 go through
`r += 256` strides (row ownership in k_cq_gates and the bundle, the row constants in LDS of k_cq_solve / k_cq_settle)
and through k_cq_receipt's 256-row emit rounds (uncapped) or its rank count (capped)."""
import numpy as np

N_ROWS = 1200
N_QUERIES = 3

# (D, top_k): what it reaches
SHAPES = [
    (257, 100),    # NC = 2 with one live column in the second group; ldn 288 > D (pad columns)
    (300, 300),    # NC = 2; the second row per thread is partly filled
    (520, 64),     # NC = 3, D not a multiple of 32
    (800, 257),    # NC = 4; exactly one row in the second round
    (1040, 100),   # ceil(ldn / 256) = 5 -> NC = 6 with the last group fully masked
    (1100, 300),   # the same, with K > 256
    (1290, 100),   # NC = 6, ragged last group (ldn 1312)
    (1536, 1024),  # both limits at once
    (96, 1024),    # NC = 1 with four rows per thread (separates a row bug from a column bug)
    (1536, 7),     # widest columns on the smallest lattice
]

KNEIGHBORS = 6
K = 8
ALPHA = 0.5
GATE_BETA = 1.0
GATE_GAMMA = 0.15
GATE_KW = {"gates": "diffusion", "gate_beta": GATE_BETA, "gate_gamma": GATE_GAMMA}

# (D, top_k, k, lattice settings, settle_dt): two more settings rows on (520, 64)
EXTRA = [
    (520, 64, 64, {}, 1.0),  # MMR over every row
    (520, 64, 8, {"lamG": 2.0, "lamC": 1.5, "lamQ": 0.5, "row_cap_val": 0.3}, 0.5),  # cq_rounded_mul at NC = 3
]


def ldn(D):
    return (D + 31) // 32 * 32


def corpus(D, top_k):
    """1200 x D, six clusters, 3 queries; query 1 sits inside a cluster (Y[5] + 0.1 noise).  tests/_gated.corpus's recipe,
    seeded by D + top_k."""
    rng = np.random.default_rng(D + top_k)
    centers = rng.standard_normal((6, D)).astype(np.float32) * 2
    Y = (centers[rng.integers(0, 6, N_ROWS)] + 0.5 * rng.standard_normal((N_ROWS, D))).astype(np.float32)
    P = rng.standard_normal((N_QUERIES, D)).astype(np.float32)
    P[1] = Y[5] + 0.1 * rng.standard_normal(D).astype(np.float32)
    return Y, P


_CORPORA = {}


def cached_corpus(D, top_k):
    """corpus(D, top_k), built once per process and read-only."""
    key = (D, top_k)
    if key not in _CORPORA:
        Y, P = corpus(D, top_k)
        Y.setflags(write=False)
        P.setflags(write=False)
        _CORPORA[key] = (Y, P)
    return _CORPORA[key]

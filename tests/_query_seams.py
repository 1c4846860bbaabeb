"""Shared pieces of the query-seam tests (tests/test_query_seams_host.py, tests/test_gpu_query_seams.py): seeded inputs,
the shape tables, and two float64 references of `bundle_many` / `receipt_many` that share no code with the kernels.

Both references evaluate the reference's formulas (tests/_queries.py: bundle; oracle per_node_components / deltaH_trace /
null_points, restated here in float64 for a given U*) on U*(psi_q) = X + x psi_q^T:

* reference A takes (X, x) from one dense float64 solve of the lattice's own operator (`yq.dense_M`, `yq.basis`): end to end;
* reference B takes the device's own float32 basis (`lat.query_basis()`): the CG solve drops out and what remains is the
  arithmetic of the GEMM, the graph pass, the statistics and the MMR.

The same formulas also run in plain float32 numpy (`dt=np.float32`) -- only to measure, on the CPU, how far float32
arithmetic alone moves the results: the tolerance of reference B below."""
import numpy as np

from tests import _queries as yq
from tests import _receipt_yardstick as yr

NEAR_TIE = 1e-4   # bundle ids: compared up to the first MMR step whose float64 margin is below this
NEAR = 1e-3       # null points: may differ only on rows whose float64 margin is below this
A_ATOL = 2e-4     # reference A: score and align
A_RTOL = 1e-4     # reference A: the three sums (rule of test_fixtures_against_yardstick_and_loop) and deltaH_total
K = 8
ALPHA = 0.5
QMAX = 300
SUMS = ("coh_drop_sum", "anchor_pen_sum", "query_term_sum")

# Reference B's tolerance: twice the largest distance of the plain float32 numpy evaluation (basis = reference A's float64
# basis cast to float32) from the float64 evaluation, over every entry of the tables below, measured on the CPU by
# tests/test_query_seams_host.py::test_float32_distance_of_every_case (which asserts that no case exceeds these).
# The factor two allows the kernels a different, fixed summation order.  Never derived from the kernels' output.
#   score, align: absolute, over all rows of all queries;  sums: |got - want| / max(|want|, 1e-3 (|anchor| + |query|));
#   deltaH: relative.
F32_DIST = {"score": 2.93e-6, "align": 2.85e-7, "sums": 2.29e-7, "deltaH": 2.42e-7}
F32_SOURCE = {"score": "degree-built-k140",       # N = 300, D = 32, kneighbors = 140, Q = 70
              "align": "degree-empty_rows-d261",  # N = 300, D = 261, injected graph with 243 empty rows, Q = 70
              "sums": "degree-empty_rows-d261",
              "deltaH": "width-d768-plain"}       # N = 333, D = 768, kneighbors = 8, Q = 7
B_TOL = {k: 2.0 * v for k, v in F32_DIST.items()}

# ---------------------------------------------------------------------------------------------------------------- tables
# case 1 -- column widths at N = 333 (two full 128-row tiles and 77 rows), kneighbors 8, Q = 7: (D, variant, seed, reaches)
WIDTH_N, WIDTH_KNN, WIDTH_Q = 333, 8, 7
WIDTHS = [
    (3, "plain", 11, "one masked4 with three dead lanes; kpad 32 for 3 columns"),
    (5, "plain", 12, "D % 4 == 1"),
    (33, "plain", 113, "kpad 64, one column past a multiple of 32: the k < D guard of k_query_gemm"),
    (255, "plain", 14, "D % 4 == 3; the last width whose `c += 256` loops make one trip"),
    (257, "plain", 15, "first second trip of the lane loops (one live column in it); k_rm_cols two blocks high"),
    (261, "plain", 16, "second trip with a masked4 tail; kpad 288"),
    (261, "gates_chain", 17, "the same with gates and a chain: k_rm_cols' scalar sums at blockIdx.y == 0 only"),
    (515, "plain", 18, "three trips, tail D % 4 == 3"),
    (768, "plain", 19, "the workload's width: three full trips"),
    (772, "plain", 20, "four trips, the last one a single float4; kpad 800"),
    (772, "gates_chain", 21, "the same with gates and a chain"),
]

# case 2 -- query counts: every batch is the first Q rows of one 300-row batch per lattice
QUERY_COUNTS = [
    (1, "one query: row pitch 4 > nq"),
    (2, "qs 4 > nq 2"),
    (63, "last count inside lane slot u = 0; qs 64 > nq"),
    (64, "slot u = 0 full"),
    (65, "first query of slot u = 1; qs 68"),
    (127, "qs 128 > nq"),
    (128, "one full Q tile of k_query_gemm"),
    (129, "second Q tile (blockIdx.y = 1); slot u = 2"),
    (255, "slot u = 3, qs 256 > nq"),
    (256, "one full chunk"),
    (257, "second chunk of one query"),
    (300, "second chunk of 44 queries, qs 44"),
]
QUERY_LATTICES = {  # name -> (fixture name or None, N, D, kneighbors, seed)
    "gates_chain_n333_d50_k7": ("gates_chain_n333_d50_k7", 333, 50, 7, 31),
    "n333_d261": (None, 333, 261, 8, 132),
}
A_QUERIES = (0, 63, 64, 127, 128, 255, 256)   # and Q - 1: the queries checked against reference A
EXTENDED_Q = (65, 129, 257)                   # receipt_many: null points of every query checked here

# case 3 -- row counts at D = 48, kneighbors 6, Q = 7: (N, seed, reaches)
ROWS_D, ROWS_KNN, ROWS_Q = 48, 6, 7
ROWS = [
    (127, 41, "one row short of a GEMM tile; N % 4 == 3: the last row workgroup holds three rows"),
    (128, 42, "exactly one GEMM tile"),
    (129, 43, "second GEMM tile of one row; N % 4 == 1"),
    (130, 44, "N % 4 == 2"),
    (257, 45, "third GEMM tile of one row"),
    (513, 46, "fifth GEMM tile of one row; nine column-sum partials"),
]

# case 4 -- degrees above 64 at N = 300, Q = 70
DEG_N, DEG_Q = 300, 70
# kernel-built graphs: (kneighbors, more than this many neighbours in some row, seed, shift).  The anchors are
# standard_normal plus `shift` in every column, so that most cosines are positive and the mutual lists stay long.
DEG_BUILT = [(70, 64, 51, 0.5), (140, 128, 52, 0.5)]
# injected graphs: (kind, D, seed)
DEG_INJECTED = [(kind, D, 60 + 2 * i + j) for i, kind in enumerate(["hub64", "hub65", "hub120", "hub128", "empty_rows"])
                for j, D in enumerate([32, 261])]
HUB = 17

# case 5 -- _mmr_many: (N, D, seed), Q in MMR_Q, k = 10
MMR_SHAPES = [(500, 261, 71), (500, 772, 72), (129, 5, 73)]
MMR_Q = [12, 65, 129, 257]
MMR_K = 10


# ---------------------------------------------------------------------------------------------------------------- inputs
def anchors(N, D, seed, shift=0.0):
    Y = np.random.default_rng(seed).standard_normal((N, D)) + shift
    return Y.astype(np.float32)


def own_query(D, seed):
    """the lattice's own psi (unit norm); never a row of a batch, so deltaH of a settled state stays far from zero"""
    p = np.random.default_rng(seed + 1000).standard_normal(D)
    return (p / np.linalg.norm(p)).astype(np.float32)


def gates(N, seed):
    """per-row gates in (0, 1]"""
    return (1.0 - np.random.default_rng(seed + 2000).uniform(0.0, 1.0, N)).astype(np.float32)


def chain(N):
    return [int(i) for i in range(3, N, max(1, N // 12))][:12]


def queries(Y, Q, seed):
    """The first Q rows of one seeded 300-row batch: a random query, one scaled by 3, an anchor row, psi = 0, then random
    queries, every seventh of them uniform in [-1, 1].  (Q = 1 and Q = 2 hold only the first rows.)"""
    rng = np.random.default_rng(seed + 3000)
    D = Y.shape[1]
    P = rng.standard_normal((QMAX, D))
    P[1] *= 3.0
    P[2] = Y[5]
    P[3] = 0.0
    P[4::7] = rng.uniform(-1.0, 1.0, P[4::7].shape)
    return P[:Q].astype(np.float32)


def injected_graph(kind, N, seed):
    """scipy CSR: symmetric, sorted, weights uniform in [0.05, 1] (test_source_blocked_apply_on_injected_degenerate_graphs).
    hub<n>: row HUB has exactly n neighbours, over a sparse random rest; empty_rows: most rows have no edge."""
    import scipy.sparse as sp

    rng = np.random.default_rng(seed + 4000)
    if kind.startswith("hub"):
        n = int(kind[3:])
        others = np.setdiff1d(np.arange(N), [HUB])
        rows = np.concatenate([np.full(n, HUB), rng.choice(others, 400)])
        cols = np.concatenate([rng.choice(others, n, replace=False), rng.choice(others, 400)])
    else:
        rows = rng.integers(0, 30, 150)
        cols = rng.integers(0, 60, 150)
    pairs = np.unique(rows[rows != cols].astype(np.int64) * N + cols[rows != cols])  # (a repeated pair would add up)
    A = sp.coo_matrix((rng.uniform(0.05, 1.0, pairs.size).astype(np.float32), (pairs // N, pairs % N)),
                      shape=(N, N)).tocsr()
    A = A.maximum(A.T).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return A


def mmr_scores(N, Q, seed):
    """(N, Q) float32 with the tie patterns of test_mmr_many_matches_mmr in every 64-column slot: a column of equal
    scores, a column of exact pairs whose largest value is a pair (rows 7 and 47), a column rounded to one decimal."""
    rng = np.random.default_rng(seed + 5000)
    S = rng.standard_normal((N, Q)).astype(np.float32)
    for c0 in range(0, Q, 64):
        if c0 + 3 < Q:
            S[:, c0 + 3] = 0.25
        if c0 + 4 < Q:
            S[:40, c0 + 4] = S[40:80, c0 + 4]
            S[7, c0 + 4] = S[47, c0 + 4] = np.float32(5.5)
        if c0 + 5 < Q:
            S[:, c0 + 5] = np.round(S[:, c0 + 5], 1)
    if Q > 256:
        S[:, 256] = -1.5  # the second chunk's only column: every score tied
    return S


def equal_columns(Q):
    return [c0 + 3 for c0 in range(0, Q, 64) if c0 + 3 < Q] + ([256] if Q > 256 else [])


# ------------------------------------------------------------------------------------------------------------ the operator
class Setup:
    """What the references need of a lattice (device or oracle): anchors, gates, lambdas, the capped graph as positive
    edges in row-major order and dense, sqrt_deg, and the dense float64 operator M."""

    def __init__(self, Y, B, lams, A, sqrt_deg, L_path):
        self.Y = np.asarray(Y, np.float32)
        self.N, self.D = self.Y.shape
        self.B = np.asarray(B, np.float64)
        self.lamG, self.lamC, self.lamQ, self.lamP = (float(v) for v in lams)
        self.A = np.asarray(A, np.float64)
        self.sd = np.asarray(sqrt_deg, np.float64)
        self.r, self.c = np.nonzero(self.A > 0)
        self.w = self.A[self.r, self.c]
        rowptr = np.zeros(self.N + 1, np.int64)
        np.add.at(rowptr, self.r + 1, 1)
        self.csr = (np.cumsum(rowptr), self.c, self.w)
        self.M = yq.dense_M(self.A, self.sd, self.B, self.lamG, self.lamC, self.lamQ, self.lamP,
                            L_path if self.lamP > 0 else None)

    def basis64(self):
        """reference A's basis: one dense float64 solve"""
        return yq.basis(self.M, self.Y, self.B, self.lamG, self.lamQ)


def setup_of_lattice(lat, Y):
    rowptr, col, a, _, sd = lat.graph_csr()
    A = np.zeros((lat.N, lat.N))
    A[np.repeat(np.arange(lat.N), np.diff(rowptr)), col] = a
    return Setup(Y, lat.B_diag, (lat.lamG, lat.lamC, lat.lamQ, lat.lamP), A, sd, lat.L_path if lat.lamP > 0 else None)


def setup_of_oracle(ref):
    return Setup(ref.Y, ref.B_diag, (ref.lamG, ref.lamC, ref.lamQ, ref.lamP), ref.A, ref.sqrt_deg, ref.L_path)


# ------------------------------------------------------------------------------------------------------- the two formulas
def ustar(X, x, psi, dt=np.float64):
    return np.asarray(X, dt) + np.outer(np.asarray(x, dt), np.asarray(psi, dt))


def _edge_sq(s, V, dt):
    """|Vn_i - Vn_j|^2 per positive edge, Vn = V / (sqrt_deg + 1e-12), in dt"""
    Vn = np.asarray(V, dt) / (s.sd.astype(dt)[:, None] + dt(1e-12))
    d = Vn[s.r] - Vn[s.c]
    return np.einsum("ij,ij->i", d, d)


def scores(s, Us, psi, alpha=ALPHA, dt=np.float64):
    """(score, align) of every row for the stationary state Us, in dt (lattice.py:530-568, receipts.py:28-38)."""
    Us = np.asarray(Us, dt)
    psi = np.asarray(psi, dt)
    align = (Us / (np.linalg.norm(Us, axis=1, keepdims=True) + dt(1e-12))) @ (psi / (np.linalg.norm(psi) + dt(1e-12)))
    e = dt(0.5 * s.lamC) * s.w.astype(dt) * (_edge_sq(s, s.Y, dt) - _edge_sq(s, Us, dt))
    coh = np.zeros(s.N, dt)
    np.add.at(coh, s.r, e)
    mu, sigma = coh.mean(), coh.std() + dt(1e-12)
    return dt(alpha) * (coh - mu) / sigma + dt(1.0 - alpha) * align, align


def bundle64(s, Us, psi, k=K, alpha=ALPHA):
    """(ids, score, align, margins): tests/_queries.py's bundle on the setup's graph"""
    return yq.bundle(s.Y, Us, psi, s.csr, s.sd, s.lamC, k=k, alpha=alpha)


def receipt(s, U, Us, psi, dt=np.float64, nulls=True):
    """deltaH, the three sums and (float64 only) the null points {row: col} with the margin of every row's decision,
    for the state U and the stationary state Us, in dt (receipts.py:21-83 as restated by the oracle)."""
    Us = np.asarray(Us, dt)
    psi = np.asarray(psi, dt)
    Y = s.Y.astype(dt)
    ud2 = _edge_sq(s, Us, dt)
    coh = dt(0.5 * s.lamC) * s.w.astype(dt) * (_edge_sq(s, Y, dt) - ud2)
    anc = dt(s.lamG) * np.sum((Us - Y) ** 2, axis=1)
    qp = Us - psi[None, :]
    qry = dt(s.lamQ) * s.B.astype(dt) * np.sum(qp * qp, axis=1)
    diff = np.asarray(U, dt) - Us
    out = {"deltaH": float(np.sum(diff * (s.M.astype(dt) @ diff))), "coh_drop_sum": float(np.sum(coh)),
           "anchor_pen_sum": float(np.sum(anc)), "query_term_sum": float(np.sum(qry))}
    if nulls and dt is np.float64:
        R = s.lamC * s.w * ud2
        out["margin"] = yr.null_margins(s.r, R, s.N)
        mu = np.bincount(s.r, weights=R, minlength=s.N) / s.N
        var = np.maximum(np.bincount(s.r, weights=R * R, minlength=s.N) / s.N - mu * mu, 0.0)
        sigma = np.sqrt(var) + 1e-12
        order = np.lexsort((s.c, -R, s.r))  # per row: largest R first, smallest column among ties
        rs = s.r[order]
        first = np.ones(rs.size, dtype=bool)
        first[1:] = rs[1:] != rs[:-1]
        e = order[first]
        keep = (R[e] > 0) & ((R[e] - mu[s.r[e]]) / sigma[s.r[e]] > yr.Z_TH)
        out["nulls"] = {int(i): int(j) for i, j in zip(s.r[e][keep], s.c[e][keep])}
    return out


def sums_distance(got, want):
    """largest |got - want| / max(|want|, 1e-3 (|anchor| + |query|)) over the three sums: the rule of
    test_fixtures_against_yardstick_and_loop as a ratio"""
    scale = max(abs(want["anchor_pen_sum"]) + abs(want["query_term_sum"]), 1e-12)
    return max(abs(got[k] - want[k]) / max(abs(want[k]), 1e-3 * scale) for k in SUMS)


def full_steps(margins, eps=NEAR_TIE):
    """how many leading MMR steps are compared: all of them unless a margin is below eps"""
    return next((t for t, m in enumerate(margins) if m < eps), len(margins))


def cap_holds(truncated, Q):
    """the near-tie cap: at most one query in four compared over fewer than all steps, at least one in full"""
    return 4 * truncated <= Q and truncated < Q


# ------------------------------------------------------------------------------------------------- one record per table entry
def cases():
    """Every entry of the tables above as one dict: id, N, D, knn, seed, gated, Q, shift, inject, fixture."""
    out = []

    def add(id, N, D, knn, seed, Q, gated=False, shift=0.0, inject=None, fixture=None, group=""):
        out.append(dict(id=id, N=N, D=D, knn=knn, seed=seed, Q=Q, gated=gated, shift=shift, inject=inject,
                        fixture=fixture, group=group))

    for D, variant, seed, _ in WIDTHS:
        add(f"width-d{D}-{variant}", WIDTH_N, D, WIDTH_KNN, seed, WIDTH_Q, gated=variant == "gates_chain", group="width")
    for name, (fixture, N, D, knn, seed) in QUERY_LATTICES.items():
        add(f"queries-{name}", N, D, knn, seed, QMAX, fixture=fixture, group="queries")
    for N, seed, _ in ROWS:
        add(f"rows-n{N}", N, ROWS_D, ROWS_KNN, seed, ROWS_Q, group="rows")
    for knn, _, seed, shift in DEG_BUILT:
        add(f"degree-built-k{knn}", DEG_N, 32, knn, seed, DEG_Q, shift=shift, group="degree")
    for kind, D, seed in DEG_INJECTED:
        add(f"degree-{kind}-d{D}", DEG_N, D, 6, seed, DEG_Q, inject=kind, group="degree")
    return out


def case(id):
    return next(c for c in cases() if c["id"] == id)


def case_inputs(c):
    """(Y, own psi, gates or None, chain or None, lamP, constructor kwargs, P) of a table entry"""
    if c["fixture"]:
        from tests._cases import ctor_kwargs, load_case, make_inputs, random_gates

        rc = load_case(c["fixture"])["recipe"]
        Y, psi0 = make_inputs(rc)
        g = random_gates(rc) if rc["gates"] == "random" else None
        kw = dict(kneighbors=rc["k"], deterministic_k=True, **ctor_kwargs(rc))
        return Y, psi0, g, rc["chain"] or None, rc.get("lamP", 0.2), kw, queries(Y, c["Q"], c["seed"])
    Y = anchors(c["N"], c["D"], c["seed"], c["shift"])
    g = gates(c["N"], c["seed"]) if c["gated"] else None
    ch = chain(c["N"]) if c["gated"] else None
    kw = dict(kneighbors=c["knn"], deterministic_k=True)
    return Y, own_query(c["D"], c["seed"]), g, ch, 0.2, kw, queries(Y, c["Q"], c["seed"])


def oracle_of(c):
    """(oracle lattice, Setup, P) of a table entry on the CPU: the oracle's own kNN graph, or the injected one"""
    from oracle import oscillink_oracle as orc

    Y, psi0, g, ch, lamP, kw, P = case_inputs(c)
    if c["inject"]:
        kw["graph"] = injected_graph(c["inject"], c["N"], c["seed"]).toarray().astype(np.float32)
    ref = orc.OracleLattice(Y, **kw)
    ref.set_query(psi0, gates=g)
    if ch:
        ref.add_chain(ch, lamP=lamP)
    return ref, setup_of_oracle(ref), P


def lattice_of(amd, c):
    """(device lattice, Y, P) of a table entry"""
    Y, psi0, g, ch, lamP, kw, P = case_inputs(c)
    if c["inject"]:
        A = injected_graph(c["inject"], c["N"], c["seed"])
        lat = amd.Oscillink(Y, _build_graph=False, **kw)
        lat.set_graph_csr(A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data.astype(np.float32))
    else:
        lat = amd.Oscillink(Y, **kw)
    lat.set_query(psi0, gates=g)
    if ch:
        lat.add_chain(ch, lamP=lamP)
    return lat, Y, P


def a_queries(Q):
    """the queries of a Q-row batch that are checked against reference A in the query-count cases"""
    return sorted({q for q in A_QUERIES if q < Q} | {Q - 1})

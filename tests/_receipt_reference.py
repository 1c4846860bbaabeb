"""Float64 yardstick of the receipt kernels (receipt_kernels.hip: k_receipt_rows / k_receipt_pairs / k_receipt_finish) for ONE
resident U*, on CSR input, and the cases tests/test_gpu_receipt_kernels.py and tests/test_gpu_mmr_kernels.py run.  NumPy only.

The caller hands in the U* the device holds (`lat.solve_Ustar()`), so the CG's error stays out: what is compared is the
receipt arithmetic alone.  Per row i with neighbours j (a_ij > 0, columns ascending), the header of receipt_kernels.hip:

  coh_i    = sum_j 0.5 lamC a_ij (dy_ij - du_ij),  dy = |Yn_i - Yn_j|^2, du = |Un_i - Un_j|^2, Xn = X / (sqrt_deg + 1e-12)
  mag_i    = sum_j 0.5 lamC a_ij (dy_ij + du_ij)   what the error of a coh_i formed in float32 scales with (coh_i is a
                                                   difference of positive terms)
  anchor_i = lamG |U*_i - Y_i|^2,  query_i = lamQ B_i |U*_i - psi|^2
  null     : R_ij = lamC a_ij du_ij over the DENSE row (N entries, zeros included): mu = sum R / N,
             sigma = sqrt(sum R^2 / N - mu^2) + 1e-12, candidate = first argmax in ascending column order,
             reported iff R > 0 and z = (R - mu) / sigma > z_th
  margin_i = min(relative gap of the two largest R, |z - z_th|)   (tests/_receipt_yardstick.py: null_margins)

The edges are walked in blocks of at most 2^22 / D, so nothing of size nnz x D is ever held.  tests/test_receipt_reference_host.py
ties the yardstick to oracle/oscillink_oracle.py and proves, from float64 alone, the conditions the GPU cases rest on.
"""
import functools
import math

import numpy as np

from tests import _dynamics_reference as G
from tests import _queries as yq
from tests._receipt_yardstick import null_margins

TOL = 1e-4          # tests/test_gpu_parity.py, tests/test_gpu_dynamics.py
Z_RTOL = 1e-3       # tests/test_gpu_parity.py: _check_solves, on z and R
MARGIN = 1e-3       # a row's null decision is compared unless its yardstick margin is below this
LEFT_OUT_CAP = 0.02  # ... and at most this share of the rows with an edge may be left out, per case
NEAR_TIE = 1e-4     # tests/test_gpu_bundle_many.py
LAMS = (1.0, 0.5, 4.0)  # lamG, lamC, lamQ: the lattice's defaults


class Receipt:
    """Per row: coh, anchor, query, mag; null_col (-1: the row has no edge), null_z, null_R; `r` / `R`: the flat edge rows
    and residuals in CSR order (for null_margins); `sums`: the three float64 totals."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def decide(self, z_th):
        """(is_null, margin) of every row at z_th (the float the device is handed: pass it through np.float32 first)."""
        z_th = float(z_th)
        is_null = (self.null_col >= 0) & (self.null_R > 0) & (self.null_z > z_th)
        return is_null, null_margins(self.r, self.R.astype(np.float64), self.N, z_th)

    def median_z(self):
        """The median z over the rows with an edge, as a float32 value (what osc_receipt_rows takes)."""
        return float(np.float32(np.median(self.null_z[self.null_col >= 0].astype(np.float64))))


def receipt_reference(Y, Ustar, psi, B, rowptr, col, a, sqrt_deg, lamG, lamC, lamQ, dtype=np.float64):
    """The receipt of one resident U* in `dtype` arithmetic (float64: the yardstick; float32: how far plain float32
    arithmetic is from it on the same inputs).  The inputs are the device's float32 arrays."""
    f = dtype
    rowptr = np.asarray(rowptr, dtype=np.int64)
    N = rowptr.size - 1
    Yf, Uf = np.asarray(Y, dtype=np.float32).astype(f), np.asarray(Ustar).astype(f)  # (U*: float32 from the device)
    D = Yf.shape[1]
    pf, Bf = np.asarray(psi, dtype=np.float32).astype(f), np.asarray(B, dtype=np.float32).astype(f)
    keep = np.asarray(a) > 0
    row = np.repeat(np.arange(N, dtype=np.int64), np.diff(rowptr))[keep]
    cj = np.asarray(col, dtype=np.int64)[keep]
    w = np.asarray(a, dtype=np.float32)[keep].astype(f)
    di = np.asarray(sqrt_deg, dtype=np.float32).astype(f) + f(1e-12)
    Yn, Un = Yf / di[:, None], Uf / di[:, None]
    dy, du = np.empty(row.size, dtype=f), np.empty(row.size, dtype=f)
    step = max(1, (1 << 22) // max(1, D))
    for s in range(0, row.size, step):
        r, c = row[s:s + step], cj[s:s + step]
        yd, ud = Yn[r] - Yn[c], Un[r] - Un[c]
        dy[s:s + step] = np.sum(yd * yd, axis=1)
        du[s:s + step] = np.sum(ud * ud, axis=1)
    half = (f(0.5) * f(lamC)) * w

    def per_row(x):
        return np.bincount(row, weights=x, minlength=N).astype(f) if f is np.float64 else _sum_rows_f32(row, x, N)

    coh, mag = per_row(half * (dy - du)), per_row(half * (dy + du))
    dA, dQ = Uf - Yf, Uf - pf[None, :]
    anchor = f(lamG) * np.sum(dA * dA, axis=1)
    query = f(lamQ) * Bf * np.sum(dQ * dQ, axis=1)
    R = f(lamC) * w * du
    s1, s2 = per_row(R), per_row(R * R)
    mu = s1 / f(N)
    sigma = np.sqrt(np.maximum(s2 / f(N) - mu * mu, f(0.0))) + f(1e-12)
    null_col = np.full(N, -1, dtype=np.int64)
    null_R, null_z = np.zeros(N, dtype=f), np.zeros(N, dtype=f)
    if row.size:
        order = np.lexsort((cj, -R, row))  # per row: largest R first, the smallest column among ties
        first = np.ones(row.size, dtype=bool)
        first[1:] = row[order][1:] != row[order][:-1]
        e = order[first]
        null_col[row[e]], null_R[row[e]] = cj[e], R[e]
        null_z[row[e]] = (R[e] - mu[row[e]]) / sigma[row[e]]
    sums = {"coh_drop_sum": float(np.sum(coh.astype(np.float64))), "anchor_pen_sum": float(np.sum(anchor.astype(np.float64))),
            "query_term_sum": float(np.sum(query.astype(np.float64)))}
    return Receipt(N=N, coh=coh, mag=mag, anchor=anchor, query=query, null_col=null_col, null_z=null_z, null_R=null_R, r=row,
                   c=cj, R=R, sums=sums)


def _sum_rows_f32(row, x, N):
    """Row sums accumulated in float32, in edge order (np.bincount would widen to float64)."""
    out = np.zeros(N, dtype=np.float32)
    np.add.at(out, row, x.astype(np.float32))
    return out


def compare(got, ref, z_th, null_rows, null_cols, null_z, null_R, frac=1.0):
    """The bounds of the GPU tier on (coh, anchor, query, sums) `got` and a null list (rows, columns, z, R: one entry per
    reported null point, as osc_receipt_rows returns them), against the yardstick `ref`, each scaled by `frac`.  Returns {kind: largest error as a fraction of its bound} plus `left_out` (share of rows with an edge) and
    `wrong_rows` (compared rows whose decision or column differs)."""
    coh, anchor, query, sums = got
    out = {}
    has = ref.null_col >= 0
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.abs(np.asarray(coh, np.float64) - ref.coh) / (TOL * ref.mag.astype(np.float64))
        out["coh"] = float(np.max(e[has])) if has.any() else 0.0
        out["coh_without_edges"] = float(np.max(np.abs(np.asarray(coh, np.float64)[~has]))) if (~has).any() else 0.0
        for key, x, want in (("anchor", anchor, ref.anchor), ("query", query, ref.query)):
            want = want.astype(np.float64)
            out[key] = float(np.max(np.abs(np.asarray(x, np.float64) - want) / (TOL * np.abs(want))))
    for key in ("coh_drop_sum", "anchor_pen_sum", "query_term_sum"):
        out[key] = abs(float(sums[key]) - ref.sums[key]) / (TOL * abs(ref.sums[key]))
    is_null, margin = ref.decide(z_th)
    compared = has & (margin >= MARGIN)
    out["left_out"] = float(np.count_nonzero(has & ~compared)) / max(1, int(np.count_nonzero(has)))
    dev_col = np.full(ref.N, -1, dtype=np.int64)
    dev_col[np.asarray(null_rows, dtype=np.int64)] = np.asarray(null_cols, dtype=np.int64)
    want_col = np.where(is_null, ref.null_col, -1)
    wrong = np.flatnonzero(compared & (dev_col != want_col))
    out["wrong_rows"] = [int(i) for i in wrong]
    out["nulls_among_compared"] = int(np.count_nonzero(compared & is_null))
    out["non_nulls_among_compared"] = int(np.count_nonzero(compared & ~is_null))
    out["nulls_without_edges"] = int(np.count_nonzero(dev_col[~has] >= 0))
    zr = {"z": 0.0, "R": 0.0}
    rows = np.asarray(null_rows, dtype=np.int64)
    ok = compared[rows] & (dev_col[rows] == want_col[rows]) if rows.size else np.zeros(0, dtype=bool)
    if ok.any():
        i = rows[ok]
        for key, x, want in (("z", null_z, ref.null_z), ("R", null_R, ref.null_R)):
            want = want.astype(np.float64)[i]
            zr[key] = float(np.max(np.abs(np.asarray(x, np.float64)[ok] - want) / (Z_RTOL * np.abs(want))))
    out.update(zr)
    for k in ("coh", "anchor", "query", "coh_drop_sum", "anchor_pen_sum", "query_term_sum", "z", "R"):
        out[k] = out[k] / frac
    return out


ERROR_KINDS = ("coh", "anchor", "query", "coh_drop_sum", "anchor_pen_sum", "query_term_sum", "z", "R")


def within_bounds(res):
    """The assertion of the tier on compare()'s result: message list, empty when every bound holds."""
    bad = [f"{k}: {res[k]:.3g} of its bound" for k in ERROR_KINDS if not res[k] <= 1.0]
    if res["wrong_rows"]:
        bad.append(f"null decision / column differs on compared rows {res['wrong_rows'][:10]}")
    if res["left_out"] > LEFT_OUT_CAP:
        bad.append(f"{res['left_out']:.3%} of the rows with an edge left out (cap {LEFT_OUT_CAP:.0%})")
    if res["coh_without_edges"] != 0.0 or res["nulls_without_edges"]:
        bad.append("a row without edges has a coh or a null point")
    return bad


# ------------------------------------------------------------------------------------------------------- launch geometry
def pitch(N, D, osc_ld=None):
    """The row pitch osc_create gives (osc_api.hip, "Row pitch"): D rounded up to 4; from N D >= 2^22 on rounded up to 32, plus
    32 when that is a multiple of 4 KB; OSC_LD overrides (a multiple of 4, >= the first figure)."""
    dcols = (D + 3) // 4 * 4
    ld = dcols
    if N * D >= 1 << 22:
        ld = (D + 31) // 32 * 32
        if (ld * 4) % 4096 == 0:
            ld += 32
    if osc_ld is not None and osc_ld >= dcols and osc_ld % 4 == 0:
        ld = osc_ld
    return ld


def template(nch):
    """launch_receipt_rows' choice for ceil(ld / 256) column chunks: the NCH of k_receipt_rows / k_receipt_pairs."""
    return nch if nch <= 4 else 6 if nch <= 6 else 0


def pair_form(N, ld):
    """receipt_rows() in osc_api.hip (OSC_RECEIPT_PAIR unset, N width < 2^31)."""
    return N >= 4096 and (ld + 255) // 256 <= 6


def finish_branches(rowptr, col):
    """What k_receipt_finish meets on this graph (API order = stored order): how many mirror slots are found in the first
    register (position < 64 of the lower row's list), in the second (64..127) and by the tail loop (>= 128); the largest
    number of lower neighbours within one 64-edge chunk of a row; the largest number of 64-edge chunks of a row whose
    neighbours are ALL lower than itself."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    N = rowptr.size - 1
    deg = np.diff(rowptr)
    row = np.repeat(np.arange(N, dtype=np.int64), deg)
    cj = np.asarray(col, dtype=np.int64)
    slot = np.arange(row.size) - rowptr[row]
    key = row * N + cj  # ascending: CSR order
    mirror = np.searchsorted(key, cj * N + row)
    assert np.array_equal(key[mirror], cj * N + row), "the graph is not symmetric"
    low = cj < row
    pos = slot[mirror][low]
    per_chunk = np.bincount((row * ((deg.max() + 63) // 64 + 1) + slot // 64)[low]) if low.any() else np.zeros(1, int)
    nlow = np.bincount(row[low], minlength=N)
    all_lower = (nlow == deg) & (deg > 0)
    return {"c0": int(np.count_nonzero(pos < 64)), "c1": int(np.count_nonzero((pos >= 64) & (pos < 128))),
            "tail": int(np.count_nonzero(pos >= 128)), "max_lower_in_chunk": int(per_chunk.max()),
            "all_lower_chunks": int(((deg[all_lower] + 63) // 64).max()) if all_lower.any() else 0,
            "max_deg": int(deg.max()), "deg_65_128": int(np.count_nonzero((deg >= 65) & (deg <= 128))),
            "deg_over_128": int(np.count_nonzero(deg > 128)),
            "high_rows_with_over_64_lower": int(np.count_nonzero((nlow > 64) & (np.arange(N) >= N // 2)))}


# ----------------------------------------------------------------------------------------------------------------- cases
class Case:
    def __init__(self, name, graph, Y, psi, B, osc_ld=None):
        self.name, self.osc_ld = name, osc_ld
        self.rowptr, self.col, self.a = graph
        self.Y, self.psi, self.B = Y, psi, B
        self.N, self.D = Y.shape
        self.ld = pitch(self.N, self.D, osc_ld)
        self.nch = (self.ld + 255) // 256
        self.pair = pair_form(self.N, self.ld)
        for arr in (self.rowptr, self.col, self.a, Y, psi, B):
            arr.setflags(write=False)

    @property
    def graph(self):
        return self.rowptr, self.col, self.a

    def sqrt_deg(self):
        return G.sqrt_deg_of(self.rowptr, self.a)

    def exact_ustar(self):
        """The float64 stationary state: dense solve up to 2000 rows, sparse LU beyond."""
        lamG, lamC, lamQ = LAMS
        sd = self.sqrt_deg().astype(np.float64)
        rhs = lamG * self.Y.astype(np.float64) + lamQ * self.B.astype(np.float64)[:, None] * self.psi.astype(np.float64)[None, :]
        import scipy.sparse as sp
        from scipy.sparse.linalg import splu

        row = np.repeat(np.arange(self.N), np.diff(self.rowptr))
        dm = 1.0 / sd
        W = sp.csr_matrix((self.a.astype(np.float64) * dm[row] * dm[self.col], self.col, self.rowptr), shape=(self.N, self.N))
        M = sp.diags(lamG + lamC + lamQ * self.B.astype(np.float64)) - lamC * W
        return splu(M.tocsc()).solve(rhs)

    def dense_A(self):
        A = np.zeros((self.N, self.N), dtype=np.float32)
        A[np.repeat(np.arange(self.N), np.diff(self.rowptr)), self.col] = self.a
        return A


def _inputs(rng, N, D):
    Y = rng.standard_normal((N, D)).astype(np.float32)
    psi = rng.standard_normal(D).astype(np.float32)
    return Y, psi, rng.uniform(0.1, 1.0, N).astype(np.float32)


def _weights(rng, n):
    return np.exp(0.8 * rng.standard_normal(n)).astype(np.float32)


def circulant_case(name, N, D, seed, isolated=0, osc_ld=None):
    """Degree 5 (strides 1, 2 and N / 2: odd, so the EU = 2 loop has a tail), random weights, anchors, query and gates;
    `isolated` rows of degree 0 behind it."""
    rng = np.random.default_rng(seed)
    ei, ej = G.circulant_edges(N, (1, 2, N // 2))
    g = G.csr_from_undirected(N, ei, ej, _weights(rng, ei.size))
    if isolated:
        g = G.with_isolated_rows(g, isolated)
    return Case(name, g, *_inputs(rng, N + isolated, D), osc_ld=osc_ld)


def relabel(g, new_of_old):
    """The same graph with row i called new_of_old[i]."""
    rowptr, col, a = g
    N = rowptr.size - 1
    row = np.repeat(np.arange(N, dtype=np.int64), np.diff(rowptr))
    up = row < col
    return G.csr_from_undirected(N, new_of_old[row[up]], new_of_old[col[up]], a[up])


def hub_case(name, N, D, seed, reverse=False):
    """_dynamics_reference.hub_graph: row 0 of degree 300, rows 310 / 320 / 330 of degree 65 / 100 / 130, the rest 2 - 6.
    `reverse`: row i becomes N - 1 - i, so the row of degree 300 is the last and all its neighbours are lower."""
    rng = np.random.default_rng(seed)
    g = G.hub_graph(N, rng)
    if reverse:
        g = relabel(g, N - 1 - np.arange(N, dtype=np.int64))
    return Case(name, g, *_inputs(rng, N, D))


def stars_case(stars, D, seed):
    """The exact-tie case: disjoint stars, a centre and six leaves in three twin pairs.  Within a pair the leaves share the
    anchor row, the edge weight and the gate; pair 0 lies far from the centre and carries its largest R.  The API ids are
    shuffled.  Returns (Case, centres, twins) with twins[s, p] = the two API ids of pair p of star s, the smaller first."""
    rng = np.random.default_rng(seed)
    N = 7 * stars
    ids = rng.permutation(N).astype(np.int64)
    centres, leaves = ids[:stars], ids[stars:].reshape(stars, 3, 2)
    leaves = np.sort(leaves, axis=2)
    Y = np.zeros((N, D), dtype=np.float32)
    B = np.zeros(N, dtype=np.float32)
    Y[centres] = rng.standard_normal((stars, D)).astype(np.float32)
    B[centres] = rng.uniform(0.1, 1.0, stars).astype(np.float32)
    ei, ej, w = [], [], []
    for p in range(3):
        rows = (Y[centres] + (6.0 if p == 0 else 0.3) * rng.standard_normal((stars, D))).astype(np.float32)
        gate, wt = rng.uniform(0.1, 1.0, stars).astype(np.float32), rng.uniform(0.5, 1.0, stars).astype(np.float32)
        for t in range(2):
            Y[leaves[:, p, t]], B[leaves[:, p, t]] = rows, gate
            ei.append(centres)
            ej.append(leaves[:, p, t])
            w.append(wt)
    g = G.csr_from_undirected(N, np.concatenate(ei), np.concatenate(ej), np.concatenate(w))
    psi = rng.standard_normal(D).astype(np.float32)
    return Case(f"stars_{stars}", g, Y, psi, B), centres, leaves


# name -> (builder, arguments); `nch` is what the case exists for and is asserted against pitch().  Seeds: the first that met
# every condition of tests/test_receipt_reference_host.py.
ROW_WIDTHS = {7: 1, 256: 1, 260: 2, 513: 3, 769: 4, 1024: 4, 1025: 5, 1536: 6, 1537: 7, 2100: 9}   # D -> chunks at N = 300
PAIR_WIDTHS = {7: 1, 257: 2, 513: 3, 769: 4, 1025: 5, 1536: 6}                                   # D -> chunks at N = 4096
CASES = {
    **{f"row_d{D}": (circulant_case, dict(N=300, D=D, seed=100 + D), nch) for D, nch in ROW_WIDTHS.items()},
    "row_d50_ld64": (circulant_case, dict(N=300, D=50, seed=11, osc_ld=64), 1),
    "row_d250_ld288": (circulant_case, dict(N=300, D=250, seed=12, osc_ld=288), 2),
    "row_isolated": (circulant_case, dict(N=300, D=64, seed=13, isolated=9), 1),
    "row_hub": (hub_case, dict(N=400, D=64, seed=14), 1),
    **{f"pair_d{D}": (circulant_case, dict(N=4096, D=D, seed=200 + D), nch) for D, nch in PAIR_WIDTHS.items()},
    "pair_hub": (hub_case, dict(N=4096, D=64, seed=15), 1),
    "pair_hub_reversed": (hub_case, dict(N=4096, D=64, seed=15, reverse=True), 1),
}
ROW_CASES = [n for n in CASES if n.startswith("row_")]
PAIR_CASES = [n for n in CASES if n.startswith("pair_")]
HUB_CASES = ["pair_hub", "pair_hub_reversed"]


@functools.lru_cache(maxsize=2)
def build_case(name):
    builder, kw, nch = CASES[name]
    case = builder(name, **kw)
    assert case.nch == nch, (name, case.ld, case.nch, nch)
    assert case.pair == name.startswith("pair_"), name
    return case


# ------------------------------------------------------------------------------------------------------------------- MMR
def cosine_to(rows, q):
    """rows_cosine_to (osc_api.hip) in float64: the query normalised with its own 1e-12 guard on the host, each row's dot
    product divided by (|row| + 1e-12) in the kernel."""
    rows, q = np.asarray(rows, np.float64), np.asarray(q, np.float64)
    qn = q / (np.sqrt(np.sum(q * q)) + 1e-12)
    return (rows @ qn) / (np.sqrt(np.sum(rows * rows, axis=1)) + 1e-12)


def mmr_inputs(N, D, seed, zero_rows=()):
    rng = np.random.default_rng(seed)
    Y = rng.standard_normal((N, D)).astype(np.float32)
    Y[list(zero_rows)] = 0.0
    return Y, rng.standard_normal(N).astype(np.float32)


# name -> (N, D, seed, k, lambda, zero rows).  Seeds chosen on the CPU (tests/test_receipt_reference_host.py: the near-tie cap).
MMR_CASES = {
    **{f"n{N}": (N, 6, 300 + t, 10, 0.5, ()) for t, N in enumerate((1, 3, 255, 257, 1024, 8192, 8193, 20000))},
    "n65537_strided": (65537, 4, 320, 10, 0.5, ()),
    **{f"d{D}": (500, D, 330 + t, 10, 0.5, ()) for t, D in enumerate((1, 3, 4, 50, 256, 260, 1030))},
    "lambda0": (20000, 6, 340, 10, 0.0, ()),
    "lambda1": (20000, 6, 340, 10, 1.0, ()),
    "exhaust_k_n": (257, 6, 350, 257, 0.5, ()),
    "exhaust_k_n_plus_5": (257, 6, 351, 262, 0.5, ()),
    "zero_rows": (500, 6, 352, 10, 0.5, (0, 17, 499)),
}
COSINE_WIDTHS = (1, 3, 4, 50, 256, 260, 1030)


@functools.lru_cache(maxsize=None)
def mmr_reference(name):
    """(ids, margins) of tests/_queries.mmr for a case of MMR_CASES: computed once and shared."""
    N, D, seed, k, lam, zero = MMR_CASES[name]
    Y, scores = mmr_inputs(N, D, seed, zero)
    ids, margins = yq.mmr(Y, scores, k, lam)
    return tuple(ids), tuple(margins)


def first_near_tie(margins, eps=NEAR_TIE):
    """Index of the first step whose margin is below eps (math.inf: none)."""
    return next((t for t, m in enumerate(margins) if m < eps), math.inf)


def duplicate_blocks(N, D, seed, blocks=6, size=5):
    """Exact ties: `blocks` groups of `size` identical anchor rows with identical scores (the groups' scores are the largest),
    scattered over the ids.  Returns (Y, scores, groups)."""
    rng = np.random.default_rng(seed)
    Y = rng.standard_normal((N, D)).astype(np.float32)
    scores = rng.standard_normal(N).astype(np.float32)
    ids = rng.permutation(N)[: blocks * size].reshape(blocks, size)
    for b, grp in enumerate(ids):
        Y[grp] = Y[grp[0]]
        scores[grp] = np.float32(4.0 + 0.25 * b)
    return Y, scores, np.sort(ids, axis=1)


def picks_smallest_remaining(ids, groups):
    """True iff every pick that belongs to a group is the smallest id of that group not picked before."""
    left = [list(map(int, g)) for g in groups]
    for i in ids:
        for g in left:
            if i in g:
                if i != g[0]:
                    return False
                g.pop(0)
    return True

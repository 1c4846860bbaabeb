"""A plain float64 restatement of the reference's single-step dynamics snapshot (`_compute_dynamics` / `_bfs_radius`,
lattice.py:825-927) on CSR input, vectorised over the edges -- the yardstick of tests/test_gpu_dynamics.py -- and the fixture
graphs and states those tests run it on.  tests/golden/reference_dynamics.json ties it to the reference itself
(tests/golden/make_golden_dynamics.py ran the reference on the small fixtures; tests/test_dynamics_reference_host.py
compares).  NumPy only.

What is restated, line for line:
  * move2_i = ||U_next_i - U_prev_i||^2, temperature = mean(move2)                                     (837-839)
  * step_deltaH = sum diff . (lamG I + lamC L_sym + lamQ B + lamP L_path) diff, diff = U_prev - U_next  (receipts.py:21-25);
    L_sym = I - D^-1/2 A D^-1/2 with a unit diagonal on EVERY row, isolated ones included (graph.py:86-93), and the
    reference multiplies DENSE matrices, so one non-finite entry of diff makes the whole scalar NaN (0 * inf)
  * per stored edge (i, j), a_ij > 0, in row-major order: e = 0.5 lamC a_ij ||U_i/(sqrt_deg_i + 1e-12) - U_j/(...)||^2,
    f = max(0.0, e_prev - e_next) with Python's max: a NaN difference gives 0.0                           (858-878)
  * top flows: stable sort by flow, descending, over that order: ties go to the smaller (i, j)            (880-882)
  * radius: 0 when max sqrt(move2 + 1e-12) <= 1e-9; else BFS from the rows with sqrt(move2 + 1e-12) >= 0.1 max, radius =
    largest distance among the reached rows (a NaN maximum passes the first test and seeds nothing: 0)  (885-892, 905-927)
"""
import json
import math
import os

import numpy as np

GOLDEN_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_dynamics.json")
TOP_K = 16


# ---------------------------------------------------------------------------------------------------------------- graphs
def csr_from_undirected(N, ei, ej, w):
    """Symmetric zero-diagonal CSR (rowptr int64, col int32 ascending per row, a float32) of the undirected edges."""
    ei, ej = np.asarray(ei, dtype=np.int64), np.asarray(ej, dtype=np.int64)
    w = np.asarray(w, dtype=np.float32)
    assert np.all(ei != ej), "zero diagonal"
    r, c, v = np.concatenate([ei, ej]), np.concatenate([ej, ei]), np.concatenate([w, w])
    order = np.lexsort((c, r))
    r, c, v = r[order], c[order], v[order]
    assert np.all(np.diff(r * N + c) > 0), "an edge is listed twice"
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=N))]).astype(np.int64)
    return rowptr, c.astype(np.int32), v


def circulant_edges(N, strides):
    """Undirected edges i -- (i + s) mod N of a circulant graph; a stride of N / 2 gives every row ONE edge (odd degree)."""
    ei, ej = [], []
    for s in strides:
        assert 0 < s and 2 * s <= N
        i = np.arange(N if 2 * s != N else N // 2, dtype=np.int64)
        ei.append(i)
        ej.append((i + s) % N)
    return np.concatenate(ei), np.concatenate(ej)


def circulant_degree(N, strides):
    return sum(1 if 2 * s == N else 2 for s in strides)


def circulant(N, strides, weights=None):
    """Circulant graph; default weight 1 / degree, so every row sum is exactly 1.0 when the degree is a power of two."""
    ei, ej = circulant_edges(N, strides)
    if weights is None:
        weights = np.full(ei.size, 1.0 / circulant_degree(N, strides), dtype=np.float32)
    return csr_from_undirected(N, ei, ej, weights)


def disjoint_union(g1, g2):
    """Two graphs side by side: the rows of g2 follow those of g1."""
    (rp1, c1, a1), (rp2, c2, a2) = g1, g2
    n1 = rp1.size - 1
    return (np.concatenate([rp1, rp2[1:] + rp1[-1]]).astype(np.int64), np.concatenate([c1, c2 + n1]).astype(np.int32),
            np.concatenate([a1, a2]).astype(np.float32))


def with_isolated_rows(g, extra):
    """`extra` rows of degree 0 behind the graph's own."""
    rp, c, a = g
    return np.concatenate([rp, np.full(extra, rp[-1])]).astype(np.int64), c, a


def hub_graph(N, rng):
    """One row of degree 300 (row 0), rows of degree 65 - 130 (310, 320, 330), everything else of degree 2 - 6 (half of them: 3);
    random weights.  N >= 400 (the dynamics fixtures: 400; rows from 400 on sit on the ring only)."""
    assert N >= 400
    edges = set()

    def add(i, j):
        if i != j:
            edges.add((min(i, j), max(i, j)))

    for i in range(N):  # a ring: degree 2 everywhere
        add(i, (i + 1) % N)
    for j in range(2, 300):  # the hub: 298 spokes + its two ring edges = 300
        add(0, j)
    for i in range(300, 350):  # chords for the rows the hub does not reach
        add(i, i + 50)
    for row, deg in ((310, 65), (320, 100), (330, 130)):
        have = sum(1 for e in edges if row in e)
        for j in rng.permutation(np.arange(1, 300))[: deg - have]:
            add(row, int(j))
    e = np.array(sorted(edges), dtype=np.int64)
    w = np.exp(0.8 * rng.standard_normal(e.shape[0])).astype(np.float32)
    return csr_from_undirected(N, e[:, 0], e[:, 1], w)


def sqrt_deg_of(rowptr, a):
    """graph.py:87-88 in float32: sqrt(max(row sum, 1e-12))."""
    N = rowptr.size - 1
    rows = np.repeat(np.arange(N), np.diff(rowptr))
    d = np.bincount(rows, weights=a.astype(np.float64), minlength=N).astype(np.float32)
    return np.sqrt(np.maximum(d, np.float32(1e-12))).astype(np.float32)


def bfs_dist(rowptr, col, a, seeds):
    """Level-synchronous BFS over the edges with a > 0: distance per row, -1 = not reached."""
    N = rowptr.size - 1
    dist = np.full(N, -1, dtype=np.int64)
    frontier = np.unique(np.asarray(seeds, dtype=np.int64))
    dist[frontier] = 0
    level = 0
    while frontier.size:
        lo, n = rowptr[frontier], rowptr[frontier + 1] - rowptr[frontier]
        at = np.repeat(lo - np.concatenate([[0], np.cumsum(n)[:-1]]), n) + np.arange(int(n.sum()))
        nb = col[at][a[at] > 0].astype(np.int64)
        nb = np.unique(nb[dist[nb] < 0])
        level += 1
        dist[nb] = level
        frontier = nb
    return dist


# ------------------------------------------------------------------------------------------------------------- reference
class Reference:
    """`dyn`: the snapshot with the product's keys.  Per stored CSR entry e (row-major = argwhere order): `row[e]`,
    `col[e]`, `flow[e]` and `scale[e]` = e_prev + e_next, what the error of a flow formed in float32 scales with.  `order`:
    the entries with a positive flow in the reference's ranking.  `move2`, `dist` (BFS distance, -1 = not reached)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def top(self, cap=TOP_K):
        return [{"edge": [int(self.row[e]), int(self.col[e])], "flow": float(self.flow[e])} for e in self.order[:cap]]


def _sum_neighbours(rowptr, contrib, N):
    """out[i] = sum of contrib over row i's entries (rows without entries: 0)."""
    out = np.zeros((N,) + contrib.shape[1:], dtype=contrib.dtype)
    has = np.diff(rowptr) > 0
    if contrib.shape[0]:
        out[has] = np.add.reduceat(contrib, rowptr[:-1][has], axis=0)
    return out


def dynamics_reference(rowptr, col, a, sqrt_deg, U_prev, U_next, lamG, lamC, lamQ, B, iters, chain=None, lamP=0.0,
                       dtype=np.float64):
    """The snapshot in `dtype` arithmetic (float64: the yardstick; float32: how far plain float32 arithmetic is from it)."""
    f = dtype
    rowptr = np.asarray(rowptr, dtype=np.int64)
    N = rowptr.size - 1
    Up, Un = np.asarray(U_prev, dtype=np.float32).astype(f), np.asarray(U_next, dtype=np.float32).astype(f)
    row = np.repeat(np.arange(N, dtype=np.int64), np.diff(rowptr))
    cj = np.asarray(col, dtype=np.int64)
    w = np.asarray(a, dtype=np.float32).astype(f)
    sd = np.asarray(sqrt_deg, dtype=np.float32).astype(f)
    Bv = np.ones(N, dtype=f) if B is None else np.asarray(B, dtype=np.float32).astype(f)
    with np.errstate(all="ignore"):
        dU = Un - Up
        move2 = np.sum(dU * dU, axis=1)
        temperature = float(np.mean(move2)) if N else 0.0
        # step energy
        diff = Up - Un
        if not np.all(np.isfinite(diff)):
            dH = float("nan")  # the reference's dense L_sym @ diff: 0 * inf in every row
        else:
            dm = f(1.0) / sd
            term = f(lamG) * diff + f(lamQ) * (Bv[:, None] * diff)
            term = term + f(lamC) * (diff - _sum_neighbours(rowptr, (w * dm[row] * dm[cj])[:, None] * diff[cj], N))
            if chain is not None and lamP > 0.0:
                pw = {}
                for k in range(len(chain) - 1):  # build_path_laplacian (graph.py:96-111), unit weights
                    i, j = int(chain[k]), int(chain[k + 1])
                    pw[(i, j)] = pw[(j, i)] = 1.0
                dp = np.zeros(N, dtype=f)
                for (i, j), x in pw.items():
                    dp[i] += f(x)
                dmp = f(1.0) / np.sqrt(np.maximum(dp, f(1e-12)))
                Lp = diff.copy()  # unit diagonal on every row, on the chain or not
                for (i, j), x in pw.items():
                    Lp[i] -= f(x) * dmp[i] * dmp[j] * diff[j]
                term = term + f(lamP) * Lp
            dH = float(np.sum(diff * term))
        # flows
        # (the reference adds 1e-12 to its float32 sqrt_deg IN float32, where it vanishes beside any degree above 1e-5)
        di = (np.asarray(sqrt_deg, dtype=np.float32) + np.float32(1e-12)).astype(f)
        P, Q = Up / di[:, None], Un / di[:, None]
        half = (f(0.5) * f(lamC)) * w
        e_prev, e_next = np.empty(row.size, dtype=f), np.empty(row.size, dtype=f)
        step = max(1, (1 << 22) // max(1, Up.shape[1]))
        for s in range(0, row.size, step):
            r, c = row[s:s + step], cj[s:s + step]
            yp, yn = P[r] - P[c], Q[r] - Q[c]
            e_prev[s:s + step] = half[s:s + step] * np.sum(yp * yp, axis=1)
            e_next[s:s + step] = half[s:s + step] * np.sum(yn * yn, axis=1)
        drop = e_prev - e_next
        flow = np.where((drop > 0) & (w > 0) & (row != cj), drop, f(0.0))  # max(0.0, nan) is 0.0
        pos = np.flatnonzero(flow > 0)
        order = pos[np.argsort(-flow[pos], kind="stable")]
        flow_total = float(np.sum(flow[pos]))
        # radius
        inf = np.sqrt(move2 + f(1e-12))
        mx = float(np.max(inf)) if N else 0.0
        dist = np.full(N, -1, dtype=np.int64)
        if N == 0 or mx <= 1e-9:
            radius = 0
        else:
            seeds = np.flatnonzero(inf >= 0.1 * mx)
            dist = bfs_dist(rowptr, cj, w, seeds)
            radius = int(dist.max()) if np.any(dist >= 0) else 0
        move2_max = float(np.max(move2)) if N else 0.0
    ref = Reference(row=row, col=cj, flow=flow.astype(np.float64), scale=(e_prev + e_next).astype(np.float64), order=order,
                    move2=move2, dist=dist)
    ref.dyn = {"temperature": temperature, "step_deltaH": dH, "viscosity_step": float(iters) / (abs(dH) + 1e-12),
               "flow_total": flow_total, "top_flows": ref.top(TOP_K), "radius": radius, "move2_mean": temperature,
               "move2_max": move2_max}
    return ref


# -------------------------------------------------------------------------------------------------------------- fixtures
class Fixture:
    """A graph, two states and the lattice parameters; `recipe` rebuilds it (build_fixture)."""

    def __init__(self, recipe, graph, U_prev, U_next, B=None, chain=None, lamP=0.0, lamG=1.0, lamC=0.5, lamQ=4.0, iters=3):
        self.recipe = recipe
        self.rowptr, self.col, self.a = graph
        self.N, self.D = U_prev.shape
        self.U_prev = np.ascontiguousarray(U_prev, dtype=np.float32)
        self.U_next = np.ascontiguousarray(U_next, dtype=np.float32)
        self.B, self.chain, self.lamP = B, chain, lamP
        self.lamG, self.lamC, self.lamQ, self.iters = lamG, lamC, lamQ, iters
        self.width = int(np.diff(self.rowptr).max())
        for arr in (self.rowptr, self.col, self.a, self.U_prev, self.U_next):
            arr.setflags(write=False)
        self._ref = {}

    def sqrt_deg(self):
        return sqrt_deg_of(self.rowptr, self.a)

    def reference(self, dtype=np.float64):
        """Computed once per fixture and shared; nobody writes to it."""
        if dtype not in self._ref:
            self._ref[dtype] = dynamics_reference(self.rowptr, self.col, self.a, self.sqrt_deg(), self.U_prev, self.U_next,
                                                  self.lamG, self.lamC, self.lamQ, self.B, self.iters, chain=self.chain,
                                                  lamP=self.lamP, dtype=dtype)
        return self._ref[dtype]


PATTERN = np.array([0.0, 3.0, 1.0, 0.5, 2.0])   # the tie storm: U_prev[i] = PATTERN[i % 5] * COLVEC
COLVEC = np.array([1.0, 2.0, 1.0, 0.5, 1.0, 2.0, 0.5, 1.0])


def _integers(N, D):
    """Small integers in [-5, 5], no two neighbouring rows of a circulant alike."""
    i, c = np.arange(N)[:, None], np.arange(D)[None, :]
    return (((i * 7 + c * 3 + (i // 11)) % 11) - 5).astype(np.float32)


def _poison(U, row, value):
    U = U.copy()
    if row is not None:
        U[row] = value
    return U


def storm(N, strides, D=4, window=None):
    """Exact tier.  Every flow value repeats about N / 5 times over the whole edge array: the top flows are decided by the
    caller's (row, column) ids alone.  `window` = [lo, hi): only those rows carry the pattern, so the winners -- the smallest
    ids among the tied -- are rows that a breadth-first order from row 0 stores late."""
    U_prev = (PATTERN[np.arange(N) % 5][:, None] * COLVEC[None, :D]).astype(np.float32)
    if window is not None:
        U_prev[:window[0]] = 0.0
        U_prev[window[1]:] = 0.0
    return Fixture({"builder": "storm", "N": N, "strides": list(strides), "D": D, "window": window}, circulant(N, strides),
                   U_prev, np.zeros_like(U_prev))


def sparse(N, strides, D=4, row=None):
    """Exact tier.  U_next = U_prev except `row`, which takes its right neighbour's values (row=None: no row differs)."""
    U_prev = _integers(N, D)
    U_next = U_prev if row is None else _poison(U_prev, row, U_prev[(row + 1) % N])
    return Fixture({"builder": "sparse", "N": N, "strides": list(strides), "D": D, "row": row}, circulant(N, strides),
                   U_prev, U_next)


def halved(N, strides, D=4, row=None, value=None):
    """Exact tier.  U_next = U_prev / 2 (every edge with a difference flows), then one row set to `value` ("nan", "inf")."""
    U_prev = _integers(N, D)
    U_next = _poison(U_prev * np.float32(0.5), row, {None: 0.0, "nan": np.nan, "inf": np.inf}[value])
    return Fixture({"builder": "halved", "N": N, "strides": list(strides), "D": D, "row": row, "value": value},
                   circulant(N, strides), U_prev, U_next)


def _graph_of(kind):
    if kind == "ring600":
        return circulant(600, (1, 2))
    if kind == "two_rings":  # rows 0..99 and 100..299
        return disjoint_union(circulant(100, (1,)), circulant(200, (1,)))
    if kind == "ring_plus_isolated":  # rows 296..299 have no edge
        return with_isolated_rows(circulant(296, (1, 2)), 4)
    raise KeyError(kind)


def moved_rows(kind, rows, D=4):
    """Exact tier, radius: U_next = U_prev except `rows`, every one moved by +4 in every column: they are the BFS seeds."""
    g = _graph_of(kind) if isinstance(kind, str) else circulant(kind[0], kind[1])
    N = g[0].size - 1
    U_prev = _integers(N, D)
    U_next = U_prev.copy()
    U_next[list(rows)] += 4.0
    return Fixture({"builder": "moved_rows", "kind": kind if isinstance(kind, str) else [kind[0], list(kind[1])],
                    "rows": list(rows), "D": D}, g, U_prev, U_next)


def _random_states(rng, N, D):
    U_prev = rng.standard_normal((N, D)).astype(np.float32)
    U_next = (0.7 * U_prev + 0.1 * rng.standard_normal((N, D))).astype(np.float32)
    return U_prev, U_next, rng.uniform(0.1, 1.0, N).astype(np.float32)


def widths(D, seed, chain=None, lamP=0.0):
    """Tolerance tier.  N = 300, degree 5 (strides 1, 2 and N / 2: odd), random weights, random states and gates."""
    rng = np.random.default_rng(seed)
    N = 300
    ei, ej = circulant_edges(N, (1, 2, 150))
    g = csr_from_undirected(N, ei, ej, np.exp(0.8 * rng.standard_normal(ei.size)).astype(np.float32))
    U_prev, U_next, B = _random_states(rng, N, D)
    return Fixture({"builder": "widths", "D": D, "seed": seed, "chain": chain, "lamP": lamP}, g, U_prev, U_next, B=B,
                   chain=chain, lamP=lamP)


def hub(D, seed):
    """Tolerance tier.  N = 400, ELL width 300 (hub_graph), random states and gates."""
    rng = np.random.default_rng(seed)
    g = hub_graph(400, rng)
    U_prev, U_next, B = _random_states(rng, 400, D)
    return Fixture({"builder": "hub", "D": D, "seed": seed}, g, U_prev, U_next, B=B)


_BUILDERS = {"storm": storm, "sparse": sparse, "halved": halved, "moved_rows": moved_rows, "widths": widths, "hub": hub}
_CACHE = {}


def build_fixture(recipe):
    """The fixture of a recipe (as recorded in reference_dynamics.json); built once and shared."""
    key = json.dumps(recipe, sort_keys=True)
    if key not in _CACHE:
        kw = {k: v for k, v in recipe.items() if k != "builder"}
        if recipe["builder"] == "moved_rows" and not isinstance(kw["kind"], str):
            kw["kind"] = (kw["kind"][0], tuple(kw["kind"][1]))
        _CACHE[key] = _BUILDERS[recipe["builder"]](**kw)
    return _CACHE[key]


# seeds of the tolerance tier: chosen on the CPU so that the top 17 distinct flow values are further apart than ten times the
# per-edge bound (tests/test_dynamics_reference_host.py asserts it)
WIDTH_SEEDS = {7: 12, 256: 192, 257: 4, 513: 32, 769: 82, 1025: 31, 1537: 23}
HUB_SEEDS = {64: 3, 257: 23}
CHAIN = [3, 50, 51, 200, 7]

# the small fixtures the reference itself was run on (name -> recipe)
def _recipe(builder, **kw):
    return {"builder": builder, **kw}


GOLDEN_RECIPES = {
    "storm_n257_deg8": _recipe("storm", N=257, strides=[1, 2, 3, 4], D=4, window=None),
    "storm_n300_deg2": _recipe("storm", N=300, strides=[1], D=4, window=None),
    "sparse_n300_deg4": _recipe("sparse", N=300, strides=[1, 50], D=4, row=123),
    "identical_n300_deg4": _recipe("sparse", N=300, strides=[1, 50], D=4, row=None),
    "radius_ring600": _recipe("moved_rows", kind="ring600", rows=[7], D=4),
    "radius_two_rings_seed_in_first": _recipe("moved_rows", kind="two_rings", rows=[10], D=4),
    "radius_two_rings_seeds_in_both": _recipe("moved_rows", kind="two_rings", rows=[10, 250], D=4),
    "radius_isolated_seed": _recipe("moved_rows", kind="ring_plus_isolated", rows=[298], D=4),
    "halved_n300": _recipe("halved", N=300, strides=[1, 2], D=4, row=None, value=None),
    "nan_row_n300": _recipe("halved", N=300, strides=[1, 2], D=4, row=77, value="nan"),
    "inf_row_n300": _recipe("halved", N=300, strides=[1, 2], D=4, row=77, value="inf"),
    "widths_d7_chain": _recipe("widths", D=7, seed=WIDTH_SEEDS[7], chain=CHAIN, lamP=0.3),
    **{f"widths_d{D}": _recipe("widths", D=D, seed=s, chain=None, lamP=0.0) for D, s in WIDTH_SEEDS.items()},
    **{f"hub_d{D}": _recipe("hub", D=D, seed=s) for D, s in HUB_SEEDS.items()},
}


# ------------------------------------------------------------------------------------------ the device's launch geometry
def launch_geometry(N, width):
    """nb1 / nb2 / nb3 and k_top_select's chunk as osc_dynamics (osc_api.hip) computes them."""
    ne = N * width
    nb1 = max(1, min((N + 255) // 256, 256))
    nb2 = max(1, min((ne + 255) // 256, 256))
    nb3 = max(1, min((ne + 4095) // 4096, 256))
    return {"ne": ne, "nb1": nb1, "nb2": nb2, "nb3": nb3, "chunk": (ne + nb3 - 1) // nb3}


def tie_blocks(fx):
    """The ELL positions (API row order: row * width + slot) of the entries tied at the largest flow, and the k_top_select
    blocks they fall into."""
    ref = fx.reference()
    slot = np.arange(ref.row.size) - fx.rowptr[ref.row]
    tied = np.flatnonzero(ref.flow == ref.flow.max())
    g = launch_geometry(fx.N, fx.width)
    return tied.size, np.unique((ref.row[tied] * fx.width + slot[tied]) // g["chunk"])


def distinct_top_gaps(ref, count=17):
    """Over the `count` largest DISTINCT flow values (the two directions of an edge counted once): the smallest of
    (value_k - value_k+1) / (largest scale of an entry holding either value)."""
    vals, first = np.unique(-ref.flow[ref.order], return_index=True)
    vals = -vals[:count]
    worst = math.inf
    for k in range(len(vals) - 1):
        scale = max(ref.scale[ref.order][ref.flow[ref.order] == v].max() for v in (vals[k], vals[k + 1]))
        worst = min(worst, (vals[k] - vals[k + 1]) / scale)
    return len(vals), worst

"""Plain Python / numpy references for the row-order code (csrc/bfs_order.hip, k_clustering_sample in csrc/perm_kernels.hip,
maybe_reorder in csrc/osc_graph.hip) and the hand-made graphs that tests/test_gpu_row_order.py injects.  Nothing here touches
a device; tests/test_order_reference_host.py checks these references against SciPy.

Every maker returns `(rowptr int64, col int32, a float32)`: a symmetric CSR with ascending columns in every row, no diagonal,
weights drawn from uniform(0.1, 1) and mirrored exactly -- what `osc_set_csr` accepts, and since it packs a row in ascending
column order, ELL slot order is ascending neighbour id."""
import numpy as np

NSAMPLE = 1024     # rows maybe_reorder samples for the clustering coefficient
AUTO_MIN_N = 8192  # below this the automatic mode never samples
MAX_DEPTH = 16383  # the largest level index the device form's key layout takes


# ---- the references -----------------------------------------------------------------------------------------------------
def bfs_order(rowptr, col):
    """(order int32 (N,), depth): components in order of their smallest row id, each walked by a FIFO queue from that row,
    neighbours in ascending id; depth = the largest level index over all components."""
    rp, c = np.asarray(rowptr).tolist(), np.asarray(col).tolist()
    N = len(rp) - 1
    level = [-1] * N
    order = []
    depth = 0
    for start in range(N):
        if level[start] >= 0:
            continue
        level[start] = 0
        head = len(order)
        order.append(start)
        while head < len(order):
            u = order[head]
            head += 1
            lv = level[u] + 1
            for v in c[rp[u]:rp[u + 1]]:
                if level[v] < 0:
                    level[v] = lv
                    order.append(v)
                    if lv > depth:
                        depth = lv
    return np.asarray(order, dtype=np.int32), depth


def sampled_rows(N, nsample=NSAMPLE):
    return [s * N // nsample for s in range(nsample)]


def clustering(rowptr, col, nsample=NSAMPLE):
    """(hits, pairs, hits / pairs) over the sampled rows s * N // nsample: pairs = d (d - 1) / 2 of a sampled row, hits = its
    neighbour pairs (a, b), a before b, with b in the adjacency of a.  The device divides the same two integers in double."""
    rp, c = np.asarray(rowptr).tolist(), np.asarray(col).tolist()
    N = len(rp) - 1
    hits = pairs = 0
    sets = {}
    for r in sampled_rows(N, nsample):
        nb = c[rp[r]:rp[r + 1]]
        d = len(nb)
        pairs += d * (d - 1) // 2
        for i, a in enumerate(nb):
            if a not in sets:
                sets[a] = set(c[rp[a]:rp[a + 1]])
            sa = sets[a]
            hits += sum(1 for b in nb[i + 1:] if b in sa)
    return hits, pairs, (hits / pairs if pairs else 0.0)


def bits_for(count):
    """Bits that hold the values 0 .. count - 1 (at least one)."""
    b = 1
    while (1 << b) < count:
        b += 1
    return b


def sort_passes(N, depth):
    """Passes of the final radix sort as bfs_order.hip states them: the key is root | level | position, 2 bits_for(N) +
    bits_for(levels + 1) bits sorted 8 per pass, where `levels` is what the level loop enqueued: it looks at the frontier size
    every 8 levels and stops at the first empty one it sees, so the depth + 1 levels round up to a multiple of 8, plus 1."""
    levels = 8 * ((depth + 1 + 7) // 8) + 1
    return max(1, (2 * bits_for(N) + bits_for(levels + 1) + 7) // 8)


def declines(depth):
    """The device form leaves graphs deeper than MAX_DEPTH to the host walk."""
    return depth > MAX_DEPTH


# ---- graph makers -------------------------------------------------------------------------------------------------------
def csr_from_edges(N, u, v, seed=0):
    """Symmetric CSR of the undirected edges (u[i], v[i]) (each pair once, u != v), one weight per edge on both sides."""
    u, v = np.asarray(u, dtype=np.int64).ravel(), np.asarray(v, dtype=np.int64).ravel()
    assert u.shape == v.shape and not np.any(u == v)
    lo, hi = np.minimum(u, v), np.maximum(u, v)
    assert np.unique(lo * N + hi).size == lo.size, "duplicate edge"
    w = np.random.default_rng(seed).uniform(0.1, 1.0, size=u.size).astype(np.float32)
    rows, cols, ws = np.concatenate([u, v]), np.concatenate([v, u]), np.concatenate([w, w])
    o = np.lexsort((cols, rows))
    rowptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=N), out=rowptr[1:])
    return rowptr, cols[o].astype(np.int32), ws[o]


def check_csr(rowptr, col, a):
    """The contract of the makers (used by the host tests)."""
    N = rowptr.shape[0] - 1
    assert rowptr.dtype == np.int64 and col.dtype == np.int32 and a.dtype == np.float32
    assert rowptr[0] == 0 and rowptr[-1] == col.shape[0] == a.shape[0] and np.all(np.diff(rowptr) >= 0)
    rows = np.repeat(np.arange(N), np.diff(rowptr))
    assert not np.any(rows == col) and (col.size == 0 or (col.min() >= 0 and col.max() < N))
    same_row = rows[1:] == rows[:-1]
    assert np.all(col[1:][same_row] > col[:-1][same_row])  # ascending, no duplicates
    assert a.size == 0 or (a.min() >= np.float32(0.1) and a.max() <= 1.0)
    fwd = dict(zip((rows * N + col).tolist(), a.tolist()))
    assert all(fwd.get(c * N + r) == x for r, c, x in zip(rows.tolist(), col.tolist(), a.tolist())), "not mirrored exactly"


def no_edges(N):
    return np.zeros(N + 1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32)


def one_edge():
    return csr_from_edges(2, [0], [1])


def ring(N, seed=0):
    i = np.arange(N)
    return csr_from_edges(N, i, (i + 1) % N, seed)


def shuffled_paths(N, seed=0, length=7):
    """N // length disjoint paths of `length` rows over a shuffled id set; the N % length rows left over have no edges."""
    ids = np.random.default_rng(seed).permutation(N)
    paths = ids[:(N // length) * length].reshape(-1, length)
    return csr_from_edges(N, paths[:, :-1], paths[:, 1:], seed + 1)


def star(N):
    """Hub = the last row: at level 1 one frontier row claims N - 1 children in slot order; ELL width N - 1."""
    return csr_from_edges(N, np.full(N - 1, N - 1), np.arange(N - 1), 3)


def shuffled_path(N, seed=0):
    """One path from row 0 whose ids are a random permutation along it: depth N - 1, and min-label propagation needs many
    rounds because neighbouring ids are unrelated."""
    ids = np.concatenate([[0], 1 + np.random.default_rng(seed).permutation(N - 1)])
    return csr_from_edges(N, ids[:-1], ids[1:], seed + 1)


def id_path(N):
    """The path 0 - 1 - ... - N - 1: depth N - 1."""
    return csr_from_edges(N, np.arange(N - 1), np.arange(1, N), 5)


def interleaved_combs(k=8, seed=0):
    """Two components: the even ids form one, the odd ids the other, each a root over layers of m rows in which row (l, i) is
    adjacent to rows (l + 1, i), (l + 1, i + 1) and (l + 1, i + 3) (mod m).  Every row below the first layer has three
    parents in the frontier above it, so the smallest (parent position, slot) decides who claims it.  The even component has
    m = 8 and 5 k layers, the odd one m = 5 and 8 k layers (1 + 40 k rows each); within a component ids are shuffled."""
    n = 1 + 40 * k
    rng = np.random.default_rng(seed)
    us, vs = [], []
    for comp, (m, layers) in enumerate(((8, 5 * k), (5, 8 * k))):
        local = np.concatenate([[0], 1 + rng.permutation(n - 1)])  # the root keeps the component's smallest id
        gid = 2 * local + comp
        node = lambda l, i: gid[1 + l * m + (i % m)]
        i = np.arange(m)
        us.append(np.full(m, gid[0]))
        vs.append(node(0, i))
        for l in range(layers - 1):
            for shift in (0, 1, 3):
                us.append(node(l, i))
                vs.append(node(l + 1, i + shift))
    return csr_from_edges(2 * n, np.concatenate(us), np.concatenate(vs), seed + 1)


def random_sparse(N, avg_degree, seed=0, ids=None):
    """Edges of a sparse random symmetric graph over `ids` (default: all N rows): (u, v), each pair once."""
    rng = np.random.default_rng(seed)
    ids = np.arange(N) if ids is None else np.asarray(ids)
    m = ids.size * avg_degree // 2
    p, q = rng.integers(0, ids.size, size=m), rng.integers(0, ids.size, size=m)
    keep = p != q
    lo, hi = np.minimum(p[keep], q[keep]), np.maximum(p[keep], q[keep])
    key = np.unique(lo * ids.size + hi)
    return ids[key // ids.size], ids[key % ids.size]


def sparse_remainder(N=9000, seed=11):
    """The sparse random graph alone: clustering far below the 0.05 at which the automatic mode reorders."""
    return csr_from_edges(N, *random_sparse(N, 16, seed), seed + 1)


def deg_class(d):
    return 0 if d <= 64 else 1 if d <= 128 else 2


CLASS_NAMES = ("<=64", "65..128", ">128")
CLASS_DEGREE = (6, 100, 140)  # the degree a gadget gives a row of each class
# (sampled-row class, neighbour class, class of the slot at which the hit sits in the neighbour's list): what a symmetric
# graph can show -- a hit at slot s needs a neighbour of degree > s
COMBINATIONS = [(s, a, p) for s in range(3) for a in range(3) for p in range(a + 1)]


def clustering_graph(N=9000, seed=7):
    """The union the clustering case injects, built on blocks of consecutive ids that each start at a sampled row:
      * cliques of 5, 66, 130 and 200 rows (every pair of a sampled member hits; hits at every slot class);
      * a hub of degree 150 whose neighbours are mutually non-adjacent rows of degree 2 (a sampled row with no hit);
      * one gadget per (s, a, p) of COMBINATIONS with s != a: a sampled row x of class s with neighbours a0 < b, a0 of class a,
        a0 -- b adjacent, and so many private rows of a0 below b that b sits at a slot of class p in a0's list; the other
        neighbours of x and a0 are private rows of degree 1.  p = 2 is the issue's "low-degree sampled row whose neighbours
        are adjacent to each other through high ids";
      * a sparse random remainder over the ids no block uses (the hub's neighbours take one edge each into it)."""
    samples = sorted(set(sampled_rows(N)))
    us, vs = [], []
    cursor = [0]

    def block(size):  # `size` consecutive unused ids, the first one a sampled row
        start = next(r for r in samples if r >= cursor[0])
        cursor[0] = start + size
        assert cursor[0] <= N
        return np.arange(start, start + size)

    def edges(u, v):
        u, v = np.broadcast_arrays(np.asarray(u), np.asarray(v))
        us.append(u.ravel())
        vs.append(v.ravel())

    for size in (5, 66, 130, 200):
        ids = block(size)
        i, j = np.triu_indices(size, 1)
        edges(ids[i], ids[j])
    hub_block = block(151)
    hub, hub_leaves = hub_block[0], hub_block[1:]
    edges(hub, hub_leaves)
    for s, a, p in COMBINATIONS:
        if s == a:
            continue  # (the cliques)
        dx, da = CLASS_DEGREE[s], CLASS_DEGREE[a]
        slot = (3, 70, 130)[p]                  # where b sits in a0's list: x and slot - 1 private rows come before it
        ids = block(3 + (da - 2) + (dx - 2))
        x, a0 = ids[0], ids[1]
        below = ids[2:2 + slot - 1]
        b = ids[2 + slot - 1]
        above = ids[2 + slot:2 + slot + (da - 2) - (slot - 1)]
        mine = ids[3 + (da - 2):]
        assert below.size + above.size == da - 2 and mine.size == dx - 2
        edges(x, [a0, b])
        edges(a0, b)
        edges(a0, np.concatenate([below, above]))
        edges(x, mine)
    rest = np.arange(cursor[0], N)
    ru, rv = random_sparse(N, 6, seed, ids=rest)
    edges(ru, rv)
    edges(hub_leaves, rest[np.random.default_rng(seed + 1).permutation(rest.size)[:hub_leaves.size]])
    return csr_from_edges(N, np.concatenate(us), np.concatenate(vs), seed + 2)


def clustering_coverage(rowptr, col, nsample=NSAMPLE):
    """What the sampled rows of a graph reach: ({(s, a, p): hits}, rows with pairs and no hit, rows whose every pair hits)."""
    rp, c = np.asarray(rowptr).tolist(), np.asarray(col).tolist()
    N = len(rp) - 1
    table = {}
    none = every = 0
    for r in sorted(set(sampled_rows(N, nsample))):
        nb = c[rp[r]:rp[r + 1]]
        d = len(nb)
        row_hits = 0
        for i, a in enumerate(nb):
            la = c[rp[a]:rp[a + 1]]
            at = {x: k for k, x in enumerate(la)}
            for b in nb[i + 1:]:
                if b in at:
                    key = (deg_class(d), deg_class(len(la)), deg_class(at[b] + 1))  # slots 0..63 / 64..127 / >= 128
                    table[key] = table.get(key, 0) + 1
                    row_hits += 1
        if d >= 2:
            none += row_hits == 0
            every += row_hits == d * (d - 1) // 2
    return table, none, every


# ---- the order cases of tests/test_gpu_row_order.py: name -> (maker, on_device) -----------------------------------------------
ORDER_CASES = {
    "one_edge": (one_edge, 1),
    "two_rows_no_edge": (lambda: no_edges(2), 1),
    "ring17": (lambda: ring(17), 1),
    "ring33": (lambda: ring(33), 1),
    **{f"paths{N}": ((lambda N=N: shuffled_paths(N, seed=N)), 1) for N in (255, 256, 257, 1023, 1024, 1025, 4096, 4097)},
    "star2049": (lambda: star(2049), 1),
    "combs": (interleaved_combs, 1),
    "shuffled_path3000": (lambda: shuffled_path(3000), 1),
    "id_path16384": (lambda: id_path(16384), 1),
    "id_path16385": (lambda: id_path(16385), 0),
    "paths20000": (lambda: shuffled_paths(20000, seed=20000), 1),
}
BIG_N = 1_050_000
STATE_MOVE_CASES = ("paths1025", "star2049", "combs")


def big_paths():
    return shuffled_paths(BIG_N, seed=BIG_N)

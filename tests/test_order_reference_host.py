"""tests/_order_reference.py against SciPy, and the coverage that tests/test_gpu_row_order.py relies on (no device).

The reference walk and the reference clustering count are the expected outputs of the GPU cases, so they are checked here
against something that shares no code with them: scipy.sparse.csgraph for components and breadth-first order (it visits a
row's CSR entries in index order, which is ascending id for these graphs) and a dense A @ A * A triangle count."""
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse import csgraph

from tests import _order_reference as ref

SMALL = {
    "one_edge": ref.one_edge,
    "no_edges": lambda: ref.no_edges(5),
    "ring": lambda: ref.ring(33),
    "shuffled_paths": lambda: ref.shuffled_paths(60, seed=1),
    "star": lambda: ref.star(40),
    "combs": lambda: ref.interleaved_combs(k=1),
    "shuffled_path": lambda: ref.shuffled_path(50),
    "id_path": lambda: ref.id_path(30),
    "sparse_remainder": lambda: ref.sparse_remainder(300),
    **{f"random{s}": (lambda s=s: ref.csr_from_edges(80, *ref.random_sparse(80, 1 + s, seed=s), seed=s)) for s in range(4)},
}


def _matrix(g):
    rowptr, col, a = g
    N = rowptr.shape[0] - 1
    return sp.csr_matrix((a, col, rowptr), shape=(N, N))


@pytest.fixture(scope="module")
def order_cases():
    """name -> (graph, (order, depth)) of every order case but the big one: walked once, shared."""
    out = {}
    for name, (make, _) in ref.ORDER_CASES.items():
        g = make()
        out[name] = (g, ref.bfs_order(g[0], g[1]))
    return out


@pytest.fixture(scope="module")
def cluster_graph():
    return ref.clustering_graph()


@pytest.mark.parametrize("name", sorted(SMALL))
def test_makers_give_valid_symmetric_csr(name):
    ref.check_csr(*SMALL[name]())


def test_the_gpu_graphs_are_valid_symmetric_csr(order_cases, cluster_graph):
    for name, (g, _) in order_cases.items():
        if g[1].size < 50000:
            ref.check_csr(*g)
    ref.check_csr(*cluster_graph)
    ref.check_csr(*ref.sparse_remainder())


@pytest.mark.parametrize("name", sorted(SMALL))
def test_bfs_order_against_scipy(name):
    g = SMALL[name]()
    A = _matrix(g)
    N = A.shape[0]
    order, depth = ref.bfs_order(g[0], g[1])
    assert sorted(order.tolist()) == list(range(N))
    ncomp, label = csgraph.connected_components(A, directed=False)
    want, deepest, seen = [], 0, set()
    for start in range(N):
        if label[start] in seen:
            continue  # (rows ascend, so the first row of a component is its smallest)
        seen.add(label[start])
        nodes, pred = csgraph.breadth_first_order(A, start, directed=True, return_predecessors=True)
        assert sorted(nodes.tolist()) == np.flatnonzero(label == label[start]).tolist()
        want.extend(nodes.tolist())
        level = {start: 0}
        for v in nodes[1:].tolist():
            level[v] = level[int(pred[v])] + 1
        deepest = max(deepest, max(level.values()))
    assert len(seen) == ncomp
    assert order.tolist() == want
    assert depth == deepest


def _dense_clustering(g, nsample):
    N = g[0].shape[0] - 1
    if N <= 400:
        A = (_matrix(g).toarray() > 0).astype(np.float64)  # (counts far below 2^53: exact)
        tri = np.rint((A @ A * A).sum(axis=1)).astype(np.int64) // 2  # per row: adjacent pairs among its neighbours
        deg = A.sum(axis=1).astype(np.int64)
    else:  # the same product kept sparse
        A = sp.csr_matrix((np.ones(g[1].size, dtype=np.int64), g[1], g[0]), shape=(N, N))
        tri = np.asarray((A @ A).multiply(A).sum(axis=1)).ravel() // 2
        deg = np.diff(g[0])
    rows = [s * A.shape[0] // nsample for s in range(nsample)]
    return int(tri[rows].sum()), int((deg[rows] * (deg[rows] - 1) // 2).sum())


@pytest.mark.parametrize("name", sorted(SMALL))
@pytest.mark.parametrize("nsample", [7, 1024])
def test_clustering_against_dense_triangle_count(name, nsample):
    g = SMALL[name]()
    hits, pairs, value = ref.clustering(g[0], g[1], nsample)
    assert (hits, pairs) == _dense_clustering(g, nsample)
    assert value == (hits / pairs if pairs else 0.0)


def test_clustering_of_the_gpu_graphs_against_dense_triangle_count(cluster_graph):
    for g, lo, hi in ((cluster_graph, 0.05, 1.0), (ref.sparse_remainder(), 0.0, 0.05)):
        hits, pairs, value = ref.clustering(g[0], g[1])
        assert (hits, pairs) == _dense_clustering(g, ref.NSAMPLE)
        assert hits > 0 and lo < value < hi, (hits, pairs)  # which side of the automatic mode's 0.05 it must fall on
        N = g[0].shape[0] - 1
        assert N >= ref.AUTO_MIN_N and N % ref.NSAMPLE != 0  # the kernel samples, and its stride is not constant


def test_pass_count_and_depth_limit_restatements():
    assert [ref.bits_for(c) for c in (1, 2, 3, 4, 5, 256, 257, 1 << 20, (1 << 20) + 1)] == [1, 1, 2, 2, 3, 8, 9, 20, 21]
    assert ref.sort_passes(2, 0) == ref.sort_passes(2, 1) == 1       # 2 + bits_for(10) = 6 bits
    assert ref.sort_passes(64, 7) == 2 and ref.sort_passes(65, 7) == 3  # 12 + 4 = 16 bits, 14 + 4
    assert ref.sort_passes(64, 8) == 3                                # levels 17: bits_for(18) = 5
    assert ref.sort_passes(16384, 16383) == 6                         # 28 + bits_for(16386) = 43 bits
    assert not ref.declines(16383) and ref.declines(16384)


def test_order_cases_cover_what_they_claim(order_cases):
    print()
    passes = {}
    for name, (g, (order, depth)) in order_cases.items():
        N = g[0].shape[0] - 1
        passes[name] = ref.sort_passes(N, depth)
        print(f"{name}: N {N}, width {int(np.diff(g[0]).max())}, depth {depth}, sort passes {passes[name]}, "
              f"declines {ref.declines(depth)}")
        assert ref.declines(depth) == (ref.ORDER_CASES[name][1] == 0), name
    big_depth = 6  # disjoint paths of 7 walked from their smallest row: at most 6 levels (the GPU case asserts the real one)
    passes["big"] = ref.sort_passes(ref.BIG_N, big_depth)
    assert set(passes.values()) == {1, 2, 3, 4, 5, 6}, passes
    assert passes["one_edge"] == 1 and passes["ring17"] == 2 and passes["paths1024"] == 3 and passes["paths1025"] == 4
    assert passes["paths20000"] == 5 and passes["id_path16384"] == 6 and passes["big"] == 6
    depth = {name: d for name, (_, (_, d)) in order_cases.items()}
    assert depth["id_path16384"] == ref.MAX_DEPTH and depth["id_path16385"] == ref.MAX_DEPTH + 1
    assert depth["shuffled_path3000"] == 2999 and depth["star2049"] == 2  # (row 0, the hub, every other row)
    # the seams of the 1024-entry scan and sort tiles
    assert -(-ref.BIG_N // 1024) == 1026  # the second chunk of k_scan_sums, with a carry
    assert 256 * -(-4096 // 1024) == 1024 and 256 * -(-4097 // 1024) > 1024  # the histogram scan crosses one scan tile
    # many components whose roots interleave: in the path cases consecutive roots are not consecutive ids
    for N in (255, 1025, 4097):
        g, (order, _) = order_cases[f"paths{N}"]
        assert csgraph.connected_components(_matrix(g), directed=False)[0] == N // 7 + N % 7


def test_the_combs_make_parents_compete(order_cases):
    """Even ids one component, odd ids the other; most rows have several neighbours one level up, so which parent claims a
    row is decided by (parent position, slot), and the claiming parent is not always the row's smallest-id parent."""
    g, (order, depth) = order_cases["combs"]
    rowptr, col, _ = g
    A = _matrix(g)
    ncomp, label = csgraph.connected_components(A, directed=False)
    assert ncomp == 2 and all(label[v] == label[v % 2] for v in range(A.shape[0]))
    pos = np.empty(order.size, dtype=np.int64)
    pos[order] = np.arange(order.size)
    dist = csgraph.shortest_path(A, unweighted=True, indices=[0, 1]).min(axis=0)
    contested = not_smallest_id = 0
    for v in range(A.shape[0]):
        parents = [int(u) for u in col[rowptr[v]:rowptr[v + 1]] if dist[u] == dist[v] - 1]
        if len(parents) > 1:
            contested += 1
            not_smallest_id += min(parents, key=lambda u: pos[u]) != min(parents)
    assert contested > A.shape[0] // 2 and not_smallest_id > contested // 4, (contested, not_smallest_id)


def test_clustering_graph_reaches_every_class(cluster_graph):
    table, none, every = ref.clustering_coverage(cluster_graph[0], cluster_graph[1])
    print("\nhits found among the sampled rows, by (sampled-row degree, degree of neighbour a, slot of the hit in a's list)")
    for s, a, p in ref.COMBINATIONS:
        print(f"  row {ref.CLASS_NAMES[s]:>8}  a {ref.CLASS_NAMES[a]:>8}  slot {('0..63', '64..127', '>=128')[p]:>8}: "
              f"{table.get((s, a, p), 0)}")
    print(f"  sampled rows with pairs and no hit: {none}; sampled rows whose every pair hits: {every}")
    assert len(ref.COMBINATIONS) == 18 and set(table) <= set(ref.COMBINATIONS)
    missing = [c for c in ref.COMBINATIONS if table.get(c, 0) == 0]
    assert not missing, missing
    assert none > 0 and every > 0
    # the structures the issue names
    rowptr, col, _ = cluster_graph
    deg = np.diff(rowptr)
    sampled = sorted(set(ref.sampled_rows(rowptr.shape[0] - 1)))
    assert {4, 65, 129, 199, 150} <= set(deg[sampled].tolist())  # a member of every clique and the hub are sampled

"""chain_receipt_many without a device: the float64 yardstick shows that the cases of
tests/test_gpu_chain_receipt_many.py do not rest on a knife edge -- for every fixture, chain and query used there every
edge's max(z) is at least 1 % away from both thresholds, both verdicts occur across the two thresholds, and every walk chain
lies in the graph and has a gain to get wrong -- and the dict form is assembled from hand-made arrays, the k = -1 weakest
link included."""
import numpy as np
import pytest

from tests import _chain_many as cm


@pytest.mark.parametrize("own", [False, True], ids=["plain", "own"])
@pytest.mark.parametrize("name", cm.FIXTURES)
def test_yardstick_margins(name, own):
    inp = cm.inputs(name)
    y = cm.Yardstick(inp, own)
    P = cm.queries(inp)
    verdicts = {z_th: set() for z_th in cm.Z_THS}
    worst = np.inf
    for cname, chain in cm.chains(inp).items():
        if cname == "walk":  # every edge in the graph
            assert all(y.A[chain[t], chain[t + 1]] > 0 for t in range(len(chain) - 1)), (name, chain)
        for q in range(P.shape[0]):
            r = y.chain(P[q], chain)
            for z_th in cm.Z_THS:
                margin = float(np.min(np.abs(r["zmax"] - z_th)))
                worst = min(worst, margin / z_th)
                assert margin >= 1e-2 * z_th, (name, cname, q, z_th, r["zmax"].tolist())
                verdicts[z_th].add(bool(np.all(r["zmax"] <= z_th)))
            if cname == "walk":
                # lamC = 0: the gain is 0.5 lamC a (...) = 0 exactly, whatever the state; there is no magnitude to ask for
                assert (r["gain_magnitude"] > 0) == (y.lamC > 0), (name, q, r["gain_magnitude"])
                assert np.all(r["r_struct"] > 0) == (y.lamC > 0)
    print(f"{name} {'own' if own else 'plain'}: smallest |max(z) - z_th| / z_th {worst:.4f}  verdicts {verdicts}")
    assert set().union(*verdicts.values()) == {True, False}, verdicts


def test_walk_and_weakest_rule():
    rowptr = np.array([0, 2, 4, 5, 5])
    col = np.array([1, 2, 0, 2, 0])
    assert cm.walk(rowptr, col, 0, 4) == [0, 1, 2]  # 2's only neighbour is visited: a dead end
    assert cm.mixed([0, 1, 2, 3, 4, 5]) == [0, 1, 2, 2, 1, 0, 5]
    assert cm.weakest([0.5, 0.5, 0.7, 0.2]) == (2, 0.7)
    assert cm.weakest([-2.0, -1.0]) == (-1, -1.0) and cm.weakest([float("nan"), 0.0]) == (1, 0.0)


def test_chain_block_and_errors():
    from oscillink_amd import _receipts as rc

    lists, off, nodes = rc.chain_block([3, 1, 1, 0], 3, 5)
    assert lists == [[3, 1, 1, 0]] * 3 and off.tolist() == [0, 4, 8, 12] and off.dtype == np.int64
    assert nodes.tolist() == [3, 1, 1, 0] * 3 and nodes.dtype == np.int32
    lists, off, nodes = rc.chain_block([[0, 1], np.array([4, 4, 2]), (1, 0)], 3, 5)
    assert lists == [[0, 1], [4, 4, 2], [1, 0]] and off.tolist() == [0, 2, 5, 7] and nodes.tolist() == [0, 1, 4, 4, 2, 1, 0]
    assert rc.chain_block(np.array([[0, 1, 2], [2, 1, 0]]), 2, 3)[0] == [[0, 1, 2], [2, 1, 0]]
    assert rc.chain_block(np.array([0, 1, 2]), 2, 3)[0] == [[0, 1, 2]] * 2
    lists, off, nodes = rc.chain_block([], 0, 5)
    assert lists == [] and off.tolist() == [0] and nodes.size == 0 and nodes.dtype == np.int32
    assert rc.chain_block([0, 1], 0, 5)[0] == []
    for bad, msg in (([[0, 1]], "hold 2 chains"), ([[0, 1], [0, 5]], "query 1: chain indices out of bounds"),
                     ([[0, -1], [0, 1]], "query 0: chain indices out of bounds"), ([0, 5], "chain: chain indices out of bounds"),
                     ([[0, 1], [3]], "query 1: chain must contain at least two indices"), ([2], "at least two indices"),
                     ([[0, 1] * 512 + [0], [0, 1]], "query 0: a chain has at most 1024 indices"),
                     ([[0, 1.5], [0, 1]], "query 0: a chain must be a sequence of integers"), (7, "chains must be")):
        with pytest.raises(ValueError, match=msg):
            rc.chain_block(bad, 2, 5)
    assert len(rc.chain_block([[0, 1] * 512, [0, 1]], 2, 5)[0][0]) == 1024


def test_dicts_are_assembled_from_the_arrays():
    from oscillink_amd import _receipts as rc

    f32 = np.float32
    arr = dict(chain_offsets=np.array([0, 3, 4, 4 + 2], np.int64),
               chain_z_struct=np.array([0.1, 2.7, -0.3, -1.5, 0.25, 7.0], f32),
               chain_z_path=np.array([1.1, 0.5, -0.7, -2.0, 0.5, 6.0], f32),
               chain_r_struct=np.array([0.01, 0.02, 0.0, 0.0, 0.3, 0.4], f32),
               chain_r_path=np.array([0.5, 0.6, 0.0, 0.0, 0.7, 0.8], f32),
               chain_gain=np.array([0.125, 0.0, -3.5]), chain_verdict=np.array([False, True, False]),
               chain_weakest_k=np.array([1, -1, 1], np.int32), chain_weakest_z=np.array([2.7, -1.0, 7.0], f32))
    chains = [[4, 9, 9, 2], [7, 3], [1, 0, 1]]
    got = rc.chain_receipt_dicts(chains, arr)
    assert [list(g) for g in got] == [["verdict", "weakest_link", "coherence_gain", "edges"]] * 3
    assert got[0]["weakest_link"] == {"k": 1, "edge": [9, 9], "zscore": float(f32(2.7))}
    assert got[1] == {"verdict": True, "weakest_link": {"k": -1, "edge": [-1, -1], "zscore": -1.0}, "coherence_gain": 0.0,
                      "edges": [{"k": 0, "edge": [7, 3], "z_struct": -1.5, "z_path": -2.0, "r_struct": 0.0, "r_path": 0.0}]}
    assert got[2]["weakest_link"] == {"k": 1, "edge": [0, 1], "zscore": 7.0} and got[2]["coherence_gain"] == -3.5
    assert [e["edge"] for e in got[0]["edges"]] == [[4, 9], [9, 9], [9, 2]] and [e["k"] for e in got[0]["edges"]] == [0, 1, 2]
    for q, g in enumerate(got):
        s = int(arr["chain_offsets"][q])
        assert type(g["verdict"]) is bool and type(g["coherence_gain"]) is float and type(g["weakest_link"]["k"]) is int
        for t, ed in enumerate(g["edges"]):
            assert list(ed) == ["k", "edge", "z_struct", "z_path", "r_struct", "r_path"]
            for key in ("z_struct", "z_path", "r_struct", "r_path"):
                assert type(ed[key]) is float and ed[key] == float(arr["chain_" + key][s + t])
    assert rc.chain_receipt_dicts([], dict(arr, chain_offsets=np.zeros(1, np.int64))) == []


def test_row_yardstick_equals_the_dense_one():
    """chain_yardstick_rows (the route lattices' bounds, no N x N array) against tests/_refine_chains.chain_yardstick"""
    inp = cm.inputs("gates_chain_n333_d50_k7")
    P = cm.queries(inp)
    for own in (False, True):
        y = cm.Yardstick(inp, own)
        for chain in cm.chains(inp).values():
            want = y.chain(P[1], chain)
            path = cm.own_chain(inp)[:2] if own else (chain, None)
            got = cm.chain_yardstick_rows(y.ustar(P[1]), inp["Y"], inp["csr"], y.sd, y.lamC, path, chain)
            assert set(got) == set(want)
            for key in want:
                assert np.allclose(got[key], want[key], rtol=1e-12, atol=0), (own, key)

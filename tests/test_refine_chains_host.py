"""Corpus.refine_many(chains=...) without a device: the chain arguments are checked before any
native call, with add_chain's messages; and the oracle shows that the cases of tests/test_gpu_refine_chains.py do not rest
on a knife edge -- every residual of the settle and U* histories of a chain lattice is at least 1 % away from its
tolerance (so identical iteration counts can be asked for), every chain edge's max(z) is at least 1 % away from
chain_z_th (so equal verdicts can be asked for) -- and that the tie structure the GPU test's weakest-link rule rests on is
real: on a row with a single path neighbour z_path is sqrt(K - 1) whatever the data."""
import numpy as np
import pytest

from tests import _gated as yg
from tests import _refine_chains as rc


def _fake_corpus(N=50, D=8):
    from oscillink_amd.corpus import Corpus

    c = Corpus.__new__(Corpus)
    c._h, c.N, c.D = object(), N, D

    def no_native(name, *args):
        raise AssertionError(f"native call {name} before validation")

    c._call = no_native
    return c


@pytest.mark.parametrize("bad,msg", [
    (dict(chains=[[0, 1], [0, 1]], lamP=-0.1), "lamP must be >= 0"),
    (dict(chains=[[0, 1], [0, 10]]), "query 1: chain indices out of bounds"),
    (dict(chains=[[0, -1], None]), "query 0: chain indices out of bounds"),
    (dict(chains=[None, [3]]), "query 1: chain must contain at least two indices"),
    (dict(chains=[[0, 1, 2], None], chain_weights=[[1.0], None]), r"query 0: weights length must equal len\(chain\)-1"),
    (dict(chains=[[0, 1, 2], None], chain_weights=[[1.0, float("nan")], None]), "query 0: chain weights must be finite"),
    (dict(chains=[[0, 1, 2], None], chain_weights=[[1.0, float("inf")], None]), "query 0: chain weights must be finite"),
    (dict(chains=[[0, 1]]), "chains must hold 2 entries"),
    (dict(chains=np.zeros((3, 4), np.int64)), "chains must hold 2 entries"),
    (dict(chains=np.zeros((2, 4), np.float32)), "integer"),
    (dict(chains=[[0, 1] * 513, None]), "query 0: a chain has at most 1024 indices"),
    (dict(chains=[[0, 1], [0, 1]], chain_weights=[[1.0]]), "chain_weights must be None or hold 2 entries"),
    (dict(chains=[[0, 1.5], None]), "query 0: chain must be None or a sequence of integers"),
    (dict(chains=[[0, 1], None], chain_z_th=float("nan")), "chain_z_th"),
    (dict(chain_weights=[[1.0], None]), "chain_weights given without chains"),
])
def test_chain_arguments_are_checked_before_any_native_call(bad, msg):
    c = _fake_corpus()
    P = np.ones((2, 8), np.float32)
    for more in ({}, {"receipts": "full", "as_arrays": True}, {"gates": "diffusion"}):
        with pytest.raises(ValueError, match=msg):
            c.refine_many(P, 10, **bad, **more)
    c._h = None  # (so that __del__ has nothing to destroy)


def test_chain_bound_is_K_not_top_k_and_valid_chains_reach_the_new_entry_point():
    c = _fake_corpus(N=5)
    P = np.ones((2, 8), np.float32)
    with pytest.raises(ValueError, match="query 0: chain indices out of bounds"):  # top_k 10 > N 5: K = 5
        c.refine_many(P, 10, chains=[[0, 5], None])
    for kw in ({}, {"receipts": "light"}, {"gates": "diffusion", "receipts": "full"}):
        with pytest.raises(AssertionError, match="osc_corpus_refine_chains"):
            c.refine_many(P, 10, chains=[[0, 4], None], **kw)
    with pytest.raises(AssertionError, match="osc_corpus_refine before"):  # chains=None goes where it went
        c.refine_many(P, 10)
    with pytest.raises(AssertionError, match="osc_corpus_refine_receipts before"):
        c.refine_many(P, 10, receipts="full")
    c._h = None


def test_chain_block_layout():
    from oscillink_amd.corpus import Corpus

    b = Corpus._chains([[0, 3, 3], None, np.array([2, 1]), (4, 4, 4, 0)], [None, None, [0.5], None], 0.3, 2.5, 4, 5)
    assert b["offsets"].tolist() == [0, 3, 3, 5, 9] and b["edge_offsets"].tolist() == [0, 2, 2, 3, 6]
    assert b["nodes"].tolist() == [0, 3, 3, 2, 1, 4, 4, 4, 0] and b["nodes"].dtype == np.int32
    assert b["weights"].tolist() == [1.0, 1.0, 0.5, 1.0, 1.0, 1.0] and b["weights"].dtype == np.float32
    assert b["lists"] == [[0, 3, 3], None, [2, 1], [4, 4, 4, 0]] and b["lamP"] == 0.3
    assert Corpus._chains([[0, 1], None], None, 0.0, 2.5, 2, 5)["weights"] is None
    same = Corpus._chains(np.array([[0, 1, 2], [2, 1, 0]]), None, 0.2, 2.5, 2, 5)
    assert same["lists"] == [[0, 1, 2], [2, 1, 0]]
    assert Corpus._chains(None, None, -1.0, 2.5, 2, 5) is None  # chains=None: nothing is read


@pytest.mark.parametrize("name,top_k,chain,weights,lamP", rc.CASES)
def test_oracle_margins_and_tie_structure(name, top_k, chain, weights, lamP):
    from oracle import oscillink_oracle as orc

    Y, P = rc.corpus(name)
    cos = yg.host_cos(Y, P)
    Ap = rc.path_adjacency(top_k, chain, weights)
    single = [t for t in range(len(chain) - 1) if np.count_nonzero(Ap[chain[t]]) == 1 and chain[t] != chain[t + 1]]
    assert single or name == "weights64", "every other case has a chain edge that leaves a row with one path neighbour"
    worst_s = worst_u = worst_z = np.inf
    for q in range(P.shape[0]):
        cand = np.lexsort((np.arange(Y.shape[0]), -cos[q]))[:top_k]
        o = orc.OracleLattice(Y[cand], kneighbors=rc.KNEIGHBORS)
        o.set_query(P[q])
        o.add_chain(chain, lamP=lamP, weights=weights)
        assert np.array_equal(np.asarray(o.A_path, np.float32), Ap)
        s = dict(o.settle())
        hs = list(o.history)
        Us = o.solve_Ustar()
        hu = list(o.history)
        assert s["res"] <= 1e-3 and o.last_ustar["converged"]
        ms = min(abs(x - 1e-3) / 1e-3 for x in hs)
        mu = min(abs(x - 1e-4) / 1e-4 for x in hu)
        y = rc.chain_yardstick(Us, Y[cand], np.asarray(o.A), o.sqrt_deg, o.lamC, Ap, chain)
        mz = float(np.min(np.abs(y["zmax"] - rc.Z_TH)))
        print(f"{name} q{q}: settle {s['iters']} margin {ms:.4f}  ustar {o.last_ustar['iters']} margin {mu:.4f}  "
              f"min |max(z) - z_th| {mz:.4f}  gain {y['gain']:.6g}  zmax {np.round(y['zmax'], 4).tolist()}")
        worst_s, worst_u, worst_z = min(worst_s, ms), min(worst_u, mu), min(worst_z, mz)
        for t in single:  # one nonzero among K entries: z = sqrt(K - 1), whatever its value
            assert abs(y["z_path"][t] - np.sqrt(top_k - 1)) <= 1e-9 * np.sqrt(top_k - 1), (name, q, t, y["z_path"][t])
    assert worst_s >= 0.01 and worst_u >= 0.01, (worst_s, worst_u)
    assert worst_z >= 0.01 * rc.Z_TH, worst_z

"""Corpus.refine_many(chains=...): a chain prior and a chain receipt on every candidate lattice of
a batch, against the per-query loop on the device (Oscillink(Y[cand]) -> add_chain -> set_query -> settle -> bundle ->
receipt -> chain_receipt), against the oracle, and the byte identities that tie a call with chains to the call without.

Tolerances are the project's (tests/test_gpu_refine_receipts.py): identical settle and U* iteration counts, 1e-4 relative on
deltaH, the sums, the residuals and r_struct / r_path, null points by the near-tie rule, state_sig and the non-fixed meta
keys equal.  tests/test_refine_chains_host.py proves on the CPU that no residual of these cases is closer than 1 % to its
tolerance and no edge's max(z) closer than 1 % to chain_z_th.

Chain receipt: z within 1e-4 (|R_ij| + |mu_i|) / sigma_i of the loop's value (the rounding of the subtraction R - mu, which
a relative bound on z cannot express near z = 0), the gain within 1e-4 of the sum of the magnitudes it adds up, the verdict
equal, the weakest link's z-score within 1e-4 relative.  The weakest link's k need not be equal: on a row with a single path
neighbour z_path is exactly sqrt(K - 1), so the maximum is often an exact tie between edges and rounding picks the first.
The edge the batch names must have, in the loop's edge list, a max(z) within 1e-4 relative of the loop's maximum; where the
loop's top-two gap exceeds 1e-3 relative, k and edge must be equal."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests import _gated as yg
from tests import _queries as yq
from tests import _receipt_yardstick as yr
from tests import _refine_chains as rc
from tests import _refine_shapes as rs
from tests import test_gpu_refine_receipts as rr

pytestmark = pytest.mark.gpu

ROOT = rr.ROOT
REL = rr.REL
CHAIN_KEYS = ("chain_offsets", "chain_z_struct", "chain_z_path", "chain_r_struct", "chain_r_path", "chain_gain",
              "chain_verdict", "chain_weakest_k", "chain_weakest_z")
EDGE_KEYS = CHAIN_KEYS[1:5]
KW = {"kneighbors": rc.KNEIGHBORS}


@pytest.fixture(scope="module")
def amd():
    import oscillink_amd

    return oscillink_amd


def loop(amd, Yc, psi, chain, weights, lamP, gates=None, detail="full", settle=True):
    """The reference's loop body with a chain on one handle: what it returned, the residual histories, the null margins, the
    chain receipt and the float64 restatement of the chain receipt on the loop's own U*."""
    lat = amd.Oscillink(Yc, **yg.lattice_kw(KW))
    lat.add_chain(chain, lamP=lamP, weights=weights)
    lat.set_receipt_detail(detail)
    lat.set_query(psi, gates=gates)
    out = {}
    if settle:
        out["settle"] = lat.settle(dt=1.0, max_iters=12, tol=1e-3)
        out["s_hist"] = lat.residual_history()
    out["bundle"] = lat.bundle(rc.K_BUNDLE, rc.ALPHA)
    out["u_hist"] = lat.residual_history()
    if settle:
        out["receipt"] = lat.receipt()
    out["chain"] = lat.chain_receipt(chain, z_th=rc.Z_TH)
    rowptr, col, a, _, sd = lat.graph_csr()
    Us = lat.solve_Ustar()
    r = np.repeat(np.arange(lat.N), np.diff(rowptr))
    keep = a > 0
    r, c, w = r[keep], col[keep], a[keep].astype(np.float64)
    Un = Us.astype(np.float64) / (sd.astype(np.float64)[:, None] + 1e-12)
    d = Un[r] - Un[c]
    out["margin"] = yr.null_margins(r, lat.lamC * w * np.einsum("ij,ij->i", d, d), lat.N)
    out["csr"], out["sd"], out["Us"] = (rowptr, col, a), sd, Us
    out["y64"] = rc.chain_yardstick(Us, Yc, yg.dense_adj((rowptr, col, a), lat.N), sd, lat.lamC,
                                    rc.path_adjacency(lat.N, chain, weights), chain)
    lat.close()
    return out


def check_chain(tag, q, arr, chain, lp, dct=None):
    """The chain receipt of query q (arrays, and the dict form if given) against the loop's."""
    want, y = lp["chain"], lp["y64"]
    s, e = int(arr["chain_offsets"][q]), int(arr["chain_offsets"][q + 1])
    assert e - s == len(chain) - 1 == len(want["edges"])
    worst = {"z": 0.0, "r": 0.0}
    for t, ed in enumerate(want["edges"]):
        for name in ("struct", "path"):
            gz, gr = float(arr["chain_z_" + name][s + t]), float(arr["chain_r_" + name][s + t])
            wz, wr = ed["z_" + name], ed["r_" + name]
            bound = 1e-4 * y["bound_" + name][t]
            worst["z"] = max(worst["z"], abs(gz - wz) / max(bound, 1e-300))
            worst["r"] = max(worst["r"], abs(gr - wr) / max(abs(wr), 1e-300))
            assert abs(gz - wz) <= bound, (tag, q, t, name, gz, wz, bound)
            assert abs(gr - wr) <= REL * abs(wr), (tag, q, t, name, gr, wr)
    gain = float(arr["chain_gain"][q])
    assert abs(gain - want["coherence_gain"]) <= 1e-4 * y["gain_magnitude"], (tag, q, gain, want["coherence_gain"])
    assert bool(arr["chain_verdict"][q]) == want["verdict"]
    wz = want["weakest_link"]["zscore"]
    assert abs(float(arr["chain_weakest_z"][q]) - wz) <= REL * abs(wz), (tag, q, float(arr["chain_weakest_z"][q]), wz)
    k = int(arr["chain_weakest_k"][q])
    zmax = np.array([max(ed["z_struct"], ed["z_path"]) for ed in want["edges"]])
    assert 0 <= k < len(zmax) and abs(zmax[k] - wz) <= REL * abs(wz), (tag, q, k, zmax.tolist())
    top = np.sort(zmax)[::-1]
    gap = (top[0] - top[1]) / abs(top[0]) if len(top) > 1 else np.inf
    if gap > 1e-3:
        assert k == want["weakest_link"]["k"], (tag, q, k, want["weakest_link"], gap)
    print(f"{tag} q{q}: chain gain {gain:.9g}/{want['coherence_gain']:.9g} weakest k {k}/{want['weakest_link']['k']} z "
          f"{float(arr['chain_weakest_z'][q]):.7g}/{wz:.7g} top-two gap {gap:.3g}  worst z deviation {worst['z']:.3g} of "
          f"its bound, worst r deviation {worst['r']:.3g} relative")
    if dct is not None:
        got = dct["chain_receipt"]
        assert set(got) == set(want) and set(got["weakest_link"]) == set(want["weakest_link"])
        assert got["verdict"] == bool(arr["chain_verdict"][q]) and got["coherence_gain"] == gain
        assert got["weakest_link"] == {"k": k, "edge": [chain[k], chain[k + 1]], "zscore": float(arr["chain_weakest_z"][q])}
        if gap > 1e-3:
            assert got["weakest_link"]["edge"] == want["weakest_link"]["edge"]
        assert [(ed["k"], ed["edge"]) for ed in got["edges"]] == [(ed["k"], ed["edge"]) for ed in want["edges"]]
        for t, ed in enumerate(got["edges"]):
            assert set(ed) == set(want["edges"][t])
            for name in ("z_struct", "z_path", "r_struct", "r_path"):
                assert ed[name] == float(arr["chain_" + name][s + t])


def run_case(amd, name, gate_kw, receipts):
    _, top_k, chain, weights, lamP = rc.CASE[name]
    Y, P = rc.corpus(name)
    Q = P.shape[0]
    kw = dict(KW, chains=[chain] * Q, lamP=lamP, chain_weights=None if weights is None else [weights] * Q,
              chain_z_th=rc.Z_TH, receipts=receipts, **gate_kw)
    with amd.Corpus(Y) as c:
        arr = c.refine_many(P, top_k, rc.K_BUNDLE, rc.ALPHA, as_arrays=True, **kw)
        dcts = c.refine_many(P, top_k, rc.K_BUNDLE, rc.ALPHA, **kw)
    return Y, P, chain, weights, lamP, arr, dcts


VARIANTS = [(c[0], "ungated", "full") for c in rc.CASES] + \
           [(c[0], g, r) for c in rc.CASES[:2] for g, r in (("gated", "full"), ("ungated", "light"))]


@pytest.mark.parametrize("name,gating,receipts", VARIANTS)
def test_chains_against_loop(amd, name, gating, receipts):
    gate_kw = rs.GATE_KW if gating == "gated" else {}
    Y, P, chain, weights, lamP, arr, dcts = run_case(amd, name, gate_kw, receipts)
    tag = f"{name}/{gating}/{receipts}"
    keys = set(rr.BUNDLE_KEYS) | set(CHAIN_KEYS) | set(rr.NEW_KEYS[:6] if receipts == "light" else rr.NEW_KEYS)
    assert set(arr) == keys | ({"gates", "gate_iters", "gate_res"} if gate_kw else set())
    assert arr["chain_offsets"].dtype == np.int64 and arr["chain_gain"].dtype == np.float64
    assert arr["chain_verdict"].dtype == np.bool_ and arr["chain_weakest_k"].dtype == np.int32
    assert all(arr[k].dtype == np.float32 for k in EDGE_KEYS + ("chain_weakest_z",))
    rows = near = 0
    for q in range(P.shape[0]):
        cand = arr["candidates"][q]
        gates = arr["gates"][q] if gate_kw else None
        lp = loop(amd, Y[cand], P[q], chain, weights, lamP, gates=gates, detail=receipts)
        if receipts == "full":
            n, t = rr.check_query(tag, q, arr, dcts[q], lp)
            rows += n
            near += t
        else:  # light: deltaH and the solves; no sums, no null points
            rec, lrec = dcts[q]["receipt"], lp["receipt"]
            assert rec["cg_iters"] == lrec["cg_iters"] == int(arr["settle_iters"][q])
            assert rec["meta"]["ustar_iters"] == lrec["meta"]["ustar_iters"]
            assert rr.close(rec["deltaH_total"], lrec["deltaH_total"]) and rr.close(rec["residual"], lrec["residual"], floor=1e-7)
            assert rec["meta"]["state_sig"] == lrec["meta"]["state_sig"] and rec["meta"]["receipt_detail"] == "light"
            assert rec["null_points"] == [] and set(rec["meta"]) == set(lrec["meta"]) | {"ustar_source"}
        assert dcts[q]["receipt"]["meta"]["state_sig"] == lp["receipt"]["meta"]["state_sig"]
        check_chain(tag, q, arr, chain, lp, dcts[q])
    assert near <= 0.05 * max(rows, 1), (tag, near, rows)


def test_chains_without_receipts(amd):
    name = "plain100"
    Y, P, chain, weights, lamP, arr, lists = run_case(amd, name, {}, None)
    _, _, _, _, _, full, _ = run_case(amd, name, {}, "full")
    assert set(arr) == set(rr.BUNDLE_KEYS) | set(CHAIN_KEYS)
    for key in arr:  # U*, the bundle and the chain receipt do not depend on the settle
        assert arr[key].tobytes() == full[key].tobytes(), key
    assert [[d["id"] for d in l] for l in lists] == arr["ids"].tolist()  # the list form stays Q bundles
    assert all(set(d) == {"id", "score", "align"} for l in lists for d in l)
    for q in range(P.shape[0]):
        cand = arr["candidates"][q]
        lp = loop(amd, Y[cand], P[q], chain, weights, lamP, settle=False)
        _, _, _, margins = yq.bundle(Y[cand], lp["Us"].astype(np.float64), P[q], lp["csr"], lp["sd"], 0.5, k=rc.K_BUNDLE,
                                     alpha=rc.ALPHA)
        want = [int(cand[b["id"]]) for b in lp["bundle"]]
        ok, _ = yq.same_until_near_tie(arr["ids"][q].tolist(), want, margins, 1e-3)
        assert ok, (q, arr["ids"][q].tolist(), want)
        for t in range(len(want)):
            if margins[t] < 1e-3:
                break
            assert abs(arr["score"][q][t] - lp["bundle"][t]["score"]) <= 1e-4
            assert abs(arr["align"][q][t] - lp["bundle"][t]["align"]) <= 1e-5
        check_chain("no-receipts", q, arr, chain, lp)


def per_query(r, q, keys):
    """Query q's share of every array key, as bytes (flat keys by their offsets)."""
    out = {}
    for key in keys:
        if key in ("null_offsets", "chain_offsets"):
            continue
        if key in ("null_i", "null_j", "null_z", "null_r"):
            s, e = int(r["null_offsets"][q]), int(r["null_offsets"][q + 1])
        elif key in EDGE_KEYS:
            s, e = int(r["chain_offsets"][q]), int(r["chain_offsets"][q + 1])
        else:
            s, e = q, q + 1
        out[key] = r[key][s:e].tobytes()
    return out


def test_chainless_queries_and_lamP_zero_give_the_chainless_bytes(amd):
    _, top_k, chain, weights, lamP = rc.CASE["weights64"]
    Y, P = rc.corpus("weights64")
    mixed = [chain, None, chain, None, chain]
    wmixed = [weights, None, None, None, weights]
    with amd.Corpus(Y) as c:
        info = c.info(top_k, rc.KNEIGHBORS, rc.K_BUNDLE)
        for gate_kw in ({}, rs.GATE_KW):
            for receipts in ("full", None):
                kw = dict(KW, as_arrays=True, receipts=receipts, **gate_kw)
                plain = c.refine_many(P, top_k, rc.K_BUNDLE, rc.ALPHA, **kw)
                got = c.refine_many(P, top_k, rc.K_BUNDLE, rc.ALPHA, chains=mixed, lamP=lamP, chain_weights=wmixed, **kw)
                assert set(got) == set(plain) | set(CHAIN_KEYS)
                assert got["chain_offsets"].tolist() == [0, 6, 6, 12, 12, 18]
                for q in (1, 3):  # a lattice without a chain, beside lattices with one
                    assert per_query(got, q, plain) == per_query(plain, q, plain), (gate_kw, receipts, q)
                    assert int(got["chain_weakest_k"][q]) == -1 and not bool(got["chain_verdict"][q])
                    assert float(got["chain_gain"][q]) == 0.0 and float(got["chain_weakest_z"][q]) == 0.0
                for q in (0, 2, 4):  # and the chain does act where there is one
                    assert per_query(got, q, ("ustar_res",)) != per_query(plain, q, ("ustar_res",)), q
                zero = c.refine_many(P, top_k, rc.K_BUNDLE, rc.ALPHA, chains=[chain] * 5, lamP=0.0,
                                     chain_weights=[weights] * 5, **kw)
                for key in plain:  # a chain at lamP = 0: only state_sig / chain_* differ
                    assert zero[key].dtype == plain[key].dtype and zero[key].tobytes() == plain[key].tobytes(), (receipts, key)
                none = c.refine_many(P, top_k, rc.K_BUNDLE, rc.ALPHA, chains=[None] * 5, lamP=lamP, **kw)
                for key in plain:
                    assert none[key].tobytes() == plain[key].tobytes(), key
                assert none["chain_offsets"].tolist() == [0] * 6 and none["chain_weakest_k"].tolist() == [-1] * 5
                again = c.refine_many(P, top_k, rc.K_BUNDLE, rc.ALPHA, **kw)
                for key in plain:  # the call without chains after calls with chains
                    assert again[key].tobytes() == plain[key].tobytes(), key
        dz = c.refine_many(P[:2], top_k, rc.K_BUNDLE, rc.ALPHA, chains=[chain, None], lamP=0.0, receipts="full", **KW)
        dp = c.refine_many(P[:2], top_k, rc.K_BUNDLE, rc.ALPHA, receipts="full", **KW)
        assert dz[0]["receipt"]["meta"]["state_sig"] != dp[0]["receipt"]["meta"]["state_sig"]
        assert dz[1]["receipt"] == dp[1]["receipt"] and dz[1]["chain_receipt"] is None and "chain_receipt" not in dp[1]
        assert c.info(top_k, rc.KNEIGHBORS, rc.K_BUNDLE) == info


CHUNK_CODE = """
import numpy as np, sys
sys.path.insert(0, %r)
from oscillink_amd import Corpus
from tests import _refine_chains as rc
_, top_k, chain, weights, lamP = rc.CASE["weights64"]
Y, P = rc.corpus("weights64")
c = Corpus(Y)
assert c.info(top_k)["chunk"] == 2
r = c.refine_many(P, top_k, rc.K_BUNDLE, rc.ALPHA, kneighbors=rc.KNEIGHBORS, as_arrays=True, receipts="full",
                  chains=[chain, None, chain, chain, None], lamP=lamP, chain_weights=[weights, None, None, weights, None])
np.savez(sys.argv[1], **r)
"""


def test_chain_lattice_is_independent_of_its_batch(amd):
    _, top_k, chain, weights, lamP = rc.CASE["weights64"]
    Y, P = rc.corpus("weights64")
    chains = [chain, None, chain, chain, None]
    ws = [weights, None, None, weights, None]
    kw = dict(KW, as_arrays=True, receipts="full", lamP=lamP)
    with amd.Corpus(Y) as c:
        full = c.refine_many(P, top_k, rc.K_BUNDLE, rc.ALPHA, chains=chains, chain_weights=ws, **kw)
        keys = tuple(full)
        for q in (0, 2, 3):
            alone = c.refine_many(P[q:q + 1], top_k, rc.K_BUNDLE, rc.ALPHA, chains=[chains[q]], chain_weights=[ws[q]], **kw)
            assert per_query(alone, 0, keys) == per_query(full, q, keys), q
        moved = c.refine_many(P[::-1].copy(), top_k, rc.K_BUNDLE, rc.ALPHA, chains=chains[::-1], chain_weights=ws[::-1], **kw)
        for q in range(5):
            assert per_query(moved, 4 - q, keys) == per_query(full, q, keys), q
        given = c.refine_many(P, top_k, rc.K_BUNDLE, rc.ALPHA, candidates=full["candidates"], chains=chains,
                              chain_weights=ws, **kw)
        for key in keys:
            assert given[key].tobytes() == full[key].tobytes(), key
        assert c.info(top_k)["chunk"] == 256
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "r.npz")
        r = subprocess.run([sys.executable, "-c", CHUNK_CODE % ROOT, out], env=dict(os.environ, OSC_CORPUS_CHUNK="2"),
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:]
        chunked = np.load(out)
        for key in keys:
            assert chunked[key].tobytes() == full[key].tobytes(), key


def test_chains_against_oracle(amd):
    from oracle import oscillink_oracle as orc

    name, top_k, chain, weights, lamP = rc.CASE["weights64"]
    Y, P = rc.corpus(name)
    with amd.Corpus(Y) as c:
        arr = c.refine_many(P, top_k, rc.K_BUNDLE, rc.ALPHA, as_arrays=True, receipts="full", chains=[chain] * 5, lamP=lamP,
                            chain_weights=[weights] * 5, **KW)
        for q in (0, 3):
            cand = arr["candidates"][q]
            rowptr, col, a, w, sd = c._candidate_graph(cand, top_k, rc.KNEIGHBORS, 1.0)
            ref = orc.OracleLattice(Y[cand], graph=yg.dense_adj((rowptr, col, a), top_k).astype(np.float32),
                                    **yg.lattice_kw(KW))
            ref.set_query(P[q])
            ref.add_chain(chain, lamP=lamP, weights=weights)
            s = dict(ref.settle(dt=1.0, max_iters=12, tol=1e-3))
            Us = ref.solve_Ustar()
            dH = float(ref.deltaH(Us))
            print(f"oracle q{q}: settle {int(arr['settle_iters'][q])}/{s['iters']} ustar {int(arr['ustar_iters'][q])}/"
                  f"{ref.last_ustar['iters']} dH {float(arr['deltaH'][q]):.9g}/{dH:.9g}")
            assert int(arr["settle_iters"][q]) == s["iters"] and int(arr["ustar_iters"][q]) == ref.last_ustar["iters"]
            assert rr.close(float(arr["settle_res"][q]), s["res"], floor=1e-7)
            assert rr.close(float(arr["ustar_res"][q]), ref.last_ustar["res"], floor=1e-7)
            assert rr.close(float(arr["deltaH"][q]), dH)


def test_chain_validation_and_array_form(amd):
    rng = np.random.default_rng(11)
    Y = rng.standard_normal((40, 16)).astype(np.float32)
    P = rng.standard_normal((3, 16)).astype(np.float32)
    with amd.Corpus(Y) as c:
        for bad, msg in ((dict(chains=[[0, 1]] * 3, lamP=-1.0), "lamP must be >= 0"),
                         (dict(chains=[[0, 1], [0, 30], None]), "query 1: chain indices out of bounds"),
                         (dict(chains=[[0, 1], None, [2]]), "query 2: chain must contain at least two indices"),
                         (dict(chains=[[0, 1, 2]] * 3, chain_weights=[[1.0]] * 3), r"query 0: weights length must equal len\(chain\)-1"),
                         (dict(chains=[[0, 1]] * 3, chain_weights=[[np.nan]] * 3), "query 0: chain weights must be finite"),
                         (dict(chains=[[0, 1] * 512 + [0], None, None]), "query 0: a chain has at most 1024 indices"),
                         (dict(chains=[[0, 1]] * 2), "chains must hold 3 entries")):
            with pytest.raises(ValueError, match=msg):
                c.refine_many(P, 30, receipts="full", **bad)
        with pytest.raises(ValueError, match="query 0: chain indices out of bounds"):  # top_k 100 > N 40: K = 40
            c.refine_many(P, 100, chains=[[0, 40], None, None])
        lists = [[0, 5, 29, 5], [3, 3, 4, 1], [7, 8, 9, 29]]
        a = c.refine_many(P, 30, as_arrays=True, receipts="full", chains=lists, lamP=0.4)
        b = c.refine_many(P, 30, as_arrays=True, receipts="full", chains=np.array(lists), lamP=0.4)
        assert set(a) == set(b)
        for key in a:
            assert a[key].tobytes() == b[key].tobytes(), key
        # the longest chain and every row of the lattice on it: 1024 nodes over K = 30 rows
        long = [int(v) for v in rng.integers(0, 30, 1024)]
        r = c.refine_many(P, 30, as_arrays=True, receipts="light", chains=[long, None, [0, 1]], lamP=0.2)
        assert r["chain_offsets"].tolist() == [0, 1023, 1023, 1024] and np.all(np.isfinite(r["chain_z_path"]))
        lat = amd.Oscillink(Y[r["candidates"][0]])
        lat.add_chain(long, lamP=0.2)
        lat.set_query(P[0])
        s = lat.settle()
        dH = lat.receipt()["deltaH_total"]
        cr = lat.chain_receipt(long)
        lat.close()
        print(f"1024-node chain: settle {int(r['settle_iters'][0])}/{s['iters']} dH {float(r['deltaH'][0]):.9g}/{dH:.9g} "
              f"weakest z {float(r['chain_weakest_z'][0]):.7g}/{cr['weakest_link']['zscore']:.7g}")
        if int(r["settle_iters"][0]) == s["iters"]:  # (no margin is proven for this lattice: the numbers where the solves agree)
            assert rr.close(float(r["deltaH"][0]), dH)
        assert rr.close(float(r["chain_weakest_z"][0]), cr["weakest_link"]["zscore"])
        # Q = 0
        empty = c.refine_many(np.zeros((0, 16), np.float32), 10, as_arrays=True, chains=[])
        assert empty["chain_offsets"].tolist() == [0] and empty["chain_gain"].shape == (0,)

"""Corpus.refine_many(receipts=...): settle and receipt of every candidate lattice of a batch,
against the per-query loop on the device (Oscillink(Y[cand]) -> set_query -> settle -> bundle -> receipt), against the
oracle, light against full detail, independence of batch position and chunking, the null cap and the edge cases.

Tolerances are the project's parity gate (1e-4 relative, identical CG iteration counts) and test_gpu_receipt_many.py's
near-tie rule (a null-point decision may differ only on a row whose float64 margin is below 1e-3).  On the corpora of
`check_against_loop` the closest deciding residual of any settle or U* solve is 3.1 % away from its tolerance
(tests/test_refine_receipts_host.py proves that on the CPU), so no iteration-count exception is accepted there."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests import _gated as yg
from tests import _receipt_yardstick as yr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEAR = 1e-3
REL = 1e-4
SUMS = ("coh_drop_sum", "anchor_pen_sum", "query_term_sum")
FIXED = {"t_ms": 0.0}
META_FIXED = {"ustar_solve_ms": 0.0, "graph_build_ms": 0.0, "last_settle_ms": 0.0, "ustar_cached": False, "ustar_solves": 1,
              "ustar_cache_hits": 0, "ustar_source": "corpus_batch"}
BUNDLE_KEYS = ("ids", "local", "score", "align", "candidates", "ustar_iters", "ustar_res")
NEW_KEYS = ("settle_iters", "settle_res", "deltaH", "coh_drop_sum", "anchor_pen_sum", "query_term_sum", "null_total",
            "null_offsets", "null_i", "null_j", "null_z", "null_r")
UNGATED = [
    (100, 8, 0.5, {}),
    (64, 1, 0.0, {"kneighbors": 16}),
    (64, 64, 1.0, {"lamC": 0.0, "lamQ": 0.0}),
    (30, 40, 0.5, {"lamG": 2.0, "lamC": 1.5, "lamQ": 0.5, "row_cap_val": 0.3}),
    (7, 8, 0.5, {"kneighbors": 2000}),
]


@pytest.fixture(scope="module")
def amd():
    import oscillink_amd

    return oscillink_amd


def clustered(top_k, k):
    """test_refine_many_against_loop's corpus: 2000 x 96, six clusters, seed = top_k + k, five queries."""
    rng = np.random.default_rng(top_k + k)
    centers = rng.standard_normal((6, 96)).astype(np.float32) * 2
    Y = (centers[rng.integers(0, 6, 2000)] + 0.5 * rng.standard_normal((2000, 96))).astype(np.float32)
    P = rng.standard_normal((5, 96)).astype(np.float32)
    return Y, P


def loop(amd, Yc, psi, k, alpha, kw, gates=None, detail="full", settle=(1.0, 12, 1e-3)):
    """The reference's loop body on one handle; returns what it returned plus the residual histories and the margins."""
    lat = amd.Oscillink(Yc, **yg.lattice_kw(kw))
    lat.set_receipt_detail(detail)
    lat.set_query(psi, gates=gates)
    s = lat.settle(dt=settle[0], max_iters=settle[1], tol=settle[2])
    s_hist = lat.residual_history()
    b = lat.bundle(k, alpha)
    u_hist = lat.residual_history()
    rec = lat.receipt()
    rowptr, col, a, _, sd = lat.graph_csr()
    r = np.repeat(np.arange(lat.N), np.diff(rowptr))
    keep = a > 0
    r, c, w = r[keep], col[keep], a[keep].astype(np.float64)
    Un = lat.solve_Ustar().astype(np.float64) / (sd.astype(np.float64)[:, None] + 1e-12)
    d = Un[r] - Un[c]
    margin = yr.null_margins(r, lat.lamC * w * np.einsum("ij,ij->i", d, d), lat.N)
    lat.close()
    return {"settle": s, "bundle": b, "receipt": rec, "s_hist": s_hist, "u_hist": u_hist, "margin": margin}


def null_list(arr, q):
    s, e = int(arr["null_offsets"][q]), int(arr["null_offsets"][q + 1])
    return [{"edge": [int(i), int(j)], "z": float(z), "residual": float(r)} for i, j, z, r in
            zip(arr["null_i"][s:e], arr["null_j"][s:e], arr["null_z"][s:e], arr["null_r"][s:e])]


def close(got, want, rel=REL, floor=0.0):
    return abs(got - want) <= rel * abs(want) + floor


def check_query(tag, q, arr, dct, lp, settle_tol=1e-3, exact_zero=False, allow_iter_exception=False, sum_floor=False,
                res_floor=1e-7):
    """One query of a batch (arrays `arr`, dict `dct`) against the loop's result `lp`.  Returns (rows, near-tie rows).
    sum_floor (the degenerate lattices of the edge test only): a sum that cancels to far below the lattice's energy scale is
    held to test_gpu_receipt_many.py's bound, 1e-4 of max(|want|, 1e-3 (|anchor_pen_sum| + |query_term_sum|)).
    res_floor: the absolute part of the residual bound, 1e-7 unless the caller gives the lattice's own (rounding_floor)."""
    rec, lrec = dct["receipt"], lp["receipt"]
    print(f"{tag} q{q}: settle {int(arr['settle_iters'][q])}/{lp['settle']['iters']} res {float(arr['settle_res'][q]):.6e}/"
          f"{lp['settle']['res']:.6e}  ustar {int(arr['ustar_iters'][q])}/{lrec['meta']['ustar_iters']}  dH "
          f"{float(arr['deltaH'][q]):.9g}/{lrec['deltaH_total']:.9g}  sums "
          + " ".join(f"{float(arr[k][q]):.9g}/{lrec[k]:.9g}" for k in SUMS)
          + f"  nulls {int(arr['null_total'][q])}/{lrec['meta']['null_points_summary']['total_null_points']}")
    # dict form and array form say the same thing
    assert rec["deltaH_total"] == float(arr["deltaH"][q]) and rec["cg_iters"] == int(arr["settle_iters"][q])
    assert dct["settle"] == {"iters": int(arr["settle_iters"][q]), "res": float(arr["settle_res"][q])}
    assert rec["null_points"] == null_list(arr, q)
    assert [b["id"] for b in dct["bundle"]] == arr["ids"][q].tolist()
    assert set(rec) == set(lrec) and set(rec["meta"]) == set(lrec["meta"]) | {"ustar_source"}
    for key, val in FIXED.items():
        assert rec[key] == val
    for key, val in META_FIXED.items():
        assert rec["meta"][key] == val and type(rec["meta"][key]) is type(val), key
    skip_energy = False
    for name, gi, wi, hist, tol in (("settle", rec["cg_iters"], lrec["cg_iters"], lp["s_hist"], settle_tol),
                                    ("ustar", rec["meta"]["ustar_iters"], lrec["meta"]["ustar_iters"], lp["u_hist"], 1e-4)):
        if gi != wi:
            deciding = hist[min(gi, wi) - 1]
            print(f"{tag} q{q}: {name}_iters exception {gi} vs loop {wi}, loop residual {deciding:.6e}")
            assert allow_iter_exception, (tag, q, name, gi, wi, deciding)
            assert abs(deciding - tol) <= 1e-3 * tol, (tag, q, name, gi, wi, deciding)
            skip_energy = True
    K = len(lp["margin"])
    if skip_energy:
        return K, 0
    assert close(rec["residual"], lrec["residual"], floor=res_floor), (tag, q, rec["residual"], lrec["residual"])
    assert close(rec["meta"]["ustar_res"], lrec["meta"]["ustar_res"], floor=res_floor)
    if exact_zero:  # M = lamG I: every operation is exact, the batch equals the device loop absolutely
        for key in ("deltaH_total",) + SUMS:
            assert rec[key] == lrec[key], (tag, q, key, rec[key], lrec[key])
        assert rec["null_points"] == [] and rec["meta"]["null_points_summary"]["total_null_points"] == 0
        assert lrec["null_points"] == []
        near = 0
    else:
        scale = 1e-3 * (abs(lrec["anchor_pen_sum"]) + abs(lrec["query_term_sum"])) if sum_floor else 0.0
        for key in ("deltaH_total",) + SUMS:
            assert abs(rec[key] - lrec[key]) <= REL * max(abs(lrec[key]), scale), (tag, q, key, rec[key], lrec[key])
        diff = yr.differing_rows(rec["null_points"], lrec["null_points"])
        assert all(lp["margin"][i] < NEAR for i in diff), (tag, q, [(i, lp["margin"][i]) for i in diff[:5]])
        near = len(diff)
        gz = {p["edge"][0]: p for p in rec["null_points"]}
        for p in lrec["null_points"]:
            i = p["edge"][0]
            if i in diff:
                continue
            assert close(gz[i]["z"], p["z"]) and close(gz[i]["residual"], p["residual"]), (tag, q, i, gz[i], p)
        if not diff:
            assert rec["meta"]["null_points_summary"] == lrec["meta"]["null_points_summary"]
            assert [p["edge"] for p in rec["null_points"]] == [p["edge"] for p in lrec["null_points"]]
    for key in ("version",):
        assert rec[key] == lrec[key]
    for key in ("ustar_converged", "ustar_iters", "avg_degree", "edge_density", "gates_min", "gates_max", "gates_mean",
                "gates_uniform", "state_sig", "receipt_detail"):
        assert rec["meta"][key] == lrec["meta"][key], (tag, q, key, rec["meta"][key], lrec["meta"][key])
    return K, near


def rounding_floor(Yc, psi, kw):
    """A solve that ends exactly (a one-row lattice, lamC = 0: Jacobi is the inverse) leaves a residual that is nothing but
    the float32 rounding of b - A x, whose size is eps32 |b| whatever the order of evaluation; two correct kernels agree on
    it no closer than that.  |b| <= (1 + lamG) |Y|_F + lamQ sqrt(K) |psi| bounds the right-hand sides of both solves."""
    lk = yg.lattice_kw(kw)
    b = (1.0 + lk["lamG"]) * np.linalg.norm(Yc.astype(np.float64)) + lk["lamQ"] * np.sqrt(len(Yc)) * np.linalg.norm(psi)
    return 1e-7 + float(np.finfo(np.float32).eps) * float(b)


def check_against_loop(amd, Y, P, top_k, k, alpha, kw, gate_kw, tag, queries=None, exact_zero=False,
                       allow_iter_exception=False, settle_dt=1.0):
    """Check 5 for one case.  gate_kw: {} or refine_many's gates arguments; in gated cases the loop gets the batch's gates.
    settle_dt: the step of both the batch's settle and the loop's."""
    with amd.Corpus(Y) as c:
        info = c.info(top_k, kw.get("kneighbors", 6), k)
        plain = c.refine_many(P, top_k, k, alpha, as_arrays=True, **kw, **gate_kw)
        arr = c.refine_many(P, top_k, k, alpha, as_arrays=True, receipts="full", settle_dt=settle_dt, **kw, **gate_kw)
        dcts = c.refine_many(P, top_k, k, alpha, receipts="full", settle_dt=settle_dt, **kw, **gate_kw)
        assert c.info(top_k, kw.get("kneighbors", 6), k) == info
        again = c.refine_many(P, top_k, k, alpha, as_arrays=True, **kw, **gate_kw)
    for key in plain:  # receipts=None after a receipts call: the same bytes as before it
        assert again[key].tobytes() == plain[key].tobytes(), (tag, key)
    for key in plain:  # bundle fields: receipts=None's bytes
        assert arr[key].dtype == plain[key].dtype and arr[key].tobytes() == plain[key].tobytes(), (tag, key)
    assert set(arr) == set(plain) | set(NEW_KEYS)
    assert arr["settle_iters"].dtype == np.int32 and arr["settle_res"].dtype == np.float32
    assert all(arr[key].dtype == np.float64 for key in ("deltaH",) + SUMS)
    rows = near = 0
    for q in (range(P.shape[0]) if queries is None else queries):
        cand = arr["candidates"][q]
        gates = arr["gates"][q] if gate_kw else None
        lp = loop(amd, Y[cand], P[q], k, alpha, kw, gates=gates, settle=(settle_dt, 12, 1e-3))
        n, t = check_query(tag, q, arr, dcts[q], lp, exact_zero=exact_zero, allow_iter_exception=allow_iter_exception)
        rows += n
        near += t
    print(f"{tag}: near-tie rows {near} of {rows}")
    assert near <= 0.05 * rows, (tag, near, rows)


@pytest.mark.parametrize("top_k,k,alpha,kw", UNGATED)
def test_receipts_against_loop(amd, top_k, k, alpha, kw):
    Y, P = clustered(top_k, k)
    zero = kw.get("lamC", 0.5) == 0.0 and kw.get("lamQ", 4.0) == 0.0
    check_against_loop(amd, Y, P, top_k, k, alpha, kw, {}, f"ungated{top_k}", exact_zero=zero)


@pytest.mark.parametrize("top_k,k,kw,beta,gamma", yg.SETTINGS)
def test_receipts_against_loop_gated(amd, top_k, k, kw, beta, gamma):
    Y, P = yg.corpus(top_k, k)
    check_against_loop(amd, Y, P, top_k, k, 0.5, kw, {"gates": "diffusion", "gate_beta": beta, "gate_gamma": gamma},
                       f"gated{top_k}")
    with amd.Corpus(Y) as c:  # given gates take the same path
        first = c.refine_many(P, top_k, k, 0.5, as_arrays=True, receipts="full", gates="diffusion", gate_beta=beta,
                              gate_gamma=gamma, **kw)
        given = c.refine_many(P, top_k, k, 0.5, as_arrays=True, receipts="full", gates=first["gates"], **kw)
    for key in NEW_KEYS:
        assert given[key].tobytes() == first[key].tobytes(), key


def oracle_receipt(Yc, psi, kw, gates, graph, settle_dt=1.0):
    """The oracle's settle / U* / deltaH / components / nulls on the device's candidate graph."""
    from oracle import oscillink_oracle as orc

    lk = yg.lattice_kw(kw)
    ref = orc.OracleLattice(Yc, graph=yg.dense_adj(graph, Yc.shape[0]).astype(np.float32), **lk)
    ref.set_query(psi, gates=gates)
    s = dict(ref.settle(dt=settle_dt, max_iters=12, tol=1e-3))
    Us = ref.solve_Ustar()
    dH = float(ref.deltaH(Us))
    coh, anc, qry = ref.components(Us)
    nulls = ref.nulls(Us, 3.0)
    A, sd = np.asarray(ref.A, np.float64), np.asarray(ref.sqrt_deg, np.float64)
    r, _, R = yr.edge_residuals(Us, A, sd, lk["lamC"])
    return {"settle": s, "ustar": ref.last_ustar, "deltaH": dH, "sums": [float(np.sum(v, dtype=np.float64)) for v in (coh, anc, qry)],
            "nulls": nulls, "margin": yr.null_margins(r, R, Yc.shape[0])}


@pytest.mark.parametrize("case", ["ungated100", "ungated30", "gated100"])
def test_receipts_against_oracle(amd, case):
    if case == "gated100":
        top_k, k, kw, beta, gamma = yg.SETTINGS[0]
        Y, P = yg.corpus(top_k, k)
        gate_kw = {"gates": "diffusion", "gate_beta": beta, "gate_gamma": gamma}
    else:
        top_k, k, _, kw = UNGATED[0] if case == "ungated100" else UNGATED[3]
        Y, P = clustered(top_k, k)
        gate_kw = {}
    with amd.Corpus(Y) as c:
        arr = c.refine_many(P, top_k, k, 0.5, as_arrays=True, receipts="full", **kw, **gate_kw)
        for q in (0, 3):
            cand = arr["candidates"][q]
            rowptr, col, a, w, sd = c._candidate_graph(cand, top_k, kw.get("kneighbors", 6), kw.get("row_cap_val", 1.0))
            want = oracle_receipt(Y[cand], P[q], kw, arr["gates"][q] if gate_kw else None, (rowptr, col, a))
            print(f"{case} q{q}: settle {int(arr['settle_iters'][q])}/{want['settle']['iters']} ustar "
                  f"{int(arr['ustar_iters'][q])}/{want['ustar']['iters']} dH {float(arr['deltaH'][q]):.9g}/{want['deltaH']:.9g}")
            assert int(arr["settle_iters"][q]) == want["settle"]["iters"]
            assert int(arr["ustar_iters"][q]) == want["ustar"]["iters"]
            assert close(float(arr["settle_res"][q]), want["settle"]["res"], floor=1e-7)
            assert close(float(arr["ustar_res"][q]), want["ustar"]["res"], floor=1e-7)
            assert close(float(arr["deltaH"][q]), want["deltaH"])
            for key, val in zip(SUMS, want["sums"]):
                assert close(float(arr[key][q]), val), (case, q, key)
            got = null_list(arr, q)
            diff = yr.differing_rows(got, want["nulls"])
            assert all(want["margin"][i] < NEAR for i in diff), (case, q, diff[:5])
            assert len(diff) <= 0.05 * top_k
            if not diff:
                assert int(arr["null_total"][q]) == len(want["nulls"])


def test_light_against_full(amd):
    Y, P = clustered(100, 8)
    with amd.Corpus(Y) as c:
        for gate_kw in ({}, {"gates": "diffusion", "gate_gamma": 0.15}):
            full = c.refine_many(P, 100, 8, as_arrays=True, receipts="full", **gate_kw)
            light = c.refine_many(P, 100, 8, as_arrays=True, receipts="light", **gate_kw)
            for key in ("deltaH", "settle_iters", "settle_res") + BUNDLE_KEYS:
                assert light[key].tobytes() == full[key].tobytes(), key
            for key in SUMS:
                assert np.array_equal(light[key], np.zeros(5))
            assert not any(key.startswith("null_") for key in light)
            dl = c.refine_many(P, 100, 8, receipts="light", **gate_kw)
            for q in range(5):
                rec = dl[q]["receipt"]
                assert rec["null_points"] == [] and rec["meta"]["receipt_detail"] == "light"
                assert rec["meta"]["null_points_summary"] == {"total_null_points": 0, "returned_null_points": 0,
                                                              "null_cap_applied": False}
                assert rec["deltaH_total"] == float(full["deltaH"][q])


def test_receipts_independence_and_chunking(amd):
    rng = np.random.default_rng(5)
    Y = rng.standard_normal((1500, 64)).astype(np.float32)
    P = rng.standard_normal((9, 64)).astype(np.float32)

    def per_query(r, q):
        s, e = int(r["null_offsets"][q]), int(r["null_offsets"][q + 1])
        out = {key: r[key][q].tobytes() for key in NEW_KEYS[:7] + BUNDLE_KEYS}
        out.update({key: r[key][s:e].tobytes() for key in NEW_KEYS[8:]})
        return out

    with amd.Corpus(Y) as c:
        for gate_kw in ({}, {"gates": "diffusion"}):
            full = c.refine_many(P, 50, 8, as_arrays=True, receipts="full", **gate_kw)
            assert int(full["null_total"].sum()) > 0
            for q in (0, 8, 4):
                alone = c.refine_many(P[q:q + 1], 50, 8, as_arrays=True, receipts="full", **gate_kw)
                assert per_query(alone, 0) == per_query(full, q), q
            moved = c.refine_many(P[::-1].copy(), 50, 8, as_arrays=True, receipts="full", **gate_kw)
            for q in range(9):
                assert per_query(moved, 8 - q) == per_query(full, q), q
            given = c.refine_many(P, 50, 8, candidates=full["candidates"], as_arrays=True, receipts="full", **gate_kw)
            for key in NEW_KEYS:
                assert given[key].tobytes() == full[key].tobytes(), key
        full = c.refine_many(P, 50, 8, as_arrays=True, receipts="full")
        chunk_plain = c.info(50)["chunk"]
    code = ("import numpy as np, sys; sys.path.insert(0, %r); from oscillink_amd import Corpus; "
            "rng = np.random.default_rng(5); Y = rng.standard_normal((1500, 64)).astype(np.float32); "
            "P = rng.standard_normal((9, 64)).astype(np.float32); c = Corpus(Y); assert c.info(50)['chunk'] == 4; "
            "r = c.refine_many(P, 50, 8, as_arrays=True, receipts='full'); "
            "np.savez(sys.argv[1], **r)") % ROOT
    assert chunk_plain == 256
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "r.npz")
        env = dict(os.environ, OSC_CORPUS_CHUNK="4")
        r = subprocess.run([sys.executable, "-c", code, out], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:]
        chunked = np.load(out)
        for key in NEW_KEYS + BUNDLE_KEYS:
            assert chunked[key].tobytes() == full[key].tobytes(), key


def test_null_cap(amd, monkeypatch):
    Y, P = clustered(100, 8)
    with amd.Corpus(Y) as c:
        monkeypatch.delenv("OSCILLINK_RECEIPT_NULL_CAP", raising=False)
        free = c.refine_many(P, 100, 8, as_arrays=True, receipts="full")
        assert int(free["null_total"].max()) > 3
        monkeypatch.setenv("OSCILLINK_RECEIPT_NULL_CAP", "3")
        capped = c.refine_many(P, 100, 8, as_arrays=True, receipts="full")
        dcts = c.refine_many(P, 100, 8, receipts="full")
    assert np.array_equal(capped["null_total"], free["null_total"])
    for key in ("deltaH", "settle_iters") + SUMS:
        assert capped[key].tobytes() == free[key].tobytes()
    for q in range(5):
        full_list = null_list(free, q)
        total = int(free["null_total"][q])
        z = np.array([p["z"] for p in full_list], dtype=np.float32)
        want = full_list if total <= 3 else [full_list[i] for i in np.argsort(-z, kind="stable")[:3]]
        assert null_list(capped, q) == want, q
        assert dcts[q]["receipt"]["null_points"] == want
        assert dcts[q]["receipt"]["meta"]["null_points_summary"] == {
            "total_null_points": total, "returned_null_points": min(total, 3), "null_cap_applied": total > 3}


def test_receipt_edges(amd):
    rng = np.random.default_rng(9)
    Y = rng.standard_normal((300, 16)).astype(np.float32)
    Y[7] = 0.0
    P = rng.standard_normal((3, 16)).astype(np.float32)
    P[1] = 0.0
    cand = np.stack([np.r_[7, np.arange(20, 39)], np.arange(40, 60), np.r_[np.arange(100, 119), 7]]).astype(np.int32)
    with amd.Corpus(Y) as c:
        # K = 1 (no edges), K = 2, lamC = 0, lamQ = 0, a zero query (P[1]) and a zero anchor row (candidate 7) among them
        for top_k, kw, cands in ((1, {}, None), (2, {}, None), (20, {}, cand), (20, {"lamC": 0.0}, cand),
                                 (20, {"lamQ": 0.0}, cand)):
            arr = c.refine_many(P, top_k, 4, as_arrays=True, receipts="full", candidates=None if cands is None else cands,
                                **kw)
            dcts = c.refine_many(P, top_k, 4, receipts="full", candidates=None if cands is None else cands, **kw)
            for q in range(3):
                lp = loop(amd, Y[arr["candidates"][q]], P[q], 4, 0.5, kw)
                check_query(f"edge K={top_k} {kw}", q, arr, dcts[q], lp, allow_iter_exception=True, sum_floor=True,
                            res_floor=rounding_floor(Y[arr["candidates"][q]], P[q], kw))
            if top_k == 1:
                assert np.array_equal(arr["null_total"], np.zeros(3)) and arr["null_i"].size == 0
        # k = 0 with receipts on: no bundle, the receipt stands
        none = c.refine_many(P, 20, 0, as_arrays=True, receipts="full", candidates=cand)
        some = c.refine_many(P, 20, 4, as_arrays=True, receipts="full", candidates=cand)
        assert none["ids"].shape == (3, 0)
        for key in NEW_KEYS:
            assert none[key].tobytes() == some[key].tobytes(), key
        assert c.refine_many(P, 20, 0, receipts="light", candidates=cand)[0]["bundle"] == []
        # settle_max_iters = 1: not converged, no raise, the loop's numbers
        arr = c.refine_many(P, 20, 4, as_arrays=True, receipts="full", candidates=cand, settle_max_iters=1)
        dcts = c.refine_many(P, 20, 4, receipts="full", candidates=cand, settle_max_iters=1)
        assert np.array_equal(arr["settle_iters"], np.ones(3)) and np.all(arr["settle_res"] > 1e-3)
        for q in range(3):
            lp = loop(amd, Y[cand[q]], P[q], 4, 0.5, {}, settle=(1.0, 1, 1e-3))
            check_query("max_iters=1", q, arr, dcts[q], lp, sum_floor=True, res_floor=rounding_floor(Y[cand[q]], P[q], {}))
        # other settle settings reach the kernel
        arr = c.refine_many(P, 20, 4, as_arrays=True, receipts="light", candidates=cand, settle_dt=0.5, settle_tol=1e-5)
        for q in range(3):
            lat = amd.Oscillink(Y[cand[q]])
            lat.set_query(P[q])
            s = lat.settle(dt=0.5, max_iters=12, tol=1e-5)
            dH = lat.receipt()["deltaH_total"]
            lat.close()
            assert int(arr["settle_iters"][q]) == s["iters"] and close(float(arr["deltaH"][q]), dH)
        # Q = 0
        empty = c.refine_many(np.zeros((0, 16), np.float32), 10, as_arrays=True, receipts="full")
        assert empty["deltaH"].shape == (0,) and empty["null_offsets"].tolist() == [0] and empty["null_i"].shape == (0,)
        assert empty["settle_iters"].dtype == np.int32 and empty["ids"].shape == (0, 8)
        assert c.refine_many(np.zeros((0, 16), np.float32), 10, receipts="light") == []
    with pytest.raises(ValueError, match="closed"):
        c.refine_many(P, 10, receipts="full")

"""Corpus.refine_many's per-lattice kernels (k_cq_solve plain and gated, k_cq_settle, k_cq_gates, k_cq_bundle,
k_cq_receipt) beyond 256 columns and 256 rows, on the shapes of tests/_refine_shapes.py: every
columns-per-thread instantiation NC in {1, 2, 3, 4, 6}, the 5 -> 6 fall-through, ragged and fully masked column groups,
pad columns, and one, part of and four times a 256-row round in the row-owning loops, the LDS row constants and the
null-point emit (uncapped rounds and the capped rank count).

The yardstick's margins on these corpora are proved on the CPU by tests/test_refine_shapes_host.py: no settle or U*
solve decides within 10 % of its tolerance, so iteration counts must be identical and no exception is accepted; at most
2 % of a shape's rows decide their null point inside the 1e-3 band; every k = 8 pick is decided by more than 1e-4."""
import numpy as np
import pytest

from tests import _gated as yg
from tests import _queries as yq
from tests import _receipt_yardstick as yr
from tests import _refine_shapes as rs
from tests.test_gated_refine_yardstick import MIN_SPREAD
from tests.test_gpu_refine_gated import GATE_ATOL, NEAR_TIE
from tests.test_gpu_refine_receipts import (BUNDLE_KEYS, NEAR, NEW_KEYS, SUMS, check_against_loop, close, null_list,
                                            oracle_receipt)

pytestmark = pytest.mark.gpu

NEAR_FRACTION = 0.02
PAD_REL = 1e-6
CASES = [(D, tk, rs.K, {}, 1.0) for D, tk in rs.SHAPES] + rs.EXTRA
PAD_SHAPES = [(D, tk) for D, tk in rs.SHAPES if D in (257, 520, 1290)]
CAP_SHAPES = [(300, 300), (1536, 1024)]


@pytest.fixture(scope="module")
def amd():
    import oscillink_amd

    return oscillink_amd


def _rel(got, want, floor=0.0):
    return abs(got - want) / max(abs(want), floor, 1e-300)


def _same_bytes(got, want, keys, tag):
    for key in keys:
        assert got[key].dtype == want[key].dtype and got[key].tobytes() == want[key].tobytes(), (tag, key)


@pytest.mark.parametrize("D,top_k,k,kw,dt", CASES)
def test_shapes_against_float64_and_oracle(amd, D, top_k, k, kw, dt):
    """Independent of every device kernel but the graph: the oracle's settle / U* / receipt and the float64 bundle and gates,
    all on the device's candidate graph."""
    Y, P = rs.cached_corpus(D, top_k)
    lk = yg.lattice_kw(kw)
    with amd.Corpus(Y) as c:
        for gate_kw in ({}, rs.GATE_KW):
            tag = f"D={D} top_k={top_k} k={k} {'gated' if gate_kw else 'ungated'}" + (f" {kw} dt={dt}" if kw else "")
            arr = c.refine_many(P, top_k, k, rs.ALPHA, as_arrays=True, receipts="full", settle_dt=dt, **kw, **gate_kw)
            assert arr["candidates"].shape == (rs.N_QUERIES, top_k) and arr["ids"].shape == (rs.N_QUERIES, min(k, top_k))
            near = compared = picks = gates_checked = 0
            worst = {key: 0.0 for key in ("settle_res", "ustar_res", "deltaH") + SUMS + ("score", "align", "gates")}
            iters = []
            for q in range(rs.N_QUERIES):
                cand = arr["candidates"][q]
                Yc = Y[cand]
                csr = c._candidate_graph(cand, top_k, rs.KNEIGHBORS, lk["row_cap_val"])
                gates = arr["gates"][q] if gate_kw else None
                want = oracle_receipt(Yc, P[q], kw, gates, csr[:3], settle_dt=dt)
                got_it = (int(arr["settle_iters"][q]), int(arr["ustar_iters"][q]))
                iters.append(got_it)
                print(f"{tag} q{q}: settle {got_it[0]}/{want['settle']['iters']} res {float(arr['settle_res'][q]):.6e}/"
                      f"{want['settle']['res']:.6e}  ustar {got_it[1]}/{want['ustar']['iters']} res "
                      f"{float(arr['ustar_res'][q]):.6e}/{want['ustar']['res']:.6e}  dH {float(arr['deltaH'][q]):.9g}/"
                      f"{want['deltaH']:.9g}  sums "
                      + " ".join(f"{float(arr[key][q]):.9g}/{val:.9g}" for key, val in zip(SUMS, want["sums"]))
                      + f"  nulls {int(arr['null_total'][q])}/{len(want['nulls'])}")
                assert got_it == (want["settle"]["iters"], want["ustar"]["iters"]), (tag, q)  # no exception accepted
                pairs = [("settle_res", float(arr["settle_res"][q]), want["settle"]["res"], 1e-7),
                         ("ustar_res", float(arr["ustar_res"][q]), want["ustar"]["res"], 1e-7),
                         ("deltaH", float(arr["deltaH"][q]), want["deltaH"], 0.0)]
                pairs += [(key, float(arr[key][q]), val, 0.0) for key, val in zip(SUMS, want["sums"])]
                for key, g, w, floor in pairs:
                    worst[key] = max(worst[key], _rel(g, w, floor))
                    assert close(g, w, floor=floor), (tag, q, key, g, w)
                # null points
                got = null_list(arr, q)
                diff = yr.differing_rows(got, want["nulls"])
                assert all(want["margin"][i] < NEAR for i in diff), (tag, q, [(i, want["margin"][i]) for i in diff[:5]])
                near += len(diff)
                if not diff:
                    assert int(arr["null_total"][q]) == len(want["nulls"]) == len(got), (tag, q)
                    assert [p["edge"] for p in got] == [[int(v) for v in p["edge"]] for p in want["nulls"]], (tag, q)
                if (D, top_k) == (1536, 7):
                    assert got == [] and int(arr["null_total"][q]) == 0, (tag, q)
                # the bundle from the exact float64 U*
                A = yg.dense_adj(csr, top_k)
                B = np.ones(top_k) if gates is None else gates.astype(np.float64)
                M = yq.dense_M(A, csr[4], B, lk["lamG"], lk["lamC"], lk["lamQ"])
                U = yq.ustar(M, Yc, B, P[q], lk["lamG"], lk["lamQ"])
                ids64, score64, align64, margins = yq.bundle(Yc, U, P[q], csr[:3], csr[4], lk["lamC"], k=k, alpha=rs.ALPHA)
                ok, _ = yq.same_until_near_tie(arr["local"][q].tolist(), ids64, margins, NEAR_TIE)
                assert ok, (tag, q, arr["local"][q].tolist(), ids64, margins)
                assert np.array_equal(arr["ids"][q], cand[arr["local"][q]])
                cut = next((t for t, m in enumerate(margins) if m < NEAR_TIE), len(ids64))
                picks += len(ids64)
                compared += cut
                for t in range(cut):
                    worst["score"] = max(worst["score"], abs(float(arr["score"][q][t]) - score64[t]))
                    worst["align"] = max(worst["align"], abs(float(arr["align"][q][t]) - align64[t]))
                    assert abs(float(arr["score"][q][t]) - score64[t]) <= 1e-4, (tag, q, t)
                    assert abs(float(arr["align"][q][t]) - align64[t]) <= 1e-5, (tag, q, t)
                if gate_kw:
                    g64, raw64, _ = yg.gates64(A, csr[4], Yc, P[q], rs.GATE_BETA, rs.GATE_GAMMA)
                    spread = float(raw64.max() - raw64.min())
                    err = float(np.abs(arr["gates"][q] - g64).max())
                    print(f"{tag} q{q}: gate spread {spread:.4f} |gates - float64| {err:.2e} gate_iters "
                          f"{int(arr['gate_iters'][q])}")
                    if spread >= MIN_SPREAD:  # below it fp32 round-off / spread is the gates' error
                        gates_checked += 1
                        worst["gates"] = max(worst["gates"], err)
                        np.testing.assert_allclose(arr["gates"][q], g64, atol=GATE_ATOL, rtol=0)
            rows = rs.N_QUERIES * top_k
            print(f"{tag}: iters (settle, ustar) {iters}  near-tie null rows {near} of {rows}  picks compared {compared}/"
                  f"{picks}  gates checked {gates_checked}  worst "
                  + " ".join(f"{key} {val:.2e}" for key, val in worst.items()))
            assert near <= NEAR_FRACTION * rows, (tag, near, rows)
            if k == rs.K:  # the host test's licence: no k = 8 pick is a near tie, the whole list is compared
                assert compared == picks, (tag, compared, picks)


@pytest.mark.parametrize("D,top_k,k,kw,dt", CASES)
def test_shapes_against_device_loop(amd, D, top_k, k, kw, dt):
    """Against Oscillink(Y[cand]) -> set_query -> settle -> bundle -> receipt on the device; at K = 1024, D = 1536 the loop's
    lattice goes through whichever settle route its own plan picks."""
    Y, P = rs.cached_corpus(D, top_k)
    for gate_kw in ({}, rs.GATE_KW):
        tag = f"D={D} top_k={top_k} k={k} {'gated' if gate_kw else 'ungated'}"
        check_against_loop(amd, Y, P, top_k, k, rs.ALPHA, kw, gate_kw, tag, allow_iter_exception=False, settle_dt=dt)


@pytest.mark.parametrize("D,top_k,k,kw,dt", CASES)
def test_shapes_identities(amd, D, top_k, k, kw, dt):
    """Byte identities that pin the template dispatch: the gated and the ungated instantiation of one NC, the given-gates
    and the computed-gates route, light and full detail, and a call before and after a receipts call."""
    Y, P = rs.cached_corpus(D, top_k)
    tag = f"D={D} top_k={top_k} k={k}"
    ones = np.ones((rs.N_QUERIES, top_k), np.float32)
    with amd.Corpus(Y) as c:
        def run(**more):
            return c.refine_many(P, top_k, k, rs.ALPHA, as_arrays=True, settle_dt=dt, **kw, **more)

        before = run()
        for receipts in (None, "full"):
            plain = run(receipts=receipts)
            got = run(receipts=receipts, gates=ones)
            assert set(got) == set(plain) | {"gates", "gate_iters", "gate_res"}
            assert np.array_equal(got["gates"], ones)
            _same_bytes(got, plain, plain.keys(), (tag, "ones", receipts))
        full = plain
        _same_bytes(run(), before, before.keys(), (tag, "receipts=None after receipts"))
        _same_bytes(full, before, before.keys(), (tag, "bundle keys with receipts"))
        first = run(receipts="full", **rs.GATE_KW)
        given = run(receipts="full", gates=first["gates"])
        assert set(given) == set(first) and first["gate_iters"].min() >= 1 and not given["gate_iters"].any()
        _same_bytes(given, first, [key for key in first if key not in ("gate_iters", "gate_res")], (tag, "given gates"))
        assert set(NEW_KEYS) <= set(first)
        for name, ref, gate_kw in (("ungated", full, {}), ("gated", first, rs.GATE_KW)):
            light = run(receipts="light", **gate_kw)
            _same_bytes(light, ref, ("deltaH", "settle_iters", "settle_res") + BUNDLE_KEYS, (tag, "light", name))
            assert not any(key.startswith("null_") for key in light)
            for key in SUMS:
                assert np.array_equal(light[key], np.zeros(rs.N_QUERIES))


@pytest.mark.parametrize("D,top_k", PAD_SHAPES)
def test_pad_columns_are_inert(amd, D, top_k):
    """A corpus widened with zero columns to the next multiple of 32 (the device's own row stride for D) gives the same
    lattices.  Held to: equal candidates, picks, iteration counts and null points, and deltaH / the sums within 1e-6
    relative -- the fold order of the 64-lane sums follows ldn, which is in fact equal on both sides."""
    Y, P = rs.cached_corpus(D, top_k)
    pad = rs.ldn(D) - D
    assert pad > 0
    Y2 = np.hstack([Y, np.zeros((Y.shape[0], pad), np.float32)])
    P2 = np.hstack([P, np.zeros((P.shape[0], pad), np.float32)])
    for gate_kw in ({}, rs.GATE_KW):
        with amd.Corpus(Y) as c:
            a = c.refine_many(P, top_k, rs.K, rs.ALPHA, as_arrays=True, receipts="full", **gate_kw)
        with amd.Corpus(Y2) as c:
            b = c.refine_many(P2, top_k, rs.K, rs.ALPHA, as_arrays=True, receipts="full", **gate_kw)
        tag = f"D={D}->{rs.ldn(D)} top_k={top_k} {'gated' if gate_kw else 'ungated'}"
        assert set(a) == set(b)
        same = sorted(key for key in a if a[key].tobytes() == b[key].tobytes())
        print(f"{tag}: byte-equal keys {len(same)}/{len(a)}; not byte-equal: {sorted(set(a) - set(same))}; worst relative "
              + " ".join(f"{key} {float(np.max(np.abs(a[key] - b[key]) / np.abs(a[key]))):.2e}" for key in ("deltaH",) + SUMS))
        exact = ("candidates", "ids", "local", "settle_iters", "ustar_iters", "null_total", "null_offsets", "null_i", "null_j")
        _same_bytes(b, a, exact + (("gate_iters",) if gate_kw else ()), tag)
        for key in ("deltaH",) + SUMS:
            assert np.all(np.abs(b[key] - a[key]) <= PAD_REL * np.abs(a[key])), (tag, key, a[key], b[key])


@pytest.mark.parametrize("D,top_k", CAP_SHAPES)
def test_null_cap_beyond_256_rows(amd, monkeypatch, D, top_k):
    """OSCILLINK_RECEIPT_NULL_CAP with more than 256 rows: 3, 300 (more slots than a round of rows; capped at K = 1024, not
    at K = 300) and 2000 (>= K, never capped), against the uncapped list stably sorted by float32 z and truncated."""
    Y, P = rs.cached_corpus(D, top_k)
    with amd.Corpus(Y) as c:
        monkeypatch.delenv("OSCILLINK_RECEIPT_NULL_CAP", raising=False)
        free = c.refine_many(P, top_k, rs.K, rs.ALPHA, as_arrays=True, receipts="full")
        assert int(free["null_total"].min()) > 0.6 * top_k  # (the host test: more than 256 at K = 1024, fewer than 300 at 300)
        for cap in (3, 300, 2000):
            monkeypatch.setenv("OSCILLINK_RECEIPT_NULL_CAP", str(cap))
            capped = c.refine_many(P, top_k, rs.K, rs.ALPHA, as_arrays=True, receipts="full")
            dcts = c.refine_many(P, top_k, rs.K, rs.ALPHA, receipts="full")
            assert np.array_equal(capped["null_total"], free["null_total"])
            _same_bytes(capped, free, ("deltaH", "settle_iters", "settle_res") + SUMS + BUNDLE_KEYS, (D, top_k, cap))
            for q in range(rs.N_QUERIES):
                full_list = null_list(free, q)
                total = int(free["null_total"][q])
                assert total == len(full_list)
                z = np.array([p["z"] for p in full_list], dtype=np.float32)
                want = full_list if total <= cap else [full_list[i] for i in np.argsort(-z, kind="stable")[:cap]]
                print(f"D={D} top_k={top_k} cap={cap} q{q}: total {total} kept {len(null_list(capped, q))}")
                assert null_list(capped, q) == want, (cap, q)
                assert dcts[q]["receipt"]["null_points"] == want, (cap, q)
                assert dcts[q]["receipt"]["meta"]["null_points_summary"] == {
                    "total_null_points": total, "returned_null_points": min(total, cap), "null_cap_applied": total > cap}
        if top_k == 1024:
            assert int(free["null_total"].min()) > 300  # the cap of 300 bites here: the rank count fills 300 slots
        else:
            assert int(free["null_total"].max()) < 300  # and does not here: the uncapped rounds run with slots = 300

"""Corpus.refine_many(receipts=...) without a device: the new entry point is exported, declared
the same way in the header and the ctypes table and rejects a NULL handle; the Python-side checks of the receipts
arguments run before any native call; and the yardstick the GPU tests lean on -- the oracle's settle / U* / deltaH /
components / null points on the candidate lattices of tests/test_gpu_refine_receipts.py -- shows the margins those tests
rely on: no settle or U* solve decides closer than 3 % to its tolerance (so the GPU test accepts no iteration-count
exception), and at most 5 % of a case's rows decide their null point inside the 1e-3 near-tie band."""
import os
import re

import numpy as np
import pytest

from tests import _gated as yg
from tests import _receipt_yardstick as yr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNGATED = [(100, 8, {}), (64, 1, {"kneighbors": 16}), (64, 64, {"lamC": 0.0, "lamQ": 0.0}),
           (30, 40, {"lamG": 2.0, "lamC": 1.5, "lamQ": 0.5, "row_cap_val": 0.3}), (7, 8, {"kneighbors": 2000})]
CASES = [("ungated", tk, k, kw, None, None) for tk, k, kw in UNGATED] + \
        [("gated", tk, k, kw, b, g) for tk, k, kw, b, g in yg.SETTINGS]


def _ungated_corpus(top_k, k):
    rng = np.random.default_rng(top_k + k)
    centers = rng.standard_normal((6, 96)).astype(np.float32) * 2
    Y = (centers[rng.integers(0, 6, 2000)] + 0.5 * rng.standard_normal((2000, 96))).astype(np.float32)
    P = rng.standard_normal((5, 96)).astype(np.float32)
    return Y, P


def test_entry_point_is_exported_declared_and_rejects_a_null_handle():
    from oscillink_amd import _build, _native as nat

    _build.build()
    lib = nat.lib()
    res, args = nat.SIGNATURES["osc_corpus_refine_receipts"]
    with open(os.path.join(ROOT, "include", "oscillink_hip.h")) as f:
        header = f.read()
    m = re.search(r"int osc_corpus_refine_receipts\((.*?)\);", header, re.S)
    assert m, "include/oscillink_hip.h does not declare osc_corpus_refine_receipts"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert len(params) == len(args) == 53

    def ctype_of(p):
        p = re.sub(r"\b\w+$", "", p).replace("const", "").replace(" ", "")
        return {"osc_corpus_handle": nat.Handle, "float*": nat.c_f32p, "int32_t*": nat.c_i32p, "int64_t*": nat.c_i64p,
                "double*": nat.c_f64p, "int32_t": nat.C.c_int32, "int64_t": nat.C.c_int64, "float": nat.C.c_float}[p]

    assert [ctype_of(p) for p in params] == list(args)
    call = [None, None, 0, 1, None, 0, None, 1.0, 0.1, 0, 1e-4, 256, 6, 1.0, 1.0, 0.5, 4.0, 1e-4, 64, 8, 0.5, 1.0, 12, 1e-3,
            1, 3.0, 0] + [None] * 21 + [0, None, None, None, 2048]
    assert len(call) == 53
    assert lib.osc_corpus_refine_receipts(*call) == nat.OSC_E_INVALID
    call[0] = nat.Handle()
    assert lib.osc_corpus_refine_receipts(*call) == nat.OSC_E_INVALID


def _fake_corpus():
    """A Corpus object with no device behind it: any native call is an error."""
    from oscillink_amd.corpus import Corpus

    c = Corpus.__new__(Corpus)
    c._h, c.N, c.D = object(), 50, 8

    def no_native(name, *args):
        raise AssertionError(f"native call {name} before validation")

    c._call = no_native
    return c


@pytest.mark.parametrize("bad,name", [
    (dict(receipts="medium"), "receipts"), (dict(receipts=True), "receipts"), (dict(receipts=""), "receipts"),
    (dict(receipts="full", settle_dt=0.0), "settle_dt"), (dict(receipts="full", settle_dt=-1.0), "settle_dt"),
    (dict(receipts="light", settle_dt=float("nan")), "settle_dt"), (dict(receipts="full", settle_dt=float("inf")), "settle_dt"),
    (dict(receipts="full", settle_max_iters=0), "settle_max_iters"), (dict(receipts="light", settle_tol=float("nan")), "settle_tol"),
    (dict(receipts="full", settle_tol=float("inf")), "settle_tol"),
])
def test_receipts_arguments_are_checked_before_any_native_call(bad, name):
    c = _fake_corpus()
    P = np.ones((2, 8), np.float32)
    with pytest.raises(ValueError, match=name):
        c.refine_many(P, 10, **bad)
    with pytest.raises(ValueError, match=name):
        c.refine_many(P, 10, as_arrays=True, gates="diffusion", **bad)
    c._h = None  # (so that __del__ has nothing to destroy)


def test_receipt_settings_values():
    from oscillink_amd.corpus import Corpus

    assert Corpus._receipt_settings(None, 1.0, 12, 1e-3) == (None, 1.0, 12, 1e-3)
    assert Corpus._receipt_settings("light", 0.5, 1, 0.0) == (0, 0.5, 1, 0.0)
    assert Corpus._receipt_settings("full", 2, 3, -1.0) == (1, 2.0, 3, -1.0)  # a tolerance nothing meets: no raise
    c = _fake_corpus()
    with pytest.raises(AssertionError, match="osc_corpus_refine_receipts"):  # valid arguments do reach the new entry point
        c.refine_many(np.ones((2, 8), np.float32), 10, receipts="light")
    with pytest.raises(AssertionError, match="osc_corpus_refine "):  # and receipts=None still goes where it went
        try:
            c.refine_many(np.ones((2, 8), np.float32), 10)
        except AssertionError as e:
            raise AssertionError(str(e).replace("before", " before")) from None
    c._h = None


@pytest.mark.parametrize("kind,top_k,k,kw,beta,gamma", CASES)
def test_oracle_yardstick_margins(kind, top_k, k, kw, beta, gamma):
    from oracle import oscillink_oracle as orc

    Y, P = _ungated_corpus(top_k, k) if kind == "ungated" else yg.corpus(top_k, k)
    lk = yg.lattice_kw(kw)
    cos = yg.host_cos(Y, P)
    zero = lk["lamC"] == 0.0 and lk["lamQ"] == 0.0
    near = rows = 0
    worst = 1.0
    for q in range(P.shape[0]):
        cand = np.lexsort((np.arange(Y.shape[0]), -cos[q]))[:top_k]
        Yc = Y[cand]
        g = None
        if kind == "gated":
            g = orc.diffusion_gates(Yc, P[q], kneighbors=lk["kneighbors"], row_cap_val=lk["row_cap_val"], beta=beta,
                                    gamma=gamma)
        o = orc.OracleLattice(Yc, **lk)
        o.set_query(P[q], gates=g)
        s = dict(o.settle())
        hs = list(o.history)
        Us = o.solve_Ustar()
        hu = list(o.history)
        dH = float(o.deltaH(Us))
        coh, anc, qry = o.components(Us)
        nulls = o.nulls(Us)
        dec = min(min(abs(x - 1e-3) / 1e-3 for x in hs), min(abs(x - 1e-4) / 1e-4 for x in hu))
        worst = min(worst, dec)
        r, _, R = yr.edge_residuals(Us, np.asarray(o.A), o.sqrt_deg, o.lamC)
        m = yr.null_margins(r, R, top_k)
        print(f"{kind} top_k={top_k} q={q}: settle {s['iters']} ustar {o.last_ustar['iters']} dH {dH:.6g} sums "
              f"{float(coh.sum()):.6g} {float(anc.sum()):.6g} {float(qry.sum()):.6g} nulls {len(nulls)} "
              f"near-tie rows {int(np.sum(m < 1e-3))} closest deciding residual {dec:.4f}")
        assert 1 <= s["iters"] <= 6 and 1 <= o.last_ustar["iters"] <= 7
        assert s["res"] <= 1e-3 and o.last_ustar["converged"]
        if zero:  # M = lamG I: U+ = U* = Y exactly, everything is 0.0 and no row has a null point
            assert s["iters"] == 1 and o.last_ustar["iters"] == 1
            assert dH == 0.0 and float(coh.sum()) == 0.0 and float(anc.sum()) == 0.0 and float(qry.sum()) == 0.0
            assert nulls == [] and np.all(R == 0.0)
            continue
        assert 6.7 <= dH <= 4905.0 * (1 + 1e-4), dH
        near += int(np.sum(m < 1e-3))
        rows += top_k
    assert worst >= 0.03, worst
    if not zero:
        assert near <= 0.05 * rows, (near, rows)

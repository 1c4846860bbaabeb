"""Per-query settings of Corpus.refine_many, the parts that need no GPU: osc_corpus_settings is
exported, bound and declared with the reference seams it stands for, a NULL handle is OSC_E_INVALID, the Python checks raise
before any native call and name the first offending query, a call with all ten arguments scalar makes exactly the native
calls it made before and arms nothing, and corpus_settings.hpp's arithmetic survives its sweep under
-fsanitize=address,undefined (a stand-alone program, the pattern of test_refine_ragged_host.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.test_host_logic_sanitized import _build_and_run
from tests.test_receipt_records_host import fake_corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEAMS = ("cloud/app/main.py:887-947", "cloud/app/learners.py:148-192", "scripts/benchmark_adaptive.py:186-232")
TEN = ("lamG", "lamC", "lamQ", "lamP", "kneighbors", "k", "alpha", "settle_dt", "settle_max_iters", "settle_tol")


def test_the_entry_point_is_exported_and_bound():
    from oscillink_amd import _native as nat

    f = nat.lib().osc_corpus_settings
    assert f.restype is C.c_int and f.argtypes[0] is nat.Handle and len(f.argtypes) == 3
    # the record the binding fills is the header's struct: seven floats, three int32, in its order
    assert nat.SETTING_DTYPE.itemsize == 40
    assert nat.SETTING_DTYPE.names == ("lamG", "lamC", "lamQ", "lamP", "alpha", "settle_dt", "settle_tol", "kneighbors", "k",
                                       "settle_max_iters")


def test_the_entry_point_is_declared_with_the_reference_seams():
    with open(os.path.join(ROOT, "include", "oscillink_hip.h")) as f:
        text = f.read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int osc_corpus_settings\(osc_corpus_handle h, const osc_corpus_setting\* per_query,"
                  r" int32_t Q\);", text, re.S)
    assert m, "osc_corpus_settings is not declared behind a comment"
    for seam in SEAMS:
        assert seam in m.group(1), seam
    s = re.search(r"typedef struct osc_corpus_setting \{(.*?)\} osc_corpus_setting;", text, re.S)
    assert s and re.sub(r"\s+", " ", s.group(1)).strip() == (
        "float lamG, lamC, lamQ, lamP, alpha, settle_dt, settle_tol; int32_t kneighbors, k, settle_max_iters;")


def test_a_null_handle_is_invalid():
    from oscillink_amd import _native as nat

    rec = np.zeros(3, dtype=nat.SETTING_DTYPE)
    assert nat.lib().osc_corpus_settings(nat.Handle(), rec.ctypes.data_as(C.c_void_p), 3) == nat.OSC_E_INVALID
    assert nat.lib().osc_corpus_settings(nat.Handle(), None, 0) == nat.OSC_E_INVALID


def _recording(c):
    """c's `_call` wrapped: every native call's name is kept in c.names; the arming calls are served here."""
    inner = c._call
    c.names, c.armed = [], []

    def call(name, *args):
        c.names.append(name)
        if name == "osc_corpus_settings":
            c.armed.append(args[1])
            return None
        return inner(name, *args)

    c._call = call
    return c


BAD = [("lamG", [1.0, 2.0, 0.0], r"query 2: lamG must be > 0"), ("lamG", [1.0, -1.0, 0.0], r"query 1: lamG must be > 0"),
       ("lamC", [0.0, 0.5, -0.1], r"query 2: lamC must be >= 0"), ("lamC", [np.inf, 0.5, -0.1], r"query 0: lamC must be >= 0"),
       ("lamQ", [4.0, np.nan, 1.0], r"query 1: lamQ must be >= 0"), ("lamP", [0.0, 0.2, -1.5], r"query 2: lamP must be >= 0"),
       ("kneighbors", [1, 0, 0], r"query 1: kneighbors must be >= 1"),
       ("kneighbors", [6, 6, 500], r"query 2: min\(kneighbors, K - 1\) = 199 exceeds the limit of 128"),
       ("settle_dt", [1.0, 0.5, 0.0], r"query 2: settle_dt must be finite and > 0"),
       ("settle_dt", [np.inf, 0.5, 0.0], r"query 0: settle_dt must be finite and > 0"),
       ("settle_max_iters", [12, 1, 0], r"query 2: settle_max_iters must be >= 1"),
       ("settle_tol", [1e-3, 0.0, np.nan], r"query 2: settle_tol must be finite"),
       ("alpha", [0.0, np.inf, np.nan], r"query 1: alpha must be finite")]


@pytest.mark.parametrize("name,values,message", BAD)
def test_every_value_gets_the_scalars_check_before_any_native_call(name, values, message):
    c = _recording(fake_corpus(K=5))
    c.N = 300
    P = np.ones((3, 8), dtype=np.float32)
    top_k = 200 if "199" in message else 5
    for form in (list, np.asarray, tuple):
        with pytest.raises(ValueError, match=message):
            c.refine_many(P, top_k, receipts="full", chains=[[0, 1], None, [1, 2]], **{name: form(values)})
    if name == "kneighbors":
        with pytest.raises(ValueError, match=message):
            c.diffusion_gates_many(P, top_k, kneighbors=values)
    assert c.names == []


@pytest.mark.parametrize("name", TEN)
def test_a_shape_other_than_q_is_refused(name):
    c = _recording(fake_corpus(K=5))
    P = np.ones((3, 8), dtype=np.float32)
    for bad in ([1, 1], [1, 1, 1, 1], np.ones((3, 1)), np.ones((1, 3)), []):
        with pytest.raises(ValueError, match=rf"{name} must be a scalar or a \(3,\) array"):
            c.refine_many(P, 5, **{name: bad})
    assert c.names == []


MODES = {"plain": ({}, "osc_corpus_refine"), "gated": ({"gates": "diffusion"}, "osc_corpus_refine_gated"),
         "receipts": ({"receipts": "full"}, "osc_corpus_refine_receipts"),
         "chains": ({"chains": [[0, 1], None], "receipts": "light"}, "osc_corpus_refine_chains")}
SCALARS = dict(lamG=2.0, lamC=0.25, lamQ=3.0, lamP=0.5, kneighbors=3, k=2, alpha=0.75, settle_dt=0.5, settle_max_iters=7,
               settle_tol=1e-4)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_all_scalars_is_the_call_it_was_and_arms_nothing(mode):
    extra, entry = MODES[mode]
    P = np.ones((2, 8), dtype=np.float32)
    seen = []
    for form in (lambda v: v, lambda v: np.asarray(v), lambda v: np.asarray(v)[()]):
        c = _recording(fake_corpus(K=5, kk=2))
        kw = {n: form(v) for n, v in SCALARS.items()}
        out = c.refine_many(P, 5, as_arrays=True, **kw, **extra)
        assert c.names == [entry] and c.armed == [], (mode, c.names)
        assert "picks" not in out
        seen.append(c.events)
    for ev in seen[1:]:  # a 0-d array and a NumPy scalar are scalars: the same native arguments
        assert ev == seen[0]
    scalars = seen[0][0][1]
    solve = [3, 1.0, 2.0, 0.25, 3.0, 1e-4, 64, 2, 0.75]  # kneighbors, row_cap, lamG, lamC, lamQ, tol, max_iters, k, alpha
    at = next(i for i in range(len(scalars)) if scalars[i:i + len(solve)] == solve)
    assert scalars[:2] == [2, 5] and at >= 2
    if mode in ("receipts", "chains"):
        assert scalars[at + len(solve):at + len(solve) + 3] == [0.5, 7, 1e-4]
    if mode == "chains":
        assert 0.5 in scalars[at + len(solve) + 3:]  # lamP


def test_a_per_query_argument_arms_the_records_for_the_call():
    c = _recording(fake_corpus(K=5, kk=3))
    P = np.ones((2, 8), dtype=np.float32)
    out = c.refine_many(P, 5, as_arrays=True, k=[1, 3], lamG=np.array([0.5, 2.0]), lamC=0.25, settle_tol=[0.0, 1e-6],
                        receipts="light")
    assert c.names == ["osc_corpus_settings", "osc_corpus_refine_receipts"] and c.armed == [2]
    assert out["picks"].dtype == np.int32 and out["picks"].tolist() == [1, 3]
    assert out["local"].shape == (2, 3)
    c = _recording(fake_corpus(K=5, kk=3))
    out = c.refine_many(P, 5, as_arrays=True, k=3, lamG=[0.5, 2.0])
    assert c.names == ["osc_corpus_settings", "osc_corpus_refine"] and "picks" not in out


def test_corpus_settings_sweep_under_address_and_undefined_sanitizers(tmp_path):
    out = _build_and_run(str(tmp_path), "sweep_corpus_settings.cpp",
                         ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    assert "corpus settings sweep ok" in out and "ERROR" not in out and "runtime error" not in out

"""Ragged corpus refine, the parts that need no GPU: the two entry points are exported, bound and
declared with the reference seam they stand for, a NULL handle is OSC_E_INVALID, `ragged` is a keyword of the three Python
calls, and corpus_ragged.hpp's arithmetic survives its sweep under -fsanitize=address,undefined (the pattern of
test_corpus_plan_sanitized.py: a stand-alone program)."""
import ctypes as C
import inspect
import os
import re

from tests.test_host_logic_sanitized import _build_and_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("osc_corpus_ragged", "osc_corpus_ragged_rows")


def test_the_entry_points_are_exported_and_bound():
    from oscillink_amd import _native as nat

    L = nat.lib()
    for name in SYMBOLS:
        f = getattr(L, name)
        assert f.restype is C.c_int and f.argtypes[0] is nat.Handle and len(f.argtypes) == 3, name


def test_the_entry_points_are_declared_with_the_reference_seam():
    with open(os.path.join(ROOT, "include", "oscillink_hip.h")) as f:
        text = f.read()
    for name in SYMBOLS:
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int " + name + r"\(osc_corpus_handle h,", text, re.S)
        assert m, f"{name} is not declared behind a comment"
        assert "proof_hallucination.py:203-221" in m.group(1), f"{name}'s comment does not cite the reference seam"


def test_a_null_handle_is_invalid():
    from oscillink_amd import _native as nat

    L = nat.lib()
    rows = (C.c_int32 * 4)(1, 2, 3, 4)
    null = nat.Handle()
    assert L.osc_corpus_ragged(null, rows, 4) == nat.OSC_E_INVALID
    assert L.osc_corpus_ragged(null, None, 4) == nat.OSC_E_INVALID
    assert L.osc_corpus_ragged_rows(null, rows, 4) == nat.OSC_E_INVALID


def test_ragged_is_a_keyword_of_the_three_calls():
    from oscillink_amd import Corpus

    for name in ("search", "refine_many", "diffusion_gates_many"):
        p = inspect.signature(getattr(Corpus, name)).parameters
        assert "ragged" in p, name
        assert p["ragged"].kind is inspect.Parameter.KEYWORD_ONLY and p["ragged"].default is False, name


def test_corpus_ragged_sweep_under_address_and_undefined_sanitizers(tmp_path):
    out = _build_and_run(str(tmp_path), "sweep_corpus_ragged.cpp",
                         ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    assert "corpus ragged sweep ok" in out and "ERROR" not in out and "runtime error" not in out

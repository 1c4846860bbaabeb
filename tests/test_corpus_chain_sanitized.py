"""Sanitizer build of the chain prior's host logic (oscillink_amd/csrc/corpus_chain.hpp and the chain blocks of
corpus_plan.hpp), swept by tests/host_logic/sweep_corpus_chain.cpp under -fsanitize=address,undefined on the CPU (the
pattern of test_corpus_receipts_plan_sanitized.py)."""
from tests.test_host_logic_sanitized import _build_and_run


def test_corpus_chain_sweep_under_address_and_undefined_sanitizers(tmp_path):
    out = _build_and_run(str(tmp_path), "sweep_corpus_chain.cpp",
                         ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    assert "corpus chain sweep ok" in out and "ERROR" not in out and "runtime error" not in out

"""Sanitizer build of the mutable corpus's row-store arithmetic (oscillink_amd/csrc/corpus_store.hpp), swept by
tests/host_logic/sweep_corpus_store.cpp under -fsanitize=address,undefined on the CPU (the pattern of
test_corpus_plan_sanitized.py)."""
from tests.test_host_logic_sanitized import _build_and_run


def test_corpus_store_sweep_under_address_and_undefined_sanitizers(tmp_path):
    out = _build_and_run(str(tmp_path), "sweep_corpus_store.cpp",
                         ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    assert "corpus store sweep ok" in out and "ERROR" not in out and "runtime error" not in out

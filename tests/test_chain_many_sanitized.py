"""Sanitizer build of chain_receipt_many's host logic (oscillink_amd/csrc/chain_many.hpp over corpus_chain.hpp's
build_chain_path), swept by tests/host_logic/sweep_chain_many.cpp under -fsanitize=address,undefined on the CPU (the pattern
of test_corpus_chain_sanitized.py)."""
from tests.test_host_logic_sanitized import _build_and_run


def test_chain_many_sweep_under_address_and_undefined_sanitizers(tmp_path):
    out = _build_and_run(str(tmp_path), "sweep_chain_many.cpp",
                         ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    assert "chain many sweep ok" in out and "ERROR" not in out and "runtime error" not in out

"""The anchor-start chain's validity (oscillink_amd/csrc/derived_state.hpp: Level, held, begin_build, built) beside a model of
the per-level transitions it replaced, over every reachable state: tests/host_logic/sweep_anchor_chain.cpp, a stand-alone
program built and run under -fsanitize=address,undefined on the CPU (the pattern of test_host_logic_sanitized.py)."""
from tests.test_host_logic_sanitized import _build_and_run


def test_anchor_chain_sweep_under_address_and_undefined_sanitizers(tmp_path):
    out = _build_and_run(str(tmp_path), "sweep_anchor_chain.cpp",
                         ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    assert "anchor chain sweep ok" in out and "ERROR" not in out and "runtime error" not in out

"""Sanitizer build of the chunk / layout / fix-unit arithmetic of osc_chain_gated_many
(oscillink_amd/csrc/chain_gated_plan.hpp), swept by tests/host_logic/sweep_chain_gated_plan.cpp under
-fsanitize=address,undefined on the CPU (the pattern of test_bundle_gated_plan_sanitized.py)."""
from tests.test_host_logic_sanitized import _build_and_run


def test_chain_gated_plan_sweep_under_address_and_undefined_sanitizers(tmp_path):
    out = _build_and_run(str(tmp_path), "sweep_chain_gated_plan.cpp",
                         ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    assert "chain gated plan sweep ok" in out and "ERROR" not in out and "runtime error" not in out

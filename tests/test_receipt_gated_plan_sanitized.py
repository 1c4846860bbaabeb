"""Sanitizer build of the chunk / layout arithmetic of osc_receipt_gated_many
(oscillink_amd/csrc/receipt_gated_plan.hpp), swept by tests/host_logic/sweep_receipt_gated_plan.cpp under
-fsanitize=address,undefined on the CPU (the pattern of test_bundle_gated_plan_sanitized.py)."""
from tests.test_host_logic_sanitized import _build_and_run


def test_receipt_gated_plan_sweep_under_address_and_undefined_sanitizers(tmp_path):
    out = _build_and_run(str(tmp_path), "sweep_receipt_gated_plan.cpp",
                         ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    assert "receipt gated plan sweep ok" in out and "ERROR" not in out and "runtime error" not in out

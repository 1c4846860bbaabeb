"""Sanitizer build of the update planner (oscillink_amd/csrc/update_plan.hpp), swept by
tests/host_logic/sweep_update_plan.cpp under -fsanitize=address,undefined on the CPU, as its own process (the pattern of
test_remove_plan_sanitized.py)."""
from tests.test_host_logic_sanitized import _build_and_run


def test_update_plan_sweep_under_address_and_undefined_sanitizers(tmp_path):
    out = _build_and_run(str(tmp_path), "sweep_update_plan.cpp",
                         ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    assert "update plan sweep ok" in out and "ERROR" not in out and "runtime error" not in out

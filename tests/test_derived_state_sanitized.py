"""Sanitizer build of the handle's cache dependency table (oscillink_amd/csrc/derived_state.hpp), swept by
tests/host_logic/sweep_derived_state.cpp under -fsanitize=address,undefined on the CPU (the pattern of
test_host_logic_sanitized.py)."""
from tests.test_host_logic_sanitized import _build_and_run


def test_derived_state_sweep_under_address_and_undefined_sanitizers(tmp_path):
    out = _build_and_run(str(tmp_path), "sweep_derived_state.cpp",
                         ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    assert "derived state sweep ok" in out and "ERROR" not in out and "runtime error" not in out

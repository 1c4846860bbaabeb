"""The streamed first apply's host logic (oscillink_amd/csrc/host_logic.hpp: gates_uniform, anchor_ap_route,
anchor_ap_fits), swept by tests/host_logic/sweep_anchor_ap.cpp on the CPU: once as a plain build, once under
-fsanitize=address,undefined (the pattern of test_x_ring_host.py)."""
import pytest

from tests.test_host_logic_sanitized import _build_and_run


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]],
                         ids=["plain", "address_undefined"])
def test_anchor_ap_sweep(tmp_path, flags):
    out = _build_and_run(str(tmp_path), "sweep_anchor_ap.cpp", flags)
    assert "anchor ap sweep ok" in out and "ERROR" not in out and "runtime error" not in out

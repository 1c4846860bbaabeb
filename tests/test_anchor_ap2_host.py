"""The streamed second apply's host logic (oscillink_amd/csrc/host_logic.hpp: anchor_ap2_route, cg_ap_source, and
cg_host_loop against a model of the launches), swept by tests/host_logic/sweep_anchor_ap2.cpp on the CPU: once as a plain
build, once under -fsanitize=address,undefined (the pattern of test_x_ring_host.py)."""
import pytest

from tests.test_host_logic_sanitized import _build_and_run


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]],
                         ids=["plain", "address_undefined"])
def test_anchor_ap2_sweep(tmp_path, flags):
    out = _build_and_run(str(tmp_path), "sweep_anchor_ap2.cpp", flags)
    assert "anchor ap2 sweep ok" in out and "ERROR" not in out and "FAIL" not in out and "runtime error" not in out

"""The direction ring's host logic (oscillink_amd/csrc/host_logic.hpp: plan_x_ring, CgXRing), swept by
tests/host_logic/sweep_x_ring.cpp against a model of the device's gating on the CPU: once as a plain build, once under
-fsanitize=address,undefined (the pattern of test_host_logic_sanitized.py)."""
import pytest

from tests.test_host_logic_sanitized import _build_and_run


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]],
                         ids=["plain", "address_undefined"])
def test_x_ring_sweep(tmp_path, flags):
    out = _build_and_run(str(tmp_path), "sweep_x_ring.cpp", flags)
    assert "x ring sweep ok" in out and "ERROR" not in out and "runtime error" not in out

"""The append planner (oscillink_amd/csrc/append_plan.hpp) swept by tests/host_logic/sweep_append_plan.cpp in a plain
host build: the eligibility table, chunk bounds, alignment and sizes near 2^31.  No GPU, no native library."""
import re

from tests.test_host_logic_sanitized import _build_and_run


def test_append_plan_sweep_plain_build(tmp_path):
    out = _build_and_run(str(tmp_path), "sweep_append_plan.cpp", ["-O2", "-Wall", "-Wextra", "-Werror"])
    m = re.search(r"append plan sweep ok \((\d+) cases\)", out)
    assert m and int(m.group(1)) > 500 and "ERROR" not in out

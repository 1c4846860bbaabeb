"""The removal planner (oscillink_amd/csrc/remove_plan.hpp) swept by tests/host_logic/sweep_remove_plan.cpp in a plain
host build: the id map against a brute-force one, sizes near 2^31, the eligibility table and the chunk bounds at N' columns.
No GPU, no native library."""
import re

from tests.test_host_logic_sanitized import _build_and_run


def test_remove_plan_sweep_plain_build(tmp_path):
    out = _build_and_run(str(tmp_path), "sweep_remove_plan.cpp", ["-O2", "-Wall", "-Wextra", "-Werror"])
    m = re.search(r"remove plan sweep ok \((\d+) cases\)", out)
    assert m and int(m.group(1)) > 500 and "ERROR" not in out

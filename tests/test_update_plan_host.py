"""The update planner (oscillink_amd/csrc/update_plan.hpp) swept by tests/host_logic/sweep_update_plan.cpp in a plain host
build: the id check against a brute-force one, the eligibility table, the threshold and the replaced rows' part of every
chunk.  No GPU, no native library."""
import re

from tests.test_host_logic_sanitized import _build_and_run


def test_update_plan_sweep_plain_build(tmp_path):
    out = _build_and_run(str(tmp_path), "sweep_update_plan.cpp", ["-O2", "-Wall", "-Wextra", "-Werror"])
    m = re.search(r"update plan sweep ok \((\d+) cases\)", out)
    assert m and int(m.group(1)) > 500 and "ERROR" not in out

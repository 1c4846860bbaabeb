"""Sanitizer build of the chunk / partition / layout arithmetic of osc_gates_many (oscillink_amd/csrc/gates_many_plan.hpp),
swept by tests/host_logic/sweep_gates_many_plan.cpp under -fsanitize=address,undefined on the CPU (the pattern of
test_corpus_gates_plan_sanitized.py)."""
from tests.test_host_logic_sanitized import _build_and_run


def test_gates_many_plan_sweep_under_address_and_undefined_sanitizers(tmp_path):
    out = _build_and_run(str(tmp_path), "sweep_gates_many_plan.cpp",
                         ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"])
    assert "gates many plan sweep ok" in out and "ERROR" not in out and "runtime error" not in out

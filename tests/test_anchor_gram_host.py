"""The fused two-step anchor start's host side (oscillink_amd/csrc/host_logic.hpp: anchor_gram_route; anchor_gram.hpp: the CG
scalars of iterations 1 and 2 from float64 Gram sums), swept by tests/host_logic/sweep_anchor_gram.cpp on the CPU: the route's
truth table, the algebra against two CG iterations on explicit vectors, the fp32 model against CG with directly summed scalars,
and the usable flag.  Once as a plain build, once under -fsanitize=address,undefined (the pattern of test_anchor_ap2_host.py)."""
import pytest

from tests.test_host_logic_sanitized import _build_and_run


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]],
                         ids=["plain", "address_undefined"])
def test_anchor_gram_sweep(tmp_path, flags):
    out = _build_and_run(str(tmp_path), "sweep_anchor_gram.cpp", flags)
    print(out)
    assert "anchor gram sweep ok" in out and "ERROR" not in out and "FAIL" not in out and "runtime error" not in out

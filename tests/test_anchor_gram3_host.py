"""The three-step anchor start's host side (oscillink_amd/csrc/host_logic.hpp: anchor_gram3_route; anchor_gram.hpp: three_steps,
the CG scalars of iteration 3 from float64 sums of nine vectors), swept by tests/host_logic/sweep_anchor_gram3.cpp on the CPU: the
route's truth table, the algebra against three CG iterations on explicit vectors, the fp32 model against CG with summed scalars
(its printed maxima are what the GPU tolerances of tests/test_gpu_anchor_gram3.py are judged by), and the usable3 flag.  Once as a
plain build, once under -fsanitize=address,undefined (the pattern of test_anchor_gram_host.py)."""
import pytest

from tests.test_host_logic_sanitized import _build_and_run


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]],
                         ids=["plain", "address_undefined"])
def test_anchor_gram3_sweep(tmp_path, flags):
    out = _build_and_run(str(tmp_path), "sweep_anchor_gram3.cpp", flags)
    print(out)
    assert "anchor gram3 sweep ok" in out and "ERROR" not in out and "FAIL" not in out and "runtime error" not in out

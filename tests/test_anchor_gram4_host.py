"""The four-step anchor start's host side (oscillink_amd/csrc/host_logic.hpp: anchor_gram4_route, anchor_gram4_last_form;
anchor_gram.hpp: four_steps, alpha4 and |r4| from float64 sums of eleven vectors), swept by tests/host_logic/sweep_anchor_gram4.cpp
on the CPU: the route's truth table and the host's decision, the algebra against four CG iterations on explicit vectors (1e-9, and
the first three iterations equal to three_steps() with ==), the fp32 model against the three-step route and against CG with summed
scalars, the usable4 flag, and cg_host_loop against a model of the solve's launches for every prediction, stop, max_iters <= 12
and ring size.  Once as a plain build, once under -fsanitize=address,undefined (the pattern of test_anchor_gram3_host.py).

The fp32 model's printed maxima (225 columns: seeds 1-3, three sizes, five operators), which the GPU tolerances of
tests/test_gpu_anchor_gram4.py are judged by -- against the three-step route: alpha4 6.4e-7, res4 5.5e-7, x4 9.3e-8; against CG with
every scalar summed: alpha4 8.4e-8, res4 7.3e-7, x4 2.2e-7 (relative).  Every column stops in iteration 4 on both routes under a
tolerance between residuals 3 and 4."""
import pytest

from tests.test_host_logic_sanitized import _build_and_run


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]],
                         ids=["plain", "address_undefined"])
def test_anchor_gram4_sweep(tmp_path, flags):
    out = _build_and_run(str(tmp_path), "sweep_anchor_gram4.cpp", flags)
    print(out)
    assert "anchor gram4 sweep ok" in out and "ERROR" not in out and "FAIL" not in out and "runtime error" not in out

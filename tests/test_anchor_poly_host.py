"""The polynomial last form of an anchor start that ends in iteration 4, host side (oscillink_amd/csrc/anchor_gram.hpp: poly4_coeffs;
cg_kernels.hip: k_settle_poly's order of operations as an fp32 model), swept by tests/host_logic/sweep_poly4.cpp on the CPU over
random small symmetric W with row sums <= 1, an isolated row, a psi = 0 column and operators whose solve stops in iteration 4 as well
as ones whose solve would run on: x4 evaluated in float64 from the coefficients equals a plain float64 CG's x4 within 1e-12, and the
fp32 evaluation in the kernel's order errs against that CG no more than a gathered fp32 CG does, per configuration over the whole
array (both figures are printed).  Once as a plain build, once under -fsanitize=address,undefined (the pattern of
test_gram4_fold_host.py)."""
import pytest

from tests.test_host_logic_sanitized import _build_and_run


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]],
                         ids=["plain", "address_undefined"])
def test_poly4_sweep(tmp_path, flags):
    out = _build_and_run(str(tmp_path), "sweep_poly4.cpp", flags)
    print(out)
    assert "poly4 sweep ok" in out and "ERROR" not in out and "FAIL" not in out and "runtime error" not in out

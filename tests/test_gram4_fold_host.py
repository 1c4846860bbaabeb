"""The folded last form of the four-step anchor start, host side (oscillink_amd/csrc/host_logic.hpp: anchor_gram4_device_words, the
tail of k_anchor_gram_scalars that writes go[2], against anchor_gram4_last_form; cg_kernels.hip: two_steps_elem's fold stage and
k_apply_blocked's FMODE 3 epilogue as an fp32 model), swept by tests/host_logic/sweep_gram4_fold.cpp on the CPU: the device word
equals the host's decision over residuals at, beside and far from tol, NaN, +-0, denormals and the zeroing of an unusable solve;
the folded x4 against the unfolded one and both against float64 on the CG data of sweep_anchor_gram4.cpp.  Once as a plain build,
once under -fsanitize=address,undefined (the pattern of test_anchor_gram4_host.py).

The fp32 model's printed maxima (225 columns: seeds 1-3, three sizes, five operators).  In the suite's norm, |a - b|_2 / |b|_2 over
a column: unfolded against float64 2.9e-8, folded 4.0e-8, folded against unfolded 5.0e-8.  Relative to max |x4| of the column:
5.9e-8, 1.0e-7 and 1.2e-7.  The sweep fails, in either norm, where the folded error exceeds 2 sqrt(unfolded^2 + (2^-24)^2) -- one
more rounding at the size of x -- or the forms differ by more than 2e-6 (measured: 0.31 and 0.71 of that bound at the most)."""
import pytest

from tests.test_host_logic_sanitized import _build_and_run


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]],
                         ids=["plain", "address_undefined"])
def test_gram4_fold_sweep(tmp_path, flags):
    out = _build_and_run(str(tmp_path), "sweep_gram4_fold.cpp", flags)
    print(out)
    assert "gram4 fold sweep ok" in out and "ERROR" not in out and "FAIL" not in out and "runtime error" not in out

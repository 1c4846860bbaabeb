"""The planner of the one-launch LDS solve (oscillink_amd/csrc/small_plan.hpp) swept by
tests/host_logic/sweep_small_plan.cpp in a plain host build and, as the same stand-alone program, under
-fsanitize=address,undefined; and the seams of the plan by value through the library's own entry point, osc_small_plan,
which needs no device.  No GPU."""
import ctypes
import re

import pytest

from tests.test_host_logic_sanitized import _build_and_run

# (N, D) -> (cols, workgroups, lds_bytes or None): the last and first size of every width, the LDS limit met exactly, the
# 256-workgroup launches, and what lies just outside -- the 257- and 512-workgroup shapes among it, which the planner chose
# until the GPU tests showed that they never co-reside (tests/test_gpu_small_solve.py runs all of them)
SEAMS = {
    (2395, 64): (4, 16, 153600),
    (2396, 64): (2, 32, None),
    (4794, 96): (2, 48, 153600),
    (4795, 96): (1, 96, None),
    (6000, 64): (1, 64, None),
    (6001, 64): (0, 0, 0),
    (1259, 1024): (4, 256, 80896),
    (1259, 1028): (0, 0, 0),  # 257 workgroups: k_settle_small<4>'s registers admit one workgroup per CU, not two
    (1259, 2048): (0, 0, 0),  # 512 workgroups
    (1260, 1028): (0, 0, 0),
    (2395, 1024): (4, 256, 153600),
    (4794, 516): (0, 0, 0),
    (5000, 3): (1, 4, None),
}


def _check_sweep(out):
    m = re.search(r"small plan sweep ok \((\d+) cases; cols 0/1/2/4: (\d+)/(\d+)/(\d+)/(\d+); off the two-per-CU rule: (\d+)\)", out)
    assert m and "ERROR" not in out and "runtime error" not in out, out[-2000:]
    cases, c0, c1, c2, c4, two = map(int, m.groups())
    assert cases > 10_000_000 and min(c0, c1, c2, c4) > 0
    assert two == 1259 * 256  # N <= 1259 (64 N + 320 <= 79 KiB), pitches 1028, 1032, ..., 2048


def test_small_plan_sweep_plain_build(tmp_path):
    _check_sweep(_build_and_run(str(tmp_path), "sweep_small_plan.cpp", ["-O2", "-Wall", "-Wextra", "-Werror"]))


def test_small_plan_sweep_under_address_and_undefined_sanitizers(tmp_path):
    _check_sweep(_build_and_run(str(tmp_path), "sweep_small_plan.cpp",
                                ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]))


@pytest.fixture(scope="module")
def amd():
    import oscillink_amd
    from oscillink_amd import _build

    _build.build()
    return oscillink_amd


@pytest.mark.parametrize("shape", sorted(SEAMS), ids=lambda s: f"{s[0]}x{s[1]}")
def test_small_plan_seams_through_the_library(amd, shape):
    cols, wgs, lds = SEAMS[shape]
    plan = amd.small_plan(*shape)
    assert (plan["cols"], plan["workgroups"]) == (cols, wgs)
    if lds is not None:
        assert plan["lds_bytes"] == lds
    if cols:  # the kernel's state, its [8][cols] doubles of reduction scratch and the 64-byte tail
        assert plan["lds_bytes"] == shape[0] * cols * 16 + 64 * cols + 64 <= 150 * 1024


def test_small_plan_entry_point_needs_no_handle_and_validates(amd):
    from oscillink_amd import _native

    lib = _native.lib()
    cols = ctypes.c_int32(-1)
    assert lib.osc_small_plan(700, 40, ctypes.byref(cols), None, None) == _native.OSC_OK and cols.value == 4
    assert lib.osc_small_plan(700, 40, None, None, None) == _native.OSC_OK  # any pointer may be NULL
    for bad in ((0, 8), (8, 0), (-3, 8), (8, -3)):
        assert lib.osc_small_plan(*bad, ctypes.byref(cols), None, None) == _native.OSC_E_INVALID
        with pytest.raises(ValueError):
            amd.small_plan(*bad)
    # a pitch is D rounded up to 4: D = 1021..1024 are one plan, 1025 is past the 256 workgroups
    assert [amd.small_plan(1259, D)["workgroups"] for D in (1021, 1024, 1025)] == [256, 256, 0]
    assert amd.small_plan(10 ** 6, 2 ** 31 - 1) == {"cols": 0, "workgroups": 0, "lds_bytes": 0}

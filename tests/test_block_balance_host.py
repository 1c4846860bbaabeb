"""The balanced source-block order's host reference (oscillink_amd/csrc/block_balance.hpp), swept by
tests/host_logic/sweep_block_balance.cpp on the CPU: once as a plain build, once as a stand-alone program under
-fsanitize=address,undefined (the pattern of test_host_logic_sanitized.py).

The fixture graph (tests/golden/block_balance_knn4096.bin: int32 N, int32 nnz, int32 rowptr[N + 1], uint16 col[nnz]) is
the oracle's mutual-kNN graph of default_rng(0).standard_normal((4096, 64)) float32 anchors at k = 32: 118 324 directed
edges, mean degree 28.9, 20.2 % of the rows at degree 32.  With 8 blocks of 4 slots the API order displaces 17 701 edges
(15.0 %), the host reference's order 9 193 (7.8 %): 0.5193 of the API order's.  The sweep asserts at most that plus 10 %,
0.572."""
import os

import pytest

from tests.test_host_logic_sanitized import ROOT, _build_and_run

FIXTURE = os.path.join(ROOT, "tests", "golden", "block_balance_knn4096.bin")
FIXTURE_FRACTION = "0.572"


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]],
                         ids=["plain", "address_undefined"])
def test_block_balance_sweep(tmp_path, flags):
    out = _build_and_run(str(tmp_path), "sweep_block_balance.cpp", flags, args=[FIXTURE, FIXTURE_FRACTION])
    assert "block balance sweep ok" in out and "fixture:" in out and "ERROR" not in out and "runtime error" not in out

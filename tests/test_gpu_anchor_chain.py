"""The life cycle of the anchor-start chain as a whole (oscillink_amd/csrc/derived_state.hpp: Level -- W.Y, W.W.Y, W^3 Y, the Gram
sums of steps two, three and four, W^4 Y): a lattice settles from its anchors until every level is held; then one change of each
kind that the dependency table says drops `anchor_wy` -- new anchors (update), a rebuilt graph, a rebuilt graph in another row
order -- and

  * every anchor_*_bytes of build_info() reads 0 at once,
  * the anchor starts that follow raise every *_builds by exactly one and hold every level again,
  * their U, iteration counts and residual histories are those of a fresh handle on the same inputs, to the bit: nothing of the
    levels formed before the change is read.

(A change of the column window is reachable only by joining a communicator, under which the Gram levels are never formed.)

Shape: the smallest of tests/test_gpu_anchor_gram.py's SHAPES that reaches the polynomial form -- 20011 x 200 at a pitch of 224, a
row count that is no multiple of the rows per trip -- with every OSC_ANCHOR_* switch set to 1; k = 16."""
import numpy as np
import pytest

from tests import test_gpu_anchor_gram as two
from tests import test_gpu_anchor_gram4 as four
from tests import test_gpu_anchor_poly as poly

pytestmark = pytest.mark.gpu

SPEC = two.SHAPES["ragged"]
K = 16
LEVELS = ("anchor_ap", "anchor_ap2", "anchor_gram", "anchor_gram3", "anchor_gram4", "anchor_poly")
SWITCHES = ("OSC_ANCHOR_SLAB", "OSC_ANCHOR_WY", "OSC_ANCHOR_AP", "OSC_ANCHOR_AP2", "OSC_ANCHOR_GRAM", "OSC_ANCHOR_GRAM3",
            "OSC_ANCHOR_GRAM4", "OSC_ANCHOR_POLY")


@pytest.fixture(scope="module")
def amd():
    import oscillink_amd
    from oscillink_amd import _native

    assert _native.device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return oscillink_amd


def _bytes(lat):
    info = lat.build_info()
    return [info["anchor_wy_bytes"]] + [info[level + "_bytes"] for level in LEVELS]


def _builds(lat):
    info = lat.build_info()
    return [info[level + "_builds"] for level in LEVELS]


def _starts(lat, tol4=None):
    """Anchor starts until every level is held and used: the first gathers and leaves W.Y, the second forms every other level, the
    third ends in iteration 4 behind a longer prediction (the folded form), the fourth behind that one (the polynomial form).
    Returns the four results and the tolerance that ends a solve in iteration 4."""
    outs = [two._anchor_start(lat, tol=1e-6) for _ in range(2)]
    if tol4 is None:
        tol4 = four._tols(lat.residual_history())[4]
    outs += [two._anchor_start(lat, tol=tol4) for _ in range(2)]
    return outs, tol4


def _new_anchors(amd, lat, Y):
    rows = np.array([3, 777, 19999])
    Y2 = Y.copy()
    Y2[rows] = two._inputs(3, Y.shape[1], seed=9)[0]
    lat.update(rows, Y2[rows])
    return dict(Y=Y2)


def _rebuilt_graph(amd, lat, Y):
    lat.rebuild_graph(kneighbors=12)
    return dict(Y=Y, kneighbors=12)


def _row_order(amd, lat, Y):
    lat.rebuild_graph()  # (under OSC_BALANCE=1, set by the test: the build's switches are read again)
    assert lat.build_info()["order_kind"] == "balanced"
    return dict(Y=Y)


CHANGES = {"new_anchors": _new_anchors, "rebuilt_graph": _rebuilt_graph, "row_order": _row_order}


@pytest.mark.parametrize("kind", sorted(CHANGES))
def test_a_change_drops_every_level_and_the_next_starts_form_each_once(amd, kind, monkeypatch):
    poly._clean_env(monkeypatch)
    for name, value in SPEC["env"].items():
        monkeypatch.setenv(name, value)
    for name in SWITCHES:
        monkeypatch.setenv(name, "1")
    N, D = SPEC["N"], SPEC["D"]
    Y, psi, _, _ = two._inputs(N, D)
    lat = amd.Oscillink(Y, kneighbors=K)
    fresh = None
    try:
        lat.set_query(psi)
        outs, _ = _starts(lat)
        assert all(b > 0 for b in _bytes(lat)), _bytes(lat)
        assert _builds(lat) == [1] * len(LEVELS), _builds(lat)
        info = lat.build_info()
        assert info["poly_four_step_solves"] == 1 and outs[3][0] == 4, (info, outs[3][0])
        assert info["order_kind"] == "none", info

        if kind == "row_order":
            monkeypatch.setenv("OSC_BALANCE", "1")
        inputs = CHANGES[kind](amd, lat, Y)
        assert _bytes(lat) == [0] * (1 + len(LEVELS)), (kind, _bytes(lat))
        b0 = _builds(lat)

        fresh = amd.Oscillink(inputs.pop("Y"), **dict(dict(kneighbors=K), **inputs))
        fresh.set_query(psi)
        want, tol4 = _starts(fresh)
        got, _ = _starts(lat, tol4)
        for trip, (x, y) in enumerate(zip(want, got)):
            two._same(x, y, (kind, "start", trip))
        assert [b - a for a, b in zip(b0, _builds(lat))] == [1] * len(LEVELS), (kind, b0, _builds(lat))
        assert _builds(fresh) == [1] * len(LEVELS), _builds(fresh)
        assert _bytes(lat) == _bytes(fresh) and all(b > 0 for b in _bytes(lat)), (kind, _bytes(lat), _bytes(fresh))
        for key in ("poly_four_step_solves", "fused_four_step_solves"):
            assert lat.build_info()[key] - (0 if kind == "new_anchors" else info[key]) == fresh.build_info()[key], (kind, key)
    finally:
        lat.close()
        if fresh is not None:
            fresh.close()

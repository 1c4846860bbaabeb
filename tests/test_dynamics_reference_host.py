"""The float64 yardstick of the dynamics snapshot (tests/_dynamics_reference.py) against the reference's own outputs, and the
conditions the fixtures of tests/test_gpu_dynamics.py have to meet.  CPU only; the reference is not needed on disk:
tests/golden/reference_dynamics.json holds what it computed (tests/golden/make_golden_dynamics.py).

Scalars to 1e-6 relative (the reference works in float32 arrays, the helper in float64), radius and the top-flow edges
identical, in order; NaN against NaN, infinity against infinity."""
import json
import math

import numpy as np
import pytest

from tests import _dynamics_reference as R

GOLDEN = json.load(open(R.GOLDEN_JSON))
SCALARS = ("temperature", "step_deltaH", "viscosity_step", "flow_total", "move2_mean", "move2_max")
TOL = 1e-4            # the tolerance tier's figure (tests/test_gpu_dynamics.py)
LARGE = (140100, (1, 2, 374, 375))  # the large circulant of the GPU tests: N, strides


def same_scalar(got, want, rel):
    if math.isnan(want):
        return math.isnan(got)
    if math.isinf(want):
        return got == want
    return got == pytest.approx(want, rel=rel, abs=0.0)


def test_the_golden_file_covers_every_recipe():
    assert set(GOLDEN) == set(R.GOLDEN_RECIPES)
    for name, recipe in R.GOLDEN_RECIPES.items():
        assert GOLDEN[name]["recipe"] == recipe, name
        assert GOLDEN[name]["N"] <= 600
    assert any(GOLDEN[n]["recipe"].get("chain") for n in GOLDEN)


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_helper_reproduces_the_reference(name):
    entry = GOLDEN[name]
    fx = R.build_fixture(entry["recipe"])
    assert (fx.N, fx.D) == (entry["N"], entry["D"])
    got, want = fx.reference().dyn, entry["expect"]
    for key in SCALARS:
        assert same_scalar(got[key], want[key], 1e-6), (key, got[key], want[key])
    assert got["radius"] == want["radius"]
    assert [f["edge"] for f in got["top_flows"]] == [f["edge"] for f in want["top_flows"]]
    assert np.allclose([f["flow"] for f in got["top_flows"]], [f["flow"] for f in want["top_flows"]], rtol=1e-6, atol=0.0)


def test_non_finite_rows_do_what_the_reference_recorded():
    """The recorded semantics the device is held to: a NaN row gives NaN statistics, radius 0 and no flow on its edges; an
    infinite row gives infinite statistics, a BFS from that row alone and no flow on its edges either."""
    nan, inf, base = (GOLDEN[n]["expect"] for n in ("nan_row_n300", "inf_row_n300", "halved_n300"))
    assert math.isnan(nan["move2_max"]) and math.isnan(nan["temperature"]) and math.isnan(nan["step_deltaH"])
    assert nan["radius"] == 0 and math.isfinite(nan["flow_total"]) and nan["flow_total"] < base["flow_total"]
    assert inf["move2_max"] == math.inf and inf["temperature"] == math.inf and math.isnan(inf["step_deltaH"])
    assert inf["radius"] == 75 and inf["flow_total"] == nan["flow_total"]
    for e in (nan, inf):
        assert all(77 not in f["edge"] for f in e["top_flows"])


# ---------------------------------------------------------------------------------------- conditions of the exact tier
STORMS = [(257, (1, 2, 3, 4)), (5001, (1, 2, 3, 4)), LARGE]


@pytest.mark.parametrize("N,strides", STORMS, ids=lambda v: str(v) if isinstance(v, int) else "s" + "-".join(map(str, v)))
def test_tie_storm_ties_the_cut_across_blocks(N, strides):
    """The largest flow is tied in at least 33 entries (more than a block's 32 candidates), and they lie in at least two
    k_top_select blocks wherever there are two; chunk boundaries fall inside rows from N = 5001 on; the large graph uses all
    256 blocks with a chunk above 4096 and makes k_sum_max stride."""
    fx = R.storm(N, strides)
    g = R.launch_geometry(fx.N, fx.width)
    tied, blocks = R.tie_blocks(fx)
    assert fx.width == 8 and tied >= 33 and len(blocks) >= min(2, g["nb3"])
    if N == 257:
        assert g["nb3"] == 1
    else:
        assert g["chunk"] % fx.width != 0 and len(blocks) == g["nb3"]  # ties in every block
    if N == 5001:
        assert (g["nb3"], g["chunk"]) == (10, 4001)
    if N == LARGE[0]:
        assert g["ne"] > 1048576 and g["nb3"] == 256 and g["chunk"] == 4379 and g["nb1"] == 256 and N > 65536
    # exactness: degree 8 at weight 1/8 gives unit row sums, and the states are small multiples of 1/4
    assert np.all(fx.sqrt_deg() == np.float32(1.0)) and np.float32(1.0) / (np.float32(1.0) + np.float32(1e-12)) == 1.0
    assert np.all(fx.U_prev * 4 == np.round(fx.U_prev * 4)) and np.abs(fx.U_prev).max() <= 6
    ref = fx.reference()
    assert np.all(ref.flow * 2 ** 9 == np.round(ref.flow * 2 ** 9)) and ref.dyn["flow_total"] < 2 ** 24


def test_windowed_storm_puts_the_winners_late_in_a_breadth_first_order():
    """Only rows 2000..3199 carry the pattern: the tied maxima still fill more than a block's candidates in two blocks, and
    the smallest tied ids sit in the second half of a breadth-first order from row 0 (which alternates between both sides)."""
    fx = R.storm(5001, (1, 2, 3, 4), window=[2000, 3200])
    tied, blocks = R.tie_blocks(fx)
    assert tied >= 33 and len(blocks) >= 2
    winners = np.array([f["edge"][0] for f in fx.reference().dyn["top_flows"]])
    depth = R.bfs_dist(fx.rowptr, fx.col, fx.a, [0])
    assert winners.min() >= 1996 and np.all(depth[winners] > 0.7 * depth.max())


def test_sparse_flows_are_fewer_than_the_cap_and_leave_blocks_empty():
    fx = R.sparse(3000, (1, 50), row=1234)
    ref = fx.reference()
    g = R.launch_geometry(fx.N, fx.width)
    slot = np.arange(ref.row.size) - fx.rowptr[ref.row]
    blocks = np.unique((ref.row[ref.order] * fx.width + slot[ref.order]) // g["chunk"])
    assert 0 < len(ref.order) < R.TOP_K and g["nb3"] == 3 and len(blocks) < g["nb3"]
    same = R.sparse(3000, (1, 50), row=None).reference()
    assert same.dyn["top_flows"] == [] and same.dyn["flow_total"] == 0 and same.dyn["radius"] == 0
    assert np.all(same.dist == 0)  # every row is a seed: sqrt(1e-12) > 1e-9


def test_radius_fixtures():
    assert R.build_fixture(R.GOLDEN_RECIPES["radius_ring600"]).reference().dyn["radius"] == 150
    one = R.build_fixture(R.GOLDEN_RECIPES["radius_two_rings_seed_in_first"]).reference()
    assert one.dyn["radius"] == 50 and np.all(one.dist[100:] == -1) and np.all(one.dist[:100] >= 0)
    both = R.build_fixture(R.GOLDEN_RECIPES["radius_two_rings_seeds_in_both"]).reference()
    assert both.dyn["radius"] == 100 and np.all(both.dist >= 0)
    iso = R.build_fixture(R.GOLDEN_RECIPES["radius_isolated_seed"])
    assert np.diff(iso.rowptr)[298] == 0 and iso.reference().dyn["radius"] == 0 and (iso.reference().dist >= 0).sum() == 1


def test_large_graph_bfs_stays_shallow():
    """The radius loop and the BFS re-order synchronise once per level: the strides keep the depth at a few hundred."""
    fx = R.moved_rows(LARGE, [70000])
    ref = fx.reference()
    assert np.all(ref.dist >= 0) and 100 < ref.dyn["radius"] < 400
    assert R.bfs_dist(fx.rowptr, fx.col, fx.a, [0]).max() < 400  # the re-order starts at row 0


# ------------------------------------------------------------------------------------ conditions of the tolerance tier
TOLERANCE_TIER = [f"widths_d{D}" for D in R.WIDTH_SEEDS] + [f"hub_d{D}" for D in R.HUB_SEEDS]


def tolerance_fixtures():
    return [R.build_fixture(R.GOLDEN_RECIPES[name]) for name in TOLERANCE_TIER]


@pytest.mark.parametrize("name", TOLERANCE_TIER)
def test_top_flows_are_further_apart_than_ten_error_bounds(name):
    """The device may be TOL * (e_prev + e_next) off per edge; the top 17 distinct values (mirror pairs counted once) are more
    than ten times that apart, so the device has to report the reference's edges in the reference's order."""
    count, gap = R.distinct_top_gaps(R.build_fixture(R.GOLDEN_RECIPES[name]).reference(), 17)
    assert count == 17 and gap > 10 * TOL, gap


def test_tolerance_fixture_shapes():
    w = R.widths(7, R.WIDTH_SEEDS[7])
    assert w.N == 300 and set(np.diff(w.rowptr)) == {5} and w.width == 5
    h = R.hub(64, R.HUB_SEEDS[64])
    deg = np.diff(h.rowptr)
    assert h.N == 400 and h.width == 300 and deg[0] == 300 and sorted(deg)[-4:-1] == [65, 100, 130]
    assert np.bincount(deg).argmax() == 3 and np.any(deg % 2 == 1) and np.any(deg % 2 == 0)


def test_float32_arithmetic_stays_inside_the_tolerance():
    """The helper evaluated in float32 against the helper in float64, per reported edge in units of e_prev + e_next and per
    scalar: the worst over the tolerance tier is far inside TOL / 4, so no width needs a wider figure."""
    worst_edge = worst_scalar = 0.0
    for fx in tolerance_fixtures():
        r64, r32 = fx.reference(), fx.reference(np.float32)
        top = r64.order[:R.TOP_K]
        worst_edge = max(worst_edge, float(np.max(np.abs(r32.flow[top] - r64.flow[top]) / r64.scale[top])))
        for key in ("temperature", "step_deltaH", "flow_total", "move2_max"):
            worst_scalar = max(worst_scalar, abs(r32.dyn[key] - r64.dyn[key]) / abs(r64.dyn[key]))
    print(f"float32 helper vs float64 helper: worst edge {worst_edge:.3e} of (e_prev + e_next), worst scalar {worst_scalar:.3e}")
    assert 4 * worst_edge < TOL and 4 * worst_scalar < TOL

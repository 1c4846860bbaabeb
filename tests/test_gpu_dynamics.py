"""The dynamics snapshot kernels against the float64 yardstick of tests/_dynamics_reference.py: k_sum_max, k_top_select,
k_bfs_seeds / k_bfs_level (dynamics_kernels.hip), the edge_flow / anchor outputs of k_receipt_rows<NCH> (receipt_kernels.hip)
and quad_form_of_difference, as osc_dynamics (osc_api.hip) strings them together -- at the sizes where that code branches.

Every lattice is created small-k on random anchors; `set_graph_csr` then injects the fixture graph and `_compute_dynamics`
is called in its array form.  tests/test_dynamics_reference_host.py ties the yardstick to the reference and checks the
conditions the fixtures have to meet (ties per block, gaps between the top flows, BFS depth).

Exact tier: circulant graphs of degree 2 / 4 / 8 at weight 1 / degree (unit row sums: sqrt_deg == 1.0f and
1 / (1 + 1e-12f) == 1.0f), lamC = 0.5, states that are small multiples of 1/4: every product and sum is exact in float32,
so edges, order, flow values, flow_total, move2_max and radius equal the yardstick's with `==`; move2_mean / temperature
to 1e-6 relative (the product rounds them through float32).  step_deltaH is outside this tier (the operator apply's
normalised weights 1/8 are exact, its summation order is its own): 1e-4 relative.

Tolerance tier: random float states; per reported edge |f_dev - f_ref| <= 1e-4 (e_prev + e_next), scalars to 1e-4 relative
(the project's figure in test_gpu_round2_goldens.py: _check_dynamics), edges identical, in order.  The yardstick evaluated
in float32 instead of float64 is 1.0e-7 (e_prev + e_next) per edge and 1.1e-7 per scalar away at the worst fixture: no
width needs a wider figure.

  fixture            N       width  D     nb1  nb2  nb3  chunk  k_receipt_rows  stored order
  storm_257          257     8      4     2    9    1    2056   <1>             none
  storm_5001         5001    8      4     20   157  10   4001   <1>             none / bfs / balanced (late winners)
  storm_large        140100  8      4     256  256  256  4379   <1>             bfs (auto: clustered)
  sparse_3000        3000    4      4     12   47   3    4000   <1>             none
  radius_*           300/600 2-4    4     2-3  3-10 1    ne     <1>             none
  widths_d7..d1537   300     5      7..   2    6    1    1500   <1> <1> <2> <3> <4> <6> <0> (ld 8, 256, 260, 516, 772, 1028,
                                                                 1540: nch = ceil(ld / 256) = 1, 1, 2, 3, 4, 5, 7)   none
  hub_d64 / d257     400     300    64/257 2   256  30   4000   <1> / <2>       none

The balanced order is reached at N = 5001 the way test_gpu_block_balance.py reaches it: OSC_BALANCE=1 together with the
switches that give a small lattice the blocked plan (8 source blocks, row pitch 128); OSC_BALANCE=1 alone leaves a lattice
of that size in API order, and so does OSC_REORDER=0 with it.
"""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

from tests import _dynamics_reference as R
from tests._cases import GOLDEN as GOLDEN_DIR, load_case, make_inputs, random_gates

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(R.GOLDEN_JSON))
R2 = json.load(open(os.path.join(GOLDEN_DIR, "reference_r2.json")))
TOL = 1e-4
LARGE = (140100, (1, 2, 374, 375))
SWITCHES = ("OSC_SPMM_XS", "OSC_REORDER", "OSC_SPMM_BLOCKED", "OSC_BLK_VARIANT", "OSC_BLK_INIT", "OSC_SMALL_PATH", "OSC_BALANCE",
            "OSC_BALANCE_HOST", "OSC_FAKE_COL_SHARD", "OSC_SHARD", "OSC_ROW_FAKE_SHARDS", "OSC_LD")
# the switches that give a small lattice the blocked plan, whose source blocks OSC_BALANCE=1 balances (test_gpu_block_balance.py)
BLOCKED_PLAN = {"OSC_SMALL_PATH": "0", "OSC_SPMM_XS": "1", "OSC_SPMM_BLOCKED": "8", "OSC_LD": "128"}


@pytest.fixture(scope="module")
def amd():
    import oscillink_amd
    from oscillink_amd import _native

    assert _native.device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return oscillink_amd


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)


def _lattice(amd, fx):
    """A lattice that holds the fixture's graph, gates, chain and lambdas (the anchors are random: nothing here reads them)."""
    Y = np.random.default_rng(5).standard_normal((fx.N, fx.D)).astype(np.float32)
    lat = amd.Oscillink(Y, kneighbors=4, lamG=fx.lamG, lamC=fx.lamC, lamQ=fx.lamQ)
    lat.set_graph_csr(fx.rowptr, fx.col, fx.a)
    lat.set_query(np.zeros(fx.D, dtype=np.float32), gates=fx.B)
    if fx.chain is not None:
        lat.add_chain(fx.chain, lamP=fx.lamP)
    lat._push_params()
    rowptr, col, a, _, sd = lat.graph_csr()
    assert np.array_equal(rowptr, fx.rowptr) and np.array_equal(col, fx.col) and np.array_equal(a, fx.a)
    assert np.allclose(sd, fx.sqrt_deg(), rtol=1e-6, atol=0.0)
    return lat


def _run(lat, fx):
    return lat._compute_dynamics(fx.U_prev, fx.U_next, fx.iters)


def _same(got, want, rel):
    if math.isnan(want):
        return math.isnan(got)
    if math.isinf(want) or rel == 0.0:
        return got == want
    return got == pytest.approx(want, rel=rel, abs=0.0)


def _assert_exact(dyn, want, top=None):
    """`want`: a snapshot of the yardstick or of the reference itself (the golden file); NaN matches NaN."""
    top = want["top_flows"] if top is None else top
    print({k: v for k, v in dyn.items() if k != "top_flows"}, len(dyn["top_flows"]))
    assert [f["edge"] for f in dyn["top_flows"]] == [f["edge"] for f in top]
    assert [f["flow"] for f in dyn["top_flows"]] == [f["flow"] for f in top]
    for key in ("flow_total", "move2_max"):
        assert _same(dyn[key], want[key], 0.0), (key, dyn[key], want[key])
    assert dyn["radius"] == want["radius"]
    for key in ("move2_mean", "temperature"):
        assert _same(dyn[key], want[key], 1e-6), (key, dyn[key], want[key])
    for key in ("step_deltaH", "viscosity_step"):
        assert _same(dyn[key], want[key], TOL), (key, dyn[key], want[key])


def _assert_close(dyn, ref):
    """Tolerance tier: the reference's edges in the reference's order, every flow inside TOL (e_prev + e_next)."""
    want = ref.dyn
    print({k: v for k, v in dyn.items() if k != "top_flows"}, len(dyn["top_flows"]))
    assert [f["edge"] for f in dyn["top_flows"]] == [f["edge"] for f in want["top_flows"]]
    got = np.array([f["flow"] for f in dyn["top_flows"]])
    top = ref.order[:R.TOP_K]
    err = np.abs(got - ref.flow[top]) / ref.scale[top]
    print(f"worst edge error {err.max():.3e} of (e_prev + e_next)")
    assert np.all(err <= TOL)
    for key in ("temperature", "step_deltaH", "viscosity_step", "flow_total", "move2_mean", "move2_max"):
        assert dyn[key] == pytest.approx(want[key], rel=TOL, abs=0.0), key
    assert dyn["radius"] == want["radius"]


# ------------------------------------------------------------------------------------------------------------ exact tier
@pytest.fixture(scope="module")
def large(amd):
    """The large circulant under the default switches: N > 131072 rows of degree 8, so ne > 2^20 (k_top_select on all 256
    blocks with a chunk of 4379, k_sum_max striding); clustered, so the automatic re-order stores it breadth-first."""
    with pytest.MonkeyPatch.context() as mp:
        for v in SWITCHES:
            mp.delenv(v, raising=False)
        lat = _lattice(amd, R.storm(*LARGE))
    return lat


@pytest.mark.parametrize("N", [257, 5001])
def test_tie_storm(amd, N):
    """Every flow value is tied hundreds of times over, in every block: the top 16 are decided by the caller's ids.  257: one
    block; 5001: ten blocks whose boundaries (chunk 4001) fall inside rows, the cross-block merge on the host."""
    fx = R.storm(N, (1, 2, 3, 4))
    lat = _lattice(amd, fx)
    assert lat.build_info()["order_kind"] == "none"
    _assert_exact(_run(lat, fx), fx.reference().dyn)


def test_tie_storm_on_all_256_blocks(large):
    fx = R.storm(*LARGE)
    assert large.build_info()["order_kind"] == "bfs"
    _assert_exact(_run(large, fx), fx.reference().dyn)


ORDER_CONFIGS = {  # name -> (environment, the stored order it gives)
    "reorder0": ({"OSC_REORDER": "0"}, "none"),
    "reorder0_balance1": ({"OSC_REORDER": "0", "OSC_BALANCE": "1"}, "none"),
    "reorder1": ({"OSC_REORDER": "1"}, "bfs"),
    "reorder1_balance1": ({"OSC_REORDER": "1", "OSC_BALANCE": "1"}, "bfs"),
    "auto": ({}, "none"),
    "auto_balance1": ({"OSC_BALANCE": "1"}, None),  # (balanced only where the apply plan has source blocks)
    "auto_balance1_blocked_plan": ({"OSC_BALANCE": "1", **BLOCKED_PLAN}, "balanced"),
}
LATE = {"storm": R.storm(5001, (1, 2, 3, 4)).recipe, "storm_window": R.storm(5001, (1, 2, 3, 4), window=[2000, 3200]).recipe}


@pytest.fixture(scope="module")
def late_winner_runs(amd):
    """Every stored order once: config -> (order_kind, {fixture: snapshot}).  The switches are read when the lattice is
    created and when a graph is injected."""
    out = {}
    for name, (env, _) in ORDER_CONFIGS.items():
        with pytest.MonkeyPatch.context() as mp:
            for v in SWITCHES:
                mp.delenv(v, raising=False)
            for k, v in env.items():
                mp.setenv(k, v)
            fx = R.build_fixture(LATE["storm"])
            lat = _lattice(amd, fx)
            out[name] = (lat.build_info()["order_kind"], {key: _run(lat, R.build_fixture(rc)) for key, rc in LATE.items()})
            lat.close()
    return out


@pytest.mark.parametrize("which", sorted(LATE))
@pytest.mark.parametrize("config", sorted(ORDER_CONFIGS))
def test_late_winners_under_every_stored_order(late_winner_runs, config, which):
    """The same storm whatever order the rows are stored in: ties go to the caller's smallest (row, column), not to the
    smallest stored position.  `storm_window`: only rows 2000..3199 carry the pattern -- a breadth-first order from row 0
    stores the winners (rows 2000, 2001, ...) in its eighth block of ten, interleaved with rows 3001, 3000, ..."""
    kind, runs = late_winner_runs[config]
    want_kind = ORDER_CONFIGS[config][1]
    print(config, "order_kind", kind)
    assert kind == want_kind or (want_kind is None and kind in ("none", "balanced"))
    _assert_exact(runs[which], R.build_fixture(LATE[which]).reference().dyn)


def test_late_winners_saw_every_stored_order(late_winner_runs):
    assert {kind for kind, _ in late_winner_runs.values()} == {"none", "bfs", "balanced"}


def test_sparse_flows_and_no_flows(amd):
    """One row differs: four positive flows, fewer than the cap, in one of three blocks (the others leave through the
    `pi < 0` exit at once).  No row differs: no flow at all, and radius 0 with every row a seed (sqrt(1e-12) > 1e-9)."""
    fx = R.sparse(3000, (1, 50), row=1234)
    lat = _lattice(amd, fx)
    dyn = _run(lat, fx)
    assert 0 < len(dyn["top_flows"]) < R.TOP_K
    _assert_exact(dyn, fx.reference().dyn)
    same = R.sparse(3000, (1, 50), row=None)
    dyn = _run(lat, same)
    assert dyn["top_flows"] == [] and dyn["flow_total"] == 0 and dyn["radius"] == 0 and dyn["move2_max"] == 0
    _assert_exact(dyn, same.reference().dyn)


@pytest.mark.parametrize("name,radius", [("radius_ring600", 150), ("radius_two_rings_seed_in_first", 50),
                                         ("radius_two_rings_seeds_in_both", 100), ("radius_isolated_seed", 0)])
@pytest.mark.parametrize("reorder", ["0", "1"])
def test_radius(amd, name, radius, reorder, monkeypatch):
    """One seed row on a deep ring (150 levels), on one of two disjoint rings (the other stays unreached), on a row without
    edges, seeds in both rings; in API order and in the breadth-first order."""
    monkeypatch.setenv("OSC_REORDER", reorder)
    fx = R.build_fixture(GOLDEN[name]["recipe"])
    lat = _lattice(amd, fx)
    dyn = _run(lat, fx)
    assert dyn["radius"] == radius == GOLDEN[name]["expect"]["radius"]
    _assert_exact(dyn, GOLDEN[name]["expect"])
    _assert_exact(dyn, fx.reference().dyn)


def test_radius_on_the_large_graph(large):
    fx = R.moved_rows(LARGE, [70000])
    dyn = _run(large, fx)
    assert dyn["radius"] > 100
    _assert_exact(dyn, fx.reference().dyn)


def _raw(lat, fx, cap, sentinel=-7):
    """osc_dynamics with a caller's top_cap: (top_n, top_i, top_j, top_flow)."""
    from oscillink_amd import _native as nat

    ti, tj = np.full(40, sentinel, dtype=np.int32), np.full(40, sentinel, dtype=np.int32)
    tf = np.full(40, float(sentinel), dtype=np.float64)
    tn = C.c_int32(sentinel)
    lat._call("osc_dynamics", nat.f32(fx.U_prev), nat.f32(fx.U_next), None, None, None, None, cap, nat.i32(ti), nat.i32(tj),
              tf.ctypes.data_as(nat.c_f64p), C.byref(tn), None)
    return int(tn.value), ti, tj, tf


def test_top_cap(amd):
    fx = R.storm(5001, (1, 2, 3, 4))
    lat = _lattice(amd, fx)
    ref = fx.reference()
    n, ti, tj, tf = _raw(lat, fx, 0)
    assert n == 0 and np.all(ti == -7) and np.all(tj == -7) and np.all(tf == -7.0)  # nothing written
    for cap in (1, 32):
        n, ti, tj, tf = _raw(lat, fx, cap)
        want = ref.top(cap)
        assert n == cap == len(want)
        assert [[int(i), int(j)] for i, j in zip(ti[:n], tj[:n])] == [f["edge"] for f in want]
        assert [float(x) for x in tf[:n]] == [f["flow"] for f in want]
        assert np.all(ti[n:] == -7) and np.all(tf[n:] == -7.0)
    for cap in (33, -1):
        with pytest.raises(ValueError):
            _raw(lat, fx, cap)


@pytest.mark.parametrize("name", ["nan_row_n300", "inf_row_n300"])
def test_non_finite_row_matches_what_the_reference_recorded(amd, name):
    """One NaN / +Inf row in U_next: NaN (infinite) movement statistics, NaN step energy, no flow on that row's edges, radius 0
    (NaN seeds nothing) / 75 (the infinite row is the one seed)."""
    fx = R.build_fixture(GOLDEN[name]["recipe"])
    dyn = _run(_lattice(amd, fx), fx)
    _assert_exact(dyn, GOLDEN[name]["expect"])
    _assert_exact(dyn, fx.reference().dyn)


def test_nan_row_behind_the_stride_loop(large):
    """A NaN row at index 100000 >= 65536: k_sum_max meets it in its second stride, and the host's merge of the 256 partial
    maxima has to keep it.  (N = 140100 is beyond what the reference can be run on: the yardstick stands in, its NaN rules
    are the recorded ones of the N = 300 case.)"""
    fx = R.halved(LARGE[0], LARGE[1], row=100000, value="nan")
    dyn = _run(large, fx)
    assert math.isnan(dyn["move2_max"]) and math.isnan(dyn["temperature"]) and dyn["radius"] == 0
    _assert_exact(dyn, fx.reference().dyn)


# -------------------------------------------------------------------------------------------------------- tolerance tier
@pytest.mark.parametrize("D", sorted(R.WIDTH_SEEDS))
def test_every_receipt_rows_instantiation(amd, D):
    """N = 300 at degree 5 (odd: the EU = 2 tail loop), random weights.  launch_receipt_rows takes nch = ceil(ld / 256) with
    ld = D rounded up to 4: D = 7 -> ld 8, <1>; 256 -> <1>; 257 -> ld 260, <2>; 513 -> <3>; 769 -> <4>; 1025 -> nch 5, <6>;
    1537 -> nch 7, the generic <0>."""
    fx = R.build_fixture(GOLDEN[f"widths_d{D}"]["recipe"])
    _assert_close(_run(_lattice(amd, fx), fx), fx.reference())


def test_chain_term(amd):
    fx = R.build_fixture(GOLDEN["widths_d7_chain"]["recipe"])
    _assert_close(_run(_lattice(amd, fx), fx), fx.reference())
    assert fx.reference().dyn["step_deltaH"] > 1.05 * R.build_fixture(GOLDEN["widths_d7"]["recipe"]).reference().dyn["step_deltaH"]


@pytest.mark.parametrize("D", sorted(R.HUB_SEEDS))
def test_hub_rows(amd, D):
    """ELL width 300: one row of degree 300, rows of degree 65, 100 and 130, the rest of degree 2 - 6; <1> at D = 64, <2> at
    D = 257 (ld 260)."""
    fx = R.build_fixture(GOLDEN[f"hub_d{D}"]["recipe"])
    _assert_close(_run(_lattice(amd, fx), fx), fx.reference())


# ------------------------------------------------------------------------------------------------- anchor to the reference
def _check_against_r2(dyn, want):
    """test_gpu_round2_goldens.py: _check_dynamics."""
    for key in ("temperature", "step_deltaH", "viscosity_step", "flow_total", "move2_mean", "move2_max"):
        assert dyn[key] == pytest.approx(want[key], rel=1e-4), key
    assert dyn["radius"] == want["radius"]
    assert [f["edge"] for f in dyn["top_flows"]] == [f["edge"] for f in want["top_flows"]]
    assert np.allclose([f["flow"] for f in dyn["top_flows"]], [f["flow"] for f in want["top_flows"]], rtol=1e-4)


@pytest.mark.parametrize("name", sorted(R2["dynamics"]))
def test_yardstick_reproduces_the_reference_on_real_knn_graphs(amd, name, monkeypatch):
    """The five snapshots the reference recorded after real settles: the yardstick, run on the device's own graph_csr() and
    on the (U_prev, U_next) the product used, gives the reference's numbers."""
    monkeypatch.setenv("OSCILLINK_RECEIPT_DYNAMICS", "1")
    want = R2["dynamics"][name]
    rc = load_case(name.split("__")[0])["recipe"]
    Y, psi = make_inputs(rc)
    lat = amd.Oscillink(Y, kneighbors=rc["k"], deterministic_k=rc["deterministic"])
    lat.set_query(psi, gates=random_gates(rc) if rc["gates"] == "random" else None)
    if rc["chain"]:
        lat.add_chain(rc["chain"], lamP=rc["lamP"])
    if "perturb" in want:
        Us = lat.solve_Ustar().copy()
        Us[want["perturb"]["row"]] += np.float32(want["perturb"]["delta"])
        lat.U = Us
        kw = dict(max_iters=want["perturb"]["max_iters"], tol=1e-3)
    else:
        kw = dict(max_iters=rc["settle_max_iters"], tol=rc["settle_tol"])
    U_prev = lat.U.copy()
    st = lat.settle(**kw)
    U_next = lat.U.copy()
    assert st["iters"] == want["iters"]
    rowptr, col, a, _, sd = lat.graph_csr()
    ref = R.dynamics_reference(rowptr, col, a, sd, U_prev, U_next, lat.lamG, lat.lamC, lat.lamQ, lat.B_diag, st["iters"],
                               chain=rc["chain"] or None, lamP=rc["lamP"] if rc["chain"] else 0.0)
    _check_against_r2(ref.dyn, want)
    _check_against_r2(lat._last_dynamics, ref.dyn)

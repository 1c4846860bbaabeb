"""`keep_state=True` of OscillinkLattice.append / remove / update: the state U is carried onto the new
handle on the device, U_new[a] = U_old[src[a]] where src[a] >= 0, else Y_new[a].

The yardstick for every case is a twin made by the same call and mode WITHOUT keep_state, which then receives
`twin.U = expected`, `expected` built on the host from the rule and the old `lat.U`.  `lat.U` must equal `expected` byte
for byte (compared as uint32, so the NaN and Inf entries of an assigned state count), and a settle() of both must give the
same iteration count, residual history and state, bit for bit: the twin holds the same graph in the same internal row
order, so anything else means rows, padding columns or the aliasing flag went wrong in the carry.  A source that was never
settled aliases its anchors; the carried state is then the new anchors and the twin is left as the plain call made it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STATES = ("never_settled", "settled", "assigned")


def _lat(Y, k, psi=None):
    from oscillink_amd import OscillinkLattice

    lat = OscillinkLattice(Y, kneighbors=k, deterministic_k=True)
    if psi is not None:
        lat.set_query(psi)
    return lat


def _inputs(N, D, seed=None):
    rng = np.random.default_rng(N + D if seed is None else seed)
    Y = rng.standard_normal((N, D)).astype(np.float32)
    psi = rng.standard_normal(D).astype(np.float32)
    return rng, Y, psi / np.linalg.norm(psi)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _put_state(lat, state, nonfinite=False):
    if state == "settled":
        for _ in range(3):
            lat.settle()
    elif state == "assigned":
        U = np.random.default_rng(lat.N).standard_normal((lat.N, lat.D)).astype(np.float32)
        if nonfinite:  # in the first, a middle and the last row, and in the last column
            U[0, 0], U[lat.N // 2, lat.D - 1], U[lat.N - 1, 1] = np.nan, np.inf, -np.inf
            U[1, lat.D - 1] = -0.0
        lat.U = U
    else:
        assert state == "never_settled"


def _call(lat, op, args, mode, **kw):
    if op == "append":
        return lat.append(args["rows"], mode=mode, **kw)
    if op == "remove":
        return lat.remove(args["ids"], mode=mode, **kw)
    return lat.update(args["ids"], args["rows"], mode=mode, **kw)


def _expected(U_old, op, args):
    """The rule, written out per operation (not through the package's map helpers)."""
    if op == "append":
        return np.concatenate([U_old, args["rows"]])
    if op == "remove":
        return np.delete(U_old, np.asarray(args["ids"], dtype=np.int64), axis=0)
    out = U_old.copy()
    out[np.asarray(args["ids"], dtype=np.int64)] = args["rows"]
    return out


def _carry_and_check(Y, k, psi, op, args, state, mode="incremental", nonfinite=False, after=None):
    """Runs `op` with keep_state=True on a lattice over Y brought into `state`, and holds it to the twin.  `after(lat)`:
    something done to both lattices between the carry and the settle.  Returns (lat, twin)."""
    lat, twin = _lat(Y, k, psi), _lat(Y, k, psi)
    _put_state(lat, state, nonfinite)
    U_old = lat.U.copy()
    _call(lat, op, args, mode, keep_state=True)
    _call(twin, op, args, mode)
    assert lat.last == {"iters": 0, "res": None, "t_ms": None}
    expected = _expected(U_old, op, args)
    if state == "never_settled":
        assert np.array_equal(_bits(expected), _bits(twin.Y))  # the rule gives the new anchors ...
        assert lat.build_info()["y_to_u_copies"] == 0  # ... and the new handle was left aliased: nothing was copied
    else:
        twin.U = expected
    assert lat.U.shape == expected.shape
    assert np.array_equal(_bits(lat.U), _bits(expected))
    assert np.array_equal(_bits(lat.Y), _bits(twin.Y))
    if after is not None:
        for x in (lat, twin):
            after(x)
        assert np.array_equal(_bits(lat.U), _bits(expected))
    sa, st = lat.settle(), twin.settle()
    assert sa["iters"] == st["iters"]
    assert np.array_equal(np.asarray(lat.residual_history(), dtype=np.float64).view(np.uint64),
                          np.asarray(twin.residual_history(), dtype=np.float64).view(np.uint64))
    assert np.array_equal(_bits(lat.U), _bits(twin.U))
    if not nonfinite:
        assert np.isfinite(lat.U).all()
    return lat, twin


def _args(rng, op, N, D, M):
    """M rows to add / ids to drop / rows to replace; the ids in no order and with the first and the last row among them."""
    if op == "append":
        return {"rows": rng.standard_normal((M, D)).astype(np.float32)}
    ids = np.concatenate([[N - 1, 0], rng.choice(np.arange(1, N - 1), size=M - 2, replace=False)]) if M >= 2 else np.array([N // 2])
    if op == "remove":
        return {"ids": ids}
    return {"ids": ids, "rows": rng.standard_normal((ids.size, D)).astype(np.float32)}


# ---- the one-launch path: D a multiple of the pitch's line or far from it ------------------------------------------------------
@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("op", ["append", "remove", "update"])
@pytest.mark.parametrize("N,D,k", [(40, 12, 5), (1200, 128, 16)])
def test_small_lattices_every_op_and_state(N, D, k, op, state):
    rng, Y, psi = _inputs(N, D)
    _carry_and_check(Y, k, psi, op, _args(rng, op, N, D, 5), state, nonfinite=True)


@pytest.mark.parametrize("state", ["settled", "assigned"])
@pytest.mark.parametrize("op", ["append", "remove", "update"])
def test_mode_rebuild(op, state):
    N, D, k = 300, 20, 6
    rng, Y, psi = _inputs(N, D)
    lat, _ = _carry_and_check(Y, k, psi, op, _args(rng, op, N, D, 4), state, mode="rebuild")
    assert getattr(lat, op + "_info")()["route"] == 2


def test_one_row_each():
    N, D, k = 300, 20, 6
    for op in ("append", "remove", "update"):
        rng, Y, psi = _inputs(N, D)
        _carry_and_check(Y, k, psi, op, _args(rng, op, N, D, 1), "settled")


# ---- padding columns: D = 3 in a pitch of 4, D = 200 in a pitch of 224 ------------------------------------------------------
@pytest.mark.parametrize("op", ["append", "remove", "update"])
@pytest.mark.parametrize("D,ld", [(3, None), (200, 224)])
def test_rows_with_padding_columns(D, ld, op, monkeypatch):
    """A settle's residuals add up all the columns the kernels work on, D rounded up to 4: a padding column that did not
    arrive as it was shows in the residual history.  The last row of the array ends at the array's end."""
    if ld is not None:
        monkeypatch.setenv("OSC_LD", str(ld))  # (read at every creation: both handles of a call get the pitch)
    N, k = 330, 4
    rng, Y, psi = _inputs(N, D)
    for state in ("settled", "assigned"):
        _carry_and_check(Y, k, psi, op, _args(rng, op, N, D, 7), state, mode="auto")


# ---- both handles permuted, by different permutations ------------------------------------------------------------------------
def _clustered():
    rng = np.random.default_rng(3)
    centers = rng.standard_normal((40, 48)).astype(np.float32)
    Y = (centers[rng.integers(0, 40, 9000)] + 0.05 * rng.standard_normal((9000, 48))).astype(np.float32)
    psi = rng.standard_normal(48).astype(np.float32)
    return rng, Y, psi / np.linalg.norm(psi)


@pytest.mark.parametrize("case", ["remove_scattered", "update_ends_and_middle", "append_1", "append_257"])
def test_bfs_ordered_handles(case, monkeypatch):
    monkeypatch.setenv("OSC_REORDER", "1")
    rng, Y, psi = _clustered()
    N, D = Y.shape
    if case == "remove_scattered":
        op, args = "remove", {"ids": np.concatenate([[N - 1, 0], rng.choice(np.arange(1, N - 1), size=61, replace=False)])}
    elif case == "update_ends_and_middle":
        op, args = "update", {"ids": np.array([N // 2, 0, N - 1]), "rows": Y[[17, 4000, 8000]] + np.float32(0.01)}
    else:
        M = int(case.split("_")[1])
        op, args = "append", {"rows": (Y[rng.integers(0, N, M)] + 0.02 * rng.standard_normal((M, D))).astype(np.float32)}
    before = _lat(Y, 3)
    order_before = _row_order(before)
    lat, twin = _carry_and_check(Y, 3, psi, op, args, "settled", mode="auto")
    assert lat.build_info()["reordered"] == 1 and twin.build_info()["reordered"] == 1
    order_after = _row_order(lat)
    assert not np.array_equal(order_before, np.arange(N)) and not np.array_equal(order_after, np.arange(lat.N))
    if op != "update":
        assert order_after.size != order_before.size
    print(case, "rows whose stored position changed:", int((order_after[:min(N, lat.N)] != order_before[:min(N, lat.N)]).sum()))


def _row_order(lat):
    from oscillink_amd import _native as nat

    out = np.zeros(lat.N, dtype=np.int32)
    lat._call("osc_get_row_order", nat.i32(out))
    return out


# ---- the source-blocked apply and its balanced order -------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["append", "remove", "update"])
def test_blocked_apply_and_a_later_reorder(op, monkeypatch):
    """20 000 x 64, k 8 under the source-blocked apply and its balanced row order.  The planner keeps 64-column lattices of
    this size on the plain apply, so the switches tests/test_gpu_block_balance.py uses select the plan (they are read at
    every creation: both handles of a call run it).  After the carry the graph is rebuilt with another k, which computes a
    new balanced order and moves the state into it: a carried U must move as an assigned one does."""
    for name, val in (("OSC_SMALL_PATH", "0"), ("OSC_SPMM_XS", "1"), ("OSC_SPMM_BLOCKED", "8"), ("OSC_BALANCE", "1")):
        monkeypatch.setenv(name, val)
    N, D, k = 20000, 64, 8
    rng, Y, psi = _inputs(N, D)
    orders = []

    def rebuild(x):
        orders.append(_row_order(x))
        x.rebuild_graph(kneighbors=6)
        orders.append(_row_order(x))

    lat, twin = _carry_and_check(Y, k, psi, op, _args(rng, op, N, D, 33), "settled", mode="auto", after=rebuild)
    info = lat.build_info()
    print(op, "order:", info["order_kind"], "source blocks:", info["apply_src_blocks"], "blocked applies:", info["blocked_applies"])
    assert info["order_kind"] == twin.build_info()["order_kind"] == "balanced"
    assert info["apply_src_blocks"] == 8 and info["blocked_applies"] > 0
    before, after = orders[0], orders[1]  # lat's: the order the state was carried into, and the rebuild's
    assert not np.array_equal(before, np.arange(lat.N)) and not np.array_equal(before, after)


# ---- atomicity, settings, log ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["append", "remove", "update"])
def test_a_failing_call_leaves_the_state_as_it_was(op):
    N, D, k = 120, 16, 5
    rng, Y, psi = _inputs(N, D)
    lat = _lat(Y, k, psi)
    rowptr, col, a, _, _ = lat.graph_csr()
    lat.set_graph_csr(rowptr, col, a)  # an injected graph has no kNN lists to grow, shrink or edit
    for _ in range(3):
        lat.settle()
    U0, last = lat.U.copy(), dict(lat.last)
    with pytest.raises(NotImplementedError, match="no kNN lists"):
        _call(lat, op, _args(rng, op, N, D, 3), "incremental", keep_state=True)
    lat._U_host = None  # (read the device's copy again, not the mirror)
    assert lat.N == N and lat.last == last
    assert np.array_equal(_bits(lat.U), _bits(U0))


def test_a_refused_map_destroys_nothing_of_the_lattice(monkeypatch):
    """The carry itself failing (a map of the wrong length, which no public call builds): the new handle is destroyed, the
    object and its U stay."""
    from oscillink_amd import lattice as lt

    N, D, k = 120, 16, 5
    rng, Y, psi = _inputs(N, D)
    lat = _lat(Y, k, psi)
    for _ in range(3):
        lat.settle()
    U0, sig = lat.U.copy(), lat._signature()
    monkeypatch.setattr(lt, "_state_map_update", lambda n, ids: np.arange(n + 1, dtype=np.int32))
    with pytest.raises(ValueError, match="state map"):
        lat.update([3], Y[:1] * 2, keep_state=True)
    lat._U_host = None
    assert lat.N == N and lat._signature() == sig and lat.update_info()["route"] == 0
    assert np.array_equal(_bits(lat.U), _bits(U0))


@pytest.mark.parametrize("op", ["append", "remove", "update"])
def test_settings_survive_and_the_event_says_so(op):
    N, D, k = 400, 32, 8
    rng, Y, psi = _inputs(N, D)
    args = _args(rng, op, N, D, 6)
    if op != "append":
        args["ids"] = np.setdiff1d(args["ids"], [5, 150, 300])  # (a removal may not name a chain node)
        if op == "update":
            args["rows"] = args["rows"][:args["ids"].size]
    gates = rng.uniform(0.2, 1.0, N).astype(np.float32)
    events = {"lat": [], "twin": []}
    lats = {}
    for name in ("lat", "twin"):
        x = _lat(Y, k)
        x.lamC, x.lamQ = 0.7, 3.0
        x.set_query(psi, gates)
        x.add_chain([5, 150, 300], lamP=0.3, weights=[1.0, 0.5])
        x.set_logger(lambda ev, payload, name=name: events[name].append((ev, dict(payload))))
        lats[name] = x
    lat, twin = lats["lat"], lats["twin"]
    for _ in range(3):
        lat.settle()
    U_old = lat.U.copy()
    _call(lat, op, args, "incremental", keep_state=True)
    _call(twin, op, args, "incremental")
    (e_lat,), (e_twin,) = ([p for ev, p in events[n] if ev == op] for n in ("lat", "twin"))
    assert e_lat == {**e_twin, "keep_state": True} and "keep_state" not in e_twin
    assert set(e_twin) == {"rows", "N", "route", "redo_rows"}
    assert lat.lamP == twin.lamP == 0.3 and (lat.lamC, lat.lamQ) == (0.7, 3.0)
    assert lat._chain_nodes == twin._chain_nodes and len(lat._chain_nodes) == 3
    assert np.array_equal(lat.B_diag, twin.B_diag) and np.array_equal(lat.psi, psi)
    assert lat.receipt()["meta"]["state_sig"] == twin.receipt()["meta"]["state_sig"]
    expected = _expected(U_old, op, args)
    assert np.array_equal(_bits(lat.U), _bits(expected))
    twin.U = expected
    assert lat.settle()["iters"] == twin.settle()["iters"]
    assert lat.residual_history() == twin.residual_history()
    assert np.array_equal(_bits(lat.U), _bits(twin.U))


# ---- osc_carry_state through ctypes ------------------------------------------------------------------------------------------
def test_carry_state_refuses_a_bad_map_and_unlike_handles():
    from oscillink_amd import _native as nat

    L = nat.lib()
    rng, Y, psi = _inputs(60, 8)
    src, dst, wide = _lat(Y, 4, psi), _lat(Y[:50], 4, psi), _lat(np.concatenate([Y, Y], axis=1), 4)
    src.settle()
    dst.settle()
    U_dst = dst.U.copy()
    m = np.arange(50, dtype=np.int32)
    for bad, text in ((60, b"outside"), (-2, b"outside")):
        m2 = m.copy()
        m2[49] = bad
        assert L.osc_carry_state(dst._h, src._h, nat.i32(m2)) == nat.OSC_E_INVALID
        assert text in L.osc_last_error(dst._h)
    assert L.osc_carry_state(wide._h, src._h, nat.i32(np.arange(60, dtype=np.int32))) == nat.OSC_E_INVALID
    assert b"differ in D" in L.osc_last_error(wide._h)
    assert L.osc_carry_state(dst._h, dst._h, nat.i32(m)) == nat.OSC_E_INVALID
    assert L.osc_carry_state(dst._h, src._h, None) == nat.OSC_E_INVALID
    dst._U_host = None
    assert np.array_equal(_bits(dst.U), _bits(U_dst))  # a refused call changed nothing
    # ... and the same handles with a good map: rows 59 and 0 of src, an anchor, then src's rows 3 .. 49
    m[0], m[1], m[2] = 59, 0, -1
    assert L.osc_carry_state(dst._h, src._h, nat.i32(m)) == nat.OSC_OK
    dst._U_host = None
    want = src.U[np.maximum(m, 0)]
    want[2] = dst.Y[2]
    assert np.array_equal(_bits(dst.U), _bits(want))


# ---- meaning -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["update", "append", "remove"])
def test_a_carried_state_is_far_closer_to_the_stationary_one(op):
    """200 x 24, k 6, seed 0, psi the normalised mean of Y[:6]: after three settles and a three-row change, deltaH_total of
    the carried state is below a tenth of the cold start's.  The float32 oracle on the CPU gives ratios of 0.013 (update),
    0.013-0.016 (append) and 2e-5 (remove): the bound is a condition with about six-fold room, not a measured tolerance."""
    rng = np.random.default_rng(0)
    N, D, k = 200, 24, 6
    Y = rng.standard_normal((N, D)).astype(np.float32)
    rows = rng.standard_normal((3, D)).astype(np.float32)
    args = {"rows": rows} if op == "append" else {"ids": np.array([0, 77, 199])} if op == "remove" else \
        {"ids": np.array([0, 77, 199]), "rows": rows}
    psi = Y[:6].mean(axis=0)
    psi = (psi / (np.linalg.norm(psi) + 1e-12)).astype(np.float32)
    dH = {}
    for keep in (False, True):
        lat = _lat(Y, k, psi)
        for _ in range(3):
            lat.settle()
        _call(lat, op, args, "auto", keep_state=keep)
        dH[keep] = lat.receipt()["deltaH_total"]
    print(op, "deltaH cold", dH[False], "carried", dH[True], "ratio", dH[True] / dH[False])
    assert dH[True] < 0.1 * dH[False]

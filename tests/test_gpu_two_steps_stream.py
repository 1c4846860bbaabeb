"""The two forms of the fused two-step INIT pass ("Gram sums"): `k_init_two_steps_stream`, in the update
kernels' launch geometry, against `k_init_two_steps`, in the blocked matvec's -- the reference form.  Both call one per-element
function and no output element depends on another, so two handles on the same inputs, one under OSC_TWO_STEPS=blocked and one
under OSC_TWO_STEPS=stream, must agree to the bit (np.array_equal) on iters, res, residual_history() and U, for the settle and
for the U* solve.  The route is forced as in tests/test_gpu_anchor_gram.py (OSC_ANCHOR_AP=1 OSC_ANCHOR_AP2=1 OSC_ANCHOR_GRAM=1) and
every case asserts from the counters that the fused pass ran.

Shapes, the smallest at which the route runs and the streaming form's addressing can go wrong:
  * the four rows of that file's shape table (wide kernel shape, 20 011 x 200 with a pitch of 224, the second half of a column
    window, balanced row order);
  * at 20 000 rows the first and the last width of every (lanes per row, chunks) shape the launcher picks -- <16,1> 4 and 64,
    <32,1> 68 and 128, <64,1> 132 and 256, <64,2> 260 and 512, <64,3> 516 and 768 -- where 4, 260 and 516 leave the last chunk
    a single float4 (the one-chunk shapes <32,1> and <64,1> cannot: their first widths leave 17 and 33), and 772 columns: two
    column tiles of <64,2>, the second one's last chunk a single float4;
  * 20 001 rows and 24 575 = 3 x 8192 - 1 rows: one less than a multiple of the rows of a grid trip (1024 workgroups of four
    waves, one row per wave: 4096), so the last trip is partial and ends one row short of a wave's."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SWITCHES = ("OSC_SPMM_XS", "OSC_REORDER", "OSC_SPMM_BLOCKED", "OSC_BLK_VARIANT", "OSC_BLK_INIT", "OSC_X_DEFER", "OSC_X_RING",
            "OSC_ANCHOR_SLAB", "OSC_ANCHOR_WY", "OSC_ANCHOR_AP", "OSC_ANCHOR_AP2", "OSC_ANCHOR_GRAM", "OSC_TWO_STEPS", "OSC_BALANCE",
            "OSC_SMALL_PATH", "OSC_FAKE_COL_SHARD", "OSC_SHARD", "OSC_ROW_FAKE_SHARDS", "OSC_LD", "OSCILLINK_RECEIPT_DYNAMICS")
KW = dict(max_iters=12, tol=1e-3)


@pytest.fixture(scope="module")
def amd():
    import oscillink_amd
    from oscillink_amd import _native

    assert _native.device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return oscillink_amd


_INPUTS = {}


def _inputs(N, D, seed=3):
    """Anchors and query of a shape, made once and never written."""
    key = (N, D, seed)
    if key not in _INPUTS:
        rng = np.random.default_rng(seed)
        Y = rng.standard_normal((N, D)).astype(np.float32)
        psi = rng.standard_normal(D).astype(np.float32)
        psi /= np.linalg.norm(psi)
        _INPUTS.clear()  # (one shape at a time: the wide ones are 60 MB)
        _INPUTS[key] = (Y, psi)
    return _INPUTS[key]


def _clean_env(monkeypatch, env=None):
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)


def _make(amd, monkeypatch, Y, psi, form, k=16):
    for name in ("OSC_ANCHOR_AP", "OSC_ANCHOR_AP2", "OSC_ANCHOR_GRAM"):
        monkeypatch.setenv(name, "1")
    monkeypatch.setenv("OSC_TWO_STEPS", form)
    lat = amd.Oscillink(Y, kneighbors=k)
    lat.set_query(psi)
    return lat


def _anchor_start(lat, **kw):
    lat.reset_U(wait=False)
    st = lat.settle(**dict(KW, **kw))
    return st["iters"], st["res"], np.asarray(lat.residual_history()).copy(), lat.U.copy()


def _ustar(lat):
    u = lat.solve_Ustar(use_cache=False).copy()
    hist = np.asarray(lat.residual_history()).copy()
    return len(hist), hist[-1] if len(hist) else np.nan, hist, u


def _same(x, y, what):
    assert x[0] == y[0], (what, "iters", x[0], y[0])
    assert np.array_equal(np.float32(x[1]), np.float32(y[1]), equal_nan=True), (what, "res", x[1], y[1])
    assert np.array_equal(x[2], y[2], equal_nan=True), (what, "history", x[2], y[2])
    assert np.array_equal(x[3], y[3], equal_nan=True), (what, "U")


def _fused(lat):
    return lat.build_info()["fused_two_step_solves"]


def _compare(amd, monkeypatch, N, D, env=None, forms=("blocked", "stream"), settles=2, ustars=2):
    """Two handles, the same calls: anchor starts (the first gathers, the later ones take the route) and U* solves (likewise).
    `settles` and `ustars` are the fused passes expected of each kind."""
    _clean_env(monkeypatch, env)
    Y, psi = _inputs(N, D)
    lats = [_make(amd, monkeypatch, Y, psi, form) for form in forms]
    try:
        for trip in range(3):
            outs = [_anchor_start(lat) for lat in lats]
            _same(outs[0], outs[1], ("settle", trip))
        assert [_fused(lat) for lat in lats] == [settles, settles], "the settles did not take the route as expected"
        for trip in range(3):
            outs = [_ustar(lat) for lat in lats]
            _same(outs[0], outs[1], ("U*", trip))
        assert [_fused(lat) for lat in lats] == [settles + ustars, settles + ustars], "the U* solves did not take the route as expected"
        assert all(lat.build_info()["anchor_gram_redos"] == 0 for lat in lats)
    finally:
        for lat in lats:
            lat.close()


TABLE = {
    "wide_shape": dict(N=20000, D=256, env={"OSC_BLK_VARIANT": "3"}),
    "ragged": dict(N=20011, D=200, env={"OSC_LD": "224", "OSC_SPMM_XS": "1"}),
    # (the settles of a windowed handle start from U's own copy and do not take the route; the U* solves do, from the second on)
    "column_window": dict(N=20000, D=256, env={"OSC_FAKE_COL_SHARD": "1/2"}, settles=0, ustars=2),
    "balanced_rows": dict(N=20000, D=256, env={"OSC_BALANCE": "1"}),
}


@pytest.mark.parametrize("name", sorted(TABLE))
def test_shape_table_of_the_route(amd, name, monkeypatch):
    spec = TABLE[name]
    _compare(amd, monkeypatch, spec["N"], spec["D"], spec.get("env"), settles=spec.get("settles", 2), ustars=spec.get("ustars", 2))


@pytest.mark.parametrize("D", [4, 64, 68, 128, 132, 256, 260, 512, 516, 768, 772])
def test_first_and_last_width_of_every_shape(amd, D, monkeypatch):
    env = {"OSC_SPMM_XS": "1"}  # (the slab mode, and with it the route, at every width)
    if D % 32:
        env["OSC_LD"] = str((D + 31) // 32 * 32)
    _compare(amd, monkeypatch, 20000, D, env)


@pytest.mark.parametrize("N", [20001, 24575])
def test_partial_last_trip(amd, N, monkeypatch):
    _compare(amd, monkeypatch, N, 256)


def test_gated_off_pass_gives_the_same_redo_and_bytes(amd, monkeypatch):
    """The early-stop setup of tests/test_gpu_anchor_gram.py: after a prediction of three or more, a tol between res1 and res2 or
    above res1 stops the solve early -- the fused pass was launched with its gate word off and must have written nothing in
    either form --, the solve runs again at depth 2, and both handles count one redo and hold the same bytes."""
    _clean_env(monkeypatch)
    Y, psi = _inputs(20000, 256, seed=12)
    lats = [_make(amd, monkeypatch, Y, psi, form) for form in ("blocked", "stream")]
    try:
        for trip in range(2):
            outs = [_anchor_start(lat) for lat in lats]
            _same(outs[0], outs[1], ("warm", trip))
        assert [_fused(lat) for lat in lats] == [1, 1]
        hist = outs[0][2]
        assert len(hist) >= 4, hist
        tol1 = float(hist[0]) * 1.5
        tol2 = float(np.sqrt(hist[0] * hist[1]))
        redos = 0
        for what, tol, iters in (("stop at 2", tol2, 2), ("stop at 1", tol1, 1)):
            outs = [_anchor_start(lat, tol=tol) for lat in lats]
            _same(outs[0], outs[1], what)
            redos += 1
            assert outs[1][0] == iters, (what, outs[1][0])
            assert [lat.build_info()["anchor_gram_redos"] for lat in lats] == [redos, redos], what
            for trip in range(3):  # (predicted short twice, then the route again)
                outs = [_anchor_start(lat, **({"tol": tol} if trip == 0 else {})) for lat in lats]
                _same(outs[0], outs[1], (what, "after", trip))
            assert [lat.build_info()["anchor_gram_redos"] for lat in lats] == [redos, redos], what
        assert _fused(lats[0]) == _fused(lats[1]) >= 3
    finally:
        for lat in lats:
            lat.close()


def test_two_streaming_handles_give_the_same_bytes(amd, monkeypatch):
    _compare(amd, monkeypatch, 20000, 256, forms=("stream", "stream"))

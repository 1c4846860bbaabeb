"""The MMR kernels (receipt_kernels.hip: k_mmr_argmax1, k_mmr_update_argmax, k_mmr_argmax2, behind osc_mmr / Oscillink._mmr) and
the cosine kernel (knn_kernels.hip: k_rows_cosine, behind osc_cosine_to, osc_ustar_cosine_to, osc_cosine_to_row) against
float64: tests/_queries.mmr and _receipt_reference.cosine_to.

MMR lists are compared with `same_until_near_tie` at 1e-4 (tests/test_gpu_bundle_many.py); the margins come from float64
alone, and tests/test_receipt_reference_host.py proves for these seeds that at most one list in ten is cut short, none before
its third pick.

  case                     reaches
  n1 .. n20000 (D = 6)     k_mmr_argmax1: 1 .. 79 blocks, partly filled; mmr_parts = ceil(N / 4) up to 8192, capped at 2048
                           workgroups from 8193 on (a wave of k_mmr_update_argmax takes several rows); k_mmr_argmax2: 1 .. 2048
                           partials over its 256 threads
  n65537_strided           k_mmr_argmax1's 256-block cap: the `i += gridDim.x * 256` stride loop takes a second trip
  d1 .. d1030 (N = 500)    k_mmr_update_argmax / k_mmr_argmax2: the float4 body against the scalar tail (D % 4 != 0), no
                           float4 body at all (D < 4), the `c += 256` loop (D > 256: 260, 1030)
  lambda0 / lambda1        plain top-k / an all-tie first step that id 0 wins, then pure diversity
  exhaust_*                k = N and k = N + 5 at N = 257: every row is picked once.  osc_mmr clamps k to N, so the
                           `chosen = -1` exit of k_mmr_argmax2 cannot be reached through the API; the clamp is what is checked
  zero_rows                all-zero anchor rows: cosine 0 on both sides (the 1e-12 guards)
  duplicate blocks         exact ties in value: the smaller API id wins, in API order and in a stored (breadth-first) order

Measured on an MI355X: every list equals the float64 list up to its first near tie (two of 23 lists have one: the two
exhaustion lists, at picks 77 and 164); largest cosine error 4.8e-7 (bound 1e-4).  Slips tried on scratch builds: fmin for
fmax in the running similarity -> 17 tests fail; the tie order of mmr_better turned round -> lambda1 and both exact-tie tests;
k_rows_cosine without its scalar tail -> the five widths with D % 4 != 0.
"""
import numpy as np
import pytest

from tests import _dynamics_reference as G
from tests import _queries as yq
from tests import _receipt_reference as RR

pytestmark = pytest.mark.gpu

SWITCHES = ("OSC_REORDER", "OSC_LD", "OSC_BALANCE", "OSC_SMALL_PATH", "OSC_SPMM_XS", "OSC_SPMM_BLOCKED")
COS_TOL = 1e-4  # absolute, on a quantity in [-1, 1]


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


def _device_list(amd, name):
    N, D, seed, k, lam, zero = RR.MMR_CASES[name]
    Y, scores = RR.mmr_inputs(N, D, seed, zero)
    lat = amd.Oscillink(Y, kneighbors=4, _build_graph=False)  # (osc_mmr needs no graph)
    got = lat._mmr(scores, k, lam)
    lat.close()
    return got, scores


def _assert_same(name, got, skip=0):
    want, margins = RR.mmr_reference(name)
    ok, cut = yq.same_until_near_tie(got[skip:], list(want)[skip:], list(margins)[skip:], RR.NEAR_TIE)
    compared = min(RR.first_near_tie(margins[skip:]) + skip, len(want))
    print(f"MMR {name}: {len(got)} picks, {compared} compared, smallest margin before the cut "
          f"{min(margins[skip:compared], default=float('inf')):.3e}, cut short: {cut}")
    assert ok, (name, got[:12], want[:12])
    assert len(got) == len(want) and len(set(got)) == len(got)


@pytest.mark.parametrize("name", [n for n in RR.MMR_CASES if n.startswith("n")])
def test_mmr_at_the_row_count_seams(amd, name):
    got, _ = _device_list(amd, name)
    _assert_same(name, got)


@pytest.mark.parametrize("name", [n for n in RR.MMR_CASES if n.startswith("d")])
def test_mmr_at_the_width_seams(amd, name):
    got, _ = _device_list(amd, name)
    _assert_same(name, got)


def test_mmr_lambda_0_is_plain_top_k(amd):
    got, scores = _device_list(amd, "lambda0")
    k = RR.MMR_CASES["lambda0"][3]
    assert got == np.argsort(-scores.astype(np.float64), kind="stable")[:k].tolist()
    assert got == list(RR.mmr_reference("lambda0")[0])


def test_mmr_lambda_1_is_pure_diversity(amd):
    """Every value of step 0 is (1 - 1) score = 0: id 0 wins the all-tie; from then on -maxsim alone decides."""
    got, _ = _device_list(amd, "lambda1")
    assert got[0] == 0
    _assert_same("lambda1", got, skip=1)


@pytest.mark.parametrize("name", ["exhaust_k_n", "exhaust_k_n_plus_5"])
def test_mmr_exhausts_every_row(amd, name):
    got, _ = _device_list(amd, name)
    assert sorted(got) == list(range(257))
    _assert_same(name, got)


def test_mmr_with_zero_rows(amd):
    got, _ = _device_list(amd, "zero_rows")
    _assert_same("zero_rows", got)


def test_mmr_exact_ties_without_a_graph(amd):
    Y, scores, groups = RR.duplicate_blocks(700, 10, 41)
    want, margins = yq.mmr(Y, scores, 24, 0.5)
    lat = amd.Oscillink(Y, kneighbors=4, _build_graph=False)
    got = lat._mmr(scores, 24, 0.5)
    assert margins.count(0.0) >= 10 and RR.picks_smallest_remaining(got, groups)
    assert got == want


def test_mmr_exact_ties_in_a_stored_order(amd, monkeypatch):
    """A built kNN lattice stored breadth-first: the kernels see device rows and break ties by `api_id`."""
    monkeypatch.setenv("OSC_REORDER", "1")
    Y, scores, groups = RR.duplicate_blocks(2000, 24, 42)
    want, margins = yq.mmr(Y, scores, 24, 0.5)
    lat = amd.Oscillink(Y, kneighbors=6)
    assert lat.build_info()["reordered"] == 1
    got = lat._mmr(scores, 24, 0.5)
    assert margins.count(0.0) >= 10 and RR.picks_smallest_remaining(got, groups)
    assert got == want


# ---------------------------------------------------------------------------------------------------------------- cosines
@pytest.mark.parametrize("D,osc_ld", [(D, None) for D in RR.COSINE_WIDTHS] + [(50, 64)])
def test_cosine_kernels(amd, D, osc_ld, monkeypatch):
    """osc_cosine_to (anchors), osc_ustar_cosine_to (the resident U*) and osc_cosine_to_row (row 0, the last row, an all-zero
    row) against float64 with rows_cosine_to's guards; 1e-4 absolute."""
    from oscillink_amd import _native as nat

    if osc_ld is not None:
        monkeypatch.setenv("OSC_LD", str(osc_ld))
    N, zero = 500, 123
    rng = np.random.default_rng(400 + D)
    Y = rng.standard_normal((N, D)).astype(np.float32)
    Y[zero] = 0.0
    psi = rng.standard_normal(D).astype(np.float32)
    lat = amd.Oscillink(Y, kneighbors=4, _build_graph=False)
    lat.set_graph_csr(*G.circulant(N, (1, 2)))
    lat.set_query(psi, gates=rng.uniform(0.1, 1.0, N).astype(np.float32))
    Us = lat.solve_Ustar(tol=1e-3, max_iters=16)
    out = np.full(N, 7.0, dtype=np.float32)
    worst = {}

    def check(key, want):
        assert np.all(np.isfinite(out))
        worst[key] = float(np.max(np.abs(out.astype(np.float64) - want)))
        assert worst[key] <= COS_TOL, (key, worst[key])

    lat._call("osc_cosine_to", nat.f32(psi), nat.f32(out))
    check("cosine_to", RR.cosine_to(Y, psi))
    assert out[zero] == 0.0
    lat._call("osc_ustar_cosine_to", nat.f32(psi), nat.f32(out))
    check("ustar_cosine_to", RR.cosine_to(Us, psi))
    for r in (0, N - 1, zero):
        out[:] = 7.0
        lat._call("osc_cosine_to_row", r, nat.f32(out))
        check(f"cosine_to_row[{r}]", RR.cosine_to(Y, Y[r]))
        if r == zero:
            assert np.all(out == 0.0)
        else:
            assert out[r] == pytest.approx(1.0, abs=COS_TOL) and out[zero] == 0.0
    print(f"COSINE D={D} ld={osc_ld}: largest |error|", {k: float(f"{v:.3g}") for k, v in worst.items()})
    lat.close()

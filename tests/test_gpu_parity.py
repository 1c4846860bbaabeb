"""GPU parity tests: the HIP path (through the C ABI, via oscillink_amd) against the CPU oracle and the golden
fixtures generated from the reference.  Run on the MI355X box with `pytest -m gpu`.

Tolerances: BASELINE.json asks for 1e-4 relative fp32 on U*, deltaH and residuals with identical CG iteration
counts; the asserts below use 1e-4 where the north star states it and tighter bounds where the implementation is
expected to do better (the tighter ones are regression guards, not the contract).
"""
import numpy as np
import pytest

from tests._cases import ALL_CASES, PARAM_CASES, ctor_kwargs, known_answers, load_case, make_inputs, random_gates, relerr

pytestmark = pytest.mark.gpu

TOL = 1e-4  # north_star: "within 1e-4 relative fp32 tolerance"


@pytest.fixture(scope="module")
def amd():
    import oscillink_amd
    from oscillink_amd import _native

    assert _native.device_count() >= 1, "no HIP device: the GPU tests must run on the MI355X box"
    return oscillink_amd


@pytest.fixture(scope="module")
def orc():
    from oracle import oscillink_oracle

    return oscillink_oracle


def _csr_from_case(case):
    return case["indptr"].astype(np.int64), case["indices"].astype(np.int32), case["A_data"].astype(np.float32)


def _configure(lat, case, rc, psi):
    gates = None
    if rc["gates"] == "random":
        gates = random_gates(rc)
    elif rc["gates"] == "diffusion":
        gates = case["gates"]
    lat.set_query(psi, gates=gates)
    if rc["chain"]:
        lat.add_chain(rc["chain"], lamP=rc["lamP"])


def _check_solves(lat, case, rc, tol_u=TOL):
    st = lat.settle(max_iters=rc["settle_max_iters"], tol=rc["settle_tol"])
    assert st["iters"] == int(case["settle_iters"])
    hist = lat.residual_history()
    assert len(hist) == len(case["hist_settle"])
    assert np.allclose(hist, case["hist_settle"], rtol=2e-2, atol=1e-7)
    assert st["res"] == pytest.approx(float(case["settle_res"]), rel=2e-2, abs=1e-7)
    Us = lat.solve_Ustar()
    assert lat.last_ustar["iters"] == int(case["ustar_iters"])
    assert lat.last_ustar["res"] == pytest.approx(float(case["ustar_res"]), rel=2e-2, abs=1e-7)
    assert np.allclose(lat.residual_history(), case["hist_ustar"], rtol=2e-2, atol=1e-7)
    if "U" in case:
        assert relerr(lat.U, case["U"]) < tol_u
        assert relerr(Us, case["Ustar"]) < tol_u
    assert np.allclose(lat.U.sum(axis=1), case["U_rowsum"], rtol=1e-4, atol=1e-3)
    assert np.allclose(Us.sum(axis=1), case["Ustar_rowsum"], rtol=1e-4, atol=1e-3)
    lat.set_receipt_detail(rc["detail"])
    rec = lat.receipt()
    assert rec["deltaH_total"] == pytest.approx(float(case["deltaH"]), rel=TOL)
    assert rec["cg_iters"] == int(case["settle_iters"])
    assert rec["meta"]["ustar_iters"] == int(case["ustar_iters"])
    if rc["detail"] == "full":
        assert rec["coh_drop_sum"] == pytest.approx(float(case["coh_drop_sum"]), rel=TOL)
        assert rec["anchor_pen_sum"] == pytest.approx(float(case["anchor_pen_sum"]), rel=TOL)
        assert rec["query_term_sum"] == pytest.approx(float(case["query_term_sum"]), rel=TOL)
        assert len(rec["null_points"]) == int(case["n_nulls"])
        if rec["null_points"]:
            assert np.array_equal(np.array([n["edge"] for n in rec["null_points"]]), case["null_edges"])
            assert np.allclose([n["z"] for n in rec["null_points"]], case["null_z"], rtol=1e-3)
            assert np.allclose([n["residual"] for n in rec["null_points"]], case["null_r"], rtol=1e-3)
    return rec


@pytest.mark.parametrize("name", ALL_CASES)
def test_cg_with_injected_graph_matches_reference(amd, name):
    """Solver parity isolated from kNN tie noise: the reference's graph is injected through osc_set_csr."""
    case = load_case(name)
    rc = case["recipe"]
    Y, psi = make_inputs(rc)
    lat = amd.Oscillink(Y, kneighbors=rc["k"], deterministic_k=rc["deterministic"], _build_graph=False, **ctor_kwargs(rc))
    lat.set_graph_csr(*_csr_from_case(case))
    assert np.allclose(lat.sqrt_deg, case["sqrt_deg"], rtol=2e-6)
    _configure(lat, case, rc, psi)
    rec = _check_solves(lat, case, rc, tol_u=2e-5)
    if rc["gates"] != "diffusion":
        assert rec["meta"]["state_sig"] == str(case["state_sig"])


@pytest.mark.parametrize("name", ["c2_n1200_d128_k16", "g1_n400_d64_k6_chain8", "gates_chain_n333_d50_k7"])
def test_general_multi_kernel_cg_on_small_fixtures(amd, name, monkeypatch):
    """Small lattices normally take the one-launch LDS-resident CG; OSC_SMALL_PATH=0 forces the general multi-kernel
    path (the one config 3 runs) through the same fixtures, and both must agree with the reference."""
    monkeypatch.setenv("OSC_SMALL_PATH", "0")
    case = load_case(name)
    rc = case["recipe"]
    Y, psi = make_inputs(rc)
    lat = amd.Oscillink(Y, kneighbors=rc["k"], deterministic_k=rc["deterministic"], _build_graph=False, **ctor_kwargs(rc))
    lat.set_graph_csr(*_csr_from_case(case))
    _configure(lat, case, rc, psi)
    _check_solves(lat, case, rc, tol_u=2e-5)


@pytest.mark.parametrize("name", ALL_CASES)
def test_device_knn_graph_matches_reference(amd, name):
    """Device mutual-kNN + cap + Laplacian weights against the reference's adjacency (same edge set, same weights)."""
    case = load_case(name)
    rc = case["recipe"]
    Y, _ = make_inputs(rc)
    lat = amd.Oscillink(Y, kneighbors=rc["k"], deterministic_k=rc["deterministic"], **ctor_kwargs(rc))
    rowptr, col, a, w, sd = lat.graph_csr()
    assert np.array_equal(rowptr, case["indptr"])
    assert np.array_equal(col, case["indices"])
    assert np.allclose(a, case["A_data"], rtol=1e-5, atol=1e-8)
    assert np.allclose(sd, case["sqrt_deg"], rtol=1e-5)
    # symmetric by construction
    A = lat.A
    assert np.array_equal(A, A.T)
    assert float(np.abs(np.diag(A)).max()) == 0.0


@pytest.mark.parametrize("name", ALL_CASES)
def test_end_to_end_device_path_matches_reference(amd, name):
    """Everything on the device: build -> settle -> U* -> receipt, against the reference fixture."""
    case = load_case(name)
    rc = case["recipe"]
    Y, psi = make_inputs(rc)
    lat = amd.Oscillink(Y, kneighbors=rc["k"], deterministic_k=rc["deterministic"], **ctor_kwargs(rc))
    if rc["gates"] == "diffusion":
        g = amd.compute_diffusion_gates(Y, psi, kneighbors=rc["k"], deterministic_k=True, **rc["diffusion"])
        assert np.allclose(g, case["gates"], atol=1e-4)
    _configure(lat, case, rc, psi)
    _check_solves(lat, case, rc)


@pytest.mark.parametrize("row", known_answers()["scale"], ids=lambda r: f"N{r['N']}_D{r['D']}_k{r['k']}")
def test_reference_recorded_scale_rows_on_device(amd, row):
    """The reference authors' own recorded runs (benchmarks/scale*.jsonl): deltaH, U* iterations, residual."""
    N, D, k = row["N"], row["D"], row["k"]
    rs = np.random.RandomState(0)
    Y = rs.randn(N, D).astype(np.float32)
    psi = rs.randn(D).astype(np.float32)
    lat = amd.Oscillink(Y, kneighbors=k, deterministic_k=True)
    lat.set_receipt_detail("light")
    lat.set_query(psi / (np.linalg.norm(psi) + 1e-12))
    lat.add_chain([0, 1, 2, 3])
    lat.settle(max_iters=6, tol=1e-3)
    lat.refresh_Ustar(tol=1e-4, max_iters=64)
    rec = lat.receipt()
    assert rec["meta"]["ustar_iters"] == row["ustar_iters"]
    assert rec["meta"]["ustar_res"] == pytest.approx(row["ustar_res"], rel=5e-2)
    assert rec["deltaH_total"] == pytest.approx(row["deltaH"], rel=TOL)


def test_reference_recorded_perf_snapshot_on_device(amd):
    ka = known_answers()["perf_snapshot"]
    cfg = ka["config"]
    rs = np.random.RandomState(0)
    Y = rs.randn(cfg["N"], cfg["D"]).astype(np.float32)
    psi = Y[:32].mean(axis=0).astype(np.float32)
    psi /= np.linalg.norm(psi) + 1e-12
    lat = amd.Oscillink(Y, kneighbors=cfg["kneighbors"], lamG=cfg["lamG"], lamC=cfg["lamC"], lamQ=cfg["lamQ"],
                        deterministic_k=True)
    lat.set_query(psi)
    chain = list(range(cfg["chain_len"]))
    lat.add_chain(chain, lamP=cfg["lamP"])
    lat.settle(max_iters=12, tol=1e-3)
    rec = lat.receipt()
    assert rec["deltaH_total"] == pytest.approx(ka["deltaH"], rel=TOL)
    assert rec["meta"]["ustar_iters"] == ka["ustar_iters"]
    assert len(rec["null_points"]) == ka["null_points"]
    assert rec["null_points"][0]["edge"] == ka["sample_null"]["edge"]
    assert rec["null_points"][0]["z"] == pytest.approx(ka["sample_null"]["z"], rel=1e-3)
    assert rec["null_points"][0]["residual"] == pytest.approx(ka["sample_null"]["residual"], rel=1e-3)
    cr = lat.chain_receipt(chain)
    assert cr["verdict"] == ka["chain_verdict"]
    assert cr["weakest_link"]["k"] == ka["weakest_link"]["k"]
    assert cr["weakest_link"]["edge"] == ka["weakest_link"]["edge"]
    assert cr["weakest_link"]["zscore"] == pytest.approx(ka["weakest_link"]["zscore"], rel=1e-3)


@pytest.mark.parametrize("name", ["c1_n80_d128_k8", "g1_n400_d64_k6_chain8", "gates_chain_n333_d50_k7"])
def test_bundle_matches_fixture(amd, name):
    """bundle() (lattice.py:530-568): z(coherence drop) + alignment score, MMR-diversified over Y."""
    case = load_case(name)
    rc = case["recipe"]
    Y, psi = make_inputs(rc)
    lat = amd.Oscillink(Y, kneighbors=rc["k"], deterministic_k=True)
    _configure(lat, case, rc, psi)
    lat.settle(max_iters=rc["settle_max_iters"], tol=rc["settle_tol"])
    bd = lat.bundle(k=6, alpha=0.5)
    assert [b["id"] for b in bd] == case["bundle_ids"].tolist()
    assert np.allclose([b["score"] for b in bd], case["bundle_score"], rtol=1e-3, atol=1e-4)
    assert np.allclose([b["align"] for b in bd], case["bundle_align"], rtol=1e-3, atol=1e-5)


def test_chain_receipt_matches_fixture(amd):
    case = load_case("g1_n400_d64_k6_chain8")
    rc = case["recipe"]
    Y, psi = make_inputs(rc)
    lat = amd.Oscillink(Y, kneighbors=rc["k"], deterministic_k=True)
    _configure(lat, case, rc, psi)
    lat.settle(max_iters=12, tol=1e-3)
    cr = lat.chain_receipt(rc["chain"])
    assert cr["verdict"] == bool(case["chain_verdict"])
    assert cr["weakest_link"]["k"] == int(case["chain_weakest_k"])
    assert cr["coherence_gain"] == pytest.approx(float(case["chain_gain"]), rel=1e-3, abs=1e-6)
    assert np.allclose([e["z_struct"] for e in cr["edges"]], case["chain_z_struct"], rtol=1e-3, atol=1e-4)
    assert np.allclose([e["z_path"] for e in cr["edges"]], case["chain_z_path"], rtol=1e-3, atol=1e-4)


# ---------------------------------------------------------------------------------------------------
# edge cases the reference tests
# ---------------------------------------------------------------------------------------------------
def test_degenerate_and_clamped_inputs(amd):
    lat = amd.Oscillink(np.ones((1, 4), dtype=np.float32), kneighbors=3)  # tests/test_graph_helpers.py:6-10
    assert lat.A.shape == (1, 1) and float(lat.A[0, 0]) == 0.0
    st = lat.settle()
    assert st["iters"] >= 1 and np.isfinite(st["res"])
    Y = np.random.default_rng(0).standard_normal((10, 8)).astype(np.float32)
    lat = amd.Oscillink(Y, kneighbors=50)  # tests/test_kneighbors_clamp.py:8-18
    assert lat._kneighbors == 9
    lat.settle()
    assert lat.receipt()["deltaH_total"] >= -1e-5


def test_all_ties_deterministic_neighbors(amd, orc):
    """tests/test_new_invariants.py:28-40: identical rows -> every similarity ties; (sim desc, idx asc) order."""
    Yt = np.ones((40, 6), dtype=np.float32)
    a = amd.Oscillink(Yt, kneighbors=3, deterministic_k=True)
    b = amd.Oscillink(Yt, kneighbors=3, deterministic_k=True)
    assert np.array_equal(a.A, b.A)
    ref = orc.OracleLattice(Yt, kneighbors=3, deterministic_k=True)
    assert np.array_equal(a.A > 0, ref.A > 0)
    assert np.allclose(a.A, ref.A, rtol=1e-5)


def test_parameter_validation_errors(amd):
    Y = np.random.default_rng(0).standard_normal((12, 8)).astype(np.float32)
    for bad in (dict(kneighbors=0), dict(lamG=0.0), dict(lamC=-1.0), dict(lamQ=-0.5)):
        with pytest.raises(ValueError):
            amd.Oscillink(Y, **bad)
    with pytest.raises(ValueError):
        amd.Oscillink(Y[0])
    lat = amd.Oscillink(Y, kneighbors=3)
    with pytest.raises(ValueError):
        lat.add_chain([0])
    with pytest.raises(ValueError):
        lat.add_chain([0, 99])
    with pytest.raises(ValueError):
        lat.add_chain([0, 1, 2], weights=[1.0])
    with pytest.raises(ValueError):
        lat.add_chain([0, 1], lamP=-1.0)
    with pytest.raises(ValueError):
        lat.set_gates(np.ones(3, dtype=np.float32))
    with pytest.raises(ValueError):
        lat.set_receipt_detail("bogus")
    with pytest.raises(ValueError):
        lat.set_signature_mode("bogus")


def test_ustar_cache_rebuild_and_persistence(amd, tmp_path):
    rng = np.random.default_rng(3)
    Y = rng.standard_normal((90, 24)).astype(np.float32)
    psi = rng.standard_normal(24).astype(np.float32)
    lat = amd.Oscillink(Y, kneighbors=5, deterministic_k=True)
    lat.set_query(psi)
    lat.add_chain([1, 4, 7], lamP=0.3)
    lat.settle()
    r1 = lat.receipt()
    solves = lat.stats["ustar_solves"]
    lat.bundle(k=4)  # second consumer hits the cache (tests/test_export_import_and_cache.py:27-45)
    assert lat.stats["ustar_solves"] == solves and lat.stats["ustar_cache_hits"] >= 1
    sig = lat._signature()
    for fmt in ("json", "npz"):
        p = str(tmp_path / f"state.{fmt}")
        lat.save_state(p, format=fmt)
        lat2 = amd.OscillinkLattice.from_npz(p) if fmt == "npz" else amd.OscillinkLattice.from_state(
            __import__("json").load(open(p)))
        assert lat2._signature() == sig
        lat2.settle()
        assert lat2.receipt()["deltaH_total"] == pytest.approx(r1["deltaH_total"], rel=1e-2)
    # the reference's own format (dense A only) is still read, and a large lattice persists through the CSR triplet
    st = lat.export_state()
    dense_only = {k_: v for k_, v in st.items() if k_ != "A_csr"}
    assert amd.OscillinkLattice.from_state(dense_only)._signature() == sig
    csr_only = {k_: v for k_, v in st.items() if k_ != "A"}
    assert amd.OscillinkLattice.from_state(csr_only)._signature() == sig
    lat.rebuild_graph(kneighbors=7)  # tests/test_lattice_receipt_and_start_modes.py:63-71
    lat.receipt()
    assert lat.stats["ustar_solves"] == solves + 1


def test_start_modes_inertia_and_unpreconditioned(amd, orc):
    rng = np.random.default_rng(5)
    Y = rng.standard_normal((150, 40)).astype(np.float32)
    psi = rng.standard_normal(40).astype(np.float32)
    ref = orc.OracleLattice(Y, kneighbors=6, deterministic_k=True)
    lat = amd.Oscillink(Y, kneighbors=6, deterministic_k=True)
    for L in (ref, lat):
        L.set_query(psi)
    for kw in (dict(), dict(warm_start=False), dict(inertia=0.4), dict(precond="none", max_iters=30),
               dict(dt=0.3, tol=1e-5, max_iters=40)):
        a = ref.settle(**kw)
        b = lat.settle(**kw)
        assert a["iters"] == b["iters"], kw
        assert relerr(lat.U, ref.U) < 2e-5, kw


@pytest.mark.parametrize("name", ["c2_n1200_d128_k16", "gates_chain_n333_d50_k7", "nondet_n256_d32_k5"])
def test_prefilter_and_exact_knn_paths_agree_with_reference(amd, name, monkeypatch):
    """The fp16-prefilter + exact re-scoring build (default for N >= 4096) and the all-fp32 MFMA build are forced in
    turn on the same fixture; both must give the reference's edge set.  The all-ties input exercises the per-row
    exact fallback (no candidate list can be proven there)."""
    case = load_case(name)
    rc = case["recipe"]
    Y, _ = make_inputs(rc)
    for mode in ("prefilter", "exact"):
        monkeypatch.setenv("OSC_KNN_MODE", mode)
        lat = amd.Oscillink(Y, kneighbors=rc["k"], deterministic_k=rc["deterministic"])
        rowptr, col, a, w, sd = lat.graph_csr()
        assert np.array_equal(rowptr, case["indptr"]) and np.array_equal(col, case["indices"]), mode
        assert np.allclose(a, case["A_data"], rtol=1e-5, atol=1e-8), mode
        assert lat.build_info()["prefilter"] == (1 if mode == "prefilter" else 0)
        assert lat.build_info()["fallback_rows"] == 0  # continuous data: every candidate list is proven
    monkeypatch.setenv("OSC_KNN_MODE", "prefilter")
    Yt = np.ones((300, 6), dtype=np.float32)
    tl = amd.Oscillink(Yt, kneighbors=5, deterministic_k=True)
    bi = tl.build_info()
    assert (bi["prefilter"], bi["fallback_rows"], bi["small_solves"]) == (1, 300, 0)  # nothing provable: all redone
    ties = tl.A
    monkeypatch.setenv("OSC_KNN_MODE", "exact")
    assert np.array_equal(ties, amd.Oscillink(Yt, kneighbors=5, deterministic_k=True).A)


@pytest.mark.parametrize("name", ["c2_n1200_d128_k16", "g1_n400_d64_k6_chain8", "gates_chain_n333_d50_k7"])
@pytest.mark.parametrize("shards", ["2", "3", "8"])
def test_row_sharded_cg_on_fake_ranks_matches_reference(amd, name, shards, monkeypatch):
    """Row-sharded CG (the BASELINE north-star partitioning): OSC_ROW_FAKE_SHARDS runs the per-rank row ranges one
    after another on this GPU (the RCCL exchanges become no-ops because all rows share one memory), which exercises the
    row-range kernels and the cross-shard completion of the column sums.  Same fixtures, same tolerances."""
    monkeypatch.setenv("OSC_SHARD", "row")
    monkeypatch.setenv("OSC_ROW_FAKE_SHARDS", shards)
    case = load_case(name)
    rc = case["recipe"]
    Y, psi = make_inputs(rc)
    lat = amd.Oscillink(Y, kneighbors=rc["k"], deterministic_k=rc["deterministic"], _build_graph=False)
    lat.set_graph_csr(*_csr_from_case(case))
    _configure(lat, case, rc, psi)
    _check_solves(lat, case, rc, tol_u=2e-5)
    assert lat.build_info()["small_solves"] == 0  # the sharded driver ran, not the one-launch path


def test_row_block_sharded_knn_passes_equal_single_pass(amd, monkeypatch):
    """The multi-GPU lattice build shards 128-row blocks over ranks; OSC_KNN_FAKE_SHARDS runs the per-rank passes one
    after another on this GPU.  The assembled graph must equal the single-pass build bit for bit."""
    rng = np.random.default_rng(11)
    Y = rng.standard_normal((1000, 48)).astype(np.float32)
    lat = amd.Oscillink(Y, kneighbors=9, deterministic_k=True)
    base = [x.copy() for x in lat.graph_csr()]
    for parts in ("2", "3", "8", "16"):
        monkeypatch.setenv("OSC_KNN_FAKE_SHARDS", parts)
        lat.rebuild_graph()
        for a_, b_ in zip(base, lat.graph_csr()):
            assert np.array_equal(a_, b_), parts
    monkeypatch.delenv("OSC_KNN_FAKE_SHARDS")


def test_null_point_cap_env(amd, monkeypatch):
    """OSCILLINK_RECEIPT_NULL_CAP (lattice.py:336-356; reference tests/test_null_cap.py:15-33)."""
    Y = np.random.default_rng(2).standard_normal((120, 32)).astype(np.float32)
    lat = amd.Oscillink(Y, kneighbors=6, deterministic_k=True)
    lat.settle()
    full = lat.receipt()
    total = len(full["null_points"])
    assert total > 3 and not full["meta"]["null_points_summary"]["null_cap_applied"]
    monkeypatch.setenv("OSCILLINK_RECEIPT_NULL_CAP", "3")
    rec = lat.receipt()
    assert len(rec["null_points"]) == 3
    assert rec["meta"]["null_points_summary"] == {"total_null_points": total, "returned_null_points": 3,
                                                  "null_cap_applied": True}
    top = sorted(full["null_points"], key=lambda e: e["z"], reverse=True)[:3]
    assert [n["edge"] for n in rec["null_points"]] == [n["edge"] for n in top]
    monkeypatch.setenv("OSCILLINK_RECEIPT_NULL_CAP", "garbage")
    assert len(lat.receipt()["null_points"]) == total


def test_signed_receipt_roundtrip(amd):
    Y = np.random.default_rng(1).standard_normal((60, 16)).astype(np.float32)
    lat = amd.Oscillink(Y, kneighbors=4)
    lat.set_receipt_secret("s3cret")
    lat.settle()
    for mode in ("minimal", "extended"):
        lat.set_signature_mode(mode)
        rec = lat.receipt()
        assert amd.verify_receipt(rec, "s3cret") and not amd.verify_receipt(rec, "other")
        ok, payload = amd.verify_receipt_mode(rec, "s3cret", require_mode=mode)
        assert ok and payload["mode"] == mode
        rec["deltaH_total"] = 1.0
        rec["meta"]["signature"]["payload"]["deltaH_total"] = 1.0
        assert not amd.verify_receipt(rec, "s3cret")
    assert lat.verify_current_receipt("s3cret")


# ---------------------------------------------------------------------------------------------------
# larger sizes: oracle on the same seeded inputs where it finishes in seconds, properties at full size
# ---------------------------------------------------------------------------------------------------
def test_mid_size_against_sparse_oracle(amd, orc):
    """N=6000, D=768, k=32 (config-3 shape, scaled to oracle-seconds): full device path vs the sparse oracle."""
    rng = np.random.default_rng(0)
    N, D, k = 6000, 768, 32
    Y = rng.standard_normal((N, D)).astype(np.float32)
    psi = Y[:32].mean(axis=0)
    psi = (psi / (np.linalg.norm(psi) + 1e-12)).astype(np.float32)
    ref = orc.OracleLattice(Y, kneighbors=k, deterministic_k=True, dense=False, knn_block=2048)
    lat = amd.Oscillink(Y, kneighbors=k, deterministic_k=True)
    rp, col, a, w, sd = lat.graph_csr()
    R = ref.A.tocsr()
    same = np.array_equal(rp, R.indptr) and np.array_equal(col, R.indices)
    if not same:  # near-tie neighbour flips are legal (sgemm vs MFMA summation order); bound them
        dev = set(zip(np.repeat(np.arange(N), np.diff(rp)).tolist(), col.tolist()))
        cpu = set(zip(*R.nonzero()))
        jac = len(dev & cpu) / max(1, len(dev | cpu))
        assert jac > 1 - 1e-4, jac
        lat.set_graph_csr(R.indptr.astype(np.int64), R.indices.astype(np.int32), R.data.astype(np.float32))
    else:
        assert np.allclose(a, R.data, rtol=1e-5)
    for L in (ref, lat):
        L.set_query(psi)
    a_ = ref.settle(max_iters=12, tol=1e-3)
    b_ = lat.settle(max_iters=12, tol=1e-3)
    assert a_["iters"] == b_["iters"]
    assert b_["res"] == pytest.approx(a_["res"], rel=2e-2)
    assert relerr(lat.U, ref.U) < TOL
    Us = ref.solve_Ustar()
    Ud = lat.solve_Ustar()
    assert lat.last_ustar["iters"] == ref.last_ustar["iters"]
    assert relerr(Ud, Us) < TOL
    assert lat.receipt()["deltaH_total"] == pytest.approx(ref.deltaH(Us), rel=TOL)


def test_full_config3_properties(amd, orc, monkeypatch):
    """BASELINE config 3 at full size (N=100k, D=768, k=32): size-independent properties + sampled-row parity."""
    monkeypatch.delenv("OSC_KNN_MODE", raising=False)  # the default build path is part of what is asserted
    rng = np.random.default_rng(0)
    N, D, k = 100_000, 768, 32
    Y = rng.standard_normal((N, D)).astype(np.float32)
    psi = Y[:32].mean(axis=0)
    psi = (psi / (np.linalg.norm(psi) + 1e-12)).astype(np.float32)
    lat = amd.Oscillink(Y, kneighbors=k, deterministic_k=True)
    # the default route at this size: the register-resident-panel prefilter (2); a handful of rows may fail the proof
    assert lat.build_info()["prefilter"] == 2 and lat.build_info()["fallback_rows"] <= 8
    rp, col, a, w, sd = lat.graph_csr()
    deg = np.diff(rp)
    assert deg.max() <= k and a.min() > 0
    rows = np.repeat(np.arange(N), deg)
    # symmetry: the multiset of (i,j,a) equals that of (j,i,a)
    fwd = np.lexsort((col, rows))
    bwd = np.lexsort((rows, col))
    assert np.array_equal(rows[fwd], col[bwd]) and np.array_equal(col[fwd], rows[bwd])
    assert np.array_equal(a[fwd], a[bwd])
    # W = A / (sd_i sd_j) with sd = sqrt(row sums of the capped adjacency) (graph.py:87-90)
    rs = np.bincount(rows, weights=a.astype(np.float64), minlength=N)
    assert np.allclose(sd, np.sqrt(np.maximum(rs, 1e-12)), rtol=1e-5)
    assert np.allclose(w, a / (sd[rows] * sd[col]), rtol=1e-5)
    # 4096 sampled rows: the top-k lists (members and similarities) equal the reference's arithmetic, sgemm row block by
    # row block; rows that differ may do so only by a rank-k near-tie, proven in float64 (tests/_fullsize.py)
    from tests._fullsize import check_graph_built_from_lists, check_knn_lists_on_sample, device_knn_lists

    idx, val = device_knn_lists(lat, N, k)
    near = check_knn_lists_on_sample(orc, Y, idx, val, rng.choice(N, size=4096, replace=False), k)
    assert near <= 2, near
    # ... and from those lists the mutual test, the max-symmetrisation, the row cap and the Laplacian weights of the
    # oracle give the device's A, W, sqrt_deg on all 100 000 rows (graph.py:60-93)
    check_graph_built_from_lists(orc, N, idx, val, (rp, col, a, w, sd))
    # settle: converges in the reference's 4-5 iterations, residual history strictly decreasing, deltaH >= 0
    lat.set_query(psi)
    st = lat.settle(max_iters=12, tol=1e-3)
    hist = lat.residual_history()
    assert 3 <= st["iters"] <= 6 and all(b < a_ for a_, b in zip(hist, hist[1:]))
    lat.set_receipt_detail("light")
    rec = lat.receipt()
    assert rec["deltaH_total"] >= -1e-3 and rec["meta"]["ustar_converged"]
    # linearity of the settle map in (U, Y, psi): settling 2x the inputs gives 2x the output (same graph)
    lat2 = amd.Oscillink(2.0 * Y, kneighbors=k, deterministic_k=True, _build_graph=False)
    lat2.set_graph_csr(rp, col, a)
    lat2.set_query(2.0 * psi)
    lat2.settle(max_iters=st["iters"], tol=0.0)
    lat.reset_U()
    lat.settle(max_iters=st["iters"], tol=0.0)
    assert relerr(lat2.U[:2000], 2.0 * lat.U[:2000]) < 1e-5


@pytest.mark.parametrize("N,D,k", [(700, 40, 48), (600, 36, 64), (500, 24, 100), (300, 20, 128)])
def test_wide_neighbor_lists_against_oracle(amd, orc, N, D, k):
    """k in (32, 64] uses two list entries per lane, k in (64, 128] the one-wave-per-SIMD variant; same graph,
    same solve as the oracle."""
    rng = np.random.default_rng(k)
    Y = rng.standard_normal((N, D)).astype(np.float32)
    psi = rng.standard_normal(D).astype(np.float32)
    ref = orc.OracleLattice(Y, kneighbors=k, deterministic_k=True)
    lat = amd.Oscillink(Y, kneighbors=k, deterministic_k=True)
    rp, col, a, w, sd = lat.graph_csr()
    r, c, wv = orc._edges(ref.A)
    assert np.array_equal(np.repeat(np.arange(N), np.diff(rp)), r) and np.array_equal(col, c)
    assert np.allclose(a, wv, rtol=1e-5)
    for L in (ref, lat):
        L.set_query(psi)
        L.add_chain([4, 9, 2, 7], lamP=0.3, weights=[1.0, 0.5, 2.0])
    a_ = ref.settle(tol=1e-4)
    b_ = lat.settle(tol=1e-4)
    assert a_["iters"] == b_["iters"] and relerr(lat.U, ref.U) < 2e-5
    assert lat.receipt()["deltaH_total"] == pytest.approx(ref.deltaH(), rel=TOL)


@pytest.mark.parametrize("N,D,k", [(400, 24, 129), (700, 40, 200), (301, 16, 1000), (9000, 32, 150)])
def test_kneighbors_above_128_against_oracle(amd, orc, N, D, k):
    """The reference takes any k <= N - 1 (lattice.py:60).  k > 128 leaves the register-resident lists for the dense
    similarity rows + radix select route (any N: the last case is past the small-lattice limit, the third clamps k to
    N - 1 = a complete graph before the mutual test)."""
    rng = np.random.default_rng(k)
    Y = rng.standard_normal((N, D)).astype(np.float32)
    psi = rng.standard_normal(D).astype(np.float32)
    ref = orc.OracleLattice(Y, kneighbors=k, deterministic_k=True, dense=False, knn_block=2048)
    lat = amd.Oscillink(Y, kneighbors=k, deterministic_k=True)
    assert lat._kneighbors == min(k, N - 1)
    rp, col, a, w, sd = lat.graph_csr()
    r, c, wv = orc._edges(ref.A)
    rows = np.repeat(np.arange(N), np.diff(rp))
    if rows.size == r.size and np.array_equal(rows, r) and np.array_equal(col, c):
        assert np.allclose(a, wv, rtol=1e-5)
    else:  # near-tie neighbour flips are legal (sgemm vs MFMA summation order, 81 M similarities at D = 32); bound them
        dev, cpu = set(zip(rows.tolist(), col.tolist())), set(zip(r.tolist(), c.tolist()))
        assert N >= 4096 and len(dev & cpu) / len(dev | cpu) > 1 - 1e-4
        R = ref.A.tocsr()
        lat.set_graph_csr(R.indptr.astype(np.int64), R.indices.astype(np.int32), R.data.astype(np.float32))
    for L in (ref, lat):
        L.set_query(psi)
    a_ = ref.settle(tol=1e-4)
    b_ = lat.settle(tol=1e-4)
    assert a_["iters"] == b_["iters"] and relerr(lat.U, ref.U) < 2e-5
    assert lat.receipt()["deltaH_total"] == pytest.approx(ref.deltaH(), rel=TOL)


def test_kneighbors_above_128_ties_go_to_the_smaller_index(amd, orc):
    """All rows identical: every similarity ties, so each list must hold the k smallest indices (graph.py:46-49)."""
    N, D, k = 300, 8, 140
    Y = np.tile(np.linspace(1.0, 2.0, D, dtype=np.float32), (N, 1))
    lat = amd.Oscillink(Y, kneighbors=k, deterministic_k=True)
    import ctypes as C

    from oscillink_amd import _native as nat

    idx = np.zeros((N, k), dtype=np.int32)
    ke = C.c_int32(0)
    lat._call("osc_get_knn_lists", nat.i32(idx), None, C.byref(ke))
    assert ke.value == k
    for i in (0, 1, 139, 140, 141, 299):
        want = [j for j in range(N) if j != i][:k]
        assert sorted(idx[i].tolist()) == want
    ref = orc.OracleLattice(Y, kneighbors=k, deterministic_k=True)
    rp, col, a, _, _ = lat.graph_csr()
    r, c, wv = orc._edges(ref.A)
    assert np.array_equal(np.repeat(np.arange(N), np.diff(rp)), r) and np.array_equal(col, c)


def test_config5_shape_gates_chain_properties(amd, orc):
    """BASELINE config 5 shape on one GPU (N=200k, D=1536, k=64, diffusion gates + chain): the lamQ diag term and the
    receipt breakdown at full size; kNN parity on 512 sampled rows against sgemm row blocks of the reference's arithmetic and,
    from the device's lists, the oracle's mutual test / cap / Laplacian weights against the device graph on every row."""
    rng = np.random.default_rng(5)
    N, D, k = 200_000, 1536, 64
    Y = rng.standard_normal((N, D)).astype(np.float32)
    psi = Y[:32].mean(axis=0)
    psi = (psi / (np.linalg.norm(psi) + 1e-12)).astype(np.float32)
    lat = amd.Oscillink(Y, kneighbors=k)
    # (round 4: D > 768 builds through the thresholds-and-hits prefilter on the tile core, k_tile_thr, half sweep)
    assert lat.build_info()["prefilter"] == 2 and lat.build_info()["fallback_rows"] <= 8
    rp, col, a, w, sd = lat.graph_csr()
    deg = np.diff(rp)
    assert deg.max() <= k and deg.min() >= 0 and a.min() > 0
    from tests._fullsize import check_graph_built_from_lists, check_knn_lists_on_sample, device_knn_lists

    idx, val = device_knn_lists(lat, N, k)
    near = check_knn_lists_on_sample(orc, Y, idx, val, rng.choice(N, size=512, replace=False), k, chunk=128)
    assert near <= 2, near
    check_graph_built_from_lists(orc, N, idx, val, (rp, col, a, w, sd))
    gates = amd.compute_diffusion_gates(Y, psi, kneighbors=k, gamma=0.15, method="cg", lattice=lat)
    assert gates.shape == (N,) and 0.0 <= gates.min() and gates.max() == 1.0 and gates.std() > 0
    lat.set_query(psi, gates=gates)
    lat.add_chain(list(range(8)), lamP=0.2)
    st = lat.settle(max_iters=12, tol=1e-3)
    hist = lat.residual_history()
    assert st["iters"] <= 8 and all(y < x for x, y in zip(hist, hist[1:]))
    lat.set_receipt_detail("full")
    rec = lat.receipt()
    assert rec["deltaH_total"] >= -1e-3 and rec["meta"]["ustar_converged"]
    assert rec["anchor_pen_sum"] > 0 and rec["query_term_sum"] > 0
    assert rec["meta"]["null_points_summary"]["total_null_points"] == len(rec["null_points"])
    # energy identity at the stationary point: with U = U*, deltaH = 0 exactly
    lat.U = lat.solve_Ustar()
    assert abs(lat.receipt()["deltaH_total"]) < 1e-6 * max(1.0, rec["anchor_pen_sum"])


def test_concurrent_lattices_on_threads(amd, orc):
    """The reference's service settles independent lattices on a thread pool (cloud/app/main.py:1030-1061): handles are
    independent (own stream, no shared mutable state), ctypes drops the GIL, results must not interfere."""
    import threading

    rng = np.random.default_rng(21)
    jobs = []
    for t in range(6):
        N, D, k = 300 + 50 * t, 24 + 8 * t, 5 + t
        Y = rng.standard_normal((N, D)).astype(np.float32)
        psi = rng.standard_normal(D).astype(np.float32)
        ref = orc.OracleLattice(Y, kneighbors=k, deterministic_k=True)
        ref.set_query(psi)
        ref.settle()
        jobs.append((Y, psi, k, ref.U, ref.last["iters"], ref.deltaH()))
    out = [None] * len(jobs)

    def work(i):
        Y, psi, k, *_ = jobs[i]
        for _ in range(5):  # repeat to overlap with the other threads
            lat = amd.Oscillink(Y, kneighbors=k, deterministic_k=True)
            lat.set_query(psi)
            st = lat.settle()
            out[i] = (lat.U.copy(), st["iters"], lat.receipt()["deltaH_total"])
            lat.close()

    threads = [threading.Thread(target=work, args=(i,)) for i in range(len(jobs))]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    for (Y, psi, k, U, iters, dH), got in zip(jobs, out):
        assert got is not None and got[1] == iters
        assert relerr(got[0], U) < 2e-5
        assert got[2] == pytest.approx(dH, rel=TOL)


def test_config4_shape_on_one_gpu(amd):
    """BASELINE config 4 shape (N=1M, D=384, k=16) on ONE GPU: size/indexing limits of the build and the solver
    (the 8-GPU run shards exactly these arrays by row block / column slab)."""
    rng = np.random.default_rng(4)
    N, D, k = 1_000_000, 384, 16
    Y = rng.standard_normal((N, D), dtype=np.float32)
    psi = Y[:32].mean(axis=0)
    psi = (psi / (np.linalg.norm(psi) + 1e-12)).astype(np.float32)
    lat = amd.Oscillink(Y, kneighbors=k)
    nnz, max_deg, build_ms = lat.graph_stats()
    assert 0 < nnz <= N * k and max_deg <= k
    rp, col, a, w, sd = lat.graph_csr()
    rows = np.repeat(np.arange(N), np.diff(rp))
    # symmetry on a sample of edges: (j, i) exists with the same weight
    pick = rng.choice(nnz, size=2000, replace=False)
    for e in pick[:200]:
        i, j = int(rows[e]), int(col[e])
        seg = col[rp[j]: rp[j + 1]]
        pos = np.searchsorted(seg, i)
        assert pos < seg.size and seg[pos] == i and a[rp[j] + pos] == a[e]
    # the neighbour lists of the panel route with column splits (6 K steps, D = 384), against the reference's arithmetic on
    # 512 sampled rows, and the graph built from them on all 1 000 000 rows
    from oracle import oscillink_oracle as orc
    from tests._fullsize import check_graph_built_from_lists, check_knn_lists_on_sample, device_knn_lists

    assert lat.build_info()["prefilter"] == 2
    idx, val = device_knn_lists(lat, N, k)
    near = check_knn_lists_on_sample(orc, Y, idx, val, rng.choice(N, size=512, replace=False), k, chunk=64)
    assert near <= 2, near
    check_graph_built_from_lists(orc, N, idx, val, (rp, col, a, w, sd))
    lat.set_query(psi)
    st = lat.settle(max_iters=12, tol=1e-3)
    hist = lat.residual_history()
    assert st["iters"] <= 8 and all(y < x for x, y in zip(hist, hist[1:]))
    lat.set_receipt_detail("light")
    rec = lat.receipt()
    assert rec["deltaH_total"] >= -1e-2 and rec["meta"]["ustar_converged"]
    print(f"config4 shape: build {build_ms:.0f} ms, nnz {nnz}, settle {st['t_ms']:.1f} ms / {st['iters']} it, "
          f"ustar {rec['meta']['ustar_solve_ms']:.1f} ms")


@pytest.mark.parametrize("N,D,k", [(2, 3, 1), (3, 1, 2), (5, 2, 4), (17, 7, 3), (64, 2500, 5), (40, 4100, 6)])
def test_tiny_and_very_wide_shapes(amd, orc, N, D, k, monkeypatch):
    """Smallest lattices (N = 2, 3, 5; D = 1, 2, 3: pitch padding) and D beyond one 2048-column launch window, on
    both CG paths."""
    rng = np.random.default_rng(N * 1000 + D)
    Y = rng.standard_normal((N, D)).astype(np.float32)
    psi = rng.standard_normal(D).astype(np.float32)
    ref = orc.OracleLattice(Y, kneighbors=k, deterministic_k=True)
    ref.set_query(psi)
    a_ = ref.settle(tol=1e-5, max_iters=30)
    # (the reference squeezes a single column to 1-D, solver.py:31,37; the product keeps (N, 1))
    ref.U = np.asarray(ref.U).reshape(N, D)
    dH = orc.deltaH_trace(ref.U, np.asarray(ref.solve_Ustar()).reshape(N, D), ref.M_mul)
    for small in ("1", "0"):
        monkeypatch.setenv("OSC_SMALL_PATH", small)
        lat = amd.Oscillink(Y, kneighbors=k, deterministic_k=True)
        assert np.allclose(lat.A, ref.A, rtol=1e-5, atol=1e-8)
        lat.set_query(psi)
        b_ = lat.settle(tol=1e-5, max_iters=30)
        assert a_["iters"] == b_["iters"], small
        assert relerr(lat.U, ref.U) < 2e-5, small
        assert lat.receipt()["deltaH_total"] == pytest.approx(dH, rel=TOL, abs=1e-6), small


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_random_operation_sequences_track_the_oracle(amd, orc, seed):
    """State-machine check: a seeded random sequence of the public calls (queries, gates, chains, lams, settles with
    every start mode, U* refreshes, receipts, graph rebuilds) is applied to the product and to the oracle; after every
    step the settled state, the iteration count and deltaH must agree.  Guards the host-side cache/invalidations."""
    rng = np.random.default_rng(100 + seed)
    N, D, k = int(rng.integers(40, 400)), int(rng.integers(3, 70)), int(rng.integers(2, 9))
    Y = rng.standard_normal((N, D)).astype(np.float32)
    ref = orc.OracleLattice(Y, kneighbors=k, deterministic_k=True)
    lat = amd.Oscillink(Y, kneighbors=k, deterministic_k=True)
    assert np.allclose(lat.A, ref.A, rtol=1e-5, atol=1e-8)
    lat.set_receipt_detail("light")
    for step in range(30):
        op = int(rng.integers(0, 9))
        if op == 0:
            psi = rng.standard_normal(D).astype(np.float32)
            ref.set_query(psi)
            lat.set_query(psi)
        elif op == 1:
            g = rng.uniform(0.0, 1.0, N).astype(np.float32)
            ref.set_gates(g)
            lat.set_gates(g)
        elif op == 2:
            chain = rng.integers(0, N, size=int(rng.integers(2, 7))).tolist()
            w = rng.uniform(0.2, 2.0, len(chain) - 1).tolist() if rng.random() < 0.5 else None
            lp = float(rng.choice([0.0, 0.2, 0.7]))
            ref.add_chain(chain, lamP=lp, weights=w)
            lat.add_chain(chain, lamP=lp, weights=w)
        elif op == 3:
            ref.clear_chain()
            lat.clear_chain()
        elif op == 4:
            lc, lq = float(rng.uniform(0.0, 1.5)), float(rng.uniform(0.0, 5.0))
            ref.lamC, ref.lamQ = lc, lq
            lat.lamC, lat.lamQ = lc, lq
        elif op == 5:
            kw = [dict(), dict(warm_start=False), dict(inertia=float(rng.uniform(0.1, 0.9))),
                  dict(dt=float(rng.uniform(0.2, 2.0))), dict(precond="none", max_iters=25),
                  dict(tol=1e-5, max_iters=40)][int(rng.integers(0, 6))]
            a_ = ref.settle(**kw)
            b_ = lat.settle(**kw)
            assert a_["iters"] == b_["iters"], (step, kw)
        elif op == 6:
            lat.refresh_Ustar()
        elif op == 7 and step % 3 == 0:
            k2 = int(rng.integers(2, 9))
            lat.rebuild_graph(kneighbors=k2)
            ref = _rebuild_oracle(orc, ref, k2)
        # every step ends with a receipt on both sides
        assert relerr(lat.U, ref.U) < 5e-5, (step, op)
        dH = ref.deltaH()
        got = lat.receipt()["deltaH_total"]
        assert got == pytest.approx(dH, rel=2e-4, abs=2e-4 * max(1.0, abs(dH))), (step, op)


def _rebuild_oracle(orc, old, k):
    new = orc.OracleLattice(old.Y, kneighbors=k, deterministic_k=True)
    new.U = old.U.copy()
    new.set_query(old.psi, gates=old.B_diag)
    new.lamG, new.lamC, new.lamQ = old.lamG, old.lamC, old.lamQ
    if old._chain_nodes is not None:
        new.A_path, new.W_path, new.L_path = old.A_path, old.W_path, old.L_path
        new.lamP, new._chain_nodes = old.lamP, old._chain_nodes
    return new


def _assert_edge_flips_are_near_ties(orc, Y, k, flipped):
    """Edges present in one lattice and absent in the other: for one endpoint of each, the k-th and (k+1)-th best
    similarities (float64) are within the fp32 summation noise of each other -- the row's list boundary is a near-tie."""
    Y64 = Y.astype(np.float64)
    Yn = Y64 / (np.linalg.norm(Y64, axis=1, keepdims=True) + 1e-12)
    for i, j in flipped:
        gaps = []
        for r in (i, j):
            s = Yn @ Yn[r]
            s[r] = -np.inf
            top = np.sort(s)[::-1]
            gaps.append(top[k - 1] - top[k] if k < len(top) - 1 else 0.0)
        assert min(gaps) < 1e-6, (i, j, gaps)


def test_random_shapes_prefilter_vs_exact_vs_oracle(amd, orc, monkeypatch):
    """Differential sweep over ragged shapes (N not a multiple of the 128-row tile, D not a multiple of 4/32/64, k across
    the list-width classes): the fp16-prefilter build, the all-fp32 build and (for the smaller ones) the oracle must
    produce the same lattice."""
    rng = np.random.default_rng(2024)
    shapes = [(int(rng.integers(2, 2600)), int(rng.integers(1, 260)), int(rng.integers(1, 66))) for _ in range(28)]
    shapes += [(129, 33, 32), (257, 65, 33), (1025, 31, 64), (4097, 20, 7), (640, 64, 80), (127, 5, 126)]
    for N, D, k in shapes:
        Y = rng.standard_normal((N, D)).astype(np.float32)
        graphs = {}
        for mode in ("prefilter", "exact"):
            monkeypatch.setenv("OSC_KNN_MODE", mode)
            lat = amd.Oscillink(Y, kneighbors=k, deterministic_k=True)
            graphs[mode] = lat.graph_csr()
            lat.close()
        a, b = graphs["prefilter"], graphs["exact"]
        same = np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        if not same:  # only a genuine near-tie (gap below fp32 summation noise) may differ between the two paths
            ea = set(zip(np.repeat(np.arange(N), np.diff(a[0])).tolist(), a[1].tolist()))
            eb = set(zip(np.repeat(np.arange(N), np.diff(b[0])).tolist(), b[1].tolist()))
            assert len(ea ^ eb) <= 4, (N, D, k, len(ea ^ eb))
            _assert_edge_flips_are_near_ties(orc, Y, k, ea ^ eb)
        else:
            assert np.allclose(a[2], b[2], rtol=2e-5, atol=1e-8), (N, D, k)
        if N <= 900:
            ref = orc.OracleLattice(Y, kneighbors=k, deterministic_k=True)
            r, c, w = orc._edges(ref.A)
            eo = set(zip(r.tolist(), c.tolist()))
            eb = set(zip(np.repeat(np.arange(N), np.diff(b[0])).tolist(), b[1].tolist()))
            assert len(eo ^ eb) <= 4, (N, D, k, len(eo ^ eb))


def _knn_sets(lat, N, k):
    import ctypes as C

    from oscillink_amd import _native as nat

    idx = np.zeros((N, k), dtype=np.int32)
    ke = C.c_int32(0)
    lat._call("osc_get_knn_lists", nat.i32(idx), None, C.byref(ke))
    assert ke.value == k
    return np.sort(idx, axis=1)


@pytest.mark.parametrize("N,D,k,kind", [(16500, 300, 16, "iid"), (20000, 600, 32, "iid"), (40000, 768, 64, "iid"),
                                        (16384, 384, 8, "iid"), (20000, 700, 32, "clustered"),
                                        (16400, 130, 24, "dups")])
def test_panel_prefilter_route_gives_the_exact_lists(amd, N, D, k, kind, monkeypatch):
    """The three device routes to the per-row top-k lists -- panel prefilter (register-resident query panel, sampled
    thresholds, appended hits; the planner's own choice from 6144 rows at D >= 512, 7168 at D >= 320 and 8193 otherwise;
    forced here), tile prefilter (in-kernel sorted lists) and the all-fp32 kernel -- on inputs that stress the panel
    route's assumptions: ragged N and D (both K depths, 6 and 12 steps), k up to 64 (keep 96: narrower sub-ranges in the
    select), tight clusters (thresholds near the top of the range, most rows fail the proof and are redone exactly) and
    exact duplicates (ties at the threshold).  A row may differ between routes only by a rank-k near-tie (gap below
    fp32 summation noise)."""
    rng = np.random.default_rng(N + D + k)
    if kind == "iid":
        Y = rng.standard_normal((N, D), dtype=np.float32)
    elif kind == "clustered":
        nc = N // 100
        Y = rng.standard_normal((nc, D), dtype=np.float32)[np.repeat(np.arange(nc), 100)][:N]
        Y = (Y + 0.35 * rng.standard_normal((N, D), dtype=np.float32)).astype(np.float32)
    else:  # every row appears 40 times: more exact ties than k
        base = rng.standard_normal((N // 40 + 1, D), dtype=np.float32)
        Y = base[np.arange(N) % base.shape[0]].copy()
    lists, info = {}, {}
    # "panel" is the default form of a single-process build: the symmetric half sweep (row block I visits the column tiles
    # J >= I only, every score tested against its row's and its column's threshold); "panel_full" the full sweep a sharded
    # build's ranks run (OSC_KNN_PANEL_SYM=0)
    for mode in ("panel", "panel_full", "prefilter", "exact"):
        monkeypatch.setenv("OSC_KNN_MODE", mode.split("_")[0])
        monkeypatch.setenv("OSC_KNN_PANEL_SYM", "0" if mode == "panel_full" else "1")
        lat = amd.Oscillink(Y, kneighbors=k, deterministic_k=True)
        info[mode] = lat.build_info()
        lists[mode] = (_knn_sets(lat, N, k), lat.graph_csr())
        lat.close()
    assert info["panel"]["prefilter"] == 2 and info["prefilter"]["prefilter"] == 1 and info["exact"]["prefilter"] == 0
    assert info["panel_full"]["prefilter"] == 2
    if kind == "dups":  # ties are broken by index in every route: the lattice must be identical
        for mode in ("panel", "panel_full"):
            assert np.array_equal(lists[mode][1][0], lists["exact"][1][0])
            assert np.array_equal(lists[mode][1][1], lists["exact"][1][1])
        return
    # In tight clusters the k-th and (k+1)-th neighbours are often within fp32 summation noise of each other.  Every row that
    # differs between two routes is recomputed in float64 and must be such a near-tie: the similarities of the members the
    # lists disagree on lie within the noise of one fp32 similarity (~sqrt(D) x 6e-8 x the partial sums: < 1e-6 at
    # similarities ~0.15, a few 1e-6 at the ~0.9 of the clustered case); the count is bounded as well.
    from tests._fullsize import near_tie_gap

    allowed = N // 200 if kind == "clustered" else max(8, N // 2000)
    gap_tol = 4e-6 if kind == "clustered" else 1e-6

    def prove(a, b, what):
        rows = np.nonzero((lists[a][0] != lists[b][0]).any(axis=1))[0]
        for r in rows:
            members = sorted(set(lists[a][0][r].tolist()) ^ set(lists[b][0][r].tolist()))
            gap = near_tie_gap(Y, int(r), members)
            assert gap < gap_tol, (what, int(r), members, gap)
        return int(rows.size)

    for mode in ("panel", "panel_full", "prefilter"):
        differ = prove(mode, "exact", mode)
        assert differ <= allowed, (mode, differ)
    differ = prove("panel", "panel_full", "half sweep vs full sweep")
    assert differ <= (allowed if kind == "clustered" else max(4, N // 4000)), differ
    # the two prefilter routes re-score with the same arithmetic; which rows they can prove (and which go to the exact
    # kernel instead) may differ in tight clusters
    differ = prove("panel", "prefilter", "panel vs prefilter")
    assert differ <= (allowed if kind == "clustered" else max(4, N // 4000)), differ
    if kind == "iid":
        assert info["panel"]["fallback_rows"] <= 8 and info["panel_full"]["fallback_rows"] <= 8


def test_panel_prefilter_on_anchors_that_arrive_grouped(amd, monkeypatch):
    """Anchors in cluster order (documents, topics): the 32 rows of a wave of the panel kernel would all have their
    ~cluster-size best columns in the same one or two column tiles, their shared hit list would overflow and every row
    would fall back to the exact kernel.  The prefilter therefore works on an image whose rows are scattered over the
    lattice rows (KnnPanelPlan::scatter); the lattice it delivers is the one of the unscattered build and of the exact
    route, and only the rows the proof cannot decide (tight clusters) are redone."""
    rng = np.random.default_rng(123)
    N, D, k, csize = 24000, 200, 24, 120
    centers = rng.standard_normal((N // csize, D)).astype(np.float32)
    Y = (centers[np.repeat(np.arange(N // csize), csize)] + 0.35 * rng.standard_normal((N, D))).astype(np.float32)
    out = {}
    for tag, mode, scatter in (("scatter", "panel", "1"), ("plain", "panel", "0"), ("exact", "exact", "1")):
        monkeypatch.setenv("OSC_KNN_MODE", mode)
        monkeypatch.setenv("OSC_KNN_PANEL_SCATTER", scatter)
        lat = amd.Oscillink(Y, kneighbors=k, deterministic_k=True)
        out[tag] = (lat.build_info(), _knn_sets(lat, N, k), lat.graph_csr())
        lat.close()
    assert out["scatter"][0]["prefilter"] == 2 and out["plain"][0]["prefilter"] == 2
    # unscattered: (almost) every row overflows into the fallback; scattered: a small fraction
    assert out["plain"][0]["fallback_rows"] > N // 2, out["plain"][0]
    assert out["scatter"][0]["fallback_rows"] < N // 10, out["scatter"][0]
    from tests._fullsize import near_tie_gap

    for tag in ("plain", "exact"):
        rows = np.nonzero((out["scatter"][1] != out[tag][1]).any(axis=1))[0]
        assert rows.size <= N // 200, (tag, rows.size)
        for r in rows:
            members = sorted(set(out["scatter"][1][r].tolist()) ^ set(out[tag][1][r].tolist()))
            assert near_tie_gap(Y, int(r), members) < 4e-6, (tag, int(r))


def test_internal_row_order_is_invisible(amd, orc, monkeypatch):
    """Clustered anchors in shuffled order: the automatic BFS re-order kicks in (sampled clustering coefficient), an
    i.i.d. lattice stays as it is, and every API result is identical to the run with re-ordering disabled."""
    rng = np.random.default_rng(77)
    N, D, k, C_ = 9000, 48, 12, 90
    centers = rng.standard_normal((C_, D)).astype(np.float32)
    Y = (centers[np.repeat(np.arange(C_), N // C_)] + 0.3 * rng.standard_normal((N, D))).astype(np.float32)
    Y = Y[rng.permutation(N)]
    psi = rng.standard_normal(D).astype(np.float32)
    gates = rng.uniform(0.1, 1.0, N).astype(np.float32)
    out = {}
    for mode in ("auto", "0"):
        if mode == "auto":
            monkeypatch.delenv("OSC_REORDER", raising=False)
        else:
            monkeypatch.setenv("OSC_REORDER", mode)
        lat = amd.Oscillink(Y, kneighbors=k, deterministic_k=True)
        bi = lat.build_info()
        assert bi["reordered"] == (1 if mode == "auto" else 0), bi
        lat.set_query(psi, gates=gates)
        lat.add_chain([5, 700, 4242, 8999, 12], lamP=0.3)
        st = lat.settle()
        rec = lat.receipt()
        out[mode] = (lat.graph_csr(), lat.U.copy(), st["iters"], rec["deltaH_total"], rec["coh_drop_sum"],
                     [n["edge"] for n in rec["null_points"]], lat._signature(), lat.Y.copy(), lat.sqrt_deg.copy())
    a, b = out["auto"], out["0"]
    for x, y in zip(a[0], b[0]):
        assert np.array_equal(x, y) if x.dtype.kind == "i" else np.allclose(x, y, rtol=1e-6)
    assert relerr(a[1], b[1]) < 1e-5 and a[2] == b[2]
    assert a[3] == pytest.approx(b[3], rel=1e-4) and a[4] == pytest.approx(b[4], rel=1e-4)
    assert a[5] == b[5] and a[6] == b[6]
    assert np.array_equal(a[7], Y) and np.array_equal(b[7], Y) and np.allclose(a[8], b[8], rtol=1e-6)
    iid = amd.Oscillink(rng.standard_normal((9000, 48)).astype(np.float32), kneighbors=k)
    assert iid.build_info()["reordered"] == 0 and iid.build_info()["clustering"] < 0.05


@pytest.mark.parametrize("name", ["c2_n1200_d128_k16", "g1_n400_d64_k6_chain8", "gates_chain_n333_d50_k7"])
@pytest.mark.parametrize("nb", ["1", "3", "96"])
def test_xcd_affine_slab_apply_matches_reference(amd, name, nb, monkeypatch):
    """OSC_SPMM_XS=1 forces the XCD-affine 32-column-slab operator apply (chosen automatically only for 32k..131k rows)
    onto the small fixtures, including a width that is not a multiple of 32 (D = 50) and a chain prior; OSC_SMALL_PATH=0
    keeps the general multi-launch CG in play.  Same fixtures, same tolerances, same iteration counts."""
    monkeypatch.setenv("OSC_SPMM_XS", "1")
    monkeypatch.setenv("OSC_XS_NB", nb)
    monkeypatch.setenv("OSC_SMALL_PATH", "0")
    case = load_case(name)
    rc = case["recipe"]
    Y, psi = make_inputs(rc)
    lat = amd.Oscillink(Y, kneighbors=rc["k"], deterministic_k=rc["deterministic"], _build_graph=False, **ctor_kwargs(rc))
    lat.set_graph_csr(*_csr_from_case(case))
    _configure(lat, case, rc, psi)
    info = lat.build_info()
    assert info["apply_launches"] == 1 and info["apply_xs_workgroups"] >= 1
    _check_solves(lat, case, rc, tol_u=2e-5)
    assert lat.build_info()["small_solves"] == 0


def test_xcd_affine_slab_apply_is_the_default_only_in_its_window(amd, monkeypatch):
    monkeypatch.delenv("OSC_SPMM_XS", raising=False)
    monkeypatch.delenv("OSC_REORDER", raising=False)  # a forced BFS order switches the mode off
    rng = np.random.default_rng(5)
    small = amd.Oscillink(rng.standard_normal((4096, 256)).astype(np.float32), kneighbors=8)
    assert small.build_info()["apply_xs_workgroups"] == 0  # too few rows: the gathered operand sits in cache anyway
    big = amd.Oscillink(rng.standard_normal((40000, 256)).astype(np.float32), kneighbors=8)
    bi = big.build_info()
    assert bi["apply_xs_workgroups"] > 0 and bi["apply_launches"] == 1
    psi = rng.standard_normal(256).astype(np.float32)
    big.set_query(psi)
    a = big.settle(max_iters=12, tol=1e-3)
    # the same lattice with the mode switched off: identical iteration count, states equal to fp32 reduction-order noise
    monkeypatch.setenv("OSC_SPMM_XS", "0")
    off = amd.Oscillink(big.Y, kneighbors=8)
    assert off.build_info()["apply_xs_workgroups"] == 0
    off.set_query(psi)
    b = off.settle(max_iters=12, tol=1e-3)
    assert a["iters"] == b["iters"]
    assert relerr(big.U, off.U) < 1e-5


@pytest.mark.parametrize("force_xs", ["0", "1"])
@pytest.mark.parametrize("world", [2, 3, 4])
def test_column_windows_of_a_sharded_solve_match_the_full_solve(amd, world, force_xs, monkeypatch):
    """OSC_FAKE_COL_SHARD=r/w gives a handle rank r's column window of a w-rank column-sharded solve (no communicator).
    With the stop test out of the way (tol = 0: every column runs max_iters iterations) each window must reproduce
    the same columns of the unsharded solve; with OSC_SPMM_XS=1 the windows run the XCD-affine slab apply with the
    slab-major search direction at a non-zero column offset."""
    from oscillink_amd.sharding import column_shard

    monkeypatch.setenv("OSC_SMALL_PATH", "0")
    monkeypatch.setenv("OSC_SPMM_XS", force_xs)
    rng = np.random.default_rng(21)
    N, D, k = 3000, 256, 12
    Y = rng.standard_normal((N, D)).astype(np.float32)
    psi = rng.standard_normal(D).astype(np.float32)
    gates = rng.uniform(0.2, 1.0, N).astype(np.float32)
    full = amd.Oscillink(Y, kneighbors=k, deterministic_k=True)
    full.set_query(psi, gates=gates)
    full.add_chain([5, 9, 2, 77, 1500], lamP=0.3)
    full.settle(max_iters=5, tol=0.0)
    Uf = full.U.copy()
    csr = full.graph_csr()
    for r in range(world):
        monkeypatch.setenv("OSC_FAKE_COL_SHARD", f"{r}/{world}")
        part = amd.Oscillink(Y, kneighbors=k, deterministic_k=True, _build_graph=False)
        part.set_graph_csr(csr[0], csr[1], csr[2])
        part.set_query(psi, gates=gates)
        part.add_chain([5, 9, 2, 77, 1500], lamP=0.3)
        st = part.settle(max_iters=5, tol=0.0)
        assert st["iters"] == 5
        c0, c1 = column_shard(D, r, world)
        assert relerr(part.U[:, c0:c1], Uf[:, c0:c1]) < 1e-5, (r, world)
        if force_xs == "1":
            assert part.build_info()["apply_xs_workgroups"] > 0
    monkeypatch.delenv("OSC_FAKE_COL_SHARD")


@pytest.mark.parametrize("name,ld", [("c2_n1200_d128_k16", "160"), ("gates_chain_n333_d50_k7", "64"),
                                     ("gates_chain_n333_d50_k7", "96"), ("g1_n400_d64_k6_chain8", "100")])
@pytest.mark.parametrize("small", ["0", "1"])
def test_padded_row_pitch_is_invisible(amd, name, ld, small, monkeypatch):
    """Large lattices get a 128-byte-aligned row pitch (ld > D); OSC_LD forces such a pitch onto the fixtures so every
    kernel, the strided host transfers and the row fetches run with ld != D.  Same answers, same iteration counts."""
    monkeypatch.setenv("OSC_LD", ld)
    monkeypatch.setenv("OSC_SMALL_PATH", small)
    case = load_case(name)
    rc = case["recipe"]
    Y, psi = make_inputs(rc)
    lat = amd.Oscillink(Y, kneighbors=rc["k"], deterministic_k=rc["deterministic"], **ctor_kwargs(rc))
    assert np.array_equal(lat.Y, Y) and np.array_equal(lat.U, Y)
    rows = np.array([0, Y.shape[0] - 1, 7], dtype=np.int32)
    assert np.array_equal(lat._fetch_rows(1, rows), Y[rows])
    _configure(lat, case, rc, psi)
    _check_solves(lat, case, rc, tol_u=TOL)
    # (a padded pitch never reaches the one-launch kernel, whatever OSC_SMALL_PATH says: tests/test_gpu_small_solve.py has it)
    assert lat.build_info()["small_solves"] == 0
    if rc["chain"]:
        lat.chain_receipt(list(rc["chain"]))
    assert len(lat.bundle(k=5)) == 5


@pytest.mark.parametrize("name", ["c2_n1200_d128_k16", "g1_n400_d64_k6_chain8"])
@pytest.mark.parametrize("nb", ["2", "5", "16"])
def test_source_blocked_apply_matches_reference(amd, name, nb, monkeypatch):
    """OSC_SPMM_BLOCKED=n forces the source-blocked CG matvec (chosen automatically only when the 32-column slab does not
    fit an XCD's L2) onto fixtures, on top of the forced XCD-affine slabs it builds on; OSC_SMALL_PATH=0 keeps the general
    multi-launch CG in play.  The second fixture has a chain prior (the fix-up launch behind every blocked apply).  Same
    fixtures, same tolerances, same iteration counts as every other path."""
    monkeypatch.setenv("OSC_SPMM_XS", "1")
    monkeypatch.setenv("OSC_SPMM_BLOCKED", nb)
    monkeypatch.setenv("OSC_SMALL_PATH", "0")
    case = load_case(name)
    rc = case["recipe"]
    Y, psi = make_inputs(rc)
    lat = amd.Oscillink(Y, kneighbors=rc["k"], deterministic_k=rc["deterministic"], _build_graph=False, **ctor_kwargs(rc))
    lat.set_graph_csr(*_csr_from_case(case))
    _configure(lat, case, rc, psi)
    _check_solves(lat, case, rc, tol_u=2e-5)
    info = lat.build_info()
    assert info["apply_src_blocks"] == int(nb) and info["blocked_applies"] > 0 and info["small_solves"] == 0


@pytest.mark.parametrize("name", PARAM_CASES)
@pytest.mark.parametrize("path", ["general", "blocked"])
def test_constructor_parameter_fixtures_on_the_multi_kernel_paths(amd, name, path, monkeypatch):
    """The round-5 fixtures (row_cap_val 0.25 / 1e6 / 0.5, lamG 0.3 / 2.5, lamC 0 / 0.7 / 2, lamQ 0 / 1.5: tests/golden/
    make_golden.py, generated by the reference) through the paths config 3 runs: OSC_SMALL_PATH=0 keeps the one-launch
    solve out, "blocked" also forces XCD-affine slabs and the source-blocked matvec (whose epilogue folds lamG, lamQ B and
    the Jacobi diagonal into cs_const / cs_B -- exactly where a zero lambda would show).  Device-built graph: the cap
    kernels (k_row_scale / k_apply_cap) below 1, inactive, and at 0.5 against the reference's adjacency."""
    monkeypatch.setenv("OSC_SMALL_PATH", "0")
    if path == "blocked":
        monkeypatch.setenv("OSC_SPMM_XS", "1")
        monkeypatch.setenv("OSC_SPMM_BLOCKED", "3")
        monkeypatch.setenv("OSC_LD", "64")  # (the slab-major search direction needs a pitch of whole 32-column slabs; D = 48 / 40)
    case = load_case(name)
    rc = case["recipe"]
    Y, psi = make_inputs(rc)
    lat = amd.Oscillink(Y, kneighbors=rc["k"], deterministic_k=rc["deterministic"], **ctor_kwargs(rc))
    rowptr, col, a, w, sd = lat.graph_csr()
    assert np.array_equal(rowptr, case["indptr"]) and np.array_equal(col, case["indices"])
    assert np.allclose(a, case["A_data"], rtol=1e-5, atol=1e-8) and np.allclose(sd, case["sqrt_deg"], rtol=1e-5)
    if "row_cap_val" in rc and rc["row_cap_val"] >= 1e5:  # cap inactive: every scale is exactly 1 (graph.py:76-80)
        monkeypatch.setenv("OSC_SPMM_BLOCKED", "0")
        raw = amd.Oscillink(Y, kneighbors=rc["k"], deterministic_k=rc["deterministic"], row_cap_val=3.0e38)
        assert np.array_equal(raw.graph_csr()[2], a)
        raw.close()
    _configure(lat, case, rc, psi)
    _check_solves(lat, case, rc, tol_u=2e-5)
    info = lat.build_info()
    assert info["small_solves"] == 0 and info["apply_src_blocks"] == (3 if path == "blocked" else 0)


def test_rebuild_graph_with_another_cap_against_the_oracle(amd, orc):
    """rebuild_graph(row_cap_val=...) (lattice.py:760-801): the cap kernels run again on the handle's lattice; adjacency,
    sqrt_deg and the solves that follow equal the oracle's for the new cap, and going back to cap 1.0 restores the first
    graph bit for bit."""
    rng = np.random.default_rng(21)
    N, D, k = 700, 64, 10
    Y = rng.standard_normal((N, D)).astype(np.float32)
    psi = rng.standard_normal(D).astype(np.float32)
    gates = rng.uniform(0.0, 1.0, N).astype(np.float32)
    lat = amd.Oscillink(Y, kneighbors=k, deterministic_k=True, lamG=0.8, lamC=1.3, lamQ=0.0)
    first = [x.copy() for x in lat.graph_csr()]
    for cap in (0.3, 1e6, 2.0, 1.0):
        lat.rebuild_graph(row_cap_val=cap)
        lat.set_query(psi, gates=gates)
        lat.reset_U()
        ref = orc.OracleLattice(Y, kneighbors=k, deterministic_k=True, row_cap_val=cap, lamG=0.8, lamC=1.3, lamQ=0.0, dense=False)
        ref.set_query(psi, gates=gates)
        rowptr, col, a, w, sd = lat.graph_csr()
        r, c, wa = orc._edges(ref.A)
        assert np.array_equal(col, c) and np.allclose(a, wa, rtol=1e-5, atol=1e-9) and np.allclose(sd, ref.sqrt_deg, rtol=1e-5)
        st, rs = lat.settle(max_iters=12, tol=1e-4), ref.settle(max_iters=12, tol=1e-4)
        assert st["iters"] == rs["iters"] and relerr(lat.U, ref.U) < 2e-5
        Us, Ur = lat.solve_Ustar(), ref.solve_Ustar()
        assert lat.last_ustar["iters"] == ref.last_ustar["iters"] and relerr(Us, Ur) < 2e-5
    again = lat.graph_csr()
    assert all(np.array_equal(x, y) for x, y in zip(first, again))


@pytest.mark.parametrize("shape", ["0", "1", "2", "3", "4", "5", "6"])
def test_blocked_apply_kernel_shapes_against_the_plain_one(amd, shape, monkeypatch):
    """OSC_BLK_VARIANT forces one kernel shape of the blocked matvec (cg_kernels.hip: kBlkShapes; 0 = two workgroups per CU,
    one gather round in flight, tests per group; 1-6 = one workgroup per CU, four rounds in flight, 8 / 12 / 16 / 20 / 24 /
    28 test-free groups per wave -- chosen by geometry from N = 96k on; a 36 000-row lattice needs three destination slices
    under the 8-group shape and fills only part of the larger ones' groups, which exercises the padding).  Settle, U* solve, a chain prior (fix-up launch) and ragged shapes (N not a multiple of the
    row groups, D = 200: a partial last slab): same iteration counts, states equal to summation-order noise."""
    monkeypatch.delenv("OSC_SPMM_XS", raising=False)
    monkeypatch.delenv("OSC_REORDER", raising=False)
    rng = np.random.default_rng(5)
    N, D, k = 36001, 200, 20
    Y = rng.standard_normal((N, D)).astype(np.float32)
    psi = rng.standard_normal(D).astype(np.float32)
    gates = rng.uniform(0.1, 1.0, N).astype(np.float32)
    res = {}
    for mode in ("plain", "blocked"):
        monkeypatch.setenv("OSC_SPMM_BLOCKED", "0" if mode == "plain" else "6")
        monkeypatch.setenv("OSC_BLK_VARIANT", shape)
        lat = amd.Oscillink(Y, kneighbors=k)
        lat.set_query(psi, gates=gates)
        st = lat.settle(max_iters=12, tol=1e-4)
        U1 = lat.U.copy()
        Us = lat.solve_Ustar().copy()
        it_us = lat.last_ustar["iters"]
        lat.add_chain([5, 1, 36000, 18000, 7, 2], lamP=0.3)
        lat.reset_U()
        st2 = lat.settle(max_iters=12, tol=1e-4)
        info = lat.build_info()
        if mode == "blocked":
            assert info["apply_src_blocks"] == 6 and info["apply_blocked_shape"] == int(shape), info
        else:
            assert info["apply_src_blocks"] == 0, info
        res[mode] = (st["iters"], U1, Us, it_us, st2["iters"], lat.U.copy())
        lat.close()
    a, b = res["plain"], res["blocked"]
    assert a[0] == b[0] and a[3] == b[3] and a[4] == b[4]
    assert relerr(b[1], a[1]) < 1e-6 and relerr(b[2], a[2]) < 1e-6 and relerr(b[5], a[5]) < 1e-6


def test_deltaH_through_the_blocked_matvec_against_the_plain_apply_and_the_oracle(amd, orc, monkeypatch):
    """receipts.py:10-25 (deltaH_trace = sum (U - U*) . M (U - U*)).  Where the blocked matvec serves the lattice, osc_deltaH takes
    its column sums of x . (M x) (osc_api.hip: quad_form_of_difference -> osc_solve.hip: blocked_quad_form) instead of the
    plain apply's DOT form: same value to summation-order noise, with and without a chain prior (the fix-up launch adds its
    rows' partial sums), and within 1e-4 of the sparse oracle on the device-built graph."""
    monkeypatch.delenv("OSC_SPMM_XS", raising=False)
    monkeypatch.delenv("OSC_REORDER", raising=False)
    rng = np.random.default_rng(9)
    N, D, k = 36001, 200, 20
    Y = rng.standard_normal((N, D)).astype(np.float32)
    psi = rng.standard_normal(D).astype(np.float32)
    psi /= np.linalg.norm(psi)
    gates = rng.uniform(0.1, 1.0, N).astype(np.float32)
    chain = [5, 1, 36000, 18000, 7, 2]
    got = {}
    for mode in ("plain", "blocked"):
        monkeypatch.setenv("OSC_SPMM_BLOCKED", "0" if mode == "plain" else "6")
        lat = amd.Oscillink(Y, kneighbors=k)
        lat.set_query(psi, gates=gates)
        lat.settle(max_iters=3, tol=1e-9)  # (a state well away from U*: the difference is not rounding noise)
        lat.refresh_Ustar()
        before = lat.build_info()["blocked_applies"]
        dh = lat.receipt()["deltaH_total"]
        used = lat.build_info()["blocked_applies"] - before
        lat.add_chain(chain, lamP=0.3)
        lat.refresh_Ustar()
        dh_chain = lat.receipt()["deltaH_total"]
        if mode == "blocked":
            assert used >= 1, "deltaH did not take the blocked matvec"
            rowptr, col, A, W, sd = lat.graph_csr()
            U, Us = lat.U.copy(), lat.solve_Ustar().copy()
            import scipy.sparse as sp
            Wm = sp.csr_matrix((W, col, rowptr), shape=(N, N))
            Wp, _ = orc.normalized_laplacian(orc.path_adjacency(N, chain, dense=False))  # graph.py:96-111: I - Wp over all N rows
            f32 = np.float32

            def M_mul(X):  # lattice.py:173-182 / receipts.py:21-25 on the device-built graph
                return (f32(lat.lamG) * X + f32(lat.lamC) * (X - Wm @ X) + f32(lat.lamQ) * gates[:, None] * X
                        + f32(0.3) * (X - Wp @ X)).astype(f32)

            want = orc.deltaH_trace(U, Us, M_mul)
            assert abs(dh_chain - want) <= 1e-4 * abs(want), (dh_chain, want)
        else:
            assert used == 0
        got[mode] = (dh, dh_chain)
        lat.close()
    for a, b in zip(got["plain"], got["blocked"]):
        assert abs(a - b) <= 2e-6 * abs(a), got


def test_source_blocked_apply_against_the_plain_one(amd, orc, monkeypatch):
    """A lattice inside the automatic window (N = 40000, D = 256: slab 5 MB) with random gates: the blocked matvec and the
    plain one give the same iteration count and the same state to fp32 summation-order noise; rows with more than
    OSC_BLK_SLOTS edges into one block move to other blocks' slots and, with only 2 blocks at k = 24, to the epilogue
    list; a chain prior adds the fix-up launch; a rebuilt graph rebuilds the block-major copy."""
    monkeypatch.delenv("OSC_SPMM_XS", raising=False)
    monkeypatch.delenv("OSC_REORDER", raising=False)
    rng = np.random.default_rng(77)
    N, D, k = 40000, 256, 24
    Y = rng.standard_normal((N, D)).astype(np.float32)
    psi = rng.standard_normal(D).astype(np.float32)
    gates = rng.uniform(0.1, 1.0, N).astype(np.float32)
    out = {}
    for mode in ("0", "2", "3", "7"):
        monkeypatch.setenv("OSC_SPMM_BLOCKED", mode)
        lat = amd.Oscillink(Y, kneighbors=k)
        lat.set_query(psi, gates=gates)
        st = lat.settle(max_iters=12, tol=1e-4)
        info = lat.build_info()
        assert info["apply_src_blocks"] == int(mode), info
        out[mode] = (st["iters"], st["res"], lat.U.copy())
        if mode == "3":
            lat.add_chain([3, 1, 4, 15, 9, 2, 6, 39999, 20000], lamP=0.25)  # chain prior: blocked apply + fix-up launch
            lat.reset_U()
            st2 = lat.settle(max_iters=12, tol=1e-4)
            assert lat.build_info()["apply_src_blocks"] == 3
            monkeypatch.setenv("OSC_SPMM_BLOCKED", "0")
            pl = amd.Oscillink(Y, kneighbors=k)
            pl.set_query(psi, gates=gates)
            pl.add_chain([3, 1, 4, 15, 9, 2, 6, 39999, 20000], lamP=0.25)
            st2p = pl.settle(max_iters=12, tol=1e-4)
            assert pl.build_info()["apply_src_blocks"] == 0
            assert st2["iters"] == st2p["iters"] and relerr(lat.U, pl.U) < 1e-6
            pl.close()
            monkeypatch.setenv("OSC_SPMM_BLOCKED", "3")
            lat.clear_chain()
            lat.rebuild_graph(kneighbors=8)  # new graph: the block-major copy must follow
            lat.reset_U()
            st3 = lat.settle(max_iters=12, tol=1e-4)
            assert lat.build_info()["apply_src_blocks"] == 3
            monkeypatch.setenv("OSC_SPMM_BLOCKED", "0")
            ref = amd.Oscillink(Y, kneighbors=8)
            ref.set_query(psi, gates=gates)
            st4 = ref.settle(max_iters=12, tol=1e-4)
            assert st3["iters"] == st4["iters"] and relerr(lat.U, ref.U) < 1e-6
        lat.close()
    for mode in ("2", "3", "7"):
        assert out[mode][0] == out["0"][0]
        assert out[mode][1] == pytest.approx(out["0"][1], rel=1e-3)
        assert relerr(out[mode][2], out["0"][2]) < 1e-6, mode
    # and against the oracle on the device-built graph
    monkeypatch.setenv("OSC_SPMM_BLOCKED", "0")
    lat = amd.Oscillink(Y, kneighbors=k)
    import scipy.sparse as sp
    from tests._fullsize import oracle_solves, stop_iteration

    rp, col, a, w, sd = lat.graph_csr()
    A = sp.csr_matrix((a, col, rp), shape=(N, N), dtype=np.float32)
    ref = oracle_solves(orc, Y, psi, A, k=k, gates=gates, settle_iters=out["3"][0], settle_tol=1e-4, ustar_iters=8)
    assert stop_iteration(ref["hist_settle"], 1e-4) == out["3"][0]
    assert relerr(out["3"][2], ref["U"]) < 1e-5


def test_inertia_and_cold_starts_on_the_blocked_path(amd, orc, monkeypatch):
    """settle(inertia > 0) builds x0 = (1 - w) Y + w U in the A p work array; the blocked initial residual writes A x0 there
    before its elementwise tail has read x0, so such a solve must keep the gathering INIT kernel (an earlier version returned
    A x0-started iterates).  Warm, inertia and cold starts on the blocked path against the plain path and the sparse oracle
    (lattice.py:751-758)."""
    import scipy.sparse as sp

    monkeypatch.delenv("OSC_SPMM_XS", raising=False)
    monkeypatch.delenv("OSC_REORDER", raising=False)
    rng = np.random.default_rng(31)
    N, D, k = 20000, 256, 12
    Y = rng.standard_normal((N, D)).astype(np.float32)
    psi = rng.standard_normal(D).astype(np.float32)
    seq = [dict(max_iters=2, tol=1e-9), dict(inertia=0.4, max_iters=12, tol=1e-4), dict(inertia=1.0, max_iters=3, tol=1e-9),
           dict(warm_start=False, max_iters=12, tol=1e-4), dict(inertia=0.7, max_iters=12, tol=1e-5)]
    runs = {}
    for mode in ("0", "-1"):
        monkeypatch.setenv("OSC_SPMM_BLOCKED", mode)
        lat = amd.Oscillink(Y, kneighbors=k)
        lat.set_query(psi)
        runs[mode] = []
        for kw in seq:
            st = lat.settle(**kw)
            runs[mode].append((st["iters"], st["res"], lat.U.copy()))
        assert (lat.build_info()["apply_src_blocks"] > 0) == (mode == "-1")
        if mode == "0":
            rp, col, a, w, sd = lat.graph_csr()
        lat.close()
    ref = orc.OracleLattice(Y, kneighbors=k, dense=False, graph=sp.csr_matrix((a, col, rp), shape=(N, N), dtype=np.float32))
    ref.set_query(psi)
    for i, kw in enumerate(seq):
        rs = ref.settle(**kw)
        for mode in ("0", "-1"):
            it, res, U = runs[mode][i]
            assert it == rs["iters"], (mode, kw)
            assert relerr(U, ref.U) < 2e-6, (mode, kw, relerr(U, ref.U))


def test_block_major_graph_copy_equals_the_placement_rule(amd, monkeypatch):
    """The device's block-major copy of the graph (k_blk_count / k_blk_fill) against the placement rule restated here -- the
    same rule oscillink_amd/csrc/host_logic.hpp: blk_place_row models and tests/host_logic sweeps under the sanitizers: an
    edge sits in the slot row of its own block while that has room, else in the first later block (cyclically) with room
    behind that block's own edges, else in the overflow list; fillers point at their block's first row with weight 0."""
    import ctypes as C

    from oscillink_amd import _native as nat

    monkeypatch.setenv("OSC_REORDER", "0")  # (the diagnostic reads the copy in the device's row order: keep that the API's)
    rng = np.random.default_rng(8)
    N, D, k, SL = 5000, 32, 40, 4
    Y = rng.standard_normal((N, D)).astype(np.float32)
    lat = amd.Oscillink(Y, kneighbors=k)
    rp, col, a, w, sd = lat.graph_csr()
    for nb in (1, 2, 5, 9, 24, 32):
        sc = np.zeros((nb, N, SL), dtype=np.int32)
        sw = np.zeros((nb, N, SL), dtype=np.float32)
        of = np.zeros(N, dtype=np.int32)
        oc = np.zeros(N, dtype=np.int32)
        cap = int(len(col))
        ocol = np.zeros(cap, dtype=np.int32)
        ow = np.zeros(cap, dtype=np.float32)
        lat._call("osc_get_blocked_copy", nb, nat.i32(sc), nat.f32(sw), nat.i32(of), nat.i32(oc), nat.i32(ocol), nat.f32(ow), cap)
        rpb = (N + nb - 1) // nb
        for i in rng.choice(N, size=400, replace=False):
            cols, ws = col[rp[i]:rp[i + 1]], w[rp[i]:rp[i + 1]]
            blk = np.minimum(nb - 1, cols // rpb)
            cnt = np.bincount(blk, minlength=nb)
            tail = np.minimum(cnt, SL)
            want_c = np.empty((nb, SL), dtype=np.int32)
            want_w = np.zeros((nb, SL), dtype=np.float32)
            want_c[:] = np.minimum(N - 1, np.arange(nb) * rpb)[:, None]
            seen = np.zeros(nb, dtype=int)
            over = []
            for cj, wj, b in zip(cols, ws, blk):
                kb = seen[b]
                seen[b] += 1
                if kb < SL:
                    want_c[b, kb], want_w[b, kb] = cj, wj
                    continue
                for step in range(1, nb):
                    q = (b + step) % nb
                    if tail[q] < SL:
                        want_c[q, tail[q]], want_w[q, tail[q]] = cj, wj
                        tail[q] += 1
                        break
                else:
                    over.append((cj, wj))
            assert np.array_equal(sc[:, i, :], want_c) and np.array_equal(sw[:, i, :], want_w), (nb, int(i))
            assert oc[i] == len(over)
            got = list(zip(ocol[of[i]:of[i] + oc[i]].tolist(), ow[of[i]:of[i] + oc[i]].tolist()))
            assert got == [(int(c_), float(w_)) for c_, w_ in over], (nb, int(i))


def test_source_blocked_apply_when_the_last_slice_runs_far_past_the_lattice(amd, monkeypatch):
    """N = 130000 takes three destination slices whose capacity exceeds N by several thousand rows: row groups that start
    past the lattice must be skipped by the list copy and by the gathers alike (an earlier version read the block-major
    copy out of bounds there).  Also N just below / above multiples of the per-slice capacity."""
    monkeypatch.delenv("OSC_SPMM_XS", raising=False)
    monkeypatch.delenv("OSC_REORDER", raising=False)
    rng = np.random.default_rng(99)
    for N in (130000, 57345, 114700):
        D, k = 128, 8
        Y = rng.standard_normal((N, D)).astype(np.float32)
        psi = rng.standard_normal(D).astype(np.float32)
        res = {}
        for mode in ("0", "-1"):
            monkeypatch.setenv("OSC_SPMM_BLOCKED", mode)
            lat = amd.Oscillink(Y, kneighbors=k)
            lat.set_query(psi)
            st = lat.settle(max_iters=12, tol=1e-4)
            res[mode] = (st["iters"], lat.U.copy(), lat.build_info()["apply_src_blocks"])
            lat.close()
        assert res["0"][2] == 0 and res["-1"][2] >= 2
        assert res["0"][0] == res["-1"][0] and relerr(res["-1"][1], res["0"][1]) < 1e-6


@pytest.mark.parametrize("kind", ["hub", "powerlaw", "banded", "empty_rows"])
def test_source_blocked_apply_on_injected_degenerate_graphs(amd, kind, monkeypatch):
    """Graphs the kNN build never produces, injected as CSR and pushed through the blocked matvec with 2, 7 and 16 source
    blocks: a hub row that neighbours 120 others (far more edges into one block than a slot row holds: the overflow
    lists), power-law degrees, a banded graph (every edge inside the row's own block), and a graph where most rows
    have no edge at all.  State and iteration count must equal the plain apply's."""
    import scipy.sparse as sp

    monkeypatch.setenv("OSC_SPMM_XS", "1")
    monkeypatch.setenv("OSC_SMALL_PATH", "0")
    rng = np.random.default_rng(1234)
    N, D = 6000, 64
    if kind == "hub":
        rows = np.concatenate([np.full(120, 17), rng.integers(0, N, 4000)])
        cols = np.concatenate([rng.choice(np.setdiff1d(np.arange(N), [17]), 120, replace=False), rng.integers(0, N, 4000)])
    elif kind == "powerlaw":
        deg = np.minimum(100, (rng.pareto(1.2, N) + 1).astype(int))
        rows = np.repeat(np.arange(N), deg)
        cols = rng.integers(0, N, rows.size)
    elif kind == "banded":
        rows = np.repeat(np.arange(N), 6)
        cols = np.clip(rows + np.tile([-3, -2, -1, 1, 2, 3], N), 0, N - 1)
    else:
        rows = rng.integers(0, 300, 2000)
        cols = rng.integers(0, N, 2000)
    keep = rows != cols
    A = sp.coo_matrix((rng.uniform(0.05, 1.0, keep.sum()).astype(np.float32), (rows[keep], cols[keep])), shape=(N, N)).tocsr()
    A = A.maximum(A.T).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    if A.getnnz(axis=1).max() > 128:
        pytest.skip("row wider than the ELL limit of the injection path")
    Y = rng.standard_normal((N, D)).astype(np.float32)
    psi = rng.standard_normal(D).astype(np.float32)
    gates = rng.uniform(0.1, 1.0, N).astype(np.float32)
    out = {}
    for mode in ("0", "2", "7", "16"):
        monkeypatch.setenv("OSC_SPMM_BLOCKED", mode)
        lat = amd.Oscillink(Y, kneighbors=6, _build_graph=False)
        lat.set_graph_csr(A.indptr.astype(np.int64), A.indices.astype(np.int32), A.data.astype(np.float32))
        lat.set_query(psi, gates=gates)
        st = lat.settle(max_iters=16, tol=1e-5)
        Us = lat.solve_Ustar()
        assert lat.build_info()["apply_src_blocks"] == int(mode)
        out[mode] = (st["iters"], lat.U.copy(), Us.copy())
        lat.close()
    for mode in ("2", "7", "16"):
        assert out[mode][0] == out["0"][0], (kind, mode)
        assert relerr(out[mode][1], out["0"][1]) < 1e-6 and relerr(out[mode][2], out["0"][2]) < 1e-6, (kind, mode)


@pytest.mark.parametrize("path", ["plain", "slab", "blocked"])
def test_deferred_x_update_leaves_the_same_state_at_every_stop_point(amd, path, monkeypatch):
    """run_cg applies iteration it's x += alpha p inside iteration it + 1's p update (or in a kernel of its own behind an
    iteration that has no successor enqueued); OSC_X_DEFER=0 is the loop with the x update next to the r update.  The
    arithmetic per element is the same, so states, residual histories and iteration counts must be bit-identical --
    whatever the stop point is relative to the iteration count the handle guesses from its previous solve of that kind:
    convergence at the guess, before it (under a speculative iteration), after it, and max_iters without convergence."""
    monkeypatch.setenv("OSC_SMALL_PATH", "0")
    monkeypatch.delenv("OSC_REORDER", raising=False)
    if path == "plain":
        monkeypatch.setenv("OSC_SPMM_XS", "0")
    else:
        monkeypatch.setenv("OSC_SPMM_XS", "1")
        monkeypatch.setenv("OSC_SPMM_BLOCKED", "3" if path == "blocked" else "0")
    rng = np.random.default_rng(77)
    N, D, k = 3100, 96, 12
    Y = rng.standard_normal((N, D), dtype=np.float32)
    psi = (Y[:7].mean(0) / np.linalg.norm(Y[:7].mean(0))).astype(np.float32)

    def run(defer):
        monkeypatch.setenv("OSC_X_DEFER", defer)
        lat = amd.Oscillink(Y, kneighbors=k)
        lat.set_query(psi)
        lat.add_chain([3, 40, 41, 900], lamP=0.3)
        out = []
        for tol, max_iters, inertia in ((1e-3, 12, 0.0), (1e-3, 12, 0.0), (1e-6, 40, 0.0), (1e-2, 12, 0.3), (1e-7, 3, 0.0),
                                        (1e-3, 1, 0.0), (1e-3, 12, 0.0)):
            lat.reset_U()
            st = dict(lat.settle(max_iters=max_iters, tol=tol, inertia=inertia))
            out.append((st["iters"], lat.residual_history(), lat.U.copy()))
            us = lat.solve_Ustar(tol=tol, max_iters=max_iters, use_cache=False).copy()
            out.append((lat.last_ustar["iters"], lat.residual_history(), us))
        lat.close()
        return out

    a = run("1")  # deferred, and the expected last iteration in its own form (x finished there, r not stored)
    assert len({x[0] for x in a}) >= 4
    for other in ("2", "0"):  # deferred without that form; not deferred
        for (ia, ha, Ua), (ib, hb, Ub) in zip(a, run(other)):
            assert ia == ib and ha == hb
            assert np.array_equal(Ua, Ub)


@pytest.mark.parametrize("N,D,k", [(18000, 320, 16), (18000, 600, 16), (33000, 768, 40)])
def test_panel_planner_overrides_give_the_same_lattice(amd, monkeypatch, N, D, k):
    """OSC_KNN_PANEL_T / _RHO / _NRG move the half sweep's chunk length, the sample density of the thresholds and the row
    groups per wave; the lattice is the one of the planner's own choice (and of the exact route) whatever they say.
    Round 6: K depth 12 (384 < D <= 768) with TWO row groups -- k_panel<12,1,2,true>, 64-column passes, pair-form coarse
    entries -- forced here at sizes where the planner would keep one (it takes two from 720 row blocks on)."""
    rng = np.random.default_rng(5)
    Y = rng.standard_normal((N, D), dtype=np.float32)
    monkeypatch.setenv("OSC_KNN_MODE", "panel")
    want = None
    for env in ({}, {"OSC_KNN_PANEL_T": "4"}, {"OSC_KNN_PANEL_RHO": "16"}, {"OSC_KNN_PANEL_NRG": "1"}, {"OSC_KNN_PANEL_RANK": "12"},
                {"OSC_KNN_PANEL_NRG": "2"}, {"OSC_KNN_PANEL_NRG": "2", "OSC_KNN_PANEL_T": "6"},
                {"OSC_KNN_PANEL_NRG": "1", "OSC_KNN_PANEL_T": "9", "OSC_KNN_PANEL_SYM": "0"}):
        for v in ("OSC_KNN_PANEL_T", "OSC_KNN_PANEL_RHO", "OSC_KNN_PANEL_NRG", "OSC_KNN_PANEL_RANK", "OSC_KNN_PANEL_SYM"):
            monkeypatch.delenv(v, raising=False)
        for v, val in env.items():
            monkeypatch.setenv(v, val)
        lat = amd.Oscillink(Y, kneighbors=k, deterministic_k=True)
        assert lat.build_info()["prefilter"] == 2 and lat.build_info()["fallback_rows"] <= 8
        g = lat.graph_csr()[:3]
        lat.close()
        if want is None:
            want = g
        else:
            assert np.array_equal(g[0], want[0]) and np.array_equal(g[1], want[1]) and np.array_equal(g[2], want[2]), env


def test_pool_off_and_planner_overrides():
    """OSC_POOL_MB=0 (process-wide: plain hipMalloc / hipFree per block) in a process of its own: create / settle / destroy
    twice, same results as with the pool."""
    import os
    import subprocess
    import sys

    code = ("import numpy as np, sys\n"
            "from oscillink_amd import Oscillink\n"
            "Y = np.random.default_rng(0).standard_normal((3000, 64)).astype(np.float32)\n"
            "out = []\n"
            "for _ in range(2):\n"
            "    lat = Oscillink(Y, kneighbors=8, deterministic_k=True); lat.set_query(Y[0]); st = lat.settle(); out.append((st['iters'], float(lat.U.sum()))); lat.close()\n"
            "assert out[0] == out[1], out\n"
            "print(out[0][0], repr(out[0][1]))\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for mb in ("0", "16384"):
        r = subprocess.run([sys.executable, "-c", code], env={**os.environ, "OSC_POOL_MB": mb, "PYTHONPATH": root},
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        res[mb] = r.stdout.strip()
    assert res["0"] == res["16384"]


def test_wide_wave_tiles_of_the_tile_core_give_the_same_lattice(amd, monkeypatch):
    """From ~49 000 rows (k <= 32) the tile core's main sweep runs with 64 x 128 wave tiles, two row blocks against two
    column tiles per workgroup (k_tile_thr2; OSC_KNN_TILE_WIDE=0 keeps k_tile_thr<1>).  391 row blocks: odd, the last set's
    second block is the zero tile behind the image.  Same K order per score, same thresholds: the graphs are identical,
    and the lists are the exact kernel's up to float64-proven near-ties."""
    from tests._fullsize import near_tie_gap

    N, D, k = 50000, 800, 16
    Y = np.random.default_rng(77).standard_normal((N, D), dtype=np.float32)
    graphs, lists = {}, {}
    for wide in ("1", "0"):
        monkeypatch.setenv("OSC_KNN_TILE_WIDE", wide)
        lat = amd.Oscillink(Y, kneighbors=k, deterministic_k=True)
        info = lat.build_info()
        assert info["prefilter"] == 2 and info["fallback_rows"] <= 8, info
        graphs[wide] = lat.graph_csr()
        lists[wide] = _knn_sets(lat, N, k)
        lat.close()
    for a, b in zip(graphs["1"], graphs["0"]):
        assert np.array_equal(a, b)
    monkeypatch.delenv("OSC_KNN_TILE_WIDE")
    monkeypatch.setenv("OSC_KNN_MODE", "exact")
    lat = amd.Oscillink(Y, kneighbors=k, deterministic_k=True)
    exact = _knn_sets(lat, N, k)
    lat.close()
    rows = np.nonzero((lists["1"] != exact).any(axis=1))[0]
    assert rows.size <= 25, rows.size
    for r in rows:
        members = sorted(set(lists["1"][r].tolist()) ^ set(exact[r].tolist()))
        assert near_tie_gap(Y, int(r), members) < 1e-6, (int(r), members)


@pytest.mark.parametrize("N,D,k", [(17000, 1000, 32), (20000, 1536, 64), (16400, 800, 8)])
def test_tile_core_threshold_route_beyond_768_columns(amd, N, D, k, monkeypatch):
    """D > 768: a wave's query panel no longer fits its registers, so the thresholds-and-hits prefilter runs on the tile core
    (k_tile_thr: both operands through LDS, symmetric half sweep, hits to the 32-row buckets, same select / re-scoring /
    proof).  Ragged D (1000 = 15.6 K steps), 24 K steps with keep = 96, a shallow k.  The lists are those of the tile
    prefilter and of the all-fp32 kernel up to float64-proven near-ties."""
    from tests._fullsize import near_tie_gap

    rng = np.random.default_rng(N + D)
    Y = rng.standard_normal((N, D), dtype=np.float32)
    lists, info = {}, {}
    for mode in ("panel", "prefilter", "exact"):
        monkeypatch.setenv("OSC_KNN_MODE", mode)
        lat = amd.Oscillink(Y, kneighbors=k, deterministic_k=True)
        info[mode] = lat.build_info()
        lists[mode] = _knn_sets(lat, N, k)
        lat.close()
    assert info["panel"]["prefilter"] == 2 and info["prefilter"]["prefilter"] == 1 and info["exact"]["prefilter"] == 0
    # (k = 64 keeps 96 candidates: at 157 row blocks the column sample is too dense for thresholds that leave every row that
    # many -- the planner would not choose this route here, forced it sends the short rows to the exact kernel)
    assert info["panel"]["fallback_rows"] <= (8 if k <= 32 else N // 20)
    for mode in ("panel", "prefilter"):
        rows = np.nonzero((lists[mode] != lists["exact"]).any(axis=1))[0]
        assert rows.size <= max(8, N // 2000), (mode, rows.size)
        for r in rows:
            members = sorted(set(lists[mode][r].tolist()) ^ set(lists["exact"][r].tolist()))
            assert near_tie_gap(Y, int(r), members) < 1e-6, (mode, int(r), members)
    # (the automatic choice needs a lattice large enough for sampled thresholds, as at D <= 768: config 5's full-size test,
    # tests/test_gpu_fullsize.py, runs this route by default)


def test_second_stage_proof_keeps_clustered_rows_off_the_exact_kernel(amd, monkeypatch):
    """Clustered anchors: for ~1 % of the rows the exact k-th score is not delta above the keep-th fp16 score, so the first
    re-scoring cannot prove their lists.  Half-sweep builds then re-score EVERY candidate of the row's bucket and prove the
    list against tau_row (k_bucket_rescore); only what is left goes to the all-fp32 kernel.  The full sweep (no buckets)
    shows how many rows the first stage leaves; the lattices are equal."""
    rng = np.random.default_rng(21)
    N, D, k, csize = 40000, 256, 24, 100
    centers = rng.standard_normal((N // csize, D)).astype(np.float32)
    Y = (centers[np.repeat(np.arange(N // csize), csize)] + 0.35 * rng.standard_normal((N, D))).astype(np.float32)
    Y = Y[rng.permutation(N)]
    monkeypatch.setenv("OSC_KNN_MODE", "panel")
    out = {}
    for sym in ("1", "0"):
        monkeypatch.setenv("OSC_KNN_PANEL_SYM", sym)
        lat = amd.Oscillink(Y, kneighbors=k, deterministic_k=True)
        out[sym] = (lat.build_info()["fallback_rows"], lat.graph_csr()[:3])
        lat.close()
    assert out["0"][0] >= 20, out["0"][0]            # the first stage alone leaves these to the exact kernel
    assert out["1"][0] <= out["0"][0] // 4, (out["1"][0], out["0"][0])
    # same edges; the weights of the rows the two builds decided differently come from two summation orders of the same fp32
    # products (the re-scoring's lane-strided sums vs the exact kernel's MFMA tiles)
    assert np.array_equal(out["1"][1][0], out["0"][1][0]) and np.array_equal(out["1"][1][1], out["0"][1][1])
    assert np.allclose(out["1"][1][2], out["0"][1][2], rtol=2e-6, atol=1e-8)


def _anchors_with_bad_rows(N, D, seed):
    """i.i.d. anchors with NaN rows (one NaN element is enough: graph.py:35 turns the whole unit row into NaN), +-Inf
    elements (norm = inf, inf / inf = NaN) and zero rows (norm 0: the unit row is 0 / 1e-12 = 0, every similarity 0)."""
    rng = np.random.default_rng(seed)
    Y = rng.standard_normal((N, D), dtype=np.float32)
    nan_rows = [5, 4097, 8191, 12345, N - 1]
    inf_rows = [77, 10000, N - 4445]
    zero_rows = [0, 128, 9000, 16384, N - 1000]
    for t, r in enumerate(nan_rows):
        Y[r, (17 * t) % D] = np.nan
    Y[nan_rows[1]] = np.nan  # ... and a row that is NaN throughout
    Y[inf_rows[0], 3] = np.inf
    Y[inf_rows[1], D - 1] = -np.inf
    Y[inf_rows[2], ::7] = np.inf
    Y[zero_rows] = 0.0
    return Y, sorted(nan_rows + inf_rows), zero_rows


@pytest.mark.parametrize("D,mode,nrg", [(600, "panel", "1"), (600, "panel", "2"), (256, "panel", "0"), (900, "panel", "0"),
                                        (600, "prefilter", "0"), (600, "exact", "0")])
def test_non_finite_and_zero_anchor_rows_on_the_large_lattice_routes(amd, orc, D, mode, nrg, monkeypatch):
    """graph.py:35-37 with anchors that are not finite: a NaN / Inf row's similarities are NaN, which rank last in every
    other row's ordering and fail `> 0` (graph.py:51, :64) -- such a row has no edges and is nobody's neighbour; a zero
    row's similarities are all 0, not `> 0` either.  The finite rows' lists are those of the finite columns.  Until round 6
    this was held only at N = 64 through the diffusion gates; here the lattice is large enough for the thresholds-and-hits
    prefilter (fp16 image of a NaN row, tile maxima and thresholds of a NaN row, hits against a NaN column's threshold,
    bucket delivery, the proof) on the panel core at both K depths and with one / two row groups, on the tile core
    (D = 900), the list-maintaining tile prefilter and the all-fp32 kernel -- each against the oracle's graph."""
    from tests._fullsize import check_graph_built_from_lists, device_knn_lists, near_tie_gap

    N, k = 20000, 16
    Y, nonfinite, zero = _anchors_with_bad_rows(N, D, 100 + D)
    with np.errstate(invalid="ignore"):
        idx_o, _ = orc.knn_topk(Y, k, block=2048)
    monkeypatch.setenv("OSC_KNN_MODE", mode)
    monkeypatch.setenv("OSC_KNN_PANEL_NRG", nrg)
    lat = amd.Oscillink(Y, kneighbors=k)
    info = lat.build_info()
    csr = lat.graph_csr()
    idx, val = device_knn_lists(lat, N, k)
    lat.close()
    rp, col, a, w, sd = csr
    assert info["prefilter"] == {"panel": 2, "prefilter": 1, "exact": 0}[mode]
    deg = np.diff(rp)
    assert (deg[nonfinite] == 0).all() and (deg[zero] == 0).all()
    assert not np.isin(col, nonfinite + zero).any()
    assert np.isfinite(a).all() and np.isfinite(w).all() and np.isfinite(sd).all()
    # the finite rows' lists are the oracle's (as sets; a row may differ by a float64-proven rank-k near-tie) ...
    good = np.setdiff1d(np.arange(N), np.array(nonfinite + zero))
    rows = good[(np.sort(idx[good], axis=1) != np.sort(idx_o[good], axis=1)).any(axis=1)]
    assert rows.size <= 8, rows.size
    for r in rows:
        members = sorted(set(idx[r].tolist()) ^ set(idx_o[r].tolist()))
        assert not np.isin(members, nonfinite).any() and near_tie_gap(Y, int(r), members) < 1e-6, (int(r), members)
    assert not np.isin(idx[good], nonfinite).any()
    # ... and the graph is the oracle's mutual test / cap / Laplacian applied to the device's lists, on EVERY row
    with np.errstate(invalid="ignore"):
        check_graph_built_from_lists(orc, N, idx, val, csr)


def test_non_finite_anchor_rows_on_the_wide_tile_core(amd, monkeypatch):
    """The same beyond 768 columns at a size whose main sweep runs with 64 x 128 wave tiles (k_tile_thr2, from ~49 000 rows),
    against the all-fp32 route, which the test above holds to the oracle."""
    N, D, k = 50000, 800, 8
    Y, nonfinite, zero = _anchors_with_bad_rows(N, D, 7)
    graphs = {}
    for mode in ("panel", "exact"):
        monkeypatch.setenv("OSC_KNN_MODE", mode)
        lat = amd.Oscillink(Y, kneighbors=k)
        graphs[mode] = (lat.graph_csr(), lat.build_info())
        lat.close()
    (rp, col, a, _, _), info = graphs["panel"]
    (rp_e, col_e, a_e, _, _), _ = graphs["exact"]
    assert info["prefilter"] == 2
    assert (np.diff(rp)[nonfinite + zero] == 0).all() and not np.isin(col, nonfinite + zero).any()
    assert np.array_equal(rp, rp_e) and np.array_equal(col, col_e) and np.allclose(a, a_e, rtol=2e-5, atol=1e-9)


@pytest.mark.parametrize("N,D,k,kind,mode", [(20000, 700, 32, "clustered", "panel"), (16400, 768, 16, "dups", "panel"),
                                              (20000, 1000, 40, "iid", "panel"), (12000, 640, 24, "iid", "prefilter"), (24000, 384, 16, "clustered", "panel"),
                                              (33000, 768, 8, "grouped", "panel")])
def test_rescoring_every_candidate_pair_once_gives_the_same_lists(amd, N, D, k, kind, mode, monkeypatch):
    """Round 6: in single-process builds of rows of >= 384 columns the exact re-scoring scores every undirected candidate pair
    once -- row i leaves the pairs (i, j), j < i, in which it stands in j's list to row j and fetches j's result
    (k_knn_rescore_pair + k_knn_rescore_finish) -- instead of from both ends (k_knn_rescore, OSC_KNN_RESCORE_PAIR=0).  The exact
    dot product is symmetric bit for bit, so lists (indices AND similarities), proofs, fallback rows and lattices are identical:
    clustered anchors (many unproven rows), exact duplicates (ties), the tile core beyond 768 columns, the tile prefilter's
    lists, anchors that arrive cluster by cluster."""
    from tests._fullsize import device_knn_lists

    rng = np.random.default_rng(N + D)
    if kind == "iid":
        Y = rng.standard_normal((N, D), dtype=np.float32)
    elif kind == "dups":
        base = rng.standard_normal((N // 40 + 1, D), dtype=np.float32)
        Y = base[np.arange(N) % base.shape[0]].copy()
    else:
        nc = N // 100
        Y = rng.standard_normal((nc, D), dtype=np.float32)[np.repeat(np.arange(nc), 100)][:N]
        Y = (Y + 0.35 * rng.standard_normal((N, D), dtype=np.float32)).astype(np.float32)
        if kind == "clustered":
            Y = Y[rng.permutation(N)]
    monkeypatch.setenv("OSC_KNN_MODE", mode)
    got = {}
    for pair in ("1", "0"):
        monkeypatch.setenv("OSC_KNN_RESCORE_PAIR", pair)
        lat = amd.Oscillink(Y, kneighbors=k, deterministic_k=True)
        got[pair] = (device_knn_lists(lat, N, k), lat.graph_csr(), lat.build_info())
        lat.close()
    (idx1, val1), csr1, info1 = got["1"]
    (idx0, val0), csr0, info0 = got["0"]
    assert info1["prefilter"] == info0["prefilter"] and info1["fallback_rows"] == info0["fallback_rows"]
    assert np.array_equal(idx1, idx0) and np.array_equal(val1, val0)
    for a, b in zip(csr1, csr0):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("N,D,k,kind,extra", [(20000, 768, 32, "iid", ""), (9000, 128, 16, "clustered", "gates"), (12000, 1536, 48, "iid", "chain"),
                                                (6000, 300, 8, "dups", ""), (30000, 64, 6, "clustered", "reorder"), (5000, 1600, 12, "iid", ""),
                                                (5000, 128, 100, "clustered", "")])  # (rows of more than 64 edges: the finish walks them in chunks)
def test_receipt_pass_that_computes_every_edge_once_gives_the_same_receipt(amd, N, D, k, kind, extra, monkeypatch):
    """Round 6: the receipt's per-edge pass computes the two squared distances of every undirected edge ONCE (row i its edges to
    j >= i: k_receipt_pairs; k_receipt_finish fetches the mirror slots and accumulates in edge order) instead of from both ends
    (k_receipt_rows, OSC_RECEIPT_PAIR=0).  The per-edge values are symmetric bit for bit, so the node components, the null
    points (index, z, residual), the sums of the receipt and the bundle are identical -- with gates, a chain, duplicated rows
    (exact ties in the null-point argmax), a lattice stored in BFS order, rows of more than 1536 columns (no pair form there)."""
    rng = np.random.default_rng(N + D)
    if kind == "iid":
        Y = rng.standard_normal((N, D), dtype=np.float32)
    elif kind == "dups":
        base = rng.standard_normal((N // 30 + 1, D), dtype=np.float32)
        Y = base[np.arange(N) % base.shape[0]].copy()
    else:
        nc = max(1, N // 100)
        Y = rng.standard_normal((nc, D), dtype=np.float32)[np.repeat(np.arange(nc), 100)][:N]
        Y = (Y + 0.35 * rng.standard_normal((N, D), dtype=np.float32)).astype(np.float32)
        Y = Y[rng.permutation(N)]
    psi = Y[:16].mean(0)
    psi = (psi / (np.linalg.norm(psi) + 1e-12)).astype(np.float32)
    if extra == "reorder":
        monkeypatch.setenv("OSC_REORDER", "1")
    gates = rng.uniform(0.0, 1.0, N).astype(np.float32) if extra == "gates" else None
    got = {}
    for pair in ("1", "0"):
        monkeypatch.setenv("OSC_RECEIPT_PAIR", pair)
        lat = amd.Oscillink(Y, kneighbors=k, deterministic_k=True)
        lat.set_query(psi, gates=gates)
        if extra == "chain":
            lat.add_chain(list(range(0, 40, 3)), lamP=0.2)
        lat.settle(max_iters=12, tol=1e-3)
        lat.set_receipt_detail("full")
        rec = lat.receipt()
        comps = lat._components()
        nulls = sorted((tuple(d["edge"]), d["z"], d["residual"]) for d in rec["null_points"])
        got[pair] = (rec["deltaH_total"], rec["coh_drop_sum"], rec["anchor_pen_sum"], rec["query_term_sum"], nulls,
                     [np.asarray(c).copy() for c in comps], lat.bundle(k=8))
        lat.close()
    a, b = got["1"], got["0"]
    assert a[:4] == b[:4]
    assert a[4] == b[4] and (len(a[4]) > 0 or kind == "dups")  # (exact duplicates: no residual, no null point)
    for x, y in zip(a[5], b[5]):
        assert np.array_equal(x, y)
    assert a[6] == b[6]

"""CPU checks of the multi-query algebra and of the float64 yardstick the GPU tests use
(tests/_queries.py), pinned to the oracle's solve_Ustar / components and the reference's recorded bundles."""
import numpy as np
import pytest

from tests import _queries as yq
from tests._cases import ctor_kwargs, load_case, make_inputs, random_gates

CASES = ["c1_n80_d128_k8", "g1_n400_d64_k6_chain8", "gates_chain_n333_d50_k7"]


def _oracle(name):
    from oracle import oscillink_oracle as orc

    case = load_case(name)
    rc = case["recipe"]
    Y, psi = make_inputs(rc)
    N = Y.shape[0]
    A = np.zeros((N, N), dtype=np.float32)
    A[np.repeat(np.arange(N), np.diff(case["indptr"])), case["indices"]] = case["A_data"]
    kw = {k: v for k, v in ctor_kwargs(rc).items() if k != "row_cap_val"}
    ref = orc.OracleLattice(Y, kneighbors=rc["k"], deterministic_k=True, graph=A, **kw)
    gates = random_gates(rc) if rc["gates"] == "random" else case["gates"] if rc["gates"] == "diffusion" else None
    ref.set_query(psi, gates=gates)
    if rc["chain"]:
        ref.add_chain(rc["chain"], lamP=rc["lamP"])
    M = yq.dense_M(A, ref.sqrt_deg, ref.B_diag, ref.lamG, ref.lamC, ref.lamQ, ref.lamP, ref.L_path)
    return case, ref, Y, psi, A, M


@pytest.mark.parametrize("name", CASES)
def test_yardstick_matches_oracle_solve_and_components(name):
    case, ref, Y, psi, A, M = _oracle(name)
    U = yq.ustar(M, Y, ref.B_diag, psi, ref.lamG, ref.lamQ)
    # the dense operator is the oracle's
    V = np.random.default_rng(0).standard_normal(Y.shape)
    assert np.allclose(M @ V, ref.M_mul(V), atol=1e-4)
    Us = ref.solve_Ustar(tol=1e-6, max_iters=400)
    assert np.max(np.abs(Us - U)) < 1e-4
    coh = yq.coherence_drop(Y, U, A, ref.sqrt_deg, ref.lamC)
    coh_o = ref.components(Us)[0]
    assert np.allclose(coh, coh_o, rtol=1e-3, atol=1e-3)


@pytest.mark.parametrize("name", CASES)
def test_basis_algebra(name):
    case, ref, Y, psi, A, M = _oracle(name)
    X, x = yq.basis(M, Y, ref.B_diag, ref.lamG, ref.lamQ)
    rng = np.random.default_rng(1)
    for q in [psi.astype(np.float64), rng.standard_normal(Y.shape[1]), np.zeros(Y.shape[1])]:
        assert np.allclose(X + np.outer(x, q), yq.ustar(M, Y, ref.B_diag, q, ref.lamG, ref.lamQ), atol=1e-10)
    # the residual of column c of U*(psi) is r_X,c + psi_c r_x
    Xe = X + 1e-3 * rng.standard_normal(X.shape)
    xe = x + 1e-3 * rng.standard_normal(x.shape)
    Yd, Bd, pd = Y.astype(np.float64), ref.B_diag.astype(np.float64), psi.astype(np.float64)
    rX = ref.lamG * Yd - M @ Xe
    rx = ref.lamQ * Bd - M @ xe
    R = ref.lamG * Yd + ref.lamQ * Bd[:, None] * pd[None, :] - M @ (Xe + np.outer(xe, pd))
    assert np.allclose(R, rX + np.outer(rx, pd), atol=1e-9)


@pytest.mark.parametrize("name", CASES)
def test_per_query_terms_reproduce_bundle(name):
    """align and coh from the per-basis constants (c0, c2, |X_i|^2) and the per-query dots g = X psi."""
    case, ref, Y, psi, A, M = _oracle(name)
    X, x = yq.basis(M, Y, ref.B_diag, ref.lamG, ref.lamQ)
    sd = ref.sqrt_deg.astype(np.float64) + 1e-12
    P, s = X / sd[:, None], x / sd
    Yn = Y / sd[:, None]
    r, c = np.nonzero(A > 0)
    w = 0.5 * ref.lamC * A[r, c].astype(np.float64)
    N = Y.shape[0]
    c0 = np.zeros(N)
    c2 = np.zeros(N)
    np.add.at(c0, r, w * (np.sum((Yn[r] - Yn[c]) ** 2, axis=1) - np.sum((P[r] - P[c]) ** 2, axis=1)))
    np.add.at(c2, r, w * (s[r] - s[c]) ** 2)
    xn2 = np.sum(X * X, axis=1)
    for q in [psi.astype(np.float64), np.random.default_rng(2).standard_normal(Y.shape[1])]:
        U = X + np.outer(x, q)
        g = X @ q
        p = g / sd
        pn2 = float(q @ q)
        align = (g + x * pn2) / (np.sqrt(xn2 + 2 * x * g + x * x * pn2) + 1e-12) / (np.sqrt(pn2) + 1e-12)
        want_align = (U / (np.linalg.norm(U, axis=1, keepdims=True) + 1e-12)) @ (q / (np.linalg.norm(q) + 1e-12))
        assert np.allclose(align, want_align, atol=1e-12)
        cross = np.zeros(N)
        np.add.at(cross, r, 2 * w * (s[r] - s[c]) * (p[r] - p[c]))
        coh = c0 - pn2 * c2 - cross
        assert np.allclose(coh, yq.coherence_drop(Y, U, A, ref.sqrt_deg, ref.lamC), atol=1e-9)


@pytest.mark.parametrize("name", CASES)
def test_yardstick_bundle_matches_fixture(name):
    case, ref, Y, psi, A, M = _oracle(name)
    U = yq.ustar(M, Y, ref.B_diag, psi, ref.lamG, ref.lamQ)
    ids, score, align, margins = yq.bundle(Y, U, psi, A, ref.sqrt_deg, ref.lamC, k=6)
    ok, _ = yq.same_until_near_tie(ids, case["bundle_ids"].tolist(), margins, 1e-4)
    assert ok
    assert np.allclose(score, case["bundle_score"], rtol=1e-3, atol=1e-3)
    assert np.allclose(align, case["bundle_align"], rtol=1e-3, atol=1e-4)


def test_native_chunk_matches_header():
    import os
    import re

    from oscillink_amd import _native

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "oscillink_hip.h")).read()
    assert int(re.search(r"#define OSC_QUERY_CHUNK (\d+)", hdr).group(1)) == _native.OSC_QUERY_CHUNK

"""The algebra behind bundle_many(chains=..., lamP=...) in float64, without a device: bundle()'s
alignment and coherence terms on U*_q = X' + x' psi^T + G (T_q V_q), expanded over the shifted basis, the Green's columns and
per-query scalars (tests/_bundle_prior.py), against bundle() on the dense solve of M + lamP L_path.  Required on the picked
rows: max |d score| and max |d align| <= 1e-10, for both forms of dgamma^T H dgamma."""
import numpy as np
import pytest

from oracle import oscillink_oracle as orc
from tests import _bundle_prior as bp
from tests import _chain_many as cm
from tests import _queries as yq
from tests import test_chain_prior_algebra as tpa
from tests.test_gpu_bundle_many import _batch

LAMPS = (0.2, 0.5)
BOUND = 1e-10


def _cases(inp):
    rowptr, col, _ = inp["csr"]
    ch = cm.chains(inp)
    a = ch["walk"][2]
    w8 = bp.spread(rowptr, col, 8)
    c64 = bp.spread(rowptr, col, 64, start=7)
    return {"m = 8": (w8, None), "m = 8 weighted": (w8, [1.0, 0.5, 2.0, 0.7, 0.3, 1.5, 0.25]),
            "revisited edge, self-step": (ch["mixed"], cm.OWN_WEIGHTS), "[a, a]: m = 1": ([a, a], None),
            "m = 64": (c64 + [c64[0]], [0.25 + (t % 5) * 0.5 for t in range(64)])}


@pytest.mark.parametrize("name", cm.FIXTURES)
def test_expansion_against_bundle_on_the_dense_solve(name):
    inp = cm.inputs(name)
    Y = inp["Y"].astype(np.float64)
    N = Y.shape[0]
    assert N <= yq.DENSE_LIMIT
    kw = inp["kw"]
    A = cm.dense_adj(inp["csr"], N)
    sd = orc.normalized_laplacian(A.astype(np.float32))[1]
    lamG, lamC, lamQ = kw.get("lamG", 1.0), kw.get("lamC", 0.5), kw.get("lamQ", 4.0)
    B = np.asarray(np.ones(N, np.float32) if inp["gates"] is None else inp["gates"], np.float64)
    M = yq.dense_M(A, sd, B, lamG, lamC, lamQ)
    P = _batch(inp["Y"], inp["psi"]).astype(np.float64)
    worst = {"score": 0.0, "align": 0.0, "lists": 0, "of": 0}
    for lamP in LAMPS:
        Ms = M + lamP * np.eye(N)
        for cname, (chain, weights) in _cases(inp).items():
            Lp, Wp = bp.path_terms(N, chain, weights)
            for q in (0, 2, 3, 6):  # the fixture's psi, a large random query, an anchor row, psi = 0
                psi = P[q]
                Uref = yq.ustar(M + lamP * Lp, Y, B, psi, lamG, lamQ)
                ids, w_score, w_align, _ = yq.bundle(Y, Uref, psi, A, sd, lamC, k=8)
                Xs, xs, G, C, nodes = bp.pieces(Ms, Y, B, lamG, lamQ, lamP, Wp, chain, psi)
                assert len(nodes) == len(set(chain))
                for split in (True, False):
                    align, coh = bp.expansion(Y, A, sd, lamC, Xs, xs, G, C, psi, split=split)
                    score = bp.score_of(align, coh)
                    ds = float(np.max(np.abs(score[ids] - w_score)))
                    da = float(np.max(np.abs(align[ids] - w_align)))
                    worst["score"], worst["align"] = max(worst["score"], ds), max(worst["align"], da)
                    assert ds <= BOUND and da <= BOUND, (name, lamP, cname, q, split, ds, da)
                # what the prior does at this size (reported, not asserted)
                U0 = yq.ustar(M, Y, B, psi, lamG, lamQ)
                ids0, _, _, _ = yq.bundle(Y, U0, psi, A, sd, lamC, k=8)
                worst["lists"] += int(ids0 != ids)
                worst["of"] += 1
    print(f"{name}: max |d score| {worst['score']:.3g}, max |d align| {worst['align']:.3g}; the prior changes "
          f"{worst['lists']} of {worst['of']} id lists")


@pytest.mark.parametrize("name", ["gates_chain_n333_d50_k7", "lam_g03_c0_q0_n240_d40_k6"])
def test_residual_identity_of_the_implied_ustar(name):
    """Section 12.2's perturbation identity, on which `last_bundle_prior["res"]` rests: with Green's columns of residual R_e and
    a basis of residual r0, the U*_q the expansion stands for has the residual r0 + R (T_q V_q) against M_q exactly."""
    inp, Y, A, sd, (lamG, lamC, lamQ), B, cases = tpa._setup(name)
    N = Y.shape[0]
    lamP = 0.5
    M = yq.dense_M(A, sd, B, lamG, lamC, lamQ)
    Ms = M + lamP * np.eye(N)
    rng = np.random.default_rng(11)
    psi = cm.queries(inp)[2].astype(np.float64)
    rhs = lamG * Y + lamQ * B[:, None] * psi[None, :]
    for cname in ("mixed", "walk weighted", "aa"):
        chain, weights = cases[cname]
        Lp, Wp = bp.path_terms(N, chain, weights)
        nodes = sorted(set(chain))
        E = np.zeros((N, len(nodes)))
        E[nodes, range(len(nodes))] = 1.0
        G = np.linalg.solve(Ms, E) + 1e-5 * rng.standard_normal(E.shape)
        Xs, xs = yq.basis(Ms, Y, B, lamG, lamQ)
        U0 = Xs + xs[:, None] * psi[None, :] + 1e-5 * rng.standard_normal(Y.shape)
        U, TV, _, _, _ = tpa._woodbury(Ms, Y, B, lamG, lamQ, lamP, Wp, chain, psi, G=G, U0=U0)
        r = rhs - (M + lamP * Lp) @ U
        want = (rhs - Ms @ U0) + (E - Ms @ G) @ TV
        assert np.max(np.abs(r - want)) <= 1e-11 * max(1.0, float(np.max(np.abs(rhs)))), (name, cname)

"""Inputs and float64 yardstick shared by tests/test_gpu_chain_gated_many.py and tests/test_chain_gated_host.py
(chain_gated_many).  The shapes, anchors, queries, gates and seeds are tests/_receipt_gated.py's;
the chains walk the case's own graph (tests/_chain_many.py's walk and mixed); the yardstick is composed from what exists:
tests/_queries.dense_M with lamP L_path,q, tests/_receipt_yardstick.receipt, tests/_chain_many.chain_yardstick_rows,
tests/_queries.bundle and tests/_receipt_gated.cg64 with the reference's flat diagonal lamG + lamQ g + lamP.  No tolerance
is defined here."""
import numpy as np

from tests import _bundle_gated as bg
from tests import _chain_many as cm
from tests import _queries as yq
from tests import _receipt_gated as rg
from tests import _receipt_yardstick as yr
from tests import _refine_chains as rc
from tests._bundle_gated import NEAR_TIE, history_clear_of_tol  # noqa: F401  (shared, unchanged)
from tests._chain_many import OWN_WEIGHTS, Z_THS  # noqa: F401
from tests._receipt_gated import (CASES, LAMS, LEFT_OUT_CAP, LOOP_CASES, MARGIN, PARITY, SETTLE_CAPPED,  # noqa: F401
                                  SETTLE_CASE, SETTLE_DEFAULT, Z_RTOL, check_nulls, close)

LAMPS = (0.2, 0.5)
KINDS = ("walk", "mixed", "self", "revisit", "zero", "two")

# Where a case's seed fails a condition of tests/test_chain_gated_host.py -- a null-point share above LEFT_OUT_CAP, a chain
# edge's max(z) within 1 % of a threshold or of the running maximum, a history within 5 % of its tol -- the recipes of
# tests/_receipt_gated.py run on the seed given here instead (its own substitutions stay where this table has none).
SEEDS = {"d33": 114, "n33": 119}
# lamP of the tests that compare iteration counts: the loop parity (at 0.2 the U* history of reordered_n1500_d33's psi = 0
# query passes within 0.6 % of tol one step before it ends; at 0.5 every history is clear) and the settle
LOOP_LAMP, SETTLE_LAMP = 0.5, 0.2


def _seeded(fn, name, *args):
    """tests/_receipt_gated._seeded reading its seeds from that module's table overlaid with this one's: its own function
    over a copy of its globals, the way it shadows numpy itself, so nothing of that module is changed"""
    import types

    g = {**rg._seeded.__globals__, "SEEDS": {**rg.SEEDS, **SEEDS}}
    return types.FunctionType(rg._seeded.__code__, g, "_seeded", rg._seeded.__defaults__)(fn, name, *args)


def anchors(name):
    return _seeded(bg.anchors, name)


def queries(name, Y):
    return _seeded(bg.queries, name, Y)


def given_gates(name, N):
    return _seeded(bg.given_gates, name, N)


def csr_of(A):
    """(rowptr, col, a) of a dense adjacency, columns ascending"""
    A = np.asarray(A)
    r, c = np.nonzero(A > 0)
    rowptr = np.zeros(A.shape[0] + 1, dtype=np.int64)
    np.cumsum(np.bincount(r, minlength=A.shape[0]), out=rowptr[1:])
    return rowptr, c.astype(np.int64), A[r, c].astype(np.float64)


def chains(name, A):
    """kind -> (chain, weights or None) on the case's graph: a walk along graph edges, `mixed` with weights (a self-step, a
    revisited edge and non-edges), [a, a], an edge revisited with two different weights, an edge of weight 0 and the two-node
    chain.  On a graph too small for a six-node walk (n2) every kind is the chain [0, 1]."""
    rowptr, col, _ = csr_of(A)
    w = cm.walk(rowptr, col, 0)
    if len(w) < 6:
        assert A.shape[0] == 2 and A[0, 1] > 0
        return {k: ([0, 1], None) for k in KINDS}
    return {"walk": (w, None), "mixed": (cm.mixed(w), list(OWN_WEIGHTS)), "self": ([w[1], w[1]], None),
            # (a source row with one path entry has z_path = sqrt(N - 1) whatever its R: the revisit starts inside the walk, so
            # that only one of its edges leaves such a row and no two max(z) tie by construction)
            "revisit": ([w[1], w[0], w[1], w[2]], [0.5, 2.0, 1.0]), "zero": (w[:3], [1.0, 0.0]), "two": (w[:2], None)}


def kinds_of(name):
    """the chain kind of each of the case's five queries: the six kinds dealt round the cases, so every kind meets every
    slab width and every query recipe somewhere"""
    at = list(CASES).index(name)
    return [KINDS[(at + q) % len(KINDS)] for q in range(5)]


def query_chains(name, A):
    """([chain per query], [weights or None per query])"""
    ch = chains(name, A)
    picked = [ch[k] for k in kinds_of(name)]
    return [c for c, _ in picked], [w for _, w in picked]


def path_laplacian(N, chain, weights):
    """build_path_laplacian (graph.py:96-111) in float64: (L_path, A_path)"""
    Ap = rc.path_adjacency(N, chain, weights)
    dm = 1.0 / np.sqrt(np.maximum(Ap.astype(np.float64).sum(axis=1), 1e-12))
    return np.eye(N) - (Ap * dm[:, None]) * dm[None, :], Ap


def chain_M(A, sd, g, lamP, chain, weights, lams=LAMS):
    """M_q = lamG I + lamC L_sym + lamQ diag(g) + lamP L_path,q"""
    lamG, lamC, lamQ = lams
    return yq.dense_M(A, sd, g, lamG, lamC, lamQ, lamP, path_laplacian(A.shape[0], chain, weights)[0])


def diag(g, lamP, lams=LAMS):
    """the reference's flat Jacobi diagonal lamG + lamQ g + lamP (lattice.py:257-259)"""
    lamG, _, lamQ = lams
    return lamG + lamQ * np.asarray(g, np.float64) + lamP


def yardstick(Y, U, psi, g, A, sd, lamP, chain, weights, k, lams=LAMS):
    """the receipt (tests/_receipt_yardstick.receipt under M_q, with "Ustar" and "margin"), the chain receipt's rows and the
    bundle of one query, all in float64 at the exact U*_q"""
    lamG, lamC, lamQ = lams
    M = chain_M(A, sd, g, lamP, chain, weights, lams)
    rec = yr.receipt(Y, U, psi, A, sd, g, lamG, lamC, lamQ, M)
    ch = cm.chain_yardstick_rows(rec["Ustar"], Y, csr_of(A), sd, lamC, (chain, weights), chain)
    ids, score, align, margins = yq.bundle(Y, rec["Ustar"], psi, A, sd, lamC, k=k)
    return dict(M=M, receipt=rec, chain=ch, ids=ids, score=score, align=align, margins=margins)


def deltaH64(M, U, Us):
    E = np.asarray(U, np.float64) - Us
    return float(np.sum(E * (M @ E)))


def settle64(M, Y, U, psi, g, lamP, lams=LAMS, dt=1.0, max_iters=12, tol=1e-3):
    """settle(dt, max_iters, tol) from U under M_q with the diagonal 1 + dt (lamG + lamQ g + lamP): (U+, iters, res, history)"""
    return rg.cg64(rg.settle_system(M, dt), rg.settle_rhs(Y, U, psi, g, lams, dt), U, 1.0 + dt * diag(g, lamP, lams), tol,
                   max_iters)


def ustar64(M, Y, psi, g, lamP, lams=LAMS, tol=bg.TOL, max_iters=bg.LOOP_ITERS):
    """solve_Ustar()'s CG from x0 = Y in float64: (U*, iters, res, history)"""
    lamG, _, lamQ = lams
    rhs = lamG * np.asarray(Y, np.float64) + lamQ * np.asarray(g, np.float64)[:, None] * np.asarray(psi, np.float64)[None, :]
    return rg.cg64(M, rhs, Y, diag(g, lamP, lams), tol, max_iters)


def z_margin(zmax, chain=None, z_ths=Z_THS):
    """the smallest relative distance of a chain's max(z) values from a threshold, or from the running maximum that decides
    the weakest link (chain_receipt's `worst`, from -1).  With `chain`, a step that repeats an earlier step (i, j) is left
    out: it repeats that step's numbers exactly, in the yardstick as on the device, and never exceeds the running maximum."""
    zmax = np.asarray(zmax, np.float64)
    run, worst, seen = -1.0, np.inf, set()
    for t, z in enumerate(zmax):
        step = (chain[t], chain[t + 1]) if chain is not None else t
        if step in seen:
            continue
        seen.add(step)
        worst = min([worst, abs(float(z) - run) / max(abs(run), abs(float(z)), 1e-300)] +
                    [abs(float(z) - z_th) / z_th for z_th in z_ths])
        run = max(run, float(z))
    return worst


SEAM_CASE = "reordered_n1500_d33"
SEAM_LAPS = (146, 1024, 5)  # distinct nodes, chain length, seed of the permutation they are drawn from


def fix_rows():
    """kChainFixRows of oscillink_amd/csrc/chain_gated_plan.hpp: the path rows of one fix unit"""
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "oscillink_amd", "csrc", "chain_gated_plan.hpp")).read()
    return int(re.search(r"constexpr int32_t kChainFixRows = (\d+);", text).group(1))


def seam_chains(A):
    """the five chains of the path-seam test on SEAM_CASE: a 1024-node chain that laps a cycle of 146 distinct rows (revisits
    only; its path rows span more than one fix unit), [a, a], the weight-0 edge, the two-weight revisit, and the laps again"""
    m, n, seed = SEAM_LAPS
    cyc = [int(v) for v in np.random.default_rng(seed).permutation(A.shape[0])[:m]]
    laps = (cyc * (n // m + 1))[:n]
    ch = chains(SEAM_CASE, A)
    picked = [(laps, None), ch["self"], ch["zero"], ch["revisit"], (laps, None)]
    return [c for c, _ in picked], [w for _, w in picked]

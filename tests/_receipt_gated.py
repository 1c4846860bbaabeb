"""Inputs and float64 yardstick shared by tests/test_gpu_receipt_gated_many.py and tests/test_receipt_gated_host.py
(receipt_gated_many).  The shapes, anchors, queries and gates are tests/_bundle_gated.py's; the
receipt is tests/_receipt_yardstick.py's with M_q = lamG I + lamC L_sym + lamQ diag(g_q); the settle is the reference's
implicit Euler step (lattice.py:159-230) on a dense (I + dt M_q) with solver.py's iteration and stop rule restated in
float64."""
import numpy as np

from tests import _bundle_gated as bg
from tests import _queries as yq
from tests import _receipt_yardstick as yr
from tests._bundle_gated import CASES, dense_graph  # noqa: F401  (shared, unchanged)
from tests._receipt_reference import LEFT_OUT_CAP, MARGIN, Z_RTOL  # noqa: F401
from tests._receipt_yardstick import differing_rows, null_margins, receipt  # noqa: F401

LAMS = (1.0, 0.5, 4.0)
PARITY = 1e-4  # the project's relative parity gate; absolute floor PARITY * max(1, |value|)
SETTLE_DEFAULT = {"dt": 1.0, "max_iters": 12, "tol": 1e-3}
SETTLE_CAPPED = {"dt": 0.5, "max_iters": 3, "tol": 1e-3}
SETTLE_CASE = "seam_n97_d40"
LOOP_CASES = ("seam_n97_d40", "reordered_n1500_d33")  # where cg_iters is compared: the settle starts at U = Y

# The anchors, queries and gates are tests/_bundle_gated.py's recipes (anchors, queries, given_gates) on its shapes.  Where
# a case's seed leaves more than LEFT_OUT_CAP of its rows too close to call, or a settle residual within 5 % of tol
# (tests/test_receipt_gated_host.py checks both), the three recipes run on the seed given here instead.
SEEDS = {"seam_n97_d40": 104, "d1": 101, "n33": 102}


def _seeded(fn, name, *args):
    seed = SEEDS.get(name)
    if seed is None:
        return fn(name, *args)

    class _Rng:  # the recipe asks for default_rng(case seed + offset): the offset is kept, the case seed replaced
        @staticmethod
        def default_rng(s):
            return np.random.default_rng(s - CASES[name][4] + seed)

    import types

    shadow = types.FunctionType(fn.__code__, {**fn.__globals__, "np": _Shadow(_Rng)}, fn.__name__, fn.__defaults__)
    return shadow(name, *args)


class _Shadow:
    """numpy with another random.default_rng"""

    def __init__(self, rng):
        self.random = rng

    def __getattr__(self, key):
        return getattr(np, key)


def anchors(name):
    return _seeded(bg.anchors, name)


def queries(name, Y):
    return _seeded(bg.queries, name, Y)


def given_gates(name, N):
    return _seeded(bg.given_gates, name, N)


def gated_M(A, sd, g, lams=LAMS):
    lamG, lamC, lamQ = lams
    return yq.dense_M(A, sd, g, lamG, lamC, lamQ)


def settle_system(M, dt):
    """A = I + dt M"""
    return np.eye(M.shape[0]) + dt * M


def settle_rhs(Y, U, psi, g, lams, dt):
    """b = U + dt (lamG Y + lamQ g psi^T) (lattice.py:171, 184)"""
    lamG, _, lamQ = lams
    return np.asarray(U, np.float64) + dt * (lamG * np.asarray(Y, np.float64) +
                                             lamQ * np.asarray(g, np.float64)[:, None] * np.asarray(psi, np.float64)[None, :])


def settle_diag(g, lams, dt):
    """the reference's Jacobi diagonal 1 + dt (lamG + lamQ g) (lattice.py:186-192)"""
    lamG, _, lamQ = lams
    return 1.0 + dt * (lamG + lamQ * np.asarray(g, np.float64))


def cg64(A, b, x0, md, tol, max_iters):
    """solver.py:18-37 in float64 over a dense A: (x, iters, res, [res after each iteration])"""
    x = np.array(x0, np.float64)
    r = b - A @ x
    z = r / (md[:, None] + 1e-12)
    p = z.copy()
    rz_old = (r * z).sum(axis=0)
    hist = []
    it, res = 0, 0.0
    for it in range(1, max_iters + 1):
        Ap = A @ p
        alpha = rz_old / ((p * Ap).sum(axis=0) + 1e-18)
        x = x + p * alpha
        r = r - Ap * alpha
        res = float(np.linalg.norm(r, axis=0).max())
        hist.append(res)
        if res <= tol:
            break
        z = r / (md[:, None] + 1e-12)
        rz_new = (r * z).sum(axis=0)
        p = z + p * (rz_new / (rz_old + 1e-18))
        rz_old = rz_new
    return x, it, res, hist


def settle64(M, Y, U, psi, g, lams=LAMS, dt=1.0, max_iters=12, tol=1e-3):
    """settle(dt, max_iters, tol) from U (warm start, no inertia): (U+, iters, res, history)"""
    return cg64(settle_system(M, dt), settle_rhs(Y, U, psi, g, lams, dt), U, settle_diag(g, lams, dt), tol, max_iters)


def yardstick(Y, U, psi, g, A, sd, lams=LAMS):
    """tests/_receipt_yardstick.receipt under M_q"""
    lamG, lamC, lamQ = lams
    return yr.receipt(Y, U, psi, A, sd, g, lamG, lamC, lamQ, gated_M(A, sd, g, lams))


def rows_with_edge(A):
    return np.nonzero((np.asarray(A) > 0).any(axis=1))[0]


def left_out_share(margin, A):
    """share of the rows with an edge whose null-point decision is too close to compare"""
    rows = rows_with_edge(A)
    return float(np.count_nonzero(margin[rows] < MARGIN)) / max(rows.size, 1)


def close(got, want, rel=PARITY):
    """the parity gate: |got - want| <= rel * max(1, |want|)"""
    return abs(float(got) - float(want)) <= rel * max(1.0, abs(float(want)))


def check_nulls(got, want, margin, A):
    """null points equal on every row whose margin is >= MARGIN, z and R within Z_RTOL there; returns the left-out share"""
    bad = [i for i in yr.differing_rows(got, want) if margin[i] >= MARGIN]
    assert not bad, bad[:5]
    w = {int(p["edge"][0]): p for p in want}
    for p in got:
        i = int(p["edge"][0])
        if margin[i] >= MARGIN:
            assert np.isclose(p["z"], w[i]["z"], rtol=Z_RTOL, atol=0), (i, p, w[i])
            assert np.isclose(p["residual"], w[i]["residual"], rtol=Z_RTOL, atol=0), (i, p, w[i])
    return left_out_share(margin, A)

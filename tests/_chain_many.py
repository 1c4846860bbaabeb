"""Cases and float64 yardstick of OscillinkLattice.chain_receipt_many, shared by
tests/test_chain_many_host.py (the CPU proof that the cases do not rest on a knife edge) and
tests/test_gpu_chain_receipt_many.py.

Every fixture runs with a chain of its own installed and without one.  The chains walk the fixture's own graph: on these
Gaussian fixtures an index-order chain such as [0..7] has no structural edge at all, so every r_struct and the gain would
be 0 and the slot lookup would never be exercised."""
import numpy as np

from oracle import oscillink_oracle as orc
from tests import _queries as yq
from tests import _refine_chains as rc
from tests._cases import ctor_kwargs, load_case, make_inputs, random_gates

FIXTURES = ["c1_n80_d128_k8", "g1_n400_d64_k6_chain8", "gates_chain_n333_d50_k7", "seed_n400_d768_k12",
            "lam_g03_c0_q0_n240_d40_k6"]
Z_THS = (2.5, 25.0)
OWN_WEIGHTS = [1.0, 0.5, 2.0, 0.7, 0.3, 1.5]  # of the chain installed on a fixture whose recipe has none: `mixed`, 6 edges
OWN_LAMP = 0.5  # (at 0.2 an edge of c1_n80 sits 0.5 % from z_th = 2.5 on the yardstick; at 0.5 the closest is 10 % away)


def walk(rowptr, col, start, n=6):
    """From `start`, step to the first unvisited neighbour in the CSR, for n nodes (fewer at a dead end)."""
    out, seen = [int(start)], {int(start)}
    while len(out) < n:
        nxt = [int(c) for c in col[rowptr[out[-1]]: rowptr[out[-1] + 1]] if int(c) not in seen]
        if not nxt:
            break
        out.append(nxt[0])
        seen.add(nxt[0])
    return out


def mixed(w):
    """A self-step, a revisited edge and a non-edge on the nodes of a walk."""
    return w[:3] + [w[2], w[1], w[0], w[-1]]


def inputs(name):
    """What a fixture's lattice is built from: Y, psi, the gates or None, the recipe's chain (or None) and its lamP, the
    constructor's keywords and the fixture's stored graph (rowptr, col, a)."""
    case = load_case(name)
    r = case["recipe"]
    if "gen" in r:
        Y, psi = make_inputs(r)
        gates = random_gates(r) if r["gates"] == "random" else None
        kw = dict(kneighbors=r["k"], deterministic_k=True, **ctor_kwargs(r))
        chain, lamP = r["chain"], r["lamP"]
    else:  # the neighbor_seed fixtures (tests/golden/make_golden_r2.py): anchors and the edge set only
        Y = np.random.default_rng(r["seed"]).standard_normal((r["N"], r["D"])).astype(np.float32)
        psi = Y[:32].mean(axis=0)
        psi = (psi / (np.linalg.norm(psi) + 1e-12)).astype(np.float32)
        gates, chain, lamP = None, None, 0.0
        kw = dict(kneighbors=r["k"], deterministic_k=False, neighbor_seed=r["neighbor_seed"])
    return dict(name=name, Y=Y, psi=psi, gates=gates, chain=chain, lamP=lamP, kw=kw,
                csr=(case["indptr"], case["indices"], case["A_data"]))


def chains(inp):
    """name -> chain of a fixture: the walk from row 0, `mixed` on it, and the recipe's chain where there is one."""
    rowptr, col, _ = inp["csr"]
    w = walk(rowptr, col, 0)
    assert len(w) == 6, (inp["name"], w)
    out = {"walk": w, "mixed": mixed(w)}
    if inp["chain"]:
        out["recipe"] = [int(c) for c in inp["chain"]]
    return out


def own_chain(inp):
    """(chain, weights, lamP) a fixture's lattice carries in the `own` variant: the recipe's, else `mixed` with weights."""
    if inp["chain"]:
        return [int(c) for c in inp["chain"]], None, inp["lamP"]
    return chains(inp)["mixed"], OWN_WEIGHTS, OWN_LAMP


def queries(inp):
    from tests.test_gpu_receipt_many import _batch

    return _batch(inp["Y"], inp["psi"])


def dense_adj(csr, N):
    rowptr, col, a = csr
    A = np.zeros((N, N))
    A[np.repeat(np.arange(N), np.diff(rowptr)), col] = a
    return A


class Yardstick:
    """The exact dense U*(psi) of a fixture (with or without its own chain) for any query, and chain_yardstick on it."""

    def __init__(self, inp, own, csr=None, sqrt_deg=None):
        Y = inp["Y"]
        N = Y.shape[0]
        kw = inp["kw"]
        self.Y, self.N = Y, N
        self.A = dense_adj(inp["csr"] if csr is None else csr, N)
        self.sd = orc.normalized_laplacian(self.A.astype(np.float32))[1] if sqrt_deg is None else sqrt_deg
        self.lamG, self.lamC, self.lamQ = kw.get("lamG", 1.0), kw.get("lamC", 0.5), kw.get("lamQ", 4.0)
        self.B = np.ones(N, np.float32) if inp["gates"] is None else inp["gates"]
        self.own = own_chain(inp) if own else None
        Lp, lamP = None, 0.0
        if self.own:
            ch, ws, lamP = self.own
            self.Ap_own = rc.path_adjacency(N, ch, ws)
            d = self.Ap_own.astype(np.float64).sum(axis=1)
            dm = 1.0 / np.sqrt(np.maximum(d, 1e-12))
            Lp = np.eye(N) - (self.Ap_own * dm[:, None]) * dm[None, :]
        M = yq.dense_M(self.A, self.sd, self.B, self.lamG, self.lamC, self.lamQ, lamP, Lp)
        self.X, self.x = yq.basis(M, Y, self.B, self.lamG, self.lamQ)

    def ustar(self, psi):
        return self.X + self.x[:, None] * np.asarray(psi, np.float64)[None, :]

    def chain(self, psi, chain, Us=None):
        Ap = self.Ap_own if self.own else rc.path_adjacency(self.N, chain)
        return rc.chain_yardstick(self.ustar(psi) if Us is None else Us, self.Y, self.A, self.sd, self.lamC, Ap, chain)


def weakest(zmax):
    """chain_receipt's weakest link on a list of max(z): the first edge strictly greater than every earlier one, from -1."""
    k, worst = -1, -1.0
    for t, z in enumerate(zmax):
        if z > worst:
            k, worst = t, float(z)
    return k, worst


def chain_yardstick_rows(Us, Y, csr, sqrt_deg, lamC, path, chain):
    """rc.chain_yardstick without the N x N arrays (the route lattices have up to 12 000 rows): the same float64 formulas on
    dense rows built where they are needed.  csr = (rowptr, col, a); path = (chain, weights or None) of the path adjacency."""
    rowptr, col, a = csr
    N = Us.shape[0]
    di = np.asarray(sqrt_deg, np.float64) + 1e-12
    Un = np.asarray(Us, np.float64) / di[:, None]
    Yn = np.asarray(Y, np.float64) / di[:, None]
    pch, pws = path
    pws = [1.0] * (len(pch) - 1) if pws is None else pws
    prow = {}
    for t in range(len(pch) - 1):
        i, j, w = int(pch[t]), int(pch[t + 1]), float(np.float32(pws[t]))
        for r, c in ((i, j), (j, i)):
            prow.setdefault(r, {})[c] = max(prow.get(r, {}).get(c, 0.0), w)
    out = {k: [] for k in ("z_struct", "z_path", "r_struct", "r_path", "bound_struct", "bound_path", "term")}
    mag = 0.0
    for t in range(len(chain) - 1):
        i, j = int(chain[t]), int(chain[t + 1])
        d2 = np.sum((Un[i][None, :] - Un) ** 2, axis=1)
        Ai, Api = np.zeros(N), np.zeros(N)
        Ai[col[rowptr[i]: rowptr[i + 1]]] = a[rowptr[i]: rowptr[i + 1]]
        for c, w in prow.get(i, {}).items():
            Api[c] = w
        for name, R in (("struct", lamC * Ai * d2), ("path", max(lamC, 1e-6) * Api * d2)):
            mu, sig = float(R.mean()), float(R.std()) + 1e-12
            out["z_" + name].append((float(R[j]) - mu) / sig)
            out["r_" + name].append(float(R[j]))
            out["bound_" + name].append((abs(float(R[j])) + abs(mu)) / sig)
        dy, du = float(np.sum((Yn[i] - Yn[j]) ** 2)), float(d2[j])
        w = max(float(Ai[j]), 0.0)
        out["term"].append(0.5 * lamC * w * (dy - du))
        mag += 0.5 * lamC * w * (dy + du)
    out = {k: np.asarray(v) for k, v in out.items()}
    out["gain"] = float(np.sum(out["term"]))
    out["gain_magnitude"] = mag
    out["zmax"] = np.maximum(out["z_struct"], out["z_path"])
    return out

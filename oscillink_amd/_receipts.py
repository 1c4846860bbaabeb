"""The host side of a receipt, once: what `OscillinkLattice.receipt`, `receipt_many` and `Corpus.refine_many(receipts=...)`
share when they turn device numbers into the reference's receipt dict (oscillink/core/lattice.py:298-455, receipts.py).
The callers differ in where the `ustar_*` values, the clocks and the gates come from; they pass values, never a lattice.
Key order is the reference's and is part of the contract (tests/test_receipt_records_host.py).  NumPy and the standard
library only.
"""
from __future__ import annotations

import ctypes as C
import gc
import hashlib
import hmac
import json
import os
from typing import Any, Optional

import numpy as np


def null_cap() -> int:
    """OSCILLINK_RECEIPT_NULL_CAP as an int >= 0; unset, garbage or negative: 0 (no cap)."""
    try:
        return max(int(os.getenv("OSCILLINK_RECEIPT_NULL_CAP", "0").strip()), 0)
    except ValueError:
        return 0


def null_summary(total: int, cap: int) -> dict[str, Any]:
    capped = cap > 0 and total > cap
    return {"total_null_points": total, "returned_null_points": cap if capped else total, "null_cap_applied": bool(capped)}


def null_dicts(i, j, z, r, n):
    """The reference's list of {"edge": [i, j], "z": .., "residual": ..} (receipts.py:63-83).  At config 3 every row has a
    null point (a dense residual row is 29 values among 100 000 zeros), so this makes 100 000 dicts + 100 000 lists: the
    cyclic collector, which wakes up every 700 new containers and re-walks the young ones, was two thirds of the 47 ms the
    list took -- nothing built here can be part of a cycle, so it is paused for the construction."""
    il, jl, zl, rl = i[:n].tolist(), j[:n].tolist(), z[:n].astype(float).tolist(), r[:n].astype(float).tolist()
    paused = n > 2000 and gc.isenabled()
    if paused:
        gc.disable()
    try:
        return [{"edge": [a, b], "z": c, "residual": d} for a, b, c, d in zip(il, jl, zl, rl)]
    finally:
        if paused:
            gc.enable()


def check_queries(psis, D: int, finite: bool = True) -> np.ndarray:
    """`psis` as a contiguous float32 (Q, D) array with finite rows, or the ValueError every batched call raises.
    finite=False lets non-finite rows through (chain_receipt_many: such a query gets non-finite answers, as in the loop)."""
    P = np.asarray(psis)
    if P.ndim != 2 or P.shape[1] != D:
        raise ValueError(f"psis must be a (Q, {D}) array, got shape {P.shape}")
    P = np.ascontiguousarray(P, dtype=np.float32)
    bad = np.nonzero(~np.all(np.isfinite(P), axis=1))[0]
    if bad.size and finite:
        raise ValueError(f"psis row {int(bad[0])} is not finite")
    return P


MAX_CHAIN = 1024  # nodes of one query's chain (include/oscillink_hip.h)
MAX_PRIOR_NODES = 64  # distinct nodes of a chain that is its own prior (csrc/chain_prior_plan.hpp: kChainPriorMaxNodes)
CHAIN_EDGE_KEYS = ("chain_z_struct", "chain_z_path", "chain_r_struct", "chain_r_path")


def chain_block(chains, Q: int, N: int):
    """chain_receipt_many's `chains` -- one chain (a sequence of ints, shared by every query) or a sequence of Q chains --
    as (lists, offsets, nodes): per query the chain as a list of ints, the Q + 1 int64 node offsets and the int32 nodes of
    osc_chain_receipt_many.  ValueError for a chain count other than Q, a chain outside 2..MAX_CHAIN nodes, a node that is
    no integer or lies outside [0, N)."""
    def one(ch, who):
        try:
            arr = np.asarray(ch)
            if arr.ndim != 1 or (arr.size and not np.issubdtype(arr.dtype, np.integer)):
                raise TypeError
        except (TypeError, ValueError):
            raise ValueError(f"{who}: a chain must be a sequence of integers") from None
        if arr.size < 2:
            raise ValueError(f"{who}: chain must contain at least two indices")
        if arr.size > MAX_CHAIN:
            raise ValueError(f"{who}: a chain has at most {MAX_CHAIN} indices, got {arr.size}")
        if arr.min() < 0 or arr.max() >= N:
            raise ValueError(f"{who}: chain indices out of bounds")
        return [int(c) for c in arr]

    try:
        n = len(chains)
    except TypeError:
        raise ValueError("chains must be one chain (a sequence of integers) or a sequence of Q chains") from None
    first = chains[0] if n else None
    if n and (isinstance(first, (int, np.integer)) or (isinstance(chains, np.ndarray) and chains.ndim == 1)):
        lists = [one(chains, "chain")] * Q
    else:
        if n != Q:
            raise ValueError(f"chains must be one chain or hold {Q} chains, got {n}")
        lists = [one(chains[q], f"query {q}") for q in range(Q)]
    offsets = np.zeros(Q + 1, dtype=np.int64)
    np.cumsum([len(ch) for ch in lists], out=offsets[1:])
    nodes = np.array([c for ch in lists for c in ch], dtype=np.int32)
    return lists, offsets, nodes


def chain_weights_one(w, n_edges: int, who: str) -> np.ndarray:
    """One chain's weights as add_chain checks them: n_edges finite floats, as float32."""
    w = np.asarray(w, dtype=np.float32).reshape(-1)
    if w.size != n_edges:
        raise ValueError(f"{who}: weights length must equal len(chain)-1")
    if not np.all(np.isfinite(w)):
        raise ValueError(f"{who}: chain weights must be finite")
    return w


def chain_weights_flat(wlists, edge_offsets):
    """Per-query weights (None or an array each) flat over the chains' edges, or None when no query has any; None beside
    given weights: ones."""
    if not any(w is not None for w in wlists):
        return None
    weights = np.ones(max(int(edge_offsets[-1]), 1), dtype=np.float32)
    for q, w in enumerate(wlists):
        if w is not None:
            weights[int(edge_offsets[q]):int(edge_offsets[q + 1])] = w
    return weights


def chain_prior_weights(chain_weights, chains, lists, edge_offsets):
    """chain_receipt_many's `chain_weights` for its `chains` (parsed into `lists`): None, one list shared with a shared chain,
    or a sequence parallel to `chains` of None or len(chain) - 1 finite floats.  Returns the flat float32 weights or None."""
    Q = len(lists)
    if chain_weights is None:
        return None
    shared = Q > 0 and len(chains) > 0 and (isinstance(chains[0], (int, np.integer)) or
                                            (isinstance(chains, np.ndarray) and chains.ndim == 1))
    if shared:
        w = chain_weights_one(chain_weights, len(lists[0]) - 1, "chain")
        return chain_weights_flat([w] * Q, edge_offsets)
    try:
        n = len(chain_weights)
    except TypeError:
        n = -1
    if n != Q:
        raise ValueError(f"chain_weights must be None or hold {Q} entries parallel to chains, got {n}")
    wl = [None if chain_weights[q] is None else chain_weights_one(chain_weights[q], len(lists[q]) - 1, f"query {q}")
          for q in range(Q)]
    return chain_weights_flat(wl, edge_offsets)


def check_prior_lamP(fn: str, lamP, own_chain: bool) -> None:
    """What every batched call with a chain prior asks of `lamP` and of the lattice it runs on."""
    if not np.isfinite(float(lamP)) or float(lamP) < 0:
        raise ValueError("lamP must be >= 0")
    if own_chain:
        raise ValueError(f"{fn} with lamP: the lattice has a chain of its own (clear_chain first)")


def check_prior_args(fn: str, chains, lamP, chain_weights, own_chain: bool) -> bool:
    """bundle_many's and receipt_many's optional `chains` / `lamP` / `chain_weights`: True when the call carries a prior (both
    of `chains` and `lamP` given), or the ValueError for a partial set."""
    if chains is None and lamP is None:
        if chain_weights is not None:
            raise ValueError("chain_weights given without chains and lamP")
        return False
    if lamP is None:
        raise ValueError("chains given without lamP")
    if chains is None:
        raise ValueError("lamP given without chains")
    check_prior_lamP(fn, lamP, own_chain)
    return True


def prior_chain_block(chains, chain_weights, Q: int, N: int):
    """`chains` and `chain_weights` of a call with a chain prior as (lists, offsets, nodes, weights): chain_block's three, the
    flat float32 weights of chain_prior_weights (or None), and the ValueError for a chain of more than MAX_PRIOR_NODES
    distinct nodes."""
    lists, offsets, nodes = chain_block(chains, Q, N)
    weights = chain_prior_weights(chain_weights, chains, lists, offsets - np.arange(Q + 1, dtype=np.int64))
    checked = set()  # (a shared chain is one list Q times)
    for q, ch in enumerate(lists):
        if id(ch) not in checked and len(set(ch)) > MAX_PRIOR_NODES:
            raise ValueError(f"query {q}: with lamP a chain has at most {MAX_PRIOR_NODES} distinct nodes, got {len(set(ch))}")
        checked.add(id(ch))
    return lists, offsets, nodes, weights


def chain_receipt_dict(chain, *, weakest_k, weakest_z, gain, verdict, z_struct, z_path, r_struct, r_path) -> dict[str, Any]:
    """chain_receipt()'s dict (lattice.py:466-528) for one chain from the device's numbers: the per-edge arrays hold the
    chain's len(chain) - 1 edges; weakest_k = -1 (no edge's max(z) exceeds -1) reads edge [-1, -1]."""
    wk = int(weakest_k)
    return {
        "verdict": bool(verdict),
        "weakest_link": {"k": wk, "edge": [chain[wk], chain[wk + 1]] if wk >= 0 else [-1, -1], "zscore": float(weakest_z)},
        "coherence_gain": float(gain),
        "edges": [{"k": t, "edge": [chain[t], chain[t + 1]], "z_struct": float(z_struct[t]), "z_path": float(z_path[t]),
                   "r_struct": float(r_struct[t]), "r_path": float(r_path[t])} for t in range(len(chain) - 1)],
    }


def chain_receipt_dicts(chains, arr: dict) -> list[dict[str, Any]]:
    """Q chain receipts from the `as_arrays` form (chain_offsets over edges, the flat per-edge arrays, the per-query
    scalars); chains: per query the chain as a list of ints."""
    out = []
    for q, ch in enumerate(chains):
        s, e = int(arr["chain_offsets"][q]), int(arr["chain_offsets"][q + 1])
        out.append(chain_receipt_dict(ch, weakest_k=arr["chain_weakest_k"][q], weakest_z=arr["chain_weakest_z"][q],
                                      gain=arr["chain_gain"][q], verdict=arr["chain_verdict"][q],
                                      **{k[len("chain_"):]: arr[k][s:e] for k in CHAIN_EDGE_KEYS}))
    return out


def bundle_dicts(ids, score, align) -> list[dict[str, Any]]:
    """One query's bundle, the list of {"id", "score", "align"} that bundle() returns, from three parallel 1-D arrays."""
    return [{"id": int(i), "score": float(s), "align": float(a)}
            for i, s, a in zip(ids.tolist(), score.tolist(), align.tolist())]


def _ptr(a: np.ndarray, ctype):
    return a.ctypes.data_as(C.POINTER(ctype))


class ReceiptArrays:
    """The receipt buffers of a batch of Q queries, as osc_receipt_many and osc_corpus_refine_receipts fill them: the
    (4, Q) float64 sums (deltaH, coh, anchor, query), the null totals, the offsets of the kept null points and those
    points, `slots` per query at most (0 = light detail: none).  `settle=True` adds the per-query settle report that the
    Corpus entry points write in front."""

    def __init__(self, Q: int, slots: int, settle: bool = False):
        self.full = slots > 0
        self.capacity = Q * slots
        self.settle = (np.zeros(Q, dtype=np.int32), np.zeros(Q, dtype=np.float32)) if settle else None
        self.sums = np.zeros((4, Q), dtype=np.float64)
        self.total = np.zeros(Q, dtype=np.int32)
        self.offsets = np.zeros(Q + 1, dtype=np.int64)
        n = max(self.capacity, 1)
        self.i, self.j = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        self.z, self.r = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)

    def pointers(self) -> list:
        """The arrays in the entry points' order, the capacity last."""
        head = [] if self.settle is None else [_ptr(self.settle[0], C.c_int32), _ptr(self.settle[1], C.c_float)]
        return [*head, *[_ptr(self.sums[t], C.c_double) for t in range(4)], _ptr(self.total, C.c_int32),
                _ptr(self.offsets, C.c_int64), _ptr(self.i, C.c_int32), _ptr(self.j, C.c_int32), _ptr(self.z, C.c_float),
                _ptr(self.r, C.c_float), int(self.capacity)]

    def round_sums(self) -> None:
        """Once the native call has returned: the float32 rounding receipt() gives its energies (a float32 dH / np.sum
        over float32 rows)."""
        self.sums = self.sums.astype(np.float32).astype(np.float64)

    @property
    def kept(self) -> int:
        return int(self.offsets[-1])

    def scalar_arrays(self) -> dict[str, np.ndarray]:
        """The per-query scalars of the `as_arrays` form."""
        head = {} if self.settle is None else dict(settle_iters=self.settle[0], settle_res=self.settle[1])
        return dict(head, deltaH=self.sums[0], coh_drop_sum=self.sums[1], anchor_pen_sum=self.sums[2],
                    query_term_sum=self.sums[3])

    def null_arrays(self) -> dict[str, np.ndarray]:
        """The null points of the `as_arrays` form (full detail): every query's kept points, concatenated."""
        n = self.kept
        return dict(null_total=self.total.astype(np.int64), null_offsets=self.offsets, null_i=self.i[:n].copy(),
                    null_j=self.j[:n].copy(), null_z=self.z[:n].copy(), null_r=self.r[:n].copy())

    def nulls(self, q: int):
        """(query q's null point dicts, its total before the cap); ([], 0) in light detail."""
        if not self.full:
            return [], 0
        s, e = int(self.offsets[q]), int(self.offsets[q + 1])
        return null_dicts(self.i[s:e], self.j[s:e], self.z[s:e], self.r[s:e], e - s), int(self.total[q])


def degree_stats(nnz: int, n: int) -> dict[str, float]:
    return {"avg_degree": float(nnz / max(n, 1)), "edge_density": float(nnz / max(n * (n - 1), 1))}


def gate_stats(B: np.ndarray) -> dict[str, Any]:
    return {"gates_min": float(np.min(B)), "gates_max": float(np.max(B)), "gates_mean": float(np.mean(B)),
            "gates_uniform": bool(np.allclose(B, B[0]))}


def meta(*, ustar_cached, ustar_solves, ustar_cache_hits, ustar: dict, ustar_solve_ms, ustar_source: Optional[str] = None,
         graph_build_ms, last_settle_ms, degree: dict, gates: dict, state_sig: str, receipt_detail: str,
         null_points_summary: dict) -> dict[str, Any]:
    """A receipt's `meta`.  ustar = {"ustar_iters", "ustar_res", "ustar_converged"} (what sign() signs in extended mode);
    degree, gates = degree_stats() / gate_stats(), which a batch on one graph forms once; `ustar_source` only if given."""
    m = {
        "ustar_cached": bool(ustar_cached),
        "ustar_solves": int(ustar_solves),
        "ustar_cache_hits": int(ustar_cache_hits),
        "ustar_converged": ustar["ustar_converged"],
        "ustar_res": ustar["ustar_res"],
        "ustar_iters": ustar["ustar_iters"],
        "ustar_solve_ms": float(ustar_solve_ms),
        "ustar_source": ustar_source,
        "graph_build_ms": float(graph_build_ms),
        "last_settle_ms": float(last_settle_ms),
        **degree,
        **gates,
        "state_sig": state_sig,
        "receipt_detail": receipt_detail,
        "null_points_summary": null_points_summary,
    }
    if ustar_source is None:  # receipt(): the reference's keys and no more
        del m["ustar_source"]
    return m


def sign(meta: dict, secret: Optional[bytes], mode: str, *, state_sig: str, deltaH: float, ustar: dict, params: dict,
         graph: dict) -> None:
    """meta["signature"] = the HMAC-SHA256 block over the minimal or extended payload (lattice.py:380-418); nothing
    without a secret."""
    if secret is None:
        return
    payload = {"sig_v": 1, "mode": "minimal", "state_sig": state_sig, "deltaH_total": float(deltaH)}
    if mode == "extended":
        payload = {**payload, "mode": "extended", **ustar, "params": params, "graph": graph}
    raw = json.dumps(payload, sort_keys=True).encode("utf-8")
    meta["signature"] = {"algorithm": "HMAC-SHA256", "payload": payload,
                         "signature": hmac.new(secret, raw, hashlib.sha256).hexdigest()}


def record(*, version, deltaH, coh_drop_sum, anchor_pen_sum, query_term_sum, cg_iters, residual, t_ms, null_points,
           meta: dict) -> dict[str, Any]:
    """The receipt itself; callers append meta["dynamics"] afterwards."""
    return {
        "version": str(version),
        "deltaH_total": float(deltaH),
        "coh_drop_sum": float(coh_drop_sum),
        "anchor_pen_sum": float(anchor_pen_sum),
        "query_term_sum": float(query_term_sum),
        "cg_iters": int(cg_iters),
        "residual": float(residual),
        "t_ms": float(t_ms),
        "null_points": null_points,
        "meta": meta,
    }

"""`Corpus` -- the reference's retrieval loop (scripts/bench_beir.py:84-94, examples/rag_replacement.py:48-66) as one
batched device call per chunk of queries.

For each query the loop takes the top-K cosine candidates of a corpus, builds `Oscillink(Y[cand], ...)`, sets the query
and asks for `bundle(k, alpha)`.  Every query has its own K-row graph, so the shared-graph batching of `bundle_many`
does not apply; here every lattice of a chunk is built, solved and bundled by the same few launches.
"""
from __future__ import annotations

import ctypes as C
import hashlib
import operator
import os
from typing import Any, Optional

import numpy as np

from . import _masks as mk
from . import _native as nat
from . import _receipts as rc

MAX_TOP_K = 1024  # one key per thread of the per-query select (include/oscillink_hip.h)
MAX_KNEIGHBORS = 128  # the dense build route's per-row list (k_knn_select)
MAX_D = 1536  # the bundle kernel keeps the normalised query in LDS
USTAR_TOL, USTAR_MAX_ITERS = 1e-4, 64  # _ensure_device_ustar's settings
GATE_METHODS = {"direct": 0, "cg": 1}  # osc_corpus_gates' method codes
RECEIPT_DETAILS = {"light": 0, "full": 1}  # osc_corpus_refine_receipts' detail codes (set_receipt_detail's words)
RECEIPT_Z_TH = 3.0  # receipt()'s null-point threshold
EDGE_PREFIX = 2048  # edges under the state signature (OscillinkLattice._edge_prefix)
MAX_CHAIN = rc.MAX_CHAIN


class _RefineOut:
    """The result arrays of one refine_many call, zeroed, and the two forms every path hands them back in."""

    def __init__(self, Q: int, K: int, kk: int, gated: bool, rows: Optional[np.ndarray] = None,
                 picks: Optional[np.ndarray] = None):
        self.gated = gated
        self.rows = rows  # a ragged call's rows per lattice (int32 (Q,)), else None
        self.picks = picks  # a call with a per-query k: min(k[q], n_q) picks per lattice (int32 (Q,)), else None
        self.cand = np.zeros((Q, K), dtype=np.int32)
        self.local = np.zeros((Q, kk), dtype=np.int32)
        self.score = np.zeros((Q, kk), dtype=np.float32)
        self.align = np.zeros((Q, kk), dtype=np.float32)
        self.iters = np.zeros(Q, dtype=np.int32)
        self.res = np.zeros(Q, dtype=np.float32)
        self.g = np.zeros((Q, K), dtype=np.float32)
        self.g_iters = np.zeros(Q, dtype=np.int32)
        self.g_res = np.zeros(Q, dtype=np.float32)

    def pointers(self, gated: bool):
        """The arrays in the entry points' order: the gated ones take the gates second and the gate solves' report last."""
        p = [nat.i32(self.cand), nat.i32(self.local), nat.f32(self.score), nat.f32(self.align), nat.i32(self.iters),
             nat.f32(self.res)]
        return p if not gated else [p[0], nat.f32(self.g), *p[1:], nat.i32(self.g_iters), nat.f32(self.g_res)]

    def ids_and_arrays(self):
        """(ids, the `as_arrays` dict without receipts) once the native call has filled the arrays."""
        Q, kk = self.local.shape
        ids = np.take_along_axis(self.cand, self.local, axis=1) if kk else np.zeros((Q, 0), dtype=np.int32)
        if (self.rows is not None or self.picks is not None) and kk:  # behind a query's picks `local` is -1, and so is the id
            ids = np.where(self.local >= 0, np.take_along_axis(self.cand, np.maximum(self.local, 0), axis=1),
                           np.int32(-1)).astype(np.int32)
        out = {"ids": ids, "local": self.local, "score": self.score, "align": self.align, "candidates": self.cand,
               "ustar_iters": self.iters, "ustar_res": self.res}
        if self.rows is not None:
            out["rows"] = self.rows
        if self.picks is not None:
            out["picks"] = self.picks
        if self.gated:
            out.update(gates=self.g, gate_iters=self.g_iters, gate_res=self.g_res)
        return ids, out

    def bundles(self, ids):
        """Per query the list of {"id", "score", "align"} that bundle() returns."""
        if self.rows is not None or self.picks is not None:  # min(k, n_q) entries per query
            n = self.picks if self.picks is not None else np.minimum(self.rows, ids.shape[1])
            return [rc.bundle_dicts(ids[q, :n[q]], self.score[q, :n[q]], self.align[q, :n[q]]) for q in range(ids.shape[0])]
        return [rc.bundle_dicts(ids[q], self.score[q], self.align[q]) for q in range(ids.shape[0])]


class Corpus:
    """A corpus Y (N x D, finite) resident on the device as Y and its row-normalised copy Yn (osc_create's arithmetic),
    both at a row pitch of D rounded up to 32 floats: 8 N ceil32(D) bytes, no lattice solver arrays.  Per call, queries
    run in chunks whose scratch stays under 1 GiB (OSC_CORPUS_CHUNK, read at creation, caps the queries per chunk).

    The corpus can change: ids are row positions, `append` adds rows at the end, `remove`
    tombstones rows without moving the others, `compact` drops the tombstones and renumbers.  `N` counts rows including
    tombstones, `n_live` the others; the very next call sees the change."""

    _n_removed = 0  # tombstones among the N rows (the native handle's N - n_live)
    _alive = None  # alive()'s array, kept until the next append / remove / compact

    def __init__(self, Y: np.ndarray, *, device: Optional[int] = None):
        if not isinstance(Y, np.ndarray) or Y.ndim != 2 or Y.shape[0] < 1 or Y.shape[1] < 1:
            raise ValueError("Y must be a non-empty 2D numpy array")
        Yc = np.ascontiguousarray(Y, dtype=np.float32)
        if not np.all(np.isfinite(Yc)):
            raise ValueError("Y must be finite")
        self.N, self.D = Yc.shape
        if self.D > MAX_D:
            raise ValueError(f"Corpus supports D <= {MAX_D}, got {self.D}")
        if device is None:
            device = int(os.environ.get("OSCILLINK_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        self._h = None
        L = nat.lib()
        if nat.device_count() < 1:
            raise nat.NativeError("no HIP device visible: oscillink_amd runs on MI355X (gfx950) only, no CPU fallback")
        h = nat.Handle()
        rc = L.osc_corpus_create(nat.f32(Yc), self.N, self.D, int(device), C.byref(h))
        if rc != nat.OSC_OK:
            msg = L.osc_corpus_last_error(None)
            text = msg.decode("utf-8", "replace") if msg else "osc_corpus_create"
            if rc == nat.OSC_E_INVALID:
                raise ValueError(text)
            raise nat.NativeError(f"osc_corpus_create failed ({rc}): {text}")
        self._h = h

    # ------------------------------------------------------------------ lifetime
    def close(self) -> None:
        h = getattr(self, "_h", None)
        if h is not None:
            try:
                nat.lib().osc_corpus_destroy(h)
            finally:
                self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self) -> "Corpus":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def _call_filtered(self, allow: Optional[np.ndarray], name: str, *args, ragged: Optional[np.ndarray] = None,
                       settings: Optional[np.ndarray] = None) -> None:
        """_call(name, ...) with `allow` (_allow's words or None) armed as the call's filter: the native call consumes it.
        ragged = the rows per lattice (int32 (Q,)) of a ragged call, which is armed as such; afterwards the counts the native
        call used are read back and must be these.  settings = _settings' records (one per query) of a call with per-query
        settings, armed the same way; None arms nothing."""
        if allow is not None:
            self._call("osc_corpus_filter", nat.u32(allow), allow.shape[0], allow.shape[1])
        if ragged is not None:  # with a filter the native side derives the counts itself
            self._call("osc_corpus_ragged", None if allow is not None else nat.i32(ragged), int(ragged.shape[0]))
        if settings is not None:
            self._call("osc_corpus_settings", settings.ctypes.data_as(C.c_void_p), int(settings.shape[0]))
        self._call(name, *args)
        if ragged is not None:
            used = np.zeros_like(ragged)
            self._call("osc_corpus_ragged_rows", nat.i32(used), int(used.shape[0]))
            if not np.array_equal(used, ragged):
                raise nat.NativeError(f"{name}: the native call used other row counts than the ones checked here")

    def _call(self, name: str, *args) -> None:
        if self._h is None:
            raise ValueError("Corpus is closed")
        rc = getattr(nat.lib(), name)(self._h, *args)
        if rc == nat.OSC_OK:
            return
        msg = nat.lib().osc_corpus_last_error(self._h)
        text = (msg.decode("utf-8", "replace") if msg else "") or name
        if rc == nat.OSC_E_INVALID:
            raise ValueError(text)
        raise nat.NativeError(f"{name} failed ({rc}): {text}")

    # ------------------------------------------------------------------ validation
    def _queries(self, psis) -> np.ndarray:
        if self._h is None:
            raise ValueError("Corpus is closed")
        return rc.check_queries(psis, self.D)

    def _top_k(self, top_k: int) -> int:
        if int(top_k) < 1 or int(top_k) > MAX_TOP_K:
            raise ValueError(f"top_k must be between 1 and {MAX_TOP_K}, got {top_k}")
        n_live = self.n_live
        if n_live == 0:
            raise ValueError("the corpus has no live rows")
        return min(int(top_k), n_live)

    @staticmethod
    def _knn(kneighbors: int, K: int) -> int:
        if int(kneighbors) < 1:
            raise ValueError("kneighbors must be >= 1")
        eff = min(int(kneighbors), max(1, K - 1))
        if eff > MAX_KNEIGHBORS:
            raise ValueError(f"min(kneighbors, K - 1) = {eff} exceeds the limit of {MAX_KNEIGHBORS} (the dense route)")
        return eff

    def _candidates(self, candidates, Q: int, K: int) -> np.ndarray:
        cand = np.asarray(candidates)
        if cand.shape != (Q, K):
            raise ValueError(f"candidates must be a ({Q}, {K}) array, got shape {cand.shape}")
        if cand.size and (not np.issubdtype(cand.dtype, np.integer)):
            raise ValueError("candidates must hold integer corpus ids")
        cand = np.ascontiguousarray(cand, dtype=np.int64)
        if cand.size and (cand.min() < 0 or cand.max() >= self.N):
            raise ValueError(f"candidates: corpus ids must lie in [0, {self.N})")
        if cand.size and self.n_live < self.N:
            dead = ~self._alive_mask()[cand]
            if dead.any():
                q, j = np.argwhere(dead)[0]
                raise ValueError(f"candidates: query {int(q)} names removed id {int(cand[q, j])}")
        if cand.size and np.any(np.diff(np.sort(cand, axis=1), axis=1) == 0):
            raise ValueError("candidates: repeated id within a row")
        return cand.astype(np.int32)

    def _candidates_ragged(self, candidates, Q: int, K: int):
        """`candidates` of a ragged call -- Q integer sequences of 1 .. K ids each, or the (Q, K) integer array with -1
        behind each row's ids -- as (the (Q, K) int32 array padded with -1, the rows per query int32 (Q,)); _candidates'
        checks on the real entries."""
        if isinstance(candidates, np.ndarray) and candidates.ndim == 2:
            if candidates.shape != (Q, K):
                raise ValueError(f"candidates must be a ({Q}, {K}) array or {Q} sequences, got shape {candidates.shape}")
            if candidates.size and not np.issubdtype(candidates.dtype, np.integer):
                raise ValueError("candidates must hold integer corpus ids")
            lists = []
            for q in range(Q):
                row = candidates[q]
                n = int(np.argmax(row < 0)) if (row < 0).any() else K
                if np.any(row[n:] != -1):
                    raise ValueError(f"candidates: query {q} has an id behind a -1 (the padding is -1, behind the ids)")
                lists.append(row[:n])
        else:
            try:
                lists = [np.asarray(row) for row in candidates]
            except TypeError:
                lists = None
            if lists is None or len(lists) != Q:
                raise ValueError(f"candidates must be a ({Q}, {K}) array or {Q} sequences of ids")
        cand = np.full((Q, K), -1, dtype=np.int64)
        rows = np.zeros(Q, dtype=np.int32)
        for q, row in enumerate(lists):
            if row.ndim != 1 or (row.size and not np.issubdtype(row.dtype, np.integer)):
                raise ValueError("candidates must hold integer corpus ids")
            if row.size < 1 or row.size > K:
                raise ValueError(f"candidates: query {q} has {row.size} ids, need 1 .. K = {K}")
            if row.min() < 0 and np.any(row[int(np.argmax(row < 0)):] >= 0):
                raise ValueError(f"candidates: query {q} has an id behind a -1 (the padding is -1, behind the ids)")
            if row.min() < 0 or row.max() >= self.N:
                raise ValueError(f"candidates: corpus ids must lie in [0, {self.N})")
            if self.n_live < self.N and not self._alive_mask()[row].all():
                raise ValueError(f"candidates: query {q} names removed id {int(row[~self._alive_mask()[row]][0])}")
            if np.unique(row).size != row.size:
                raise ValueError("candidates: repeated id within a row")
            cand[q, :row.size] = row
            rows[q] = row.size
        return cand.astype(np.int32), rows

    def _allow(self, allow, candidates, Q: int, K: int) -> Optional[np.ndarray]:
        """The `allow` argument of search / refine_many / diffusion_gates_many as the native filter's words, (1, W) for
        one filter or (Q, W) for one per query, or None; checked before any device work."""
        return self._allow_rows(allow, candidates, Q, K, False)[0]

    def _allow_rows(self, allow, candidates, Q: int, K: int, ragged: bool):
        """(_allow's words, the rows per lattice of a ragged call or None).  ragged: a query keeps its min(K, eligible)
        rows, and only a query without any eligible row is an error."""
        if allow is None:
            return None, (np.full(Q, K, dtype=np.int32) if ragged else None)
        if candidates is not None:
            raise ValueError("allow cannot be combined with candidates")
        a = np.asarray(allow)
        if a.dtype != np.bool_:
            raise ValueError(f"allow must be a bool array, got dtype {a.dtype}")
        if a.shape != (self.N,) and a.shape != (Q, self.N):
            raise ValueError(f"allow must have shape ({self.N},) or ({Q}, {self.N}), got {a.shape}")
        counts = np.atleast_2d(a & self._alive_mask()).sum(axis=1)
        short = np.flatnonzero(counts < (1 if ragged else K))
        if short.size and Q:
            q = int(short[0])
            raise ValueError(f"allow: query {q} has {int(counts[q])} eligible rows (live and allowed), fewer than K = {K}")
        rows = np.broadcast_to(np.minimum(counts, K), (Q,)).astype(np.int32) if ragged else None
        return mk.pack_mask(a), rows

    # refine_many's arguments that may be given per query, with the scalar's own check of one value (None = passes)
    _PER_QUERY = {
        "lamG": lambda v: None if v > 0 else "lamG must be > 0 for SPD",
        "lamC": lambda v: None if v >= 0 and np.isfinite(v) else "lamC must be >= 0",
        "lamQ": lambda v: None if v >= 0 and np.isfinite(v) else "lamQ must be >= 0",
        "lamP": lambda v: None if v >= 0 and np.isfinite(v) else "lamP must be >= 0",
        "kneighbors": lambda v: None if v >= 1 else "kneighbors must be >= 1",
        "k": lambda v: None,
        "alpha": lambda v: None if np.isfinite(v) else "alpha must be finite",
        "settle_dt": lambda v: None if np.isfinite(v) and v > 0 else "settle_dt must be finite and > 0",
        "settle_max_iters": lambda v: None if v >= 1 else "settle_max_iters must be >= 1",
        "settle_tol": lambda v: None if np.isfinite(v) else "settle_tol must be finite",
    }
    _PER_QUERY_INT = ("kneighbors", "k", "settle_max_iters")
    _PER_QUERY_DEFAULTS = {"lamG": 1.0, "lamC": 0.5, "lamQ": 4.0, "lamP": 0.2, "kneighbors": 6, "k": 8, "alpha": 0.5,
                           "settle_dt": 1.0, "settle_max_iters": 12, "settle_tol": 1e-3}

    @classmethod
    def _settings(cls, Q: int, K: int, **given):
        """The arguments of `_PER_QUERY` as given to refine_many / diffusion_gates_many (a subset for the latter; the rest
        take refine_many's defaults).  None when every one is a scalar (a 0-d array and a NumPy scalar are scalars): the
        call is the scalar call.  Otherwise (records, named, raw): `records` = Q osc_corpus_setting records, every value checked
        as the scalar is with the first offending query in the message, before any native call; `named` = the names that
        were given per query; `raw` = per name the Q values as Python numbers, as given (what a state signature holds)."""
        named = [n for n, v in given.items() if np.ndim(v) != 0]
        if not named:
            return None
        rec = np.zeros(Q, dtype=nat.SETTING_DTYPE)
        raw = {}
        for name, check in cls._PER_QUERY.items():
            v = np.asarray(given.get(name, cls._PER_QUERY_DEFAULTS[name]))
            if v.ndim != 0 and v.shape != (Q,):
                raise ValueError(f"{name} must be a scalar or a ({Q},) array, got shape {v.shape}")
            if not (np.issubdtype(v.dtype, np.number) or v.dtype == np.bool_) or np.issubdtype(v.dtype, np.complexfloating):
                raise ValueError(f"{name} must hold real numbers, got dtype {v.dtype}")
            raw[name] = v.tolist() if v.ndim else [given.get(name, cls._PER_QUERY_DEFAULTS[name])] * Q
            v = np.broadcast_to(v, (Q,))
            if name in cls._PER_QUERY_INT:  # int(x)'s truncation, as the scalar path; NaN / inf cannot be converted
                if not np.all(np.isfinite(v)):
                    raise ValueError(f"query {int(np.flatnonzero(~np.isfinite(v))[0])}: {name} must be an integer")
                col = np.clip(np.trunc(v).astype(np.int64), -2**31, 2**31 - 1).astype(np.int32)
            else:
                col = v.astype(np.float32)
            for q in range(Q):
                msg = check(col[q])
                if msg is not None:
                    raise ValueError(f"query {q}: {msg}")
            rec[name] = col
        for q in range(Q):
            eff = min(int(rec["kneighbors"][q]), max(1, K - 1))
            if eff > MAX_KNEIGHBORS:
                raise ValueError(f"query {q}: min(kneighbors, K - 1) = {eff} exceeds the limit of {MAX_KNEIGHBORS} "
                                 "(the dense route)")
        return rec, named, raw

    @staticmethod
    def _gate_settings(beta, gamma, method, max_iters, prefix: str = ""):
        """(beta, gamma, method code, max_iters) of a diffusion-gate solve, checked as compute_diffusion_gates checks
        them; `prefix` turns the names into refine_many's (gate_gamma, ...)."""
        if not float(gamma) > 0 or not np.isfinite(float(gamma)):
            raise ValueError(f"{prefix}gamma must be > 0 for SPD")
        if not np.isfinite(float(beta)):
            raise ValueError(f"{prefix}beta must be finite")
        if method not in GATE_METHODS:
            raise ValueError(f"{prefix}method must be 'direct' or 'cg', got {method!r}")
        if int(max_iters) < 1:
            raise ValueError(f"{prefix}max_iters must be >= 1")
        return float(beta), float(gamma), GATE_METHODS[method], int(max_iters)

    @staticmethod
    def _receipt_settings(receipts, settle_dt, settle_max_iters, settle_tol):
        """(detail code or None, dt, max_iters, tol) of refine_many's receipts arguments, checked before any native call."""
        if receipts is not None and (not isinstance(receipts, str) or receipts not in RECEIPT_DETAILS):
            raise ValueError(f"receipts must be None, 'light' or 'full', got {receipts!r}")
        if not np.isfinite(float(settle_dt)) or not float(settle_dt) > 0:
            raise ValueError("settle_dt must be finite and > 0")
        if int(settle_max_iters) < 1:
            raise ValueError("settle_max_iters must be >= 1")
        if not np.isfinite(float(settle_tol)):
            raise ValueError("settle_tol must be finite")
        return (None if receipts is None else RECEIPT_DETAILS[receipts], float(settle_dt), int(settle_max_iters),
                float(settle_tol))

    @staticmethod
    def _chains(chains, chain_weights, lamP, chain_z_th, Q: int, K: int, rows: Optional[np.ndarray] = None):
        """refine_many's chain arguments, checked as add_chain checks them (with the query index in front), as the entry
        point's chain block: None without chains, else a dict of `offsets` int64 (Q + 1, over nodes), `nodes` int32,
        `weights` float32 per chain edge or None, `edge_offsets` int64 (Q + 1), `lists` (per query the chain or None),
        `lamP` and `z_th`."""
        if chains is None:
            if chain_weights is not None:
                raise ValueError("chain_weights given without chains")
            return None
        if float(lamP) < 0 or not np.isfinite(float(lamP)):
            raise ValueError("lamP must be >= 0")
        if not np.isfinite(float(chain_z_th)):
            raise ValueError("chain_z_th must be finite")
        if isinstance(chains, np.ndarray) and chains.ndim == 2:
            if chains.shape[0] != Q or (chains.size and not np.issubdtype(chains.dtype, np.integer)):
                raise ValueError(f"chains must hold {Q} entries (None or a sequence of integers each), or be a ({Q}, L) "
                                 f"integer array; got an array of shape {chains.shape}, dtype {chains.dtype}")
            chains = list(chains)
        try:
            n = len(chains)
        except TypeError:
            n = -1
        if n != Q:
            raise ValueError(f"chains must hold {Q} entries (None or a sequence of integers each), or be a ({Q}, L) integer "
                             f"array; got {n if n >= 0 else type(chains).__name__}")
        if chain_weights is not None and len(chain_weights) != Q:
            raise ValueError(f"chain_weights must be None or hold {Q} entries parallel to chains, got {len(chain_weights)}")
        lists, wlists = [], []
        for q in range(Q):
            ch = chains[q]
            w = None if chain_weights is None else chain_weights[q]
            if ch is None:
                if w is not None:
                    raise ValueError(f"query {q}: weights given without a chain")
                lists.append(None)
                wlists.append(None)
                continue
            try:
                ch = [int(operator.index(c)) for c in ch]
            except TypeError:
                raise ValueError(f"query {q}: chain must be None or a sequence of integers") from None
            if any((c < 0 or c >= (K if rows is None else int(rows[q]))) for c in ch):
                raise ValueError(f"query {q}: chain indices out of bounds")
            if len(ch) < 2:
                raise ValueError(f"query {q}: chain must contain at least two indices")
            if len(ch) > MAX_CHAIN:
                raise ValueError(f"query {q}: a chain has at most {MAX_CHAIN} indices, got {len(ch)}")
            if w is not None:
                w = rc.chain_weights_one(w, len(ch) - 1, f"query {q}")
            lists.append(ch)
            wlists.append(w)
        lens = np.array([0 if ch is None else len(ch) for ch in lists], dtype=np.int64)
        offsets = np.zeros(Q + 1, dtype=np.int64)
        np.cumsum(lens, out=offsets[1:])
        edge_offsets = np.zeros(Q + 1, dtype=np.int64)
        np.cumsum(np.maximum(lens - 1, 0), out=edge_offsets[1:])
        nodes = np.array([c for ch in lists if ch is not None for c in ch], dtype=np.int32)
        weights = rc.chain_weights_flat(wlists, edge_offsets)
        return {"offsets": offsets, "nodes": nodes if nodes.size else np.zeros(1, dtype=np.int32), "weights": weights,
                "edge_offsets": edge_offsets, "lists": lists, "lamP": float(lamP), "z_th": float(chain_z_th)}

    @staticmethod
    def _warn_non_finite(gates: np.ndarray, iters: np.ndarray, res: np.ndarray, what: str) -> None:
        bad = np.nonzero(~np.all(np.isfinite(gates), axis=1))[0]
        if bad.size:  # compute_diffusion_gates hands such gates back with a warning as well
            import warnings

            q = int(bad[0])
            warnings.warn(f"{what}: the screened-diffusion solve of query {q} produced non-finite values "
                          f"(iters={int(iters[q])}, res={float(res[q])!r}; {bad.size} queries in all); returned as "
                          "computed, like the reference's cg path", RuntimeWarning, stacklevel=3)

    # ------------------------------------------------------------------ public API
    def search(self, psis, top_k: int, *, allow=None, ragged: bool = False):
        """Per query the K = min(top_k, n_live) corpus ids of the largest cosine Yn_i . psi / (|psi| + 1e-12) (fp32 on the
        device), ties to the smaller id, in that order.  Returns (ids int32 (Q, K), cos float32 (Q, K)).

        Removed rows are never returned.  `allow` narrows the search on the device: a bool array (N,) for every query or
        (Q, N) with one row per query; a row is eligible iff it is live and allowed, and the order within the eligible rows
        is the same.  Every query needs at least K eligible rows (ValueError naming the first query that has fewer).

        `ragged=True` lifts that: a query with n < K eligible rows gets all n of them, in the same
        order, with -1 in `ids` and 0 in `cos` behind them; only a query without any eligible row is an error.  Returns
        (ids, cos, rows) with rows int32 (Q,) = min(K, eligible rows)."""
        P = self._queries(psis)
        K = self._top_k(top_k)
        Q = P.shape[0]
        words, rows = self._allow_rows(allow, None, Q, K, bool(ragged))
        ids = np.zeros((Q, K), dtype=np.int32)
        cos = np.zeros((Q, K), dtype=np.float32)
        if Q:
            self._call_filtered(words, "osc_corpus_search", nat.f32(P), Q, int(top_k), nat.i32(ids), nat.f32(cos), ragged=rows)
        return (ids, cos, rows) if ragged else (ids, cos)

    # ------------------------------------------------------------------ rows
    @property
    def n_live(self) -> int:
        """Rows that have not been removed."""
        if self._h is None:
            raise ValueError("Corpus is closed")
        return self.N - self._n_removed

    @property
    def capacity(self) -> int:
        """Rows the device buffers hold before an append has to move them."""
        n, live, cap = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._call("osc_corpus_rows", C.byref(n), C.byref(live), C.byref(cap))
        assert (int(n.value), int(live.value)) == (self.N, self.N - self._n_removed)
        return int(cap.value)

    def _alive_mask(self) -> np.ndarray:
        if self._h is None:
            raise ValueError("Corpus is closed")
        if self._alive is None and self._n_removed == 0:
            self._alive = np.ones(self.N, dtype=bool)
        if self._alive is None:
            words = np.zeros(mk.words_for(self.N), dtype=np.uint32)
            self._call("osc_corpus_get_live", nat.u32(words))
            self._alive = mk.unpack_mask(words, self.N)
        return self._alive

    def alive(self) -> np.ndarray:
        """bool (N,): True for the rows that have not been removed."""
        return self._alive_mask().copy()

    def append(self, Ynew) -> np.ndarray:
        """Adds the rows of `Ynew` (M, D; finite) as ids N .. N + M - 1 and returns those ids (int64).  The rows are
        uploaded and normalised on their own; when the device buffers are full they move to max(N + M, 1.5 capacity) rows
        (rounded up to 128) by a device copy.  If that allocation fails the corpus is as it was."""
        Yn = np.asarray(Ynew)
        if Yn.ndim != 2 or Yn.shape[1] != self.D:
            raise ValueError(f"Ynew must be an (M, {self.D}) array, got shape {Yn.shape}")
        Yc = np.ascontiguousarray(Yn, dtype=np.float32)
        if not np.all(np.isfinite(Yc)):
            raise ValueError("Ynew must be finite")
        M = Yc.shape[0]
        if self.N + M >= 2 ** 31:
            raise ValueError(f"N + M must stay below 2^31, got {self.N} + {M}")
        first = C.c_int64(0)
        self._call("osc_corpus_append", nat.f32(Yc) if M else None, M, C.byref(first))
        if M:
            self.N += M
            self._alive = None
        return np.arange(first.value, first.value + M, dtype=np.int64)

    def remove(self, ids) -> int:
        """Tombstones the rows `ids`: they leave every later search, the other rows keep their ids, and removed ids are
        not reused.  An id outside [0, N) raises ValueError before anything changes; an id removed earlier is ignored.
        Returns the number of rows newly removed."""
        if self._h is None:
            raise ValueError("Corpus is closed")
        r = np.asarray(ids).reshape(-1)
        if r.size and not np.issubdtype(r.dtype, np.integer):
            raise ValueError("ids must be integers")
        r = r.astype(np.int64)
        if r.size and (r.min() < 0 or r.max() >= self.N):
            bad = int(r[(r < 0) | (r >= self.N)][0])
            raise ValueError(f"remove: id {bad} is outside [0, {self.N})")
        r32 = np.ascontiguousarray(r, dtype=np.int32)
        gone = C.c_int64(0)
        self._call("osc_corpus_remove", nat.i32(r32) if r32.size else None, int(r32.size), C.byref(gone))
        self._n_removed += int(gone.value)
        self._alive = None
        return int(gone.value)

    def update(self, ids, Ynew) -> None:
        """Row `ids[j]` gets the vector `Ynew[j]` (ids: distinct live ids; Ynew: (M, D), finite).  The rows are uploaded once
        and normalised on the device with `append`'s arithmetic, so every later answer is byte for byte that of a fresh
        `Corpus` over the changed rows.  Ids, tombstones, the capacity and an armed filter's meaning stay.  ValueError before
        anything changes for an id outside [0, N), an id that names a removed row, an id named twice, a non-finite row or
        a bad shape."""
        if self._h is None:
            raise ValueError("Corpus is closed")
        r = np.asarray(ids).reshape(-1)
        if r.size and not np.issubdtype(r.dtype, np.integer):
            raise ValueError("ids must be integers")
        r = r.astype(np.int64)
        Yn = np.asarray(Ynew)
        if Yn.ndim != 2 or Yn.shape[1] != self.D or Yn.shape[0] != r.size:
            raise ValueError(f"Ynew must be a ({r.size}, {self.D}) array, got shape {Yn.shape}")
        if r.size and (r.min() < 0 or r.max() >= self.N):
            bad = int(r[(r < 0) | (r >= self.N)][0])
            raise ValueError(f"update: id {bad} is outside [0, {self.N})")
        if np.unique(r).size != r.size:
            raise ValueError("update: an id is named twice")
        if r.size and not self._alive_mask()[r].all():
            bad = int(r[~self._alive_mask()[r]][0])
            raise ValueError(f"update: id {bad} names a removed row")
        Yc = np.ascontiguousarray(Yn, dtype=np.float32)
        if not np.all(np.isfinite(Yc)):
            raise ValueError("Ynew must be finite")
        if r.size == 0:
            return
        r32 = np.ascontiguousarray(r, dtype=np.int32)
        self._call("osc_corpus_update", nat.i32(r32), nat.f32(Yc), int(r32.size))

    def compact(self) -> np.ndarray:
        """Drops the removed rows, keeps the order of the others and renumbers them densely (a device gather of Y and Yn
        into fresh buffers).  Afterwards N == n_live.  Returns new_id_of_old: int64, one entry per old row, -1 for a
        removed row.  ValueError when every row has been removed."""
        new_id = mk.compaction_map(self._alive_mask())
        n_new = C.c_int64(0)
        self._call("osc_corpus_compact", None, C.byref(n_new))
        self.N, self._n_removed = int(n_new.value), 0
        self._alive = None
        return new_id

    def refine_many(self, psis, top_k: int, k: int = 8, alpha: float = 0.5, *, kneighbors: int = 6,
                    row_cap_val: float = 1.0, lamG: float = 1.0, lamC: float = 0.5, lamQ: float = 4.0,
                    deterministic_k: bool = False, neighbor_seed: Optional[int] = None, candidates=None,
                    as_arrays: bool = False, gates=None, gate_beta: float = 1.0, gate_gamma: float = 0.1,
                    gate_method: str = "direct", gate_tol: float = 1e-4, gate_max_iters: int = 256,
                    receipts: Optional[str] = None, settle_dt: float = 1.0, settle_max_iters: int = 12,
                    settle_tol: float = 1e-3, chains=None, lamP: float = 0.2, chain_weights=None,
                    chain_z_th: float = 2.5, allow=None, ragged: bool = False):
        """For each query q, what the reference's loop returns with `cand = search(psis, top_k)[0][q]` (or
        `candidates[q]`):

            lat = Oscillink(Y[cand], kneighbors, row_cap_val, lamG, lamC, lamQ, deterministic_k, neighbor_seed)
            lat.set_query(psis[q]); lat.bundle(k, alpha)   # with "id" mapped back to corpus ids

        `settle()` is not run and cannot change the answer: bundle() reads only U*, which is solved from x0 = Y
        (reference lattice.py:245-263) with _ensure_device_ustar's settings (tol 1e-4, 64 iterations, Jacobi).
        `deterministic_k` / `neighbor_seed` mean what they mean for Oscillink: the device uses one total order
        (similarity desc, index asc) either way.  Limits: 1 <= top_k <= 1024, min(kneighbors, K - 1) <= 128.

        `gates` selects the reference's second, "hallucination control" form of the loop (examples/rag_replacement.py:
        159-177), `lat.set_query(psis[q], gates=g)`:  None -- no gates (B = 1);  "diffusion" -- per lattice
        g = compute_diffusion_gates(Y[cand], psis[q], kneighbors=..., row_cap_val=..., beta=gate_beta, gamma=gate_gamma,
        method=gate_method, tol=gate_tol, max_iters=gate_max_iters), solved on the device on the lattice's own graph;
        a (Q, K) array -- used as given, in candidate order (finite and >= 0: a batch cannot surface one lattice's
        breakdown the way set_query's caller can).  Gates of exactly 1 give the ungated answer bit for bit.

        Returns Q lists of {"id", "score", "align"}, or with `as_arrays=True` a dict of `ids`, `local`, `score`, `align`
        (Q, min(k, K)), `candidates` (Q, K), `ustar_iters` and `ustar_res` (Q,); with gates also `gates` (Q, K) float32 and
        `gate_iters`, `gate_res` (Q,; zeros for given gates).

        `receipts="light"` or `"full"` (set_receipt_detail's words) runs the loop the reference ships with its audit trail
        (examples/rag_replacement.py:48-73): per query additionally `s = lat.settle(settle_dt, settle_max_iters, settle_tol)`
        before the bundle and `rec = lat.receipt()` after it, for the same lattice, query and gates, on the device -- a
        fresh lattice (U = Y; warm_start / inertia have nothing to act on), Jacobi preconditioning; a settle that does not
        converge does not raise.  With `as_arrays=True` the dict gains `settle_iters` int32, `settle_res` float32, `deltaH`,
        `coh_drop_sum`, `anchor_pen_sum`, `query_term_sum` float64 (Q,) with receipt()'s float32 rounding (the three sums are
        zero in light detail) and, in full detail, `null_total` (Q,), `null_offsets` (Q + 1,), `null_i`, `null_j` (local row
        ids of the candidate lattice), `null_z`, `null_r`: receipt_many's layout.  OSCILLINK_RECEIPT_NULL_CAP means what it
        means for receipt() (highest z kept, stable), applied on the device.  Otherwise Q dicts {"bundle": [...], "settle":
        {"iters", "res"}, "receipt": {...}}; "receipt" has receipt()'s keys, `state_sig` equal to the loop's, cg_iters /
        residual from the settle, ustar_* from the U* solve and meta["ustar_source"] = "corpus_batch".  Fields that describe
        one handle's clock or cache have no per-lattice meaning in a batch and are fixed: t_ms, ustar_solve_ms,
        graph_build_ms, last_settle_ms = 0.0, ustar_cached False, ustar_solves 1, ustar_cache_hits 0.  Not covered:
        HMAC-signed receipts (a Corpus has no secret), OSCILLINK_RECEIPT_DYNAMICS, and preconditioners other than "jacobi".
        `receipts=None` is the call as it was.

        `chains` puts a chain prior on the candidate lattices (examples/quickstart.py:14-23, scripts/benchmark.py:60-83):
        Q entries, each None or a sequence of 2 .. 1024 local row ids of the query's lattice -- positions in `candidates[q]`,
        the search order -- or a (Q, L) integer array.  For a query with a chain everything returned is what the loop returns
        with `lat.add_chain(chains[q], lamP=lamP, weights=chain_weights[q])` after construction (one `lamP` >= 0 for the
        call; `chain_weights` None, or parallel to `chains` with None or len(chain) - 1 finite floats each), with or without
        gates and receipts: U* and the settle gain lamP L_path, the Jacobi diagonal lamP, deltaH the path term, and
        `state_sig` carries lamP, chain_present and chain_len.  A query whose entry is None is a lattice without a chain.
        Per query with a chain `lat.chain_receipt(chains[q], z_th=chain_z_th)` is computed on the device from U*: with
        `as_arrays=True` the dict gains `chain_offsets` int64 (Q + 1, over chain edges), `chain_z_struct`, `chain_z_path`,
        `chain_r_struct`, `chain_r_path` float32 (flat), `chain_gain` float64, `chain_verdict` bool, `chain_weakest_k` int32
        (-1 without a chain) and `chain_weakest_z` float32 (Q,); with `receipts` set and the dict form each query's dict
        gains "chain_receipt" (chain_receipt()'s keys, local ids; None without a chain).  With `receipts=None` and the list
        form the return value stays Q bundles: the chain acts through U* only.  `chains=None` adds no key and calls the
        entry points called without it.

        On a corpus that has changed (`append`, `remove`, `compact`) K = min(top_k, n_live), removed rows are never
        searched and `candidates` naming one raises ValueError.  `allow` -- a bool array (N,) for every query or (Q, N)
        with one row per query -- narrows the device search to the rows that are live and allowed, as in `search`; it
        cannot be combined with `candidates`, and every query needs at least K eligible rows.  Either way the answer is
        the one a fresh `Corpus` over the eligible rows gives, ids mapped; `allow=None` on a corpus without removed rows is
        the call as it was.

        `ragged=True` runs candidate lattices of different sizes in the one batch, as the
        reference's filtered loop does (scripts/proof_hallucination.py:203-221: the lattice is built over whichever rows pass,
        with kneighbors = min(k, rows - 1)).  Query q gets a lattice of n_q rows, 1 <= n_q <= K: with `allow`, n_q =
        min(K, eligible rows) and the candidates are all eligible rows in the search order (only a query without any eligible
        row is an error); with `candidates`, Q integer sequences of 1 .. K ids each, or the (Q, K) array with -1 behind each
        row's ids; with neither, every n_q is K.  Per query: min(k, n_q) picks, min(kneighbors, n_q - 1) neighbours (a one-row
        lattice has no edge), a (Q, K) `gates` array is read and checked below n_q only, and chain ids must be < n_q.  The
        array form keeps its shapes and gains `rows` int32 (Q,) = n_q; behind n_q (or min(k, n_q)) `ids`, `local` and
        `candidates` hold -1 and `score`, `align` and `gates` 0.  The list and dict forms have min(k, n_q) bundle entries, and
        a receipt's meta and `state_sig` are those of the n_q-row lattice.  Everything returned for a query is byte for byte
        what a call over its lattice alone returns.  `ragged=False` is the call as it was.

        Per-query settings: `lamG`, `lamC`, `lamQ`, `lamP`, `kneighbors`, `k`, `alpha`, `settle_dt`,
        `settle_max_iters` and `settle_tol` each take a scalar or a length-Q sequence or 1-D array, as the reference's service
        carries them per request (cloud/app/models.py:8-23) and its adaptive profiles override and jitter them per request
        (cloud/app/learners.py:148-192).  Everything returned for query q is byte for byte what the same call returns for
        that query alone with its settings as scalars, in every mode above.  Lattice q has lists of min(kneighbors[q],
        n_q - 1) and min(k[q], n_q) picks; with a per-query `k` the (Q, .) pick arrays are min(max(k), K) wide with the ragged
        fill behind a query's own picks, and the array form gains `picks` int32 (Q,).  Each value gets the scalar's check,
        with the first offending query in the message, before any native call.  With all ten scalars (a 0-d array and a NumPy
        scalar are scalars) the call is the one it was."""
        P = self._queries(psis)
        K = self._top_k(top_k)
        st = self._settings(P.shape[0], K, lamG=lamG, lamC=lamC, lamQ=lamQ, lamP=lamP, kneighbors=kneighbors, k=k, alpha=alpha,
                            settle_dt=settle_dt, settle_max_iters=settle_max_iters, settle_tol=settle_tol)
        recs, k_per_query, raw = None, None, None
        if st is not None and P.shape[0]:
            # per-query settings: the records are armed for the native call, which ignores its scalars of those names; below
            # they stand as query 0's values (checked), and k as the widest query's
            recs, raw = st[0], st[2]
            k_per_query = recs["k"].astype(np.int64) if "k" in st[1] else None
            lamG, lamC, lamQ, lamP, alpha, settle_dt, settle_tol = (float(recs[n][0]) for n in (
                "lamG", "lamC", "lamQ", "lamP", "alpha", "settle_dt", "settle_tol"))
            kneighbors, settle_max_iters, k = int(recs["kneighbors"][0]), int(recs["settle_max_iters"][0]), int(recs["k"].max())
        elif st is not None:  # no query: nothing to arm, and nothing to read a value from
            lamG, lamC, lamQ, lamP, kneighbors, k, alpha, settle_dt, settle_max_iters, settle_tol = (
                self._PER_QUERY_DEFAULTS[n] for n in self._PER_QUERY_DEFAULTS)
        knn = self._knn(kneighbors, K)
        detail, s_dt, s_max, s_tol = self._receipt_settings(receipts, settle_dt, settle_max_iters, settle_tol)
        if float(lamG) <= 0:
            raise ValueError("lamG must be > 0 for SPD")
        for name, val in (("lamC", lamC), ("lamQ", lamQ)):
            if float(val) < 0:
                raise ValueError(f"{name} must be >= 0")
        Q = P.shape[0]
        rg = bool(ragged)
        cand_rows = None
        if candidates is not None and rg:
            cand_in, cand_rows = self._candidates_ragged(candidates, Q, K)
        else:
            cand_in = None if candidates is None else self._candidates(candidates, Q, K)
        words, rows = self._allow_rows(allow, candidates, Q, K, rg)
        rows = rows if cand_rows is None else cand_rows
        kk = min(max(int(k), 0), K)
        gates_in, gate_set = None, None
        if isinstance(gates, str):
            if gates != "diffusion":
                raise ValueError(f"gates must be None, 'diffusion' or a ({Q}, {K}) array, got {gates!r}")
            gate_set = self._gate_settings(gate_beta, gate_gamma, gate_method, gate_max_iters, prefix="gate_")
        elif gates is not None:
            gates_in = np.asarray(gates)
            if gates_in.shape != (Q, K):
                raise ValueError(f"gates must be a ({Q}, {K}) array, got shape {gates_in.shape}")
            gates_in = np.ascontiguousarray(gates_in, dtype=np.float32)
            if rg:  # only a lattice's own entries are read and checked
                gates_in = np.where(np.arange(K)[None, :] < rows[:, None], gates_in, np.float32(0.0))
            if not np.all(np.isfinite(gates_in)):
                raise ValueError("gates must be finite")
            if np.any(gates_in < 0):
                raise ValueError("gates must be >= 0")
        chain = self._chains(chains, chain_weights, lamP, chain_z_th, Q, K, rows)
        gated = gates is not None
        picks = None
        if k_per_query is not None:
            picks = np.minimum(np.maximum(k_per_query, 0), K if rows is None else rows).astype(np.int32)
        o = _RefineOut(Q, K, kk, gated, rows, picks)
        cand_arg = None if cand_in is None else nat.i32(cand_in)
        gates_arg = None if gates_in is None else nat.f32(gates_in)
        beta, gamma, method, g_max = gate_set if gate_set is not None else (1.0, 0.1, 0, 1)
        gate_args = (beta, gamma, method, float(gate_tol), g_max)
        solve_args = (int(kneighbors), float(row_cap_val), float(lamG), float(lamC), float(lamQ), USTAR_TOL,
                      USTAR_MAX_ITERS, kk, float(alpha))
        if detail is not None or chain is not None:
            return self._refine_receipts(P, o, top_k=top_k, knn=knn, cand_arg=cand_arg,
                                         mode=0 if not gated else (2 if gates_in is not None else 1), gates_arg=gates_arg,
                                         gate_args=gate_args, solve_args=solve_args, detail=detail,
                                         settle_args=(s_dt, s_max, s_tol), lam=[lamG, lamC, lamQ, 0.0],
                                         deterministic_k=deterministic_k, as_arrays=as_arrays, chain=chain, allow=words,
                                         kneighbors=int(kneighbors), settings=recs, raw=raw)
        if Q and not gated:
            self._call_filtered(words, "osc_corpus_refine", nat.f32(P), Q, int(top_k), cand_arg, *solve_args,
                                *o.pointers(False), ragged=rows, settings=recs)
        elif Q:
            self._call_filtered(words, "osc_corpus_refine_gated", nat.f32(P), Q, int(top_k), cand_arg, gates_arg, *gate_args,
                                *solve_args, *o.pointers(True), ragged=rows, settings=recs)
            if gates_in is None:
                self._warn_non_finite(o.g, o.g_iters, o.g_res, "refine_many")
        ids, arrays = o.ids_and_arrays()
        return arrays if as_arrays else o.bundles(ids)

    def _refine_receipts(self, P, o, *, top_k, knn, cand_arg, mode, gates_arg, gate_args, solve_args, detail,
                         settle_args, lam, deterministic_k, as_arrays, chain=None, allow=None, kneighbors=None,
                         settings=None, raw=None):
        """refine_many with receipts or chains, behind its validation: one osc_corpus_refine_receipts call (or, with
        chains, one osc_corpus_refine_chains call), then the arrays or the loop's dicts.  o = the result arrays; mode = the
        entry point's gate_mode; gate_args, solve_args and settle_args (dt, max_iters, tol) = its argument runs of those
        names; detail = None (chains only: no settle, no receipt), 0 or 1; lam = the state signature's lambdas, as given;
        chain = _chains' block or None; allow = _allow's words or None; kneighbors = as given (a ragged call's signatures
        take min(kneighbors, max(1, n_q - 1)) per lattice); settings = _settings' records of a call with per-query settings
        (armed for the native call; a receipt's lambdas and `k` are then the query's own, from `raw`, _settings' values as
        given) or None."""
        from .lattice import OscillinkLattice, __version__

        Q, K = o.cand.shape
        full = detail == 1
        gated = o.gated
        iters, res, g, g_iters, g_res = o.iters, o.res, o.g, o.g_iters, o.g_res
        cap_val = rc.null_cap()
        ra = rc.ReceiptArrays(Q, (min(cap_val, K) if cap_val > 0 else K) if full else 0, settle=True)
        s_iters, s_res = ra.settle
        dicts = not as_arrays and detail is not None
        nnz = np.zeros(Q, dtype=np.int64)
        pairs = np.zeros((Q if dicts else 0, EDGE_PREFIX, 2), dtype=np.int64)
        pairs_n = np.zeros(Q, dtype=np.int32)
        receipt_out = (*ra.pointers(), nat.i64(nnz) if dicts else None, nat.i64(pairs) if dicts else None,
                       nat.i32(pairs_n) if dicts else None, EDGE_PREFIX)
        if chain is not None:
            n_edges = int(chain["edge_offsets"][-1])
            c_edge = np.zeros((4, max(n_edges, 1)), dtype=np.float32)  # z_struct, z_path, r_struct, r_path
            c_gain = np.zeros(Q, dtype=np.float64)
            c_verdict = np.zeros(Q, dtype=np.int32)
            c_weak_k = np.full(Q, -1, dtype=np.int32)
            c_weak_z = np.zeros(Q, dtype=np.float32)
        if Q and chain is not None:
            self._call_filtered(allow, "osc_corpus_refine_chains", nat.f32(P), Q, int(top_k), cand_arg, mode, gates_arg,
                       *gate_args, *solve_args, *settle_args, -1 if detail is None else detail, RECEIPT_Z_TH, cap_val,
                       nat.i64(chain["offsets"]), nat.i32(chain["nodes"]),
                       None if chain["weights"] is None else nat.f32(chain["weights"]), chain["lamP"], chain["z_th"],
                       *o.pointers(True), *receipt_out, *[nat.f32(c_edge[t]) for t in range(4)],
                       c_gain.ctypes.data_as(nat.c_f64p), nat.i32(c_verdict), nat.i32(c_weak_k), nat.f32(c_weak_z),
                       ragged=o.rows, settings=settings)
        elif Q:
            self._call_filtered(allow, "osc_corpus_refine_receipts", nat.f32(P), Q, int(top_k), cand_arg, mode, gates_arg,
                       *gate_args, *solve_args, *settle_args, detail, RECEIPT_Z_TH, cap_val, *o.pointers(True), *receipt_out,
                       ragged=o.rows, settings=settings)
        if Q:
            if mode == 1:
                self._warn_non_finite(g, g_iters, g_res, "refine_many")
        ra.round_sums()
        ids, out = o.ids_and_arrays()
        if as_arrays:
            if detail is not None:
                out.update(ra.scalar_arrays())
            if full:
                out.update(ra.null_arrays())
            if chain is not None:
                out.update(chain_offsets=chain["edge_offsets"], chain_z_struct=c_edge[0, :n_edges].copy(),
                           chain_z_path=c_edge[1, :n_edges].copy(), chain_r_struct=c_edge[2, :n_edges].copy(),
                           chain_r_path=c_edge[3, :n_edges].copy(), chain_gain=c_gain, chain_verdict=c_verdict != 0,
                           chain_weakest_k=c_weak_k, chain_weakest_z=c_weak_z)
            return out
        if detail is None:  # chains without receipts, list form: the chain acts through U* only
            return o.bundles(ids)
        detail_name = "full" if full else "light"
        ones = np.ones(K, dtype=np.float32)
        bundles = o.bundles(ids)
        out = []
        for q in range(Q):
            n = K if o.rows is None else int(o.rows[q])  # the lattice's own rows: its gates, degree and signature
            B = (g[q] if gated else ones)[:n]
            adj_sig = hashlib.sha256(np.ascontiguousarray(pairs[q, :int(pairs_n[q])]).tobytes()).hexdigest()
            ch = None if chain is None else chain["lists"][q]
            lam_q, lamP_q, kn_q = lam, None if chain is None else chain["lamP"], kneighbors
            if settings is not None:  # the query's own values, as float(...) of the scalar call would hold them
                lam_q = [raw[name][q] for name in ("lamG", "lamC", "lamQ")] + [0.0]
                lamP_q, kn_q = float(raw["lamP"][q]), int(settings["kneighbors"][q])
            sig = OscillinkLattice._signature_digest(
                {"psi": np.round(P[q], 6).tolist(), "lam": lam_q if ch is None else [*lam_q[:3], lamP_q],
                 "chain_present": ch is not None, "chain_len": 0 if ch is None else len(ch),
                 "k": knn if o.rows is None and settings is None else min(kn_q, max(1, n - 1)),
                 "detk": bool(deterministic_k), "adj": adj_sig}, B)
            nulls, tot = ra.nulls(q)
            meta = rc.meta(ustar_cached=False, ustar_solves=1, ustar_cache_hits=0,
                           ustar={"ustar_iters": int(iters[q]), "ustar_res": float(res[q]),
                                  "ustar_converged": bool(float(res[q]) <= USTAR_TOL)},
                           ustar_solve_ms=0.0, ustar_source="corpus_batch", graph_build_ms=0.0, last_settle_ms=0.0,
                           degree=rc.degree_stats(int(nnz[q]), n), gates=rc.gate_stats(B), state_sig=sig,
                           receipt_detail=detail_name, null_points_summary=rc.null_summary(tot, cap_val))
            rec = rc.record(version=__version__, deltaH=ra.sums[0, q], coh_drop_sum=ra.sums[1, q],
                            anchor_pen_sum=ra.sums[2, q], query_term_sum=ra.sums[3, q], cg_iters=s_iters[q],
                            residual=s_res[q], t_ms=0.0, null_points=nulls, meta=meta)
            out.append({"bundle": bundles[q], "settle": {"iters": int(s_iters[q]), "res": float(s_res[q])}, "receipt": rec})
            if chain is not None:
                out[-1]["chain_receipt"] = None
            if ch is not None:
                e0 = int(chain["edge_offsets"][q])
                out[-1]["chain_receipt"] = rc.chain_receipt_dict(
                    ch, weakest_k=c_weak_k[q], weakest_z=c_weak_z[q], gain=c_gain[q], verdict=c_verdict[q],
                    z_struct=c_edge[0, e0:], z_path=c_edge[1, e0:], r_struct=c_edge[2, e0:], r_path=c_edge[3, e0:])
        return out

    def diffusion_gates_many(self, psis, top_k: int, *, kneighbors: int = 6, row_cap_val: float = 1.0, beta: float = 1.0,
                             gamma: float = 0.1, method: str = "direct", tol: float = 1e-4, max_iters: int = 256,
                             clamp: bool = True, candidates=None, allow=None, ragged: bool = False) -> dict[str, Any]:
        """For each query q, with `cand` its candidates (searched, or `candidates[q]`),

            compute_diffusion_gates(Y[cand], psis[q], kneighbors=..., row_cap_val=..., beta=..., gamma=..., method=...,
                                    tol=..., max_iters=..., clamp=...)

        with every lattice's graph and single-right-hand-side solve on the device (no U*) -- for `clamp=True`; with
        `clamp=False` the result is the solve's h itself, NOT clipped, whereas compute_diffusion_gates (like the reference,
        diffusion.py:123) still clips h to [0, 1]: `np.clip(out["gates"], 0, 1)` gives its answer.  method="direct" is
        served, as in compute_diffusion_gates, by the CG run to 1e-7 max(1, |s|) with at most 2048 iterations.  Non-finite
        gates come back as computed, with a RuntimeWarning naming the first such query.  `allow` narrows the search as in
        `search`.  `ragged=True` means what it means for `refine_many`: query q's lattice has n_q <= K rows, `gates` holds 0 and
        `candidates` -1 behind them, and the dict gains `rows` int32 (Q,).  `kneighbors` may be a length-Q sequence, as for
        `refine_many`: query q's lattice then has lists of min(kneighbors[q], n_q - 1), and its gates, `iters` and `res` are
        those of the one-query call with that value.

        Returns a dict of `gates` (Q, K) float32 in candidate order, `candidates` (Q, K), `iters` and `res` (Q,)."""
        P = self._queries(psis)
        K = self._top_k(top_k)
        st = self._settings(P.shape[0], K, kneighbors=kneighbors)
        recs = None
        if st is not None:  # per-query kneighbors: armed for the native call; query 0's stands in below
            recs = st[0] if P.shape[0] else None
            kneighbors = int(st[0]["kneighbors"][0]) if P.shape[0] else 6
        self._knn(kneighbors, K)
        b, g, m, mi = self._gate_settings(beta, gamma, method, max_iters)
        Q = P.shape[0]
        rg = bool(ragged)
        cand_rows = None
        if candidates is not None and rg:
            cand_in, cand_rows = self._candidates_ragged(candidates, Q, K)
        else:
            cand_in = None if candidates is None else self._candidates(candidates, Q, K)
        words, rows = self._allow_rows(allow, candidates, Q, K, rg)
        rows = rows if cand_rows is None else cand_rows
        cand = np.zeros((Q, K), dtype=np.int32)
        gates = np.zeros((Q, K), dtype=np.float32)
        iters = np.zeros(Q, dtype=np.int32)
        res = np.zeros(Q, dtype=np.float32)
        if Q:
            self._call_filtered(words, "osc_corpus_gates", nat.f32(P), Q, int(top_k),
                                None if cand_in is None else nat.i32(cand_in), int(kneighbors), float(row_cap_val), b, g, m,
                                float(tol), mi, int(bool(clamp)), nat.i32(cand), nat.f32(gates), nat.i32(iters),
                                nat.f32(res), ragged=rows, settings=recs)
            self._warn_non_finite(gates, iters, res, "diffusion_gates_many")
        out = {"gates": gates, "candidates": cand, "iters": iters, "res": res}
        if rg:
            out["rows"] = rows
        return out

    def info(self, top_k: int, kneighbors: int = 6, k: int = 8) -> dict[str, Any]:
        """Queries per chunk and one chunk's device scratch for a refine with these settings."""
        K = self._top_k(top_k)
        self._knn(kneighbors, K)
        chunk, nbytes = C.c_int32(0), C.c_int64(0)
        self._call("osc_corpus_info", int(top_k), int(kneighbors), int(k), C.byref(chunk), C.byref(nbytes))
        return {"chunk": int(chunk.value), "scratch_bytes": int(nbytes.value)}

    # ------------------------------------------------------------------ test diagnostics
    def _candidate_graph(self, psi_or_candidates, top_k: int, kneighbors: int = 6, row_cap_val: float = 1.0):
        """The candidate lattice's graph (rowptr, col, a, w, sqrt_deg) in local order, in the form of graph_csr().
        A float vector of D entries is a query (its search gives the candidates); an integer vector is the candidates."""
        K = self._top_k(top_k)
        kn = self._knn(kneighbors, K)
        v = np.asarray(psi_or_candidates)
        psi = np.zeros((1, self.D), dtype=np.float32)
        cand_in = None
        if np.issubdtype(v.dtype, np.integer):
            cand_in = self._candidates(v.reshape(1, -1), 1, K)
        else:
            psi = self._queries(v.reshape(1, -1))
        cap = max(1, K * max(1, kn))
        cand = np.zeros(K, dtype=np.int32)
        rowptr = np.zeros(K + 1, dtype=np.int64)
        col = np.zeros(cap, dtype=np.int32)
        a = np.zeros(cap, dtype=np.float32)
        w = np.zeros(cap, dtype=np.float32)
        sd = np.zeros(K, dtype=np.float32)
        nnz = C.c_int64(0)
        self._call("osc_corpus_graph", nat.f32(psi), None if cand_in is None else nat.i32(cand_in), int(top_k),
                   int(kneighbors), float(row_cap_val), nat.i32(cand), nat.i64(rowptr), nat.i32(col), nat.f32(a),
                   nat.f32(w), nat.f32(sd), cap, C.byref(nnz))
        n = int(nnz.value)
        return rowptr, col[:n].copy(), a[:n].copy(), w[:n].copy(), sd

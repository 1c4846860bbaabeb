"""`OscillinkLattice` -- the reference's Python surface (oscillink/core/lattice.py) over the MI355X library.

Same constructor, methods, attributes, return conventions and error behaviour as the reference class, so
callers of `Oscillink(...).settle()/receipt()` can switch imports.  All numerics run on the GPU through
liboscillink_hip.so (ctypes, include/oscillink_hip.h); the lattice graph is sparse (ELL on the device, CSR on
the host) instead of the reference's dense N x N arrays.  `.A` / `.L_sym` / `.L_path` / `.A_path` are lazy dense
views kept for small-N callers and tests.

Host-side only (no kernel): parameter validation, U* cache keyed by the state signature, logging, callbacks,
receipt assembly + HMAC signing, persistence.
"""
from __future__ import annotations

import ctypes as C
import hashlib
import json
import os
import time
from typing import Any, Optional

import numpy as np

from . import _native as nat
from . import _receipts as rc

__version__ = "0.1.13+mi355x.1"

_DENSE_VIEW_LIMIT = 20000  # N above which dense N x N views are refused (1.6 GB at fp32)
_DENSE_EXPORT_LIMIT = 4096  # N up to which export_state / save_state also write the reference's dense `A`


# build_info()'s anchor-start levels: (info function, key prefix, key of its solves counter, whether it reports redos)
_ANCHOR_LEVELS = (
    ("osc_anchor_ap_info", "anchor_ap", "streamed_first_applies", False),
    ("osc_anchor_ap2_info", "anchor_ap2", "streamed_second_applies", False),
    ("osc_anchor_gram_info", "anchor_gram", "fused_two_step_solves", True),
    ("osc_anchor_gram3_info", "anchor_gram3", "fused_three_step_solves", False),
    ("osc_anchor_gram4_info", "anchor_gram4", "fused_four_step_solves", False),
    ("osc_anchor_poly_info", "anchor_poly", "poly_four_step_solves", True),
)


# The maps of `keep_state=True`: per row of the lattice afterwards, the row before whose state it
# keeps, -1 for a fresh row, which starts at its anchor.  int32, the form osc_carry_state takes.
def _state_map_append(N: int, M: int) -> np.ndarray:
    return np.concatenate([np.arange(N, dtype=np.int32), np.full(M, -1, dtype=np.int32)])


def _state_map_remove(keep: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(np.nonzero(keep)[0], dtype=np.int32)


def _state_map_update(N: int, ids: np.ndarray) -> np.ndarray:
    src = np.arange(N, dtype=np.int32)
    src[ids] = -1
    return src


# What the batched bundle calls share.  Module functions: they read of a lattice only what the calls' own bodies read.
def _bundle_arrays(Q: int, kk: int):
    """The (ids, score, align) arrays a batched bundle call fills, each Q x kk."""
    return np.zeros((Q, kk), dtype=np.int32), np.zeros((Q, kk), dtype=np.float32), np.zeros((Q, kk), dtype=np.float32)


def _bundle_result(ids, score, align, as_arrays: bool):
    """A batched bundle call's return: the arrays, or one list of bundle()'s dicts per query."""
    if as_arrays:
        return ids, score, align
    return [rc.bundle_dicts(ids[q], score[q], align[q]) for q in range(ids.shape[0])]


def _gated_call_inputs(lat, fn: str, psis, gates, gate_gamma, gate_method, gate_max_iters, max_iters):
    """The refusals and argument checks `bundle_gated_many` and `receipt_gated_many` (`fn`) share.  Returns (P, Q, G,
    diffusion): the queries, their count, the (Q, N) float32 gates -- with `diffusion` the array the call's own
    "diffusion" gates are written to -- and whether the gates are to be computed."""
    if lat._has_comm:
        raise NotImplementedError(f"{fn}: lattices with a communicator (sharded / multi-rank) are not supported")
    if lat._chain_nodes is not None:
        raise NotImplementedError(f"{fn}: a lattice with a chain of its own is not supported (clear_chain first)")
    P = rc.check_queries(psis, lat.D, finite=False)
    Q = int(P.shape[0])
    diffusion = isinstance(gates, str)
    if diffusion:
        if gates != "diffusion":
            raise ValueError(f"gates must be 'diffusion' or a ({Q}, {lat.N}) array, got {gates!r}")
        if not float(gate_gamma) > 0:
            raise ValueError("gate_gamma must be > 0 for SPD")
        if gate_method not in ("direct", "cg"):
            raise ValueError(f"gate_method must be 'direct' or 'cg', got {gate_method!r}")
        if int(gate_max_iters) < 1:
            raise ValueError("gate_max_iters must be >= 1")
        G = nat.result_array((Q, lat.N)) if Q > 0 else np.zeros((0, lat.N), dtype=np.float32)
    else:
        G = lat._check_gate_rows(gates)
        if G.shape[0] != Q:
            raise ValueError(f"gates must be a ({Q}, {lat.N}) array, got shape {G.shape}")
        for q in range(Q):
            if not np.all(np.isfinite(G[q])):
                raise ValueError(f"query {q}: gates must be finite")
            if np.any(G[q] < 0):
                raise ValueError(f"query {q}: gates must be >= 0")
    if int(max_iters) < 1:
        raise ValueError("max_iters must be >= 1")
    return P, Q, G, diffusion


def _warn_diffusion_gates(G: np.ndarray) -> None:
    """`diffusion_gates_many`'s warning for gates a gated call computed itself, raised at that call's caller."""
    bad = np.nonzero(~np.all(np.isfinite(G), axis=1))[0]
    if bad.size:
        import warnings

        warnings.warn(f"diffusion_gates_many: the screened-diffusion solve of query {int(bad[0])} produced "
                      "non-finite values; returned as computed, like the reference's cg path", RuntimeWarning,
                      stacklevel=3)


class OscillinkLattice:
    """Short-term coherence lattice: mutual-kNN graph + SPD system + Jacobi-PCG settle (reference lattice.py:23-31)."""

    # ------------------------------------------------------------------ construction (lattice.py:33-110)
    def __init__(
        self,
        Y: np.ndarray,
        kneighbors: int = 6,
        row_cap_val: float = 1.0,
        lamG: float = 1.0,
        lamC: float = 0.5,
        lamQ: float = 4.0,
        deterministic_k: bool = False,
        neighbor_seed: Optional[int] = None,
        *,
        device: Optional[int] = None,
        comm: Optional[tuple] = None,
        _build_graph: bool = True,
    ):
        if not isinstance(Y, np.ndarray) or Y.ndim != 2:
            raise ValueError("Y must be a 2D numpy array")
        if kneighbors < 1:
            raise ValueError("kneighbors must be >= 1")
        if lamG <= 0:
            raise ValueError("lamG must be > 0 for SPD")
        for name, val in (("lamC", lamC), ("lamQ", lamQ)):
            if val < 0:
                raise ValueError(f"{name} must be >= 0")
        self._h = None
        # The reference keeps a private float32 copy of the anchors (lattice.py:54).  Here that copy lives on the
        # device (osc_create uploads the caller's array); the host-side `Y` attribute is fetched on first read.
        Yc = np.ascontiguousarray(Y, dtype=np.float32)
        self._Y_host: Optional[np.ndarray] = None
        self.N, self.D = Yc.shape
        k_eff = min(int(kneighbors), max(1, self.N - 1))
        self._kneighbors = k_eff
        self._kneighbors_requested = int(kneighbors)  # (append: the effective k follows the row count again)
        self._deterministic_k = bool(deterministic_k)
        self._neighbor_seed = neighbor_seed
        self._row_cap_val = float(row_cap_val)
        if device is None:
            device = int(os.environ.get("OSCILLINK_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        self._device = int(device)

        L = nat.lib()
        if nat.device_count() < 1:
            raise nat.NativeError("no HIP device visible: oscillink_amd runs on MI355X (gfx950) only, no CPU fallback")
        h = nat.Handle()
        t0 = time.time()
        # comm = (ncclUniqueId bytes, rank, world): one process per GPU.  The graph is then built row-block-sharded
        # (all-gather of the top-k lists) and the CG runs column-sharded (one all-reduce(max) per iteration).
        build_now = bool(_build_graph) and comm is None
        # (the library clamps k to N - 1 itself and keeps the requested value for osc_create_appended)
        rc = L.osc_create(nat.f32(Yc), self.N, self.D, self._kneighbors_requested, self._row_cap_val, int(self._deterministic_k),
                          -1 if neighbor_seed is None else int(neighbor_seed), self._device, int(build_now),
                          C.byref(h))
        nat.check(rc, None, "osc_create")
        self._h = h
        self._has_comm = comm is not None
        if comm is not None:
            uid, rank, world = comm
            nat.check(L.osc_comm_init(h, bytes(uid), int(rank), int(world)), h, "osc_comm_init")
            if _build_graph:
                nat.check(L.osc_rebuild_graph(h, self._kneighbors_requested, self._row_cap_val, int(self._deterministic_k),
                                              -1 if neighbor_seed is None else int(neighbor_seed)), h,
                          "osc_rebuild_graph")
        self._graph_build_ms = 1000.0 * (time.time() - t0)

        self._B = np.ones(self.N, dtype=np.float32)
        self._psi = np.zeros(self.D, dtype=np.float32)
        self.lamG, self.lamC, self.lamQ = lamG, lamC, lamQ
        self.lamP = 0.0
        self._chain_nodes: Optional[list[int]] = None
        self._chain_weights: Optional[list[float]] = None
        self.last: dict[str, Any] = {"iters": 0, "res": None, "t_ms": None}

        self._U_host: Optional[np.ndarray] = None  # host mirror of the device U, fetched on first read
        self._csr = None  # (rowptr, col, a, w, sqrt_deg) host cache
        self._state_version = 0
        self._sig_cache: Optional[tuple] = None
        self._Ustar_cache: Optional[np.ndarray] = None
        self._Ustar_sig: Optional[str] = None
        self._device_ustar_sig: Optional[str] = None
        self.stats: dict[str, int] = {"ustar_solves": 0, "ustar_cache_hits": 0, "query_basis_solves": 0}
        # query basis (bundle_many): keyed by graph / gates / chain (this counter) and the lambdas, NOT by psi
        self._qb_version = 0
        self._qb_key: Optional[tuple] = None
        self._qb_scale = 0.0
        self.last_query_basis: dict[str, Any] = {}
        # the basis of M + lamP I behind chain_receipt_many(lamP=...): a second slot, keyed like the first plus the shift
        self._qbs_key: Optional[tuple] = None
        self._qbs_scale = 0.0
        self._qbs_stats = False  # the shifted slot also holds its per-row constants (bundle_many with lamP)
        self.last_bundle_prior: dict[str, Any] = {}
        self.last_bundle_gated: dict[str, Any] = {}
        self._qbs_receipt = 0  # receipt_many with lamP: 1 = the slot holds M' x' (8 N bytes), 2 = also d_ij per ELL slot
        self.last_receipt_prior: dict[str, Any] = {}
        self.last_shifted_basis: dict[str, Any] = {}
        self.shifted_basis_solves = 0
        self._settle_callbacks: list = []
        self._logger = None
        self._receipt_secret: Optional[bytes] = None
        self._signature_mode = "minimal"
        self._receipt_detail = "full"
        self._last_dynamics: Optional[dict[str, Any]] = None
        self._log("init", {"N": self.N, "D": self.D, "kneighbors_requested": kneighbors,
                           "kneighbors_effective": k_eff, "deterministic_k": self._deterministic_k,
                           "neighbor_seed": self._neighbor_seed})

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None:
            try:
                nat.lib().osc_destroy(h)
            except Exception:
                pass
            self._h = None

    def close(self) -> None:
        """Release the device memory now (otherwise at garbage collection)."""
        self.__del__()

    def _call(self, name: str, *args) -> None:
        nat.check(getattr(nat.lib(), name)(self._h, *args), self._h, name)

    # ------------------------------------------------------------------ array attributes
    @property
    def Y(self) -> np.ndarray:
        if self._Y_host is None:
            # (kept for the lattice's lifetime: ordinary pageable memory, like the reference's own copy of Y)
            out = nat.result_array((self.N, self.D), pinned=False)
            self._call("osc_get_Y", nat.f32(out))
            self._Y_host = out
        return self._Y_host

    @property
    def U(self) -> np.ndarray:
        if self._U_host is None:
            out = nat.result_array((self.N, self.D))
            self._call("osc_get_U", nat.f32(out))
            self._U_host = out
        return self._U_host

    @U.setter
    def U(self, value: np.ndarray) -> None:
        v = np.ascontiguousarray(value, dtype=np.float32)
        if v.shape != (self.N, self.D):
            raise ValueError("U shape mismatch")
        self._call("osc_set_U", nat.f32(v))
        self._U_host = v.copy()

    def reset_U(self, wait: bool = True) -> None:
        """U <- Y on the device (the state right after construction); used by benchmark loops.  On one GPU nothing is
        copied: U aliases Y until the next settle writes it (`build_info()["y_to_u_copies"]` counts the copies a windowed
        or multi-rank handle still makes, ordered by the handle's stream).  Whatever follows sees the reset state either
        way; `wait=True` still synchronises the device, `wait=False` returns at once."""
        self._call("osc_set_U", None)
        self._U_host = None
        if wait:
            nat.check(nat.lib().osc_device_synchronize(self._device), None, "osc_device_synchronize")

    @property
    def B_diag(self) -> np.ndarray:
        return self._B

    @B_diag.setter
    def B_diag(self, gates: np.ndarray) -> None:
        g = np.ascontiguousarray(gates, dtype=np.float32)
        if g.shape[0] != self.N:
            raise ValueError("gates length mismatch N")
        self._B = g.copy()
        self._call("osc_set_query", None, nat.f32(self._B))
        self._touch()
        self._qb_version += 1

    @property
    def psi(self) -> np.ndarray:
        return self._psi

    @psi.setter
    def psi(self, psi: np.ndarray) -> None:
        p = np.ascontiguousarray(psi, dtype=np.float32).ravel()
        if p.shape[0] != self.D:
            raise ValueError("psi length mismatch D")
        self._psi = p.copy()
        self._call("osc_set_query", nat.f32(self._psi), None)
        self._touch()

    def _touch(self) -> None:
        self._state_version += 1

    # ---- graph views ----
    def _host_csr(self):
        if self._csr is None:
            nnz, _, _ = self.graph_stats()
            rowptr = np.zeros(self.N + 1, dtype=np.int64)
            col = np.zeros(max(nnz, 1), dtype=np.int32)
            a = np.zeros(max(nnz, 1), dtype=np.float32)
            w = np.zeros(max(nnz, 1), dtype=np.float32)
            sd = np.zeros(self.N, dtype=np.float32)
            self._call("osc_get_csr", nat.i64(rowptr), nat.i32(col), nat.f32(a), nat.f32(w), nat.f32(sd))
            self._csr = (rowptr, col[:nnz], a[:nnz], w[:nnz], sd)
        return self._csr

    def graph_stats(self) -> tuple[int, int, float]:
        """(stored directed edges, max degree, device build ms)."""
        nnz, mx, ms = C.c_int64(0), C.c_int32(0), C.c_double(0.0)
        self._call("osc_graph_stats", C.byref(nnz), C.byref(mx), C.byref(ms))
        return int(nnz.value), int(mx.value), float(ms.value)

    def build_info(self) -> dict[str, int]:
        """How the device paths ran: kNN prefilter use / fallback rows, one-launch solves, internal row re-order and the
        sampled clustering coefficient that decided it (diagnostic; not in the reference)."""
        pf, fb, ss = C.c_int32(0), C.c_int32(0), C.c_int64(0)
        self._call("osc_build_info", C.byref(pf), C.byref(fb), C.byref(ss))
        ro, cc = C.c_int32(0), C.c_double(0.0)
        self._call("osc_order_info", C.byref(ro), C.byref(cc))
        ln, sc, xw = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self._call("osc_spmm_plan", C.byref(ln), C.byref(sc), C.byref(xw))
        sb, ba = C.c_int32(0), C.c_int64(0)
        self._call("osc_apply_info", C.byref(sb), C.byref(ba))
        xk, xf, xp, xb = C.c_int32(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._call("osc_x_ring_info", C.byref(xk), C.byref(xf), C.byref(xp), C.byref(xb))
        ok, db, da, br, bn, bm = C.c_int32(0), C.c_int64(0), C.c_int64(0), C.c_int32(0), C.c_int32(0), C.c_double(0.0)
        bd = C.c_int32(0)
        self._call("osc_balance_info", C.byref(ok), C.byref(db), C.byref(da), C.byref(br), C.byref(bn), C.byref(bm), C.byref(bd))
        levels: dict[str, int] = {}
        for fn, prefix, solves_key, has_redos in _ANCHOR_LEVELS:
            solves, nbytes, last, builds, redos = C.c_int64(0), C.c_int64(0), C.c_int32(0), C.c_int64(0), C.c_int64(0)
            self._call(fn, C.byref(solves), C.byref(nbytes), C.byref(last), C.byref(builds), *([C.byref(redos)] if has_redos else []))
            levels.update({solves_key: int(solves.value), prefix + "_bytes": int(nbytes.value),
                           prefix + "_last_solve": int(last.value), prefix + "_builds": int(builds.value)})
            if has_redos:
                levels[prefix + "_redos"] = int(redos.value)
            if prefix == "anchor_gram4":
                folded = C.c_int64(0)
                self._call("osc_gram4_fold_info", C.byref(folded), None)
                levels["folded_four_step_solves"] = int(folded.value)
        counters = nat.Counters()
        self._call("osc_counters_get", C.byref(counters))
        return {"order_kind": ("none", "bfs", "balanced")[int(ok.value)], "displaced_edges_before": int(db.value),
                "displaced_edges_after": int(da.value), "balance_rounds": int(br.value), "balance_src_blocks": int(bn.value),
                "balance_ms": float(bm.value), "balance_on_device": int(bd.value),
                "prefilter": int(pf.value), "fallback_rows": int(fb.value), "small_solves": int(ss.value),
                "reordered": int(ro.value), "clustering": float(cc.value), "apply_launches": int(ln.value),
                "apply_slab_cols": int(sc.value), "apply_xs_workgroups": int(xw.value),
                "apply_src_blocks": int(sb.value), "blocked_applies": int(ba.value),
                "apply_blocked_shape": int(counters.blocked_shape),
                "x_ring_slots": int(xk.value), "x_ring_flushes": int(xf.value), "x_ring_passes": int(xp.value),
                "x_ring_bytes": int(xb.value),
                **levels,
                # chain_receipt_many(lamP=...) keeps the basis of M + lamP I beside the query basis: N x ld + N x 4 floats
                # (ld >= D rounded up to 4); 0 until the first such call
                "shifted_basis_bytes": (4 * self.N * (((self.D + 3) // 4) * 4 + 4) if self._qbs_key is not None else 0)
                + (28 * self.N if self._qbs_key is not None and self._qbs_stats else 0)
                # receipt_many(lamP=...): M' x' (fp64) and, full detail, |P'_i - P'_j|^2 per ELL slot (max degree wide)
                + (8 * self.N if self._qbs_key is not None and self._qbs_receipt >= 1 else 0)
                + (4 * self.N * max(1, self.graph_stats()[1]) if self._qbs_key is not None and self._qbs_receipt >= 2 else 0),
                **{name: int(getattr(counters, name)) for name, _ in nat.Counters._fields_[1:]}}

    def _anchor_sums(self, fn: str, size: int) -> np.ndarray:
        out = np.zeros(size, dtype=np.float64)
        self._call(fn, out.ctypes.data_as(C.POINTER(C.c_double)), out.size)
        return out

    def anchor_gram(self) -> np.ndarray:
        """The float64 Gram sums the fused two-step INIT pass takes its CG scalars from, as held on the device: (22 ld + 6,)
        in the layout of include/oscillink_hip.h: osc_anchor_gram_read (test aid; raises while none are held)."""
        gb = C.c_int64(0)
        self._call("osc_anchor_gram_info", None, C.byref(gb), None, None, None)
        return self._anchor_sums("osc_anchor_gram_read", max(int(gb.value) // 8, 1))

    def anchor_gram3(self) -> np.ndarray:
        """The float64 sums of the two vectors the third step adds, as held on the device: (13 ld + 4,) in the layout of
        include/oscillink_hip.h: osc_anchor_gram3_read (test aid; raises while none are held)."""
        return self._anchor_sums("osc_anchor_gram3_read", 13 * ((self.anchor_gram().size - 6) // 22) + 4)

    def anchor_gram4(self) -> np.ndarray:
        """The float64 sums of the two vectors the fourth step's scalars add, as held on the device: (16 ld + 5,) in the layout
        of include/oscillink_hip.h: osc_anchor_gram4_read (test aid; raises while none are held)."""
        return self._anchor_sums("osc_anchor_gram4_read", 16 * ((self.anchor_gram().size - 6) // 22) + 5)

    def halo_info(self) -> dict[str, int]:
        """Row-sharded runs (OSC_SHARD=row under a communicator): the rows of the search direction this rank receives
        per CG iteration.  Collective on first use per graph (include/oscillink_hip.h: osc_halo_info)."""
        need, need_max, remote, nbytes, full = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int32(0)
        self._call("osc_halo_info", C.byref(need), C.byref(need_max), C.byref(remote), C.byref(nbytes), C.byref(full))
        return {"need_rows": int(need.value), "need_rows_max": int(need_max.value), "remote_rows": int(remote.value),
                "bytes_per_iteration": int(nbytes.value), "full_exchange": int(full.value)}

    def graph_csr(self):
        """Sparse lattice graph: (rowptr int64 (N+1), col int32, A float32 (capped adjacency), W float32, sqrt_deg)."""
        return self._host_csr()

    def _dense_guard(self) -> None:
        if self.N > _DENSE_VIEW_LIMIT:
            raise MemoryError(f"dense N x N view refused for N={self.N} (> {_DENSE_VIEW_LIMIT}); use graph_csr()")

    def _dense_from(self, vals: np.ndarray) -> np.ndarray:
        rowptr, col, _, _, _ = self._host_csr()
        out = np.zeros((self.N, self.N), dtype=np.float32)
        rows = np.repeat(np.arange(self.N), np.diff(rowptr))
        out[rows, col] = vals
        return out

    @property
    def A(self) -> np.ndarray:
        self._dense_guard()
        return self._dense_from(self._host_csr()[2])

    @A.setter
    def A(self, A: np.ndarray) -> None:
        """Inject a dense symmetric adjacency (from_state path, lattice.py:709-713)."""
        A = np.asarray(A, dtype=np.float32)
        if A.shape != (self.N, self.N):
            raise ValueError("A shape mismatch")
        # The reference takes whatever adjacency a state carries (lattice.py:709-713) and only promises approximate
        # symmetry after its row cap (graph.py:69-83); the device graph is an SPD operator with unit Laplacian
        # diagonal, so a dense adjacency is brought to that contract here instead of being refused by osc_set_csr:
        # the diagonal is dropped and float drift between A_ij and A_ji is averaged over the mutual support
        # ("Injected graphs").
        if np.any(np.diagonal(A) != 0) or not np.array_equal(A, A.T):
            A = A.copy()
            diag_nonzero = int(np.count_nonzero(np.diagonal(A)))
            np.fill_diagonal(A, 0.0)
            both = (A > 0) & (A.T > 0)
            dropped = int(np.count_nonzero((A > 0) & ~both))       # one-directional edges: not in the repaired graph
            drift = float(np.max(np.abs(A - A.T), where=both, initial=0.0))
            A = np.where(both, 0.5 * (A + A.T), 0.0).astype(np.float32)
            # the repair is never silent: a state whose graph changed on the way in says so (logger event + warning)
            info = {"diagonal_entries_dropped": diag_nonzero, "one_directional_edges_dropped": dropped,
                    "max_abs_asymmetry_averaged": drift}
            self._log("adjacency_repaired", info)
            if dropped or diag_nonzero or drift > 1e-6:
                import warnings

                warnings.warn(f"Oscillink: injected adjacency was brought to the graph contract ({info}); the reference "
                              "would have used it as given (lattice.py:709-713)", RuntimeWarning, stacklevel=2)
        r, c = np.nonzero(A > 0)
        rowptr = np.zeros(self.N + 1, dtype=np.int64)
        np.add.at(rowptr, r + 1, 1)
        self.set_graph_csr(np.cumsum(rowptr), c.astype(np.int32), A[r, c].astype(np.float32))

    def set_graph_csr(self, rowptr: np.ndarray, col: np.ndarray, a: np.ndarray) -> None:
        """Inject a (symmetric, zero-diagonal, already capped) adjacency as CSR; sqrt_deg / W are recomputed."""
        rowptr = np.ascontiguousarray(rowptr, dtype=np.int64)
        col = np.ascontiguousarray(col, dtype=np.int32)
        a = np.ascontiguousarray(a, dtype=np.float32)
        if rowptr.shape[0] != self.N + 1:
            raise ValueError("rowptr must have N+1 entries")
        self._call("osc_set_csr", nat.i64(rowptr), nat.i32(col) if col.size else None, nat.f32(a) if a.size else None)
        self._csr = None
        self._touch()
        self._qb_version += 1
        self._invalidate_cache()

    @property
    def L_sym(self) -> np.ndarray:
        self._dense_guard()
        return np.eye(self.N, dtype=np.float32) - self._dense_from(self._host_csr()[3])

    @property
    def sqrt_deg(self) -> np.ndarray:
        return self._host_csr()[4]

    def _path_dense(self):
        if self._chain_nodes is None:
            return None, None
        self._dense_guard()
        A = np.zeros((self.N, self.N), dtype=np.float32)
        ws = self._chain_weights or [1.0] * (len(self._chain_nodes) - 1)
        for t in range(len(self._chain_nodes) - 1):
            i, j, w = self._chain_nodes[t], self._chain_nodes[t + 1], float(ws[t])
            A[i, j] = max(A[i, j], w)
            A[j, i] = max(A[j, i], w)
        d = A.sum(axis=1)
        dm = 1.0 / np.sqrt(np.maximum(d, 1e-12))
        Lp = np.eye(self.N, dtype=np.float32) - ((A * dm[:, None]) * dm[None, :]).astype(np.float32)
        return Lp, A

    @property
    def L_path(self):
        return self._path_dense()[0]

    @property
    def A_path(self):
        return self._path_dense()[1]

    # ------------------------------------------------------------------ public API (lattice.py:114-157)
    def set_query(self, psi: np.ndarray, gates: Optional[np.ndarray] = None) -> None:
        p = np.ascontiguousarray(psi, dtype=np.float32).ravel().copy()
        g = None
        if gates is not None:
            if gates.shape[0] != self.N:
                raise ValueError("gates length mismatch N")
            g = np.ascontiguousarray(gates, dtype=np.float32).copy()
        if p.shape[0] != self.D:
            raise ValueError("psi length mismatch D")
        self._psi = p
        if g is not None:
            self._B = g
            self._qb_version += 1
        self._call("osc_set_query", nat.f32(self._psi), nat.f32(self._B) if g is not None else None)
        self._touch()
        self._invalidate_cache()

    def set_gates(self, gates: np.ndarray) -> None:
        if gates.shape[0] != self.N:
            raise ValueError("gates length mismatch N")
        self._B = np.ascontiguousarray(gates, dtype=np.float32).copy()
        self._call("osc_set_query", None, nat.f32(self._B))
        self._touch()
        self._qb_version += 1
        self._invalidate_cache()

    def add_chain(self, chain: list[int], lamP: float = 0.2, weights: Optional[list[float]] = None) -> None:
        if lamP < 0:
            raise ValueError("lamP must be >= 0")
        if any((c < 0 or c >= self.N) for c in chain):
            raise ValueError("chain indices out of bounds")
        if len(chain) < 2:
            raise ValueError("chain must contain at least two indices")
        if weights is not None and len(weights) != len(chain) - 1:
            raise ValueError("weights length must equal len(chain)-1")
        ch = np.asarray(list(map(int, chain)), dtype=np.int32)
        ws = None if weights is None else np.asarray(weights, dtype=np.float32)
        self._call("osc_set_chain", nat.i32(ch), None if ws is None else nat.f32(ws), int(ch.size), float(lamP))
        self.lamP = float(lamP)
        self._chain_nodes = [int(c) for c in chain]
        self._chain_weights = None if weights is None else [float(w) for w in weights]
        self._touch()
        self._qb_version += 1
        self._invalidate_cache()
        self._log("add_chain", {"length": len(chain), "lamP": lamP})

    def clear_chain(self) -> None:
        self._call("osc_clear_chain")
        self.lamP = 0.0
        self._chain_nodes = None
        self._chain_weights = None
        self._touch()
        self._qb_version += 1
        self._invalidate_cache()
        self._log("clear_chain", {})

    def _push_params(self) -> None:
        """lamG/lamC/lamQ/lamP are plain attributes in the reference and may be assigned directly."""
        self._call("osc_set_lams", float(self.lamG), float(self.lamC), float(self.lamQ))
        if self._chain_nodes is not None and float(self.lamP) != getattr(self, "_lamP_dev", None):
            ch = np.asarray(self._chain_nodes, dtype=np.int32)
            ws = None if self._chain_weights is None else np.asarray(self._chain_weights, dtype=np.float32)
            self._call("osc_set_chain", nat.i32(ch), None if ws is None else nat.f32(ws), int(ch.size), float(self.lamP))
        self._lamP_dev = float(self.lamP)

    # ------------------------------------------------------------------ settle (lattice.py:159-230)
    def settle(self, dt: float = 1.0, max_iters: int = 12, tol: float = 1e-3, precond: str = "jacobi", *,
               warm_start: bool = True, inertia: float = 0.0) -> dict[str, Any]:
        """Implicit Euler step (I + dt M) U+ = U + dt (lamG Y + lamQ B 1 psi^T) by Jacobi-PCG on the GPU."""
        dyn = os.getenv("OSCILLINK_RECEIPT_DYNAMICS", "0").strip().lower() in {"1", "true", "yes"}
        self._push_params()
        if dyn:  # device-side copy of the state before the step (the reference copies U on the host, lattice.py:213-216)
            self._call("osc_dynamics_snapshot")
        iters, res, ms = C.c_int32(0), C.c_float(0.0), C.c_double(0.0)
        self._call("osc_settle", float(dt), int(max_iters), float(tol), 1 if precond == "jacobi" else 0,
                   int(bool(warm_start)), float(inertia), C.byref(iters), C.byref(res), C.byref(ms))
        self._U_host = None
        self.last = {"iters": int(iters.value), "res": float(res.value), "t_ms": float(ms.value)}
        self._log("settle", self.last)
        if self.last["res"] > tol * 10:
            self._log("settle_convergence_warn", {"res": self.last["res"], "tol": tol, "iters": self.last["iters"]})
        if dyn:
            try:
                self._last_dynamics = self._compute_dynamics(None, None, self.last["iters"])
            except Exception:
                self._last_dynamics = None
        for cb in list(self._settle_callbacks):
            try:
                cb(self, self.last)
            except Exception:
                pass
        return self.last

    def residual_history(self) -> list[float]:
        """Residual after each iteration of the last solve (diagnostic; not in the reference)."""
        buf = np.zeros(4096, dtype=np.float32)
        n = C.c_int32(0)
        self._call("osc_residual_history", nat.f32(buf), 4096, C.byref(n))
        return buf[: n.value].astype(float).tolist()

    # ------------------------------------------------------------------ U* (lattice.py:232-296)
    def solve_Ustar(self, tol: float = 1e-4, max_iters: int = 64, use_cache: bool = True) -> np.ndarray:
        sig = self._signature()
        if use_cache and self._Ustar_sig == sig and self._device_ustar_sig == sig and (
                self._Ustar_cache is not None or self._device_has_ustar()):
            self.stats["ustar_cache_hits"] += 1
            self._log("ustar_cache_hit", {"signature": sig})
            if self._Ustar_cache is None:  # solved on the device for a receipt: fetch the rows on first host use
                self._Ustar_cache = self._download_ustar()
            return self._Ustar_cache
        self._solve_ustar_device(sig, tol, max_iters, use_cache)
        out = self._download_ustar()
        if use_cache:
            self._Ustar_cache = out
        return out

    def _download_ustar(self) -> np.ndarray:
        out = nat.result_array((self.N, self.D))
        self._call("osc_get_ustar", nat.f32(out))
        return out

    def _solve_ustar_device(self, sig: str, tol: float, max_iters: int, use_cache: bool) -> None:
        """Stationary solve on the device; U* stays resident there (receipts read it in place)."""
        self._push_params()
        iters, res, ms = C.c_int32(0), C.c_float(0.0), C.c_double(0.0)
        self._call("osc_solve_ustar", float(tol), int(max_iters), None, C.byref(iters), C.byref(res), C.byref(ms))
        converged = bool(float(res.value) <= tol)
        self.last_ustar = {"iters": int(iters.value), "res": float(res.value), "converged": converged,
                           "solve_ms": float(ms.value)}
        self._device_ustar_sig = sig
        self._Ustar_cache = None
        self._Ustar_sig = sig if use_cache else None
        self.stats["ustar_solves"] += 1
        self._log("ustar_solve", {"signature": sig, "tol": tol, "max_iters": max_iters, **self.last_ustar})
        if not converged:
            self._log("ustar_convergence_warn", {"res": float(res.value), "tol": tol, "iters": int(iters.value)})

    def refresh_Ustar(self, tol: float = 1e-4, max_iters: int = 64) -> np.ndarray:
        self._invalidate_cache()
        self._log("refresh_ustar", {})
        return self.solve_Ustar(tol=tol, max_iters=max_iters, use_cache=True)

    def _ensure_device_ustar(self) -> None:
        """U* resident on the device for the receipt kernels (same cache/stat semantics as solve_Ustar())."""
        sig = self._signature()
        if self._Ustar_sig == sig and self._device_ustar_sig == sig and self._device_has_ustar():
            self.stats["ustar_cache_hits"] += 1
            self._log("ustar_cache_hit", {"signature": sig})
            return
        self._solve_ustar_device(sig, 1e-4, 64, True)

    def _device_has_ustar(self) -> bool:
        yes = C.c_int32(0)
        self._call("osc_has_ustar", C.byref(yes))
        return bool(yes.value)

    def _host_ustar(self) -> np.ndarray:
        self._ensure_device_ustar()
        if self._Ustar_cache is None:
            self._Ustar_cache = self._download_ustar()
        return self._Ustar_cache

    # ------------------------------------------------------------------ receipts (lattice.py:298-455)
    def receipt(self) -> dict[str, Any]:
        self._ensure_device_ustar()
        dH = C.c_double(0.0)
        self._call("osc_deltaH", C.byref(dH))
        dH = float(np.float32(dH.value))
        cap_val = rc.null_cap()
        if self._receipt_detail == "light":
            coh_sum = anchor_sum = query_sum = 0.0
            nulls, total = [], 0
        else:
            coh, anc, qry, (i, j, z, r, total) = self._receipt_rows(3.0)
            coh_sum, anchor_sum, query_sum = float(np.sum(coh)), float(np.sum(anc)), float(np.sum(qry))
            if cap_val > 0 and total > cap_val:  # keep the highest z (lattice.py:341-349); stable like sorted()
                keep = np.argsort(-z[:total], kind="stable")[:cap_val]
                nulls = rc.null_dicts(i[keep], j[keep], z[keep], r[keep], cap_val)
            else:
                nulls = rc.null_dicts(i, j, z, r, total)
        nnz, _, _ = self.graph_stats()
        lu = getattr(self, "last_ustar", {})
        sig = self._signature()
        ustar = {"ustar_iters": int(lu.get("iters", 0)), "ustar_res": float(lu.get("res", 0.0)),
                 "ustar_converged": bool(lu.get("converged", True))}
        settle = self._last_settle_fields()
        meta = rc.meta(ustar_cached=self._Ustar_sig is not None and self._Ustar_sig == sig,
                       ustar_solves=self.stats["ustar_solves"], ustar_cache_hits=self.stats["ustar_cache_hits"], ustar=ustar,
                       ustar_solve_ms=lu.get("solve_ms", 0.0), graph_build_ms=self._graph_build_ms,
                       last_settle_ms=settle["t_ms"], degree=rc.degree_stats(nnz, self.N), gates=rc.gate_stats(self._B),
                       state_sig=sig, receipt_detail=self._receipt_detail,
                       null_points_summary=rc.null_summary(total, cap_val))
        rc.sign(meta, self._receipt_secret, self._signature_mode, state_sig=sig, deltaH=dH, ustar=ustar,
                **self._signed_settings())
        out = rc.record(version=__version__, deltaH=dH, coh_drop_sum=coh_sum, anchor_pen_sum=anchor_sum,
                        query_term_sum=query_sum, **settle, null_points=nulls, meta=meta)
        if os.getenv("OSCILLINK_RECEIPT_DYNAMICS", "0").strip().lower() in {"1", "true", "yes"} and self._last_dynamics:
            meta["dynamics"] = self._last_dynamics
        self._log("receipt", {"deltaH_total": out["deltaH_total"], "ustar_cached": meta["ustar_cached"]})
        return out

    def _last_settle_fields(self) -> dict[str, Any]:
        """The last settle as a receipt reports it (record()'s cg_iters / residual / t_ms)."""
        return {"cg_iters": int(self.last.get("iters") or 0), "residual": float(self.last.get("res") or 0.0),
                "t_ms": float(self.last.get("t_ms") or 0.0)}

    def _signed_settings(self) -> dict[str, Any]:
        """The `params` and `graph` blocks of the extended signature payload."""
        return {"params": {"lamG": self.lamG, "lamC": self.lamC, "lamQ": self.lamQ, "lamP": self.lamP},
                "graph": {"k": self._kneighbors, "deterministic_k": self._deterministic_k,
                          "neighbor_seed": self._neighbor_seed}}

    def _components(self):
        coh = np.zeros(self.N, dtype=np.float32)
        anc = np.zeros(self.N, dtype=np.float32)
        qry = np.zeros(self.N, dtype=np.float32)
        self._call("osc_receipt_components", nat.f32(coh), nat.f32(anc), nat.f32(qry))
        return coh, anc, qry

    def _receipt_rows(self, z_th: float):
        coh = np.zeros(self.N, dtype=np.float32)
        anc = np.zeros(self.N, dtype=np.float32)
        qry = np.zeros(self.N, dtype=np.float32)
        i = np.zeros(self.N, dtype=np.int32)
        j = np.zeros(self.N, dtype=np.int32)
        z = np.zeros(self.N, dtype=np.float32)
        r = np.zeros(self.N, dtype=np.float32)
        n = C.c_int32(0)
        self._call("osc_receipt_rows", float(z_th), nat.f32(coh), nat.f32(anc), nat.f32(qry), nat.i32(i), nat.i32(j),
                   nat.f32(z), nat.f32(r), C.byref(n))
        return coh, anc, qry, (i, j, z, r, int(n.value))

    def _coherence_drop(self, Ustar: Optional[np.ndarray] = None) -> np.ndarray:
        self._ensure_device_ustar()
        return self._components()[0]

    def _null_points(self, z_th: float) -> list[dict[str, Any]]:
        i = np.zeros(self.N, dtype=np.int32)
        j = np.zeros(self.N, dtype=np.int32)
        z = np.zeros(self.N, dtype=np.float32)
        r = np.zeros(self.N, dtype=np.float32)
        n = C.c_int32(0)
        self._call("osc_null_points", float(z_th), nat.i32(i), nat.i32(j), nat.f32(z), nat.f32(r), C.byref(n))
        return rc.null_dicts(i, j, z, r, n.value)

    def verify_current_receipt(self, secret) -> bool:
        from .receipts import verify_receipt

        return verify_receipt(self.receipt(), secret)

    # ------------------------------------------------------------------ chain receipt (lattice.py:466-528), sparse
    def _fetch_rows(self, which: int, rows: np.ndarray) -> np.ndarray:
        """Selected rows (caller's ids) of Y (0), U (1) or the resident U* (2) as an (n, D) array."""
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        out = np.empty((rows.size, self.D), dtype=np.float32)
        self._call("osc_get_rows", int(which), nat.i32(rows), int(rows.size), nat.f32(out))
        return out

    def chain_receipt(self, chain: list[int], z_th: float = 2.5) -> dict[str, Any]:
        rowptr, col, a, _, sd = self._host_csr()
        di = sd + 1e-12
        N = self.N
        lamC = float(self.lamC)
        # only the chain nodes and their structural / path neighbours are read: fetch those rows of U* (and the chain's
        # rows of Y) instead of mirroring the N x D arrays on the host
        own_nodes = self._chain_nodes if self._chain_nodes is not None else [int(c) for c in chain]
        need = {int(c) for c in chain if 0 <= int(c) < N} | {int(c) for c in own_nodes if 0 <= int(c) < N}
        for c in [int(c) for c in chain if 0 <= int(c) < N]:
            need.update(int(j) for j in col[rowptr[c]: rowptr[c + 1]])
        need_ids = np.array(sorted(need), dtype=np.int64)
        if self._Ustar_cache is not None and self._Ustar_sig == self._signature():
            Ustar_rows = self._Ustar_cache[need_ids]
        else:
            self._ensure_device_ustar()
            Ustar_rows = self._fetch_rows(2, need_ids)
        slot = {int(r): t for t, r in enumerate(need_ids)}

        class _Rows:  # Ustar[i] / Ustar[js] on the fetched subset
            def __getitem__(_self, key):
                if isinstance(key, (int, np.integer)):
                    return Ustar_rows[slot[int(key)]]
                return Ustar_rows[[slot[int(t)] for t in np.asarray(key).ravel()]]

        Ustar = _Rows()
        chain_ids = np.array(sorted({int(c) for c in chain if 0 <= int(c) < N}), dtype=np.int64)
        Y_rows = self._Y_host[chain_ids] if self._Y_host is not None else self._fetch_rows(0, chain_ids)
        yslot = {int(r): t for t, r in enumerate(chain_ids)}

        def un(i):
            return Ustar[i] / di[i]

        def row_stats(i, extra=None):
            """mean / std (+1e-12) over the N entries of the dense residual row i (zeros included)."""
            R = extra
            mu = float(np.sum(R, dtype=np.float64) / N)
            var = float((np.sum((R.astype(np.float64) - mu) ** 2) + (N - R.size) * mu * mu) / N)
            return mu, float(np.sqrt(max(var, 0.0))) + 1e-12

        def struct_row(i):
            js = col[rowptr[i]: rowptr[i + 1]]
            if js.size == 0:
                return js, np.zeros(0, dtype=np.float32)
            d = un(i)[None, :] - Ustar[js] / di[js, None]
            return js, (lamC * a[rowptr[i]: rowptr[i + 1]] * np.einsum("ij,ij->i", d, d).astype(np.float32)).astype(np.float32)

        # path adjacency: the lattice's own chain if set, else the argument (lattice.py:479-483)
        nodes = self._chain_nodes if self._chain_nodes is not None else [int(c) for c in chain]
        ws = (self._chain_weights if self._chain_nodes is not None else None) or [1.0] * (len(nodes) - 1)
        padj: dict[int, dict[int, float]] = {}
        for t in range(len(nodes) - 1):
            i, j, w = nodes[t], nodes[t + 1], float(ws[t])
            if 0 <= i < N and 0 <= j < N:
                padj.setdefault(i, {})[j] = max(padj.get(i, {}).get(j, 0.0), w)
                padj.setdefault(j, {})[i] = max(padj.get(j, {}).get(i, 0.0), w)
        lam_p = max(lamC, 1e-6)

        def path_row(i):
            nb = padj.get(i, {})
            js = np.array(sorted(nb), dtype=np.int64)
            if js.size == 0:
                return js, np.zeros(0, dtype=np.float32)
            d = un(i)[None, :] - Ustar[js] / di[js, None]
            wv = np.array([nb[int(j)] for j in js], dtype=np.float32)
            return js, (lam_p * wv * np.einsum("ij,ij->i", d, d).astype(np.float32)).astype(np.float32)

        edges: list[dict[str, Any]] = []
        worst = (-1, -1.0, (-1, -1))
        gain = 0.0
        for k in range(len(chain) - 1):
            i, j = int(chain[k]), int(chain[k + 1])
            sj, sR = struct_row(i)
            pj, pR = path_row(i)
            mu_s, sig_s = row_stats(i, sR)
            mu_p, sig_p = row_stats(i, pR)
            rs = float(sR[np.nonzero(sj == j)[0][0]]) if np.any(sj == j) else 0.0
            rp = float(pR[np.nonzero(pj == j)[0][0]]) if np.any(pj == j) else 0.0
            z_struct = float((rs - mu_s) / sig_s)
            z_path = float((rp - mu_p) / sig_p)
            edges.append({"k": int(k), "edge": [i, j], "z_struct": z_struct, "z_path": z_path, "r_struct": rs,
                          "r_path": rp})
            if max(z_struct, z_path) > worst[1]:
                worst = (k, max(z_struct, z_path), (i, j))
            w_ij = float(a[rowptr[i]: rowptr[i + 1]][sj == j][0]) if np.any(sj == j) else 0.0
            ydiff = Y_rows[yslot[i]] / di[i] - Y_rows[yslot[j]] / di[j]
            udiff = un(i) - un(j)
            gain += 0.5 * lamC * max(w_ij, 0.0) * (float(ydiff @ ydiff) - float(udiff @ udiff))
        verdict = all(max(float(e["z_struct"]), float(e["z_path"])) <= float(z_th) for e in edges)
        return {"verdict": bool(verdict),
                "weakest_link": {"k": int(worst[0]), "edge": [int(worst[2][0]), int(worst[2][1])],
                                 "zscore": float(worst[1])},
                "coherence_gain": float(gain), "edges": edges}

    # ------------------------------------------------------------------ bundle (lattice.py:530-568; graph.py:114-133)
    def bundle(self, k: int = 8, alpha: float = 0.5) -> list[dict]:
        """lattice.py:530-568.  The alignment term and the MMR similarity rows are formed on the device from the resident
        U* / anchors (no N x D host copy: at N = 100k, D = 768 the NumPy form of this call took 380 ms)."""
        self._ensure_device_ustar()
        align = np.empty(self.N, dtype=np.float32)
        self._call("osc_ustar_cosine_to", nat.f32(np.ascontiguousarray(self._psi, dtype=np.float32)), nat.f32(align))
        coh = self._components()[0]
        mu, sigma = float(np.mean(coh)), float(np.std(coh) + 1e-12)
        z = (coh - mu) / sigma if sigma > 0 else np.zeros_like(coh)
        score = alpha * z + (1 - alpha) * align.squeeze()
        order = np.asarray(self._mmr(score, k, 0.5), dtype=np.intp)
        return rc.bundle_dicts(order, score[order], align[order])

    def _mmr(self, scores: np.ndarray, k: int, lambda_div: float) -> list[int]:
        """Greedy MMR over cosine similarity of Y (graph.py:114-133) as ONE device call: per step an argmax over the
        candidates and one pass over the anchors for the chosen item's similarity row (O(kND), nothing N x N)."""
        if k <= 0:
            return []
        want = min(int(k), self.N)
        out = np.zeros(want, dtype=np.int32)
        n = C.c_int32(0)
        self._call("osc_mmr", nat.f32(np.ascontiguousarray(scores, dtype=np.float32)), want, float(lambda_div),
                   nat.i32(out), C.byref(n))
        return [int(i) for i in out[: int(n.value)]]

    # ------------------------------------------------------------------ multi-query bundles (not in the reference)
    def bundle_many(self, psis: np.ndarray, k: int = 8, alpha: float = 0.5, *, tol: float = 1e-4, max_iters: int = 256,
                    as_arrays: bool = False, chains=None, lamP: Optional[float] = None, chain_weights=None):
        """`bundle(k, alpha)` for each row of `psis` (Q x D), as if `set_query(psis[q])` had been called, without touching
        the lattice's state (psi, U, the U* cache, receipts).  One query basis solve (U*(psi) =
        X + x psi^T) serves every query; a batch is then a GEMM, one graph pass, column statistics and a batched MMR on
        the device.  Returns Q lists of {"id", "score", "align"} (bundle()'s order), or with `as_arrays=True`
        (ids, score, align), each Q x min(k, N).

        With `chains` and `lamP` (>= 0) query q also carries a chain PRIOR: it gets what
        `add_chain(chains[q], lamP, chain_weights[q]); set_query(psis[q]); bundle(k, alpha)` gives on a lattice without a
        chain of its own, from the basis of the shifted operator `chain_receipt_many(lamP=...)` uses (the same slot and
        key) and one Green's column per distinct chain node.  `chains` and `chain_weights` take `chain_receipt_many`'s
        forms; a chain has at most 64 distinct nodes.  Per query the residual bound and the Green's columns' iterations
        go to `last_bundle_prior` = {"lamP", "res" (float32), "iters" (int32)}.  `lamP=0` is the plain call.

        Per-query GATES are `bundle_gated_many`'s."""
        if self._has_comm:
            raise NotImplementedError("bundle_many: lattices with a communicator (sharded / multi-rank) are not supported")
        prior = rc.check_prior_args("bundle_many", chains, lamP, chain_weights, self._chain_nodes is not None)
        P = rc.check_queries(psis, self.D)
        Q = int(P.shape[0])
        kk = min(int(k), self.N) if k > 0 else 0
        ids, score, align = _bundle_arrays(Q, kk)
        if prior:
            _, offsets, nodes, weights = rc.prior_chain_block(chains, chain_weights, Q, self.N)
            prior_res, prior_iters = np.zeros(Q, dtype=np.float32), np.zeros(Q, dtype=np.int32)
            if Q > 0 and kk > 0:
                psi_inf = float(np.max(np.abs(P)))
                if float(lamP) > 0:
                    self._ensure_shifted_basis(float(lamP), tol, max_iters, psi_inf)
                else:
                    self._ensure_query_basis(tol, max_iters, psi_inf)
                self._call("osc_bundle_prior_many", nat.f32(P), Q, nat.i64(offsets), nat.i32(nodes),
                           None if weights is None else nat.f32(weights), float(lamP), float(tol), int(max_iters), kk,
                           float(alpha), 0.5, nat.i32(ids), nat.f32(score), nat.f32(align), nat.f32(prior_res),
                           nat.i32(prior_iters))
                self._qbs_stats = self._qbs_stats or float(lamP) > 0
            self.last_bundle_prior = {"lamP": float(lamP), "res": prior_res, "iters": prior_iters}
            self._warn_chain_prior(prior_res, prior_iters, tol)
        elif Q > 0 and kk > 0:
            self._ensure_query_basis(tol, max_iters, float(np.max(np.abs(P))))
            self._call("osc_bundle_many", nat.f32(P), Q, kk, float(alpha), 0.5, nat.i32(ids), nat.f32(score), nat.f32(align))
        return _bundle_result(ids, score, align, as_arrays)

    def _check_gate_rows(self, gates) -> np.ndarray:
        """Per-query gates as a contiguous float32 (Q, N) array (Q is not checked here), or the ValueError for a single
        gate vector."""
        G = np.asarray(gates)
        if G.ndim == 1:
            raise ValueError(f"gates must be a (Q, {self.N}) array, one row per query; one gate vector for every query is "
                             "set_gates(gates) followed by bundle_many(psis)")
        if G.ndim != 2 or G.shape[1] != self.N:
            raise ValueError(f"gates must be a (Q, {self.N}) array, got shape {G.shape}")
        return np.ascontiguousarray(G, dtype=np.float32)

    def bundle_gated_many(self, psis: np.ndarray, gates, k: int = 8, alpha: float = 0.5, *, tol: float = 1e-4,
                          max_iters: int = 256, as_arrays: bool = False, gate_beta: float = 1.0, gate_gamma: float = 0.1,
                          gate_method: str = "direct", gate_tol: float = 1e-4, gate_max_iters: int = 256):
        """`bundle_many` with gates of its own for every query: query q gets what
        `set_query(psis[q], gates=G[q]); bundle(k, alpha)` gives, the lattice's own gates, psi, U, U* cache, query basis
        and receipts being neither read nor changed.  `gates` is a (Q, N) array in API row order (finite, >= 0), or
        "diffusion": `diffusion_gates_many(psis, beta=gate_beta, gamma=gate_gamma, method=gate_method, tol=gate_tol,
        max_iters=gate_max_iters)["gates"]`, computed in the same call.  M differs per query, so every query is its own
        N x D solve of `solve_Ustar` -- the reference's rule: stop at the first iteration where the query's largest column
        residual is <= `tol` -- and the Q solves run as one panel CG over the shared graph, `OSC_GATED_CHUNK` queries at
        a time.  The loop's `solve_Ustar()` runs to 1e-4 in at most 64 iterations; the default `max_iters=256` here only
        matters for a query that has not converged at 64.  Returns `bundle_many`'s forms: Q lists of {"id", "score",
        "align"}, or with `as_arrays=True` (ids, score, align).  The solve report goes to `last_bundle_gated` = {"iters"
        (int32), "res" (float32), "converged" (bool), "gates" ((Q, N) float32 for "diffusion", else None)}.  A non-finite
        query row (or non-finite diffusion gates, which raise `diffusion_gates_many`'s warning) gives that query
        non-finite answers and changes no other query's.  Its own method because `bundle_many`'s parameter list is
        pinned; per-query gates combined with per-query chain priors are `chain_gated_many`'s, and a lattice with a
        chain of its own raises NotImplementedError."""
        P, Q, G, diffusion = _gated_call_inputs(self, "bundle_gated_many", psis, gates, gate_gamma, gate_method,
                                                gate_max_iters, max_iters)
        kk = min(int(k), self.N) if k > 0 else 0
        ids, score, align = _bundle_arrays(Q, kk)
        iters = np.zeros(Q, dtype=np.int32)
        res = np.zeros(Q, dtype=np.float32)
        if Q > 0:
            self._push_params()
            self._call("osc_bundle_gated_many", nat.f32(P), Q, nat.f32(G), int(diffusion), float(gate_beta),
                       float(gate_gamma), 1 if gate_method == "cg" else 0, float(gate_tol), int(gate_max_iters), float(tol),
                       int(max_iters), kk, float(alpha), 0.5, nat.i32(ids), nat.f32(score), nat.f32(align), nat.i32(iters),
                       nat.f32(res))
        if diffusion:
            _warn_diffusion_gates(G)
        self.last_bundle_gated = {"iters": iters, "res": res, "converged": res <= np.float32(tol),
                                  "gates": G if diffusion else None}
        self._log("bundle_gated_many", {"Q": Q, "k": kk, "gates": "diffusion" if diffusion else "given",
                                        "iters_max": int(iters.max()) if Q else 0,
                                        "converged": int(np.count_nonzero(res <= np.float32(tol)))})
        return _bundle_result(ids, score, align, as_arrays)

    def _ustar_gated_many(self, psis: np.ndarray, gates: np.ndarray, tol: float = 1e-4, max_iters: int = 256):
        """The solves of bundle_gated_many alone: (U (Q, N, D) float32 in API row order, iters (Q,) int32, res (Q,)
        float32).  Private: exposed for tests, as `_mmr_many` is; neither the queries nor the gates are checked for
        finite values."""
        if self._has_comm:
            raise NotImplementedError("_ustar_gated_many: lattices with a communicator are not supported")
        P = rc.check_queries(psis, self.D, finite=False)
        G = self._check_gate_rows(gates)
        Q = int(P.shape[0])
        if G.shape[0] != Q:
            raise ValueError(f"gates must be a ({Q}, {self.N}) array, got shape {G.shape}")
        U = np.zeros((Q, self.N, self.D), dtype=np.float32)
        iters = np.zeros(Q, dtype=np.int32)
        res = np.zeros(Q, dtype=np.float32)
        if Q > 0:
            self._push_params()
            self._call("osc_ustar_gated_many", nat.f32(P), Q, nat.f32(G), float(tol), int(max_iters), nat.f32(U),
                       nat.i32(iters), nat.f32(res))
        return U, iters, res

    _GATED_SETTLE_DEFAULTS = {"dt": 1.0, "max_iters": 12, "tol": 1e-3}

    def receipt_gated_many(self, psis: np.ndarray, gates, *, settle=None, bundle_k: Optional[int] = None, alpha: float = 0.5,
                           tol: float = 1e-4, max_iters: int = 256, as_arrays: bool = False, gate_beta: float = 1.0,
                           gate_gamma: float = 0.1, gate_method: str = "direct", gate_tol: float = 1e-4,
                           gate_max_iters: int = 256):
        """The gated flow's receipt -- and optionally its settle and bundle -- for every row of `psis` in one call
        (DESIGN.md section 12.4).  `psis`, `gates` ((Q, N) in API row order, or "diffusion") and the `gate_*` arguments are
        `bundle_gated_many`'s, with its validation and errors.  The lattice's psi, gates, U, U* cache, query basis, `stats`,
        `last` and receipts are not changed; of its state only U is read.

        `settle=None`: query q gets the record of `set_query(psis[q], gates=G[q]); receipt()` with the current U held fixed
        (`receipt_many`'s contract: the settle fields are the lattice's last settle).  `settle=True` or a dict with any of
        {"dt": 1.0, "max_iters": 12, "tol": 1e-3}: the record of `set_query(...); settle(dt, max_iters, tol); receipt()`,
        every query started from the lattice's current U (warm start, no inertia) and no settled state written back;
        `cg_iters` / `residual` are the query's own settle, `t_ms` and `meta.last_settle_ms` its chunk's settle time divided
        by the chunk's queries.  U*_q is `bundle_gated_many`'s solve (`tol`, `max_iters`): `ustar_iters` / `ustar_res` /
        `ustar_converged` are the query's own, `ustar_cached` is False, `ustar_source` is "gated_panel".

        `bundle_k=None` returns the Q records; an int returns `(records, bundles)`, the bundles being
        `bundle_gated_many(psis, gates, bundle_k, alpha)`'s from the same solve, bit for bit.  `as_arrays=True` returns
        `receipt_many`'s dict of arrays plus `ustar_iters`, `ustar_res`, with `settle` also `settle_iters`, `settle_res`, and
        with `bundle_k` also `ids`, `score`, `align`.  Detail mode, OSCILLINK_RECEIPT_NULL_CAP, the secret and signature mode
        and OSCILLINK_RECEIPT_DYNAMICS behave as in `receipt_many`.  The report goes to `last_receipt_gated` = {"iters",
        "res", "converged", "settle_iters", "settle_res" (None without `settle`), "gates" (as `last_bundle_gated`)}."""
        return OscillinkLattice._gated_receipts(self, "receipt_gated_many", psis, gates, None, settle, bundle_k, alpha, tol,
                                                max_iters, as_arrays, gate_beta, gate_gamma, gate_method, gate_tol,
                                                gate_max_iters)

    def _gated_settle_arg(self, settle) -> Optional[dict]:
        """The `settle` argument of the gated calls as None or the checked dict of dt / max_iters / tol."""
        if settle is None or settle is False:
            return None
        st = dict(self._GATED_SETTLE_DEFAULTS)
        if settle is not True:
            if not isinstance(settle, dict):
                raise ValueError("settle must be None, True or a dict of dt / max_iters / tol")
            unknown = sorted(set(settle) - set(st))
            if unknown:
                raise ValueError(f"settle: unknown keys {unknown}")
            st.update(settle)
        if not float(st["dt"]) > 0:
            raise ValueError("settle: dt must be > 0")
        if int(st["max_iters"]) < 1:
            raise ValueError("settle: max_iters must be >= 1")
        return st

    def _gated_receipts(self, fn, psis, gates, chain, settle, bundle_k, alpha, tol, max_iters, as_arrays, gate_beta,
                        gate_gamma, gate_method, gate_tol, gate_max_iters):
        """`receipt_gated_many` (chain=None) and `chain_gated_many` (chain = {"chains", "lamP", "chain_weights", "z_th"}):
        one argument check, one native call, one record assembly.  With a chain the return carries the chain receipts
        behind the records, and the signature the argument's lamP, `chain_present` and the chain's length."""
        P, Q, G, diffusion = _gated_call_inputs(self, fn, psis, gates, gate_gamma, gate_method, gate_max_iters, max_iters)
        st = OscillinkLattice._gated_settle_arg(self, settle)  # (by the class: the host tests pass a stub)
        if bundle_k is not None and int(bundle_k) < 0:
            raise ValueError("bundle_k must be None or >= 0")
        lamP = None
        if chain is not None:
            rc.check_prior_lamP(fn, chain["lamP"], False)
            lamP = float(chain["lamP"])
            lists, offsets, nodes = rc.chain_block(chain["chains"], Q, self.N)
            edge_offsets = offsets - np.arange(Q + 1, dtype=np.int64)
            weights = rc.chain_prior_weights(chain["chain_weights"], chain["chains"], lists, edge_offsets)
            n_edges = int(edge_offsets[-1])
            edge = np.zeros((4, max(n_edges, 1)), dtype=np.float32)
            gain = np.zeros(Q, dtype=np.float64)
            verdict, weak_k = np.zeros(Q, dtype=np.int32), np.zeros(Q, dtype=np.int32)
            weak_z = np.zeros(Q, dtype=np.float32)
        with_bundle = bundle_k is not None
        kk = min(int(bundle_k), self.N) if with_bundle else 0
        full = self._receipt_detail != "light"
        cap_val = rc.null_cap()
        ra = rc.ReceiptArrays(Q, (min(cap_val, self.N) if cap_val > 0 else self.N) if full else 0, settle=st is not None)
        ids, score, align = _bundle_arrays(Q, kk)
        iters = np.zeros(Q, dtype=np.int32)
        res = np.zeros(Q, dtype=np.float32)
        settle_ms, solve_ms = np.zeros(Q, dtype=np.float64), np.zeros(Q, dtype=np.float64)
        if Q > 0:
            self._push_params()
            s_args = (1, float(st["dt"]), int(st["max_iters"]), float(st["tol"])) if st else (0, 1.0, 1, 0.0)
            head = [nat.f32(P), Q, nat.f32(G), int(diffusion), float(gate_beta), float(gate_gamma),
                    1 if gate_method == "cg" else 0, float(gate_tol), int(gate_max_iters)]
            tail = [float(tol), int(max_iters), *s_args, int(full), 3.0, cap_val, kk, float(alpha), 0.5,
                    *([] if st else [None, None]), *ra.pointers(), nat.i32(ids), nat.f32(score), nat.f32(align),
                    nat.i32(iters), nat.f32(res), settle_ms.ctypes.data_as(nat.c_f64p), solve_ms.ctypes.data_as(nat.c_f64p)]
            if chain is None:
                self._call("osc_receipt_gated_many", *head, *tail)
            else:
                self._call("osc_chain_gated_many", *head, nat.i64(offsets), nat.i32(nodes),
                           None if weights is None else nat.f32(weights), lamP, float(chain["z_th"]), *tail,
                           *[nat.f32(edge[t]) for t in range(4)], gain.ctypes.data_as(nat.c_f64p), nat.i32(verdict),
                           nat.i32(weak_k), nat.f32(weak_z))
        ra.round_sums()
        if diffusion:
            _warn_diffusion_gates(G)
        converged = res <= np.float32(tol)
        report = {"iters": iters, "res": res, "converged": converged, "settle_iters": ra.settle[0] if st else None,
                  "settle_res": ra.settle[1] if st else None, "gates": G if diffusion else None}
        payload = {"Q": Q, "receipt_detail": self._receipt_detail, "settle": st is not None,
                   "bundle_k": kk if with_bundle else None, "gates": "diffusion" if diffusion else "given",
                   "iters_max": int(iters.max()) if Q else 0, "converged": int(np.count_nonzero(converged)),
                   "null_points": ra.kept}
        if chain is None:
            self.last_receipt_gated = report
        else:
            self.last_chain_gated = {**report, "lamP": lamP}
            payload.update(lamP=lamP, edges=n_edges)
            carr = dict(chain_offsets=edge_offsets, chain_z_struct=edge[0, :n_edges].copy(),
                        chain_z_path=edge[1, :n_edges].copy(), chain_r_struct=edge[2, :n_edges].copy(),
                        chain_r_path=edge[3, :n_edges].copy(), chain_gain=gain, chain_verdict=verdict != 0,
                        chain_weakest_k=weak_k, chain_weakest_z=weak_z)
        self._log(fn, payload)
        if as_arrays:
            out = {**ra.scalar_arrays(), **ra.null_arrays(), "ustar_iters": iters, "ustar_res": res}
            if chain is not None:
                out.update(carr)
            if with_bundle:
                out.update(ids=ids, score=score, align=align)
            return out
        bundles = [rc.bundle_dicts(ids[q], score[q], align[q]) for q in range(Q)]
        crecs = rc.chain_receipt_dicts(lists, carr) if chain is not None else None
        if Q == 0:
            if chain is None:
                return ([], []) if with_bundle else []
            return ([], [], []) if with_bundle else ([], [])
        # everything but psi, the gates, the energies, the null points, the settle and the ustar fields is shared by the batch
        nnz, _, _ = self.graph_stats()
        adj_sig = hashlib.sha256(np.ascontiguousarray(self._edge_prefix()).tobytes()).hexdigest()
        sig_rest = {"lam": [self.lamG, self.lamC, self.lamQ, self.lamP if chain is None else lamP],
                    "chain_present": chain is not None, "chain_len": 0, "k": self._kneighbors, "detk": self._deterministic_k,
                    "adj": adj_sig}
        degree, signed = rc.degree_stats(nnz, self.N), self._signed_settings()
        if chain is not None:
            signed = {**signed, "params": {**signed["params"], "lamP": lamP}}
        last = self._last_settle_fields()
        dyn = self._last_dynamics if os.getenv("OSCILLINK_RECEIPT_DYNAMICS", "0").strip().lower() in {"1", "true", "yes"} \
            else None
        out = []
        for q in range(Q):
            if chain is not None:
                sig_rest["chain_len"] = len(lists[q])
            sig = self._signature_digest({"psi": np.round(P[q], 6).tolist(), **sig_rest}, G[q])
            dH = float(ra.sums[0, q])
            ustar = {"ustar_iters": int(iters[q]), "ustar_res": float(res[q]), "ustar_converged": bool(converged[q])}
            fields = last if st is None else {"cg_iters": int(ra.settle[0][q]), "residual": float(ra.settle[1][q]),
                                              "t_ms": float(settle_ms[q])}
            nulls, tot = ra.nulls(q)
            meta = rc.meta(ustar_cached=False, ustar_solves=self.stats["ustar_solves"],
                           ustar_cache_hits=self.stats["ustar_cache_hits"], ustar=ustar, ustar_solve_ms=float(solve_ms[q]),
                           ustar_source="gated_panel", graph_build_ms=self._graph_build_ms, last_settle_ms=fields["t_ms"],
                           degree=degree, gates=rc.gate_stats(G[q]), state_sig=sig, receipt_detail=self._receipt_detail,
                           null_points_summary=rc.null_summary(tot, cap_val))
            rc.sign(meta, self._receipt_secret, self._signature_mode, state_sig=sig, deltaH=dH, ustar=ustar, **signed)
            rec = rc.record(version=__version__, deltaH=dH, coh_drop_sum=ra.sums[1, q], anchor_pen_sum=ra.sums[2, q],
                            query_term_sum=ra.sums[3, q], **fields, null_points=nulls, meta=meta)
            if dyn:
                meta["dynamics"] = dyn
            out.append(rec)
        if chain is not None:
            return (out, crecs, bundles) if with_bundle else (out, crecs)
        return (out, bundles) if with_bundle else out

    def chain_gated_many(self, psis: np.ndarray, gates, chains, lamP: float = 0.2, *, chain_weights=None, z_th: float = 2.5,
                         settle=None, bundle_k: Optional[int] = None, alpha: float = 0.5, tol: float = 1e-4,
                         max_iters: int = 256, as_arrays: bool = False, gate_beta: float = 1.0, gate_gamma: float = 0.1,
                         gate_method: str = "direct", gate_tol: float = 1e-4, gate_max_iters: int = 256):
        """The whole request sequence under per-query gates AND a per-query chain prior, for every row of `psis` in one
        call.  On a lattice without a chain of its own, holding this lattice's U, query q gets
        what `add_chain(chains[q], lamP, chain_weights[q]); set_query(psis[q], gates=G[q]); [settle(**settle);]
        r = receipt(); c = chain_receipt(chains[q], z_th); [b = bundle(bundle_k, alpha)]` returns.  The lattice's psi,
        gates, U, U* cache, query basis, shifted-basis slot, `stats`, `last` and receipts are not changed; of its state
        only U is read.

        `psis`, `gates` ((Q, N) or "diffusion": the gates of the lattice WITHOUT the chain), `settle`, `bundle_k`, `alpha`,
        `tol`, `max_iters` and the `gate_*` arguments are `receipt_gated_many`'s, with its validation and errors.  `chains`
        and `chain_weights` take `chain_receipt_many`'s forms -- one chain shared by all queries, or Q chains of 2 to 1024
        nodes; repeated nodes, self-steps and revisited edges behave as in `add_chain` -- without the 64-distinct-node limit
        of the low-rank calls: with gates every query is its own N x D solve already, and its chain is a term of its own
        operator.  `lamP` >= 0; with `lamP == 0` the operator carries no path term and the receipts and bundles are
        `receipt_gated_many`'s bit for bit, the signature still says `chain_present`, and the chain receipt is still
        computed.

        Returns `(records, chain_records)`, with `bundle_k` `(records, chain_records, bundles)`: `receipt_gated_many`'s
        records (the signature carries the argument's lamP, `chain_present` and the chain's length; `ustar_source` is
        "gated_panel") and `chain_receipt`'s dicts.  `as_arrays=True` returns one dict: `receipt_gated_many`'s arrays,
        `chain_receipt_many`'s (`chain_offsets`, `chain_z_struct`, ... `chain_weakest_z`) and with `bundle_k` `ids`, `score`,
        `align`.  The report goes to `last_chain_gated` = `last_receipt_gated`'s keys plus "lamP".  A non-finite query row
        gives that query non-finite answers and changes no other query's bytes.  A lattice with a chain of its own or with
        a communicator raises NotImplementedError."""
        chain = {"chains": chains, "lamP": lamP, "chain_weights": chain_weights, "z_th": z_th}
        return OscillinkLattice._gated_receipts(self, "chain_gated_many", psis, gates, chain, settle, bundle_k, alpha, tol,
                                                max_iters, as_arrays, gate_beta, gate_gamma, gate_method, gate_tol,
                                                gate_max_iters)

    def receipt_many(self, psis: np.ndarray, *, tol: float = 1e-4, max_iters: int = 256, as_arrays: bool = False,
                     chains=None, lamP: Optional[float] = None, chain_weights=None):
        """`receipt()` for each row of `psis` (Q x D), as if `set_query(psis[q]); receipt()` had run with the current U,
        gates, chain, lambdas and receipt / signature settings held fixed, without touching the lattice's state.  U*(psi_q)
        comes from the query basis `bundle_many` uses (same key, cache and tolerance contract): every
        energy is a quadratic in psi over per-basis and per-call terms, and full detail adds one GEMM and one graph pass per
        256 queries.  The meta's ustar_* fields describe the basis (`"ustar_source": "query_basis"`).

        Full detail at a large N reports a null point on most rows (about N per query): set OSCILLINK_RECEIPT_NULL_CAP
        (the cap is selected on the device) or use `as_arrays=True`, which returns a dict of NumPy arrays instead of dicts:
        deltaH, coh_drop_sum, anchor_pen_sum, query_term_sum, null_total (Q each), null_offsets (Q + 1) and the kept null
        points null_i / null_j / null_z / null_r of every query, concatenated.

        With `chains` and `lamP` (>= 0) query q also carries a chain PRIOR: it gets the receipt
        that `add_chain(chains[q], lamP, chain_weights[q]); set_query(psis[q]); receipt()` returns on a lattice without a
        chain of its own, from the basis of the shifted operator `chain_receipt_many(lamP=...)` and `bundle_many(lamP=...)`
        use (the same slot and key) and one Green's column per distinct chain node, without a U* solve per query.  `chains`
        and `chain_weights` take `bundle_many`'s forms; a chain has at most 64 distinct nodes.  The signature carries the
        argument's lamP, `chain_present` and the chain's length; `meta.ustar_res` is the per-query residual bound,
        `ustar_source` is `"chain_prior_basis"`.  `as_arrays=True` adds `chain_prior_res` (float32) and `chain_prior_iters`
        (int32); both also go to `last_receipt_prior` = {"lamP", "res", "iters"}.  `lamP=0` gives the plain call's numbers."""
        if self._has_comm:
            raise NotImplementedError("receipt_many: lattices with a communicator (sharded / multi-rank) are not supported")
        prior = rc.check_prior_args("receipt_many", chains, lamP, chain_weights, self._chain_nodes is not None)
        P = rc.check_queries(psis, self.D)
        Q = int(P.shape[0])
        lists = None
        if prior:
            lists, offsets, nodes, weights = rc.prior_chain_block(chains, chain_weights, Q, self.N)
        shifted = prior and float(lamP) > 0
        full = self._receipt_detail != "light"
        cap_val = rc.null_cap()
        ra = rc.ReceiptArrays(Q, (min(cap_val, self.N) if cap_val > 0 else self.N) if full else 0)
        prior_res, prior_iters = np.zeros(Q, dtype=np.float32), np.zeros(Q, dtype=np.int32)
        solved = False
        if Q > 0:
            psi_inf_all = float(np.max(np.abs(P)))
            if shifted:
                solved = self._ensure_shifted_basis(float(lamP), tol, max_iters, psi_inf_all)
            else:
                n0 = self.stats["query_basis_solves"]
                self._ensure_query_basis(tol, max_iters, psi_inf_all)
                solved = self.stats["query_basis_solves"] != n0
            if prior:
                self._call("osc_receipt_prior_many", nat.f32(P), Q, nat.i64(offsets), nat.i32(nodes),
                           None if weights is None else nat.f32(weights), float(lamP), float(tol), int(max_iters), int(full),
                           3.0, cap_val, *ra.pointers(), nat.f32(prior_res), nat.i32(prior_iters))
                self._qbs_stats = self._qbs_stats or (shifted and full)
                self._qbs_receipt = max(self._qbs_receipt, (2 if full else 1) if shifted else 0)
            else:
                self._call("osc_receipt_many", nat.f32(P), Q, int(full), 3.0, cap_val, *ra.pointers())
        ra.round_sums()
        payload = {"Q": Q, "receipt_detail": self._receipt_detail, "basis_solved": solved, "null_points": ra.kept}
        if prior:
            payload["lamP"] = float(lamP)
            self.last_receipt_prior = {"lamP": float(lamP), "res": prior_res, "iters": prior_iters}
        self._log("receipt_many", payload)
        if prior:
            self._warn_chain_prior(prior_res, prior_iters, tol)
        if as_arrays:
            out = {**ra.scalar_arrays(), **ra.null_arrays()}
            if prior:
                out.update(chain_prior_res=prior_res, chain_prior_iters=prior_iters)
            return out
        if Q == 0:
            return []
        # everything but psi, the energies, the null points and the ustar fields is shared by the batch
        nnz, _, _ = self.graph_stats()
        qb = self.last_shifted_basis if shifted else self.last_query_basis
        res_X, res_x = float(qb["res"]["X"]), float(qb["res"]["x"])
        adj_sig = hashlib.sha256(np.ascontiguousarray(self._edge_prefix()).tobytes()).hexdigest()
        sig_rest = {"lam": [self.lamG, self.lamC, self.lamQ, float(lamP) if prior else self.lamP],
                    "chain_present": prior or self._chain_nodes is not None,
                    "chain_len": len(self._chain_nodes) if self._chain_nodes else 0, "k": self._kneighbors,
                    "detk": self._deterministic_k, "adj": adj_sig}
        degree, gates = rc.degree_stats(nnz, self.N), rc.gate_stats(self._B)
        settle, signed = self._last_settle_fields(), self._signed_settings()
        if prior:
            signed = {**signed, "params": {**signed["params"], "lamP": float(lamP)}}
        dyn = self._last_dynamics if os.getenv("OSCILLINK_RECEIPT_DYNAMICS", "0").strip().lower() in {"1", "true", "yes"} \
            else None
        psi_inf = np.max(np.abs(P), axis=1) if self.D else np.zeros(Q)
        source = "chain_prior_basis" if prior else "query_basis"
        out = []
        for q in range(Q):
            if prior:
                sig_rest["chain_len"] = len(lists[q])
            sig = self._signature_digest({"psi": np.round(P[q], 6).tolist(), **sig_rest}, self._B)
            dH = float(ra.sums[0, q])
            res_q = float(prior_res[q]) if prior else res_X + float(psi_inf[q]) * res_x
            ustar = {"ustar_iters": int(qb["iters"]["X"]), "ustar_res": float(res_q), "ustar_converged": bool(res_q <= tol)}
            nulls, tot = ra.nulls(q)
            meta = rc.meta(ustar_cached=not solved, ustar_solves=self.stats["ustar_solves"],
                           ustar_cache_hits=self.stats["ustar_cache_hits"], ustar=ustar,
                           ustar_solve_ms=float(qb["solve_ms"]) if solved else 0.0, ustar_source=source,
                           graph_build_ms=self._graph_build_ms, last_settle_ms=settle["t_ms"], degree=degree, gates=gates,
                           state_sig=sig, receipt_detail=self._receipt_detail,
                           null_points_summary=rc.null_summary(tot, cap_val))
            rc.sign(meta, self._receipt_secret, self._signature_mode, state_sig=sig, deltaH=dH, ustar=ustar, **signed)
            rec = rc.record(version=__version__, deltaH=dH, coh_drop_sum=ra.sums[1, q], anchor_pen_sum=ra.sums[2, q],
                            query_term_sum=ra.sums[3, q], **settle, null_points=nulls, meta=meta)
            if dyn:
                meta["dynamics"] = dyn
            out.append(rec)
        return out

    def chain_receipt_many(self, psis: np.ndarray, chains, z_th: float = 2.5, *, tol: float = 1e-4, max_iters: int = 256,
                           as_arrays: bool = False, lamP: Optional[float] = None, chain_weights=None):
        """`chain_receipt(chains[q], z_th)` for each row of `psis` (Q x D), as if `set_query(psis[q])` had been called, with
        the current graph, gates, own chain (add_chain), lambdas and U held fixed and without touching the lattice's state.
        `chains` is one chain (a sequence of API row ids, shared by every query) or a sequence of Q chains, 2 to 1024 nodes
        each; repeated nodes, self-steps and revisited edges behave as in chain_receipt.  The path residuals use the
        lattice's own chain with its weights when it has one, else the unit-weight path of the argument.  U*(psi_q) comes
        from the query basis `bundle_many` / `receipt_many` use (same key, cache and tolerance contract); only the rows of
        the chain nodes and their graph and path neighbours are read.  A non-finite query row gets
        non-finite answers and changes no other query's.

        With `lamP` (>= 0) every query's chain is also its chain PRIOR: query q gets what
        `add_chain(chains[q], lamP=lamP, weights=chain_weights[q]); set_query(psis[q]); chain_receipt(chains[q], z_th)` gives
        -- lamP L_path,q in the operator, the weighted path in the path residuals -- from one basis of the shifted operator
        M + lamP I (a slot of its own beside the query basis: one more N x D array) and one Green's column per distinct chain
        node.  The lattice must carry no chain of its own and a chain has at most 64 distinct nodes.  `chain_weights` is
        None, one list shared with a shared chain, or a sequence parallel to `chains` of None or len(chain) - 1 finite
        floats.  `lamP=0` reads the query basis and solves nothing.

        Returns Q dicts with chain_receipt's keys, or with `as_arrays=True` the arrays they are assembled from, under
        `Corpus.refine_many`'s names: `chain_offsets` int64 (Q + 1, over chain edges), `chain_z_struct`, `chain_z_path`,
        `chain_r_struct`, `chain_r_path` float32 (flat), `chain_gain` float64, `chain_verdict` bool, `chain_weakest_k` int32
        (-1 when no edge's max(z) exceeds -1) and `chain_weakest_z` float32; with `lamP` also `chain_prior_res` float32 (per
        query the bound on the residual of the implied U*, the stop test's quantity) and `chain_prior_iters` int32 (the most
        iterations any of the query's Green's columns took)."""
        if self._has_comm:
            raise NotImplementedError("chain_receipt_many: lattices with a communicator (sharded / multi-rank) are not "
                                      "supported")
        prior = lamP is not None
        if not prior and chain_weights is not None:
            raise ValueError("chain_weights given without lamP")
        if prior:
            rc.check_prior_lamP("chain_receipt_many", lamP, self._chain_nodes is not None)
        P = rc.check_queries(psis, self.D, finite=False)
        Q = int(P.shape[0])
        if prior:
            lists, offsets, nodes, weights = rc.prior_chain_block(chains, chain_weights, Q, self.N)
        else:
            (lists, offsets, nodes), weights = rc.chain_block(chains, Q, self.N), None
        edge_offsets = offsets - np.arange(Q + 1, dtype=np.int64)
        n_edges = int(edge_offsets[-1])
        edge = np.zeros((4, max(n_edges, 1)), dtype=np.float32)
        gain = np.zeros(Q, dtype=np.float64)
        verdict, weak_k = np.zeros(Q, dtype=np.int32), np.zeros(Q, dtype=np.int32)
        weak_z = np.zeros(Q, dtype=np.float32)
        prior_res, prior_iters = np.zeros(Q, dtype=np.float32), np.zeros(Q, dtype=np.int32)
        solved = False
        if Q > 0:
            psi_inf = float(np.max(np.abs(P), where=np.isfinite(P), initial=0.0))
            outs = [*[nat.f32(edge[t]) for t in range(4)], gain.ctypes.data_as(C.POINTER(C.c_double)), nat.i32(verdict),
                    nat.i32(weak_k), nat.f32(weak_z)]
            if prior and float(lamP) > 0:
                solved = self._ensure_shifted_basis(float(lamP), tol, max_iters, psi_inf)
            else:
                n0 = self.stats["query_basis_solves"]
                self._ensure_query_basis(tol, max_iters, psi_inf)
                solved = self.stats["query_basis_solves"] != n0
            if prior:
                self._call("osc_chain_prior_many", nat.f32(P), Q, nat.i64(offsets), nat.i32(nodes),
                           None if weights is None else nat.f32(weights), float(lamP), float(tol), int(max_iters), float(z_th),
                           *outs, nat.f32(prior_res), nat.i32(prior_iters))
            else:
                self._call("osc_chain_receipt_many", nat.f32(P), Q, nat.i64(offsets), nat.i32(nodes), float(z_th), *outs)
        payload = {"Q": Q, "edges": n_edges, "basis_solved": solved}
        if prior:
            payload["lamP"] = float(lamP)
        self._log("chain_receipt_many", payload)
        if prior:  # (a non-finite query's bound is non-finite by design)
            self._warn_chain_prior(prior_res, prior_iters, tol, rows=np.all(np.isfinite(P), axis=1))
        arr = dict(chain_offsets=edge_offsets, chain_z_struct=edge[0, :n_edges].copy(), chain_z_path=edge[1, :n_edges].copy(),
                   chain_r_struct=edge[2, :n_edges].copy(), chain_r_path=edge[3, :n_edges].copy(), chain_gain=gain,
                   chain_verdict=verdict != 0, chain_weakest_k=weak_k, chain_weakest_z=weak_z)
        if not as_arrays:
            return rc.chain_receipt_dicts(lists, arr)
        if prior:
            arr.update(chain_prior_res=prior_res, chain_prior_iters=prior_iters)
        return arr

    def _warn_chain_prior(self, prior_res: np.ndarray, prior_iters: np.ndarray, tol: float, rows=None) -> None:
        """Log the queries (of `rows`, a boolean mask, when given) whose residual bound is not within `tol`."""
        over = ~(prior_res <= tol)
        over = np.nonzero(over if rows is None else over & rows)[0]
        if over.size:
            self._log("chain_prior_convergence_warn", {"queries": int(over.size), "first": int(over[0]),
                                                       "res": float(prior_res[over[0]]), "tol": tol,
                                                       "iters": int(prior_iters[over[0]])})

    def _ensure_shifted_basis(self, lamP: float, tol: float, max_iters: int, psi_inf: float) -> bool:
        """Solve (or extend) the basis of the shifted operator M + lamP I in its own slot unless the resident one serves
        |psi|_inf at this tolerance: `_qb_key`'s fields plus the shift.  True when a solve ran.  Touches neither the query
        basis nor `stats`."""
        self._push_params()
        key = (self._qb_version, float(self.lamG), float(self.lamC), float(self.lamQ), float(self.lamP), float(tol),
               int(max_iters), float(lamP))
        scale = max(float(psi_inf), 1e-6)
        if key == self._qbs_key and scale <= self._qbs_scale:
            return False
        fresh = key != self._qbs_key
        iters = np.zeros(2, dtype=np.int32)
        res = np.zeros(2, dtype=np.float32)
        ms = C.c_double(0.0)
        self._call("osc_query_basis_shifted", float(lamP), float(tol), int(max_iters), scale, int(fresh), nat.i32(iters),
                   nat.f32(res), C.byref(ms))
        prev = self.last_shifted_basis if not fresh else {}
        it_X = int(iters[0]) if fresh else int(prev["iters"]["X"])
        res_X = float(res[0]) if fresh else float(prev["res"]["X"])
        it_x, res_x = int(iters[1]), float(res[1])
        converged = bool(res_X <= 0.5 * tol * (1 + 1e-5) and res_x * scale <= 0.5 * tol * (1 + 1e-5))
        self.last_shifted_basis = {"lamP": float(lamP), "iters": {"X": it_X, "x": it_x}, "res": {"X": res_X, "x": res_x},
                                   "converged": converged, "solve_ms": float(ms.value), "psi_inf": scale,
                                   "x_only": not fresh}
        self._qbs_key = key
        self._qbs_scale = scale
        self.shifted_basis_solves += 1
        self._log("shifted_basis_solve", {"tol": tol, "max_iters": max_iters, **self.last_shifted_basis})
        if not converged:
            self._log("shifted_basis_convergence_warn", {"res": self.last_shifted_basis["res"], "tol": tol,
                                                         "iters": self.last_shifted_basis["iters"], "psi_inf": scale})
        return True

    def diffusion_gates_many(self, psis: np.ndarray, *, beta: float = 1.0, gamma: float = 0.1, method: str = "direct",
                             tol: float = 1e-4, max_iters: int = 256, clamp: bool = True) -> dict:
        """`compute_diffusion_gates(self.Y, psis[q], ..., lattice=self)` for each row of `psis` (Q x D) in one device call
        (DESIGN.md section 17): the operator L_sym + gamma I is the same for every query, so the Q gate solves are one CG
        with Q right-hand sides over the lattice's graph, each column stopped at its own residual.  Returns `gates`
        (Q x N float32, API row order, clipped to [0, 1] for either value of `clamp`), `iters` (Q int32) and `res` (Q
        float32), each query's own iteration count and final |r_q|.  `method="direct"` means what it means there: CG to
        1e-7 max(1, |s_q|), 2048 iterations at most.  A query's row is the same to the bit whatever else the batch
        holds.  Non-finite gates come back as computed, with one RuntimeWarning naming the first such query.  Changes no
        state of the lattice."""
        if self._has_comm:
            raise NotImplementedError("diffusion_gates_many: lattices with a communicator (sharded / multi-rank) are not "
                                      "supported")
        P = rc.check_queries(psis, self.D)
        if gamma <= 0:
            raise ValueError("gamma must be > 0 for SPD")
        if method not in ("direct", "cg"):
            raise ValueError(f"method must be 'direct' or 'cg', got {method!r}")
        Q = int(P.shape[0])
        gates = nat.result_array((Q, self.N)) if Q > 0 else np.zeros((0, self.N), dtype=np.float32)
        iters = np.zeros(Q, dtype=np.int32)
        res = np.zeros(Q, dtype=np.float32)
        self._call("osc_gates_many", nat.f32(P), Q, float(beta), float(gamma), 1 if method == "cg" else 0, float(tol),
                   int(max_iters), 1 if clamp else 0, nat.f32(gates), nat.i32(iters), nat.f32(res))
        bad = np.nonzero(~np.all(np.isfinite(gates), axis=1))[0] if Q > 0 else np.zeros(0, dtype=np.intp)
        if bad.size:
            import warnings

            q = int(bad[0])
            warnings.warn(f"diffusion_gates_many: the screened-diffusion solve of query {q} produced non-finite values "
                          f"(iters={int(iters[q])}, res={float(res[q])!r}); returned as computed, like the reference's cg "
                          "path", RuntimeWarning, stacklevel=2)
        self._log("diffusion_gates_many", {"Q": Q, "method": method, "iters_max": int(iters.max()) if Q else 0})
        return {"gates": gates, "iters": iters, "res": res}

    def query_basis(self, tol: float = 1e-4, max_iters: int = 256) -> tuple[np.ndarray, np.ndarray]:
        """The query basis (X N x D, x N) in API row order: U*(psi) = X + x psi^T (diagnostic; not in the reference).
        Solved for the current psi's |psi|_inf unless a basis of the same graph, gates, chain, lambdas and tolerance is
        resident already."""
        if self._has_comm:
            raise NotImplementedError("query_basis: lattices with a communicator (sharded / multi-rank) are not supported")
        self._ensure_query_basis(tol, max_iters, float(np.max(np.abs(self._psi))) if self._psi.size else 0.0,
                                 extend=False)
        X = np.empty((self.N, self.D), dtype=np.float32)
        x = np.empty(self.N, dtype=np.float32)
        self._call("osc_get_query_basis", nat.f32(X), nat.f32(x))
        return X, x

    def _ensure_query_basis(self, tol: float, max_iters: int, psi_inf: float, extend: bool = True) -> None:
        """Solve (or extend) the query basis unless the resident one serves |psi|_inf at this tolerance.  The key leaves
        psi out on purpose: set_query keeps the basis, every change of the operator M drops it."""
        self._push_params()
        key = (self._qb_version, float(self.lamG), float(self.lamC), float(self.lamQ), float(self.lamP), float(tol),
               int(max_iters))
        scale = max(float(psi_inf), 1e-6)
        if key == self._qb_key and (scale <= self._qb_scale or not extend):
            return
        fresh = key != self._qb_key
        iters = np.zeros(2, dtype=np.int32)
        res = np.zeros(2, dtype=np.float32)
        ms = C.c_double(0.0)
        self._call("osc_query_basis", float(tol), int(max_iters), scale, int(fresh), nat.i32(iters), nat.f32(res),
                   C.byref(ms))
        prev = self.last_query_basis if not fresh else {}
        it_X = int(iters[0]) if fresh else int(prev["iters"]["X"])
        res_X = float(res[0]) if fresh else float(prev["res"]["X"])
        it_x, res_x = int(iters[1]), float(res[1])
        converged = bool(res_X <= 0.5 * tol * (1 + 1e-5) and res_x * scale <= 0.5 * tol * (1 + 1e-5))
        self.last_query_basis = {"iters": {"X": it_X, "x": it_x}, "res": {"X": res_X, "x": res_x},
                                 "converged": converged, "solve_ms": float(ms.value), "psi_inf": scale,
                                 "x_only": not fresh}
        self._qb_key = key
        self._qb_scale = scale
        self.stats["query_basis_solves"] += 1
        self._log("query_basis_solve", {"tol": tol, "max_iters": max_iters, **self.last_query_basis})
        if not converged:
            self._log("query_basis_convergence_warn", {"res": self.last_query_basis["res"], "tol": tol,
                                                       "iters": self.last_query_basis["iters"], "psi_inf": scale})

    def _mmr_many(self, scores: np.ndarray, k: int, lambda_div: float) -> np.ndarray:
        """mmr_diversify (graph.py:114-133) for every column of `scores` (N x Q) at once on the device; (Q, min(k, N))
        API ids.  Private: the batched MMR of bundle_many, exposed for tests against `_mmr`."""
        S = np.ascontiguousarray(scores, dtype=np.float32)
        if S.ndim != 2 or S.shape[0] != self.N:
            raise ValueError(f"scores must be ({self.N}, Q)")
        Q = int(S.shape[1])
        kk = min(int(k), self.N) if k > 0 else 0
        out = np.zeros((Q, kk), dtype=np.int32)
        if Q > 0 and kk > 0:
            self._call("osc_mmr_many", nat.f32(S), Q, kk, float(lambda_div), nat.i32(out))
        return out

    # ------------------------------------------------------------------ callbacks / logging (lattice.py:571-579, 930-949)
    def add_settle_callback(self, fn) -> None:
        self._settle_callbacks.append(fn)

    def remove_settle_callback(self, fn) -> None:
        try:
            self._settle_callbacks.remove(fn)
        except ValueError:
            pass

    def set_logger(self, logger_callable) -> None:
        self._logger = logger_callable

    def _log(self, event: str, payload: dict) -> None:
        if self._logger is not None:
            try:
                self._logger(event, payload)
            except Exception:
                pass

    def set_receipt_secret(self, secret) -> None:
        if secret is None:
            self._receipt_secret = None
        else:
            self._receipt_secret = secret.encode("utf-8") if isinstance(secret, str) else secret

    def set_signature_mode(self, mode: str) -> None:
        m = mode.lower().strip()
        if m not in {"minimal", "extended"}:
            raise ValueError("mode must be 'minimal' or 'extended'")
        self._signature_mode = m

    def set_receipt_detail(self, mode: str) -> None:
        m = mode.lower().strip()
        if m not in {"full", "light"}:
            raise ValueError("mode must be 'full' or 'light'")
        self._receipt_detail = m

    # ------------------------------------------------------------------ signature / cache (lattice.py:729-758)
    def _edge_prefix(self, limit: int = 2048) -> np.ndarray:
        if self._csr is None:  # a few rows of the device graph instead of the whole CSR
            pairs = np.zeros((limit, 2), dtype=np.int64)
            n = C.c_int32(0)
            self._call("osc_edge_prefix", int(limit), nat.i64(pairs), C.byref(n))
            return pairs[: n.value]
        rowptr, col, _, _, _ = self._host_csr()
        m = min(limit, col.shape[0])
        rows = np.searchsorted(rowptr, np.arange(m), side="right") - 1
        return np.stack([rows.astype(np.int64), col[:m].astype(np.int64)], axis=1)

    def _signature(self) -> str:
        key = (self._state_version, float(self.lamG), float(self.lamC), float(self.lamQ), float(self.lamP),
               self._chain_nodes is not None, len(self._chain_nodes) if self._chain_nodes else 0, self._kneighbors,
               self._deterministic_k)
        if self._sig_cache is not None and self._sig_cache[0] == key:
            return self._sig_cache[1]
        adj_sig = hashlib.sha256(np.ascontiguousarray(self._edge_prefix()).tobytes()).hexdigest()
        data = {
            "psi": np.round(self._psi, 6).tolist(),
            "lam": [self.lamG, self.lamC, self.lamQ, self.lamP],
            "chain_present": self._chain_nodes is not None,
            "chain_len": len(self._chain_nodes) if self._chain_nodes else 0,
            "k": self._kneighbors,
            "detk": self._deterministic_k,
            "adj": adj_sig,
        }
        sig = self._signature_digest(data, self._B)
        self._sig_cache = (key, sig)
        return sig

    _ones_prefix: dict = {}  # N -> sha256 object that has absorbed '{"B": [1.0, ..., 1.0]' (N ones): see _signature_digest

    @classmethod
    def _signature_digest(cls, rest: dict, B: np.ndarray) -> str:
        """sha256 of `_signature_json(rest, B)`.  An ungated lattice's JSON starts with the same 6 N bytes of ones as every
        other ungated lattice of N nodes: the hash state behind that prefix is kept per N (a handful of sizes) and copied, so
        a service that builds one lattice per request does not hash 600 KB per receipt at N = 100k (1.1 -> 0.15 ms)."""
        n = int(B.size)
        if n and bool(np.all(B == 1.0)):
            h0 = cls._ones_prefix.get(n)
            if h0 is None:
                h0 = hashlib.sha256(('{"B": [' + ", ".join(["1.0"] * n) + "]").encode("utf-8"))
                while len(cls._ones_prefix) >= 8:
                    cls._ones_prefix.pop(next(iter(cls._ones_prefix)), None)
                cls._ones_prefix[n] = h0
            h = h0.copy()
            tail = json.dumps(rest, sort_keys=True)
            assert tail.startswith("{") and not any(k < "B" for k in rest)
            h.update((", " + tail[1:] if len(rest) else "}").encode("utf-8"))
            return h.hexdigest()
        return hashlib.sha256(cls._signature_json(rest, B).encode("utf-8")).hexdigest()

    @staticmethod
    def _signature_json(rest: dict, B: np.ndarray) -> str:
        """`json.dumps({**rest, "B": np.round(B, 6).tolist()}, sort_keys=True)` (lattice.py:729-744).  "B" sorts before
        every other key (upper case), so its N numbers are spliced in front; ungated lattices (all gates 1.0, the common
        case) skip the per-element float formatting, which is most of the cost at N = 100k."""
        if B.size and bool(np.all(B == 1.0)):
            b_json = "[" + ", ".join(["1.0"] * int(B.size)) + "]"
        else:
            b_json = json.dumps(np.round(B, 6).tolist())
        tail = json.dumps(rest, sort_keys=True)
        assert tail.startswith("{") and not any(k < "B" for k in rest)
        return '{"B": ' + b_json + (", " + tail[1:] if len(rest) else "}")

    def _invalidate_cache(self) -> None:
        self._Ustar_cache = None
        self._Ustar_sig = None
        self._log("invalidate_cache", {})

    # ------------------------------------------------------------------ rebuild (lattice.py:760-801)
    def rebuild_graph(self, *, row_cap_val: Optional[float] = None, kneighbors: Optional[int] = None,
                      deterministic_k: Optional[bool] = None, neighbor_seed: Optional[int] = None) -> None:
        # the new parameters become the object's only after the device accepted them: a failed rebuild must not leave
        # the Python side describing a graph the device does not hold (_kneighbors feeds _signature and the HMAC payload)
        cap = self._row_cap_val if row_cap_val is None else float(row_cap_val)
        k_req = self._kneighbors_requested if kneighbors is None else int(kneighbors)
        k = min(k_req, max(1, self.N - 1))
        det = self._deterministic_k if deterministic_k is None else bool(deterministic_k)
        seed = self._neighbor_seed if neighbor_seed is None else neighbor_seed
        t0 = time.time()
        self._call("osc_rebuild_graph", int(k_req), float(cap), int(det), -1 if seed is None else int(seed))
        self._row_cap_val, self._kneighbors, self._deterministic_k, self._neighbor_seed = cap, k, det, seed
        self._kneighbors_requested = k_req
        self._graph_build_ms = 1000.0 * (time.time() - t0)
        self._csr = None
        self._touch()
        self._qb_version += 1
        self._invalidate_cache()
        self._log("rebuild_graph", {"k": int(self._kneighbors), "row_cap_val": float(self._row_cap_val),
                                    "deterministic_k": self._deterministic_k, "neighbor_seed": self._neighbor_seed})

    # ------------------------------------------------------------------ append (not in the reference)
    _APPEND_MODES = {"auto": 0, "incremental": 1, "rebuild": 2}

    def _mode_code(self, mode: str) -> int:
        if mode not in self._APPEND_MODES:
            raise ValueError("mode must be 'auto', 'incremental' or 'rebuild'")
        return self._APPEND_MODES[mode]

    def _become(self, op: str, cannot: str, create, rows: int, N_new: int, B_new: np.ndarray, chain_nodes,
                state_map: Optional[np.ndarray] = None) -> None:
        """What append, remove and update share once their arguments are checked: `create(new_h)` calls the operation's
        osc_create_* on this lattice's handle; lambdas, psi, the gates `B_new` and the chain (on `chain_nodes`) are carried
        to the new handle, and with `state_map` (keep_state=True: one of the `_state_map_*`) the state U, device to device;
        the new handle then replaces this object's.  A failure leaves the lattice exactly as it was."""
        if getattr(self, "_has_comm", False):
            raise nat.NativeError(f"{op}: a lattice with a communicator cannot {cannot} (multi-rank handles are out of scope)")
        new_h = nat.Handle()
        t0 = time.time()
        create(new_h)
        self._carry_settings_to(new_h, B_new, chain_nodes)
        if state_map is not None:
            self._carry_state_to(new_h, state_map, N_new)
        if chain_nodes is not None:
            self._chain_nodes = [int(c) for c in chain_nodes]
        self._swap_handle(new_h, N_new, B_new, t0)
        info = getattr(self, op + "_info")()
        payload = {"rows": rows, "N": self.N, "route": info["route"], "redo_rows": info["redo_rows"]}
        if state_map is not None:
            payload["keep_state"] = True
        self._log(op, payload)

    def _seeded_info(self, fn: str, keys: str) -> dict[str, Any]:
        """One of osc_append_info / osc_remove_info / osc_update_info: `keys` names its outputs in order (route,
        score_family and denied are int32, the *_ms doubles, the counts int64)."""
        slots = [(key, C.c_double(0.0) if key.endswith("_ms") else
                  C.c_int32(0) if key in ("route", "score_family", "denied") else C.c_int64(0)) for key in keys.split()]
        self._call(fn, *[C.byref(v) for _, v in slots])
        info: dict[str, Any] = {key: float(v.value) if key.endswith("_ms") else int(v.value) for key, v in slots}
        info["score_family"] = ("none", "mfma", "butterfly")[info["score_family"]]
        return info

    def append(self, Ynew: np.ndarray, gates: Optional[np.ndarray] = None, *, mode: str = "auto",
               keep_state: bool = False) -> np.ndarray:
        """Add the rows of `Ynew` (M x D) behind the lattice's own and return their ids N .. N + M - 1.

        The lattice afterwards is the one `OscillinkLattice(np.concatenate([Y, Ynew]), ...)` would be with this lattice's
        settings applied: same graph, U = Y (the state is NOT carried over an append unless `keep_state=True`: then every
        old row keeps its row of U bit for bit, moved on the device, and only the new rows start at their anchors), lambdas,
        psi, chain and lamP kept, gates = the old gates followed by `gates` (ones when None).  Logger, callbacks, receipt
        secret, signature and detail modes stay.  mode "incremental" grows the kNN lists from the kept ones and raises where that is not possible,
        "rebuild" builds the concatenated anchors from scratch on the device, "auto" lets the planner choose
        (`append_info()` says which).  Only `Ynew` crosses the bus.  A failure leaves the lattice exactly as it was."""
        code = self._mode_code(mode)
        if not isinstance(Ynew, np.ndarray) or Ynew.ndim != 2:
            raise ValueError("Ynew must be a 2D numpy array")
        if Ynew.shape[1] != self.D:
            raise ValueError("Ynew column count mismatch D")
        M = int(Ynew.shape[0])
        g_new = None
        if gates is not None:
            g_new = np.ascontiguousarray(gates, dtype=np.float32).ravel()
            if g_new.shape[0] != M:
                raise ValueError("gates length mismatch M")
        if M == 0:
            return np.empty(0, dtype=np.int64)
        def create(new_h) -> None:
            Yc = np.ascontiguousarray(Ynew, dtype=np.float32)
            nat.check(nat.lib().osc_create_appended(self._h, nat.f32(Yc), M, code, C.byref(new_h)), None, "osc_create_appended")

        ids = np.arange(self.N, self.N + M, dtype=np.int64)
        B_new = np.concatenate([self._B, np.ones(M, dtype=np.float32) if g_new is None else g_new]).astype(np.float32)
        self._become("append", "grow", create, M, self.N + M, B_new, self._chain_nodes,
                     _state_map_append(self.N, M) if keep_state else None)
        return ids

    def _carry_settings_to(self, new_h, B_new: np.ndarray, chain_nodes) -> None:
        """Lambdas, psi, gates and the chain onto a handle that is to replace this object's, before anything of this object
        changes; a failure destroys the new handle and leaves the object as it was."""
        L = nat.lib()
        try:
            nat.check(L.osc_set_lams(new_h, float(self.lamG), float(self.lamC), float(self.lamQ)), new_h, "osc_set_lams")
            nat.check(L.osc_set_query(new_h, nat.f32(self._psi), nat.f32(B_new)), new_h, "osc_set_query")
            if chain_nodes is not None:
                ch = np.asarray(chain_nodes, dtype=np.int32)
                ws = None if self._chain_weights is None else np.asarray(self._chain_weights, dtype=np.float32)
                nat.check(L.osc_set_chain(new_h, nat.i32(ch), None if ws is None else nat.f32(ws), int(ch.size),
                                          float(self.lamP)), new_h, "osc_set_chain")
        except Exception:
            L.osc_destroy(new_h)
            raise

    def _carry_state_to(self, new_h, state_map: np.ndarray, N_new: int) -> None:
        """This lattice's U onto a handle that is to replace this object's (osc_carry_state), row `a` of the new handle from
        row `state_map[a]`, its own anchor where that is -1; a failure destroys the new handle and leaves the object as it
        was."""
        L = nat.lib()
        try:
            m = np.ascontiguousarray(state_map, dtype=np.int32)
            if m.shape != (N_new,):
                raise ValueError("state map length mismatch the rows of the new lattice")
            nat.check(L.osc_carry_state(new_h, self._h, nat.i32(m)), new_h, "osc_carry_state")
        except Exception:
            L.osc_destroy(new_h)
            raise

    def _swap_handle(self, new_h, N_new: int, B_new: np.ndarray, t0: float) -> None:
        """The object becomes the lattice of `new_h` (U as the handle holds it: its anchors unless a state was carried onto
        it; nothing cached); the old handle is destroyed."""
        old_h, self._h = self._h, new_h
        nat.lib().osc_destroy(old_h)
        self.N = N_new
        self._B = B_new
        self._kneighbors = min(self._kneighbors_requested, max(1, self.N - 1))
        self._lamP_dev = float(self.lamP)
        self._graph_build_ms = 1000.0 * (time.time() - t0)
        self._Y_host = None
        self._U_host = None
        self._csr = None
        self._device_ustar_sig = None
        self.last = {"iters": 0, "res": None, "t_ms": None}
        self._last_dynamics = None
        self._touch()
        self._qb_version += 1
        self._qb_key = None
        self._qbs_key = None
        self._qbs_receipt = 0
        self._invalidate_cache()

    def append_info(self) -> dict[str, Any]:
        """How the handle came to be (osc_append_info): route 0 = not by `append`, 1 = incremental, 2 = rebuild; the score
        family of its kNN lists ("mfma" / "butterfly"); the incremental route's phases in ms."""
        return self._seeded_info("osc_append_info", "route new_rows merged_rows redo_rows score_family score_ms merge_ms "
                                 "back_half_ms merge_hits merge_scan_bytes denied")

    # ------------------------------------------------------------------ remove (not in the reference)
    def remove(self, ids, *, mode: str = "auto", keep_state: bool = False) -> np.ndarray:
        """Drop the rows `ids` names (any integer array-like, any order, duplicates allowed) and return `new_id_of_old`: one
        int64 entry per old row, its id afterwards, -1 for a removed row.  Kept rows are renumbered densely, in order.

        The lattice afterwards is the one `OscillinkLattice(np.delete(Y, ids, axis=0), ...)` would be with this lattice's
        settings applied: same graph, U = Y (the state is NOT carried over a removal unless `keep_state=True`: then every
        kept row keeps its row of U bit for bit, moved on the device), lambdas, psi and lamP kept, gates =
        `np.delete(B, ids)`, a chain carried with its nodes renumbered (`ids` naming a chain node raises: `clear_chain()`
        first).  Logger, callbacks, receipt secret, signature and detail modes stay.  mode "incremental" shrinks the kNN
        lists from the kept ones and raises where that is not possible, "rebuild" builds the kept anchors from scratch on the
        device, "auto" lets the planner choose (`remove_info()` says which).  No anchor crosses the bus.  A failure leaves
        the lattice exactly as it was."""
        code = self._mode_code(mode)
        arr = np.asarray(ids)
        if arr.size == 0:
            arr = arr.astype(np.int64)
        if not np.issubdtype(arr.dtype, np.integer):
            raise ValueError("ids must be integers")
        arr = arr.ravel()
        if arr.size and (int(arr.min()) < 0 or int(arr.max()) >= self.N):
            raise ValueError("ids out of bounds")
        keep = np.ones(self.N, dtype=bool)
        keep[arr.astype(np.int64)] = False
        M = self.N - int(keep.sum())
        new_id_of_old = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int64)
        if M == 0:
            return new_id_of_old
        if M == self.N:
            raise ValueError("ids name every row: a lattice keeps at least one")
        chain_new = None
        if self._chain_nodes is not None:
            chain_new = new_id_of_old[np.asarray(self._chain_nodes, dtype=np.int64)]
            if (chain_new < 0).any():
                raise ValueError("ids name a node of the chain: clear_chain() first (dropping a node from a weighted path has "
                                 "no single meaning)")
        def create(new_h) -> None:
            gone = np.ascontiguousarray(np.nonzero(~keep)[0], dtype=np.int32)
            nat.check(nat.lib().osc_create_removed(self._h, nat.i32(gone), int(gone.size), code, C.byref(new_h)), None,
                      "osc_create_removed")

        B_new = np.ascontiguousarray(self._B[keep], dtype=np.float32)
        self._become("remove", "shrink", create, M, self.N - M, B_new, chain_new,
                     _state_map_remove(keep) if keep_state else None)
        return new_id_of_old

    def remove_info(self) -> dict[str, Any]:
        """How the handle came to be (osc_remove_info): route 0 = not by `remove`, 1 = incremental, 2 = rebuild; the rows
        removed, kept with their lists and recomputed; the score family of its kNN lists; the incremental route's phases in
        ms; why the planner did not take the incremental route (0: it did, or was not asked).  It describes the creation of
        the handle, as `append_info()` does: a later `append` starts a new handle (route 0 here), while a later
        `rebuild_graph` keeps the handle and with it this record, although the graph is then the rebuild's."""
        return self._seeded_info("osc_remove_info", "route removed_rows kept_rows redo_rows score_family score_ms back_half_ms "
                                 "denied")

    # ------------------------------------------------------------------ update (not in the reference)
    def update(self, ids, Ynew: np.ndarray, gates: Optional[np.ndarray] = None, *, mode: str = "auto",
               keep_state: bool = False) -> np.ndarray:
        """Row `ids[j]` becomes `Ynew[j]` (ids: distinct integers in [0, N), any order; Ynew: M x D) and `ids` comes back as
        int64.  No row moves: N, the row pitch, the effective k and every id stay.

        The lattice afterwards is the one `OscillinkLattice(Y2, ...)` would be, `Y2 = Y.copy(); Y2[ids] = Ynew`, with this
        lattice's settings applied: same graph, U = Y2 (the state is NOT carried over an update unless `keep_state=True`:
        then every row that is not replaced keeps its row of U bit for bit, moved on the device, and a replaced row starts at
        its new anchor, since its old state describes another vector), lambdas, psi, chain and lamP kept
        (a replaced row may be a chain node: the path prior depends on node identity only), gates unchanged except
        `B[ids] = gates` where `gates` (length M) is given.  Logger, callbacks, receipt secret, signature and detail modes
        stay.  mode "incremental" keeps the kNN lists that name no replaced row and raises where that is not possible,
        "rebuild" builds the changed anchors from scratch on the device, "auto" lets the planner choose (`update_info()`
        says which).  Only `ids` and `Ynew` cross the bus.  A failure leaves the lattice exactly as it was."""
        code = self._mode_code(mode)
        arr = np.asarray(ids)
        if arr.size == 0:
            arr = arr.astype(np.int64)
        if not np.issubdtype(arr.dtype, np.integer):
            raise ValueError("ids must be integers")
        arr = arr.ravel().astype(np.int64)
        if not isinstance(Ynew, np.ndarray) or Ynew.ndim != 2:
            raise ValueError("Ynew must be a 2D numpy array")
        if Ynew.shape[1] != self.D:
            raise ValueError("Ynew column count mismatch D")
        M = int(Ynew.shape[0])
        if arr.size != M:
            raise ValueError("ids length mismatch the rows of Ynew")
        if M and (int(arr.min()) < 0 or int(arr.max()) >= self.N):
            raise ValueError("ids out of bounds")
        if np.unique(arr).size != M:
            raise ValueError("ids name a row twice: there is no single meaning for which new row wins")
        g_new = None
        if gates is not None:
            g_new = np.ascontiguousarray(gates, dtype=np.float32).ravel()
            if g_new.shape[0] != M:
                raise ValueError("gates length mismatch M")
        if M == 0:
            return arr
        def create(new_h) -> None:
            Yc = np.ascontiguousarray(Ynew, dtype=np.float32)
            i32 = np.ascontiguousarray(arr, dtype=np.int32)
            nat.check(nat.lib().osc_create_updated(self._h, nat.i32(i32), nat.f32(Yc), M, code, C.byref(new_h)), None,
                      "osc_create_updated")

        B_new = np.array(self._B, dtype=np.float32)
        if g_new is not None:
            B_new[arr] = g_new
        self._become("update", "change rows", create, M, self.N, B_new, self._chain_nodes,
                     _state_map_update(self.N, arr) if keep_state else None)
        return arr

    def update_info(self) -> dict[str, Any]:
        """How the handle came to be (osc_update_info): route 0 = not by `update`, 1 = incremental, 2 = rebuild; the rows
        replaced, the rows that kept their lists and scanned the replaced columns, the other rows recomputed; the score
        family of its kNN lists; the incremental route's phases in ms; the list entries the merge took; why the planner did
        not take the incremental route (0: it did, or was not asked).  It describes the creation of the handle, as
        `append_info()` and `remove_info()` do."""
        return self._seeded_info("osc_update_info", "route replaced_rows merged_rows redo_rows score_family score_ms merge_ms "
                                 "back_half_ms merge_hits denied")

    # ------------------------------------------------------------------ persistence (lattice.py:582-726)
    def _provenance(self) -> str:
        h = hashlib.sha256()
        h.update(self.Y.tobytes())
        h.update(self._psi.tobytes())
        h.update(self._B.tobytes())
        h.update(np.array([self.lamG, self.lamC, self.lamQ, self.lamP], dtype=np.float64).tobytes())
        h.update(np.ascontiguousarray(self._edge_prefix()).tobytes())
        return h.hexdigest()

    def export_state(self, include_graph: bool = True, include_chain: bool = True) -> dict[str, Any]:
        state: dict[str, Any] = {
            "version": str(__version__),
            "shape": [int(self.N), int(self.D)],
            "params": {"lamG": self.lamG, "lamC": self.lamC, "lamQ": self.lamQ, "lamP": self.lamP},
            "Y": self.Y.tolist(),
            "psi": self._psi.tolist(),
            "B_diag": self._B.tolist(),
            "kneighbors": int(self._kneighbors),
            "deterministic_k": bool(self._deterministic_k),
            "neighbor_seed": self._neighbor_seed,
            "provenance": self._provenance(),
        }
        if include_graph:
            # the reference stores the dense N x N adjacency; that stays readable up to the dense-view limit, and the
            # sparse triplet is always written (and preferred by from_state) so large lattices persist too
            rowptr, col, a, _, _ = self._host_csr()
            state["A_csr"] = {"indptr": rowptr.tolist(), "indices": col.tolist(), "data": a.tolist()}
            if self.N <= _DENSE_EXPORT_LIMIT:
                state["A"] = self.A.tolist()
        if include_chain and self._chain_nodes is not None:
            pairs = set()
            for t in range(len(self._chain_nodes) - 1):
                i, j = self._chain_nodes[t], self._chain_nodes[t + 1]
                if i != j:
                    pairs.add((min(i, j), max(i, j)))
            state["chain_edges"] = [[int(i), int(j)] for i, j in sorted(pairs)]
            state["chain_nodes"] = list(self._chain_nodes)
        return state

    def save_state(self, path: str, format: str = "json", include_graph: bool = True, include_chain: bool = True) -> None:
        fmt = format.lower()
        if fmt == "json":
            with open(path, "w", encoding="utf-8") as f:
                json.dump(self.export_state(include_graph=include_graph, include_chain=include_chain), f, sort_keys=True)
        elif fmt == "npz":
            state = self.export_state(include_graph=False, include_chain=include_chain)
            arrays: dict[str, np.ndarray] = {"Y": self.Y, "psi": self._psi, "B_diag": self._B}
            if include_graph:
                rowptr, col, a, _, _ = self._host_csr()
                arrays.update(A_indptr=rowptr, A_indices=col, A_data=a)
                if self.N <= _DENSE_EXPORT_LIMIT:
                    arrays["A"] = self.A
            if include_chain and self._chain_nodes is not None:
                arrays["chain_nodes"] = np.array(self._chain_nodes, dtype=np.int32)
            for key in ["Y", "psi", "B_diag", "A", "A_csr", "chain_nodes"]:
                state.pop(key, None)
            np.savez_compressed(path, __meta__=np.array(json.dumps(state, sort_keys=True)), **arrays)
        else:
            raise ValueError("format must be 'json' or 'npz'")

    @classmethod
    def from_npz(cls, path: str) -> "OscillinkLattice":
        with np.load(path, allow_pickle=False) as data:
            state = json.loads(str(data["__meta__"]))
            state["Y"] = data["Y"].astype(np.float32)
            state["psi"] = data["psi"].astype(np.float32)
            state["B_diag"] = data["B_diag"].astype(np.float32)
            if "A_indptr" in data.files:
                state["A_csr"] = {"indptr": data["A_indptr"], "indices": data["A_indices"], "data": data["A_data"]}
            elif "A" in data.files:
                state["A"] = data["A"].astype(np.float32)
            if "chain_nodes" in data.files:
                state["chain_nodes"] = data["chain_nodes"].astype(int).tolist()
        return cls.from_state(state)

    @classmethod
    def from_state(cls, state: dict[str, Any]) -> "OscillinkLattice":
        Y = np.array(state["Y"], dtype=np.float32)
        params = state.get("params", {})
        have_csr = "A_csr" in state
        have_A = have_csr or ("A" in state and np.asarray(state["A"]).shape == (Y.shape[0], Y.shape[0]))
        lat = cls(Y, kneighbors=state.get("kneighbors", 6), lamG=params.get("lamG", 1.0), lamC=params.get("lamC", 0.5),
                  lamQ=params.get("lamQ", 4.0), deterministic_k=state.get("deterministic_k", False),
                  neighbor_seed=state.get("neighbor_seed"), _build_graph=not have_A)
        psi = np.array(state.get("psi", np.zeros(Y.shape[1], dtype=np.float32)), dtype=np.float32)
        B = np.array(state.get("B_diag", np.ones(Y.shape[0], dtype=np.float32)), dtype=np.float32)
        if have_csr:  # sparse triplet written by this package
            g = state["A_csr"]
            lat.set_graph_csr(np.asarray(g["indptr"], dtype=np.int64), np.asarray(g["indices"], dtype=np.int32),
                              np.asarray(g["data"], dtype=np.float32))
        elif have_A:  # the reference's dense adjacency overrides a rebuild (lattice.py:709-713)
            lat.A = np.array(state["A"], dtype=np.float32)
        lat.set_query(psi, gates=B)
        lamP = params.get("lamP", 0.0)
        if lamP > 0:
            if "chain_nodes" in state:
                lat.add_chain(list(map(int, state["chain_nodes"])), lamP=lamP)
            elif state.get("chain_edges"):
                lat.add_chain(sorted({i for e in state["chain_edges"] for i in e}), lamP=lamP)
        if "provenance" in state:
            lat._imported_provenance = state["provenance"]
        return lat

    # ------------------------------------------------------------------ dynamics (lattice.py:825-927), env-gated
    def _compute_dynamics(self, U_prev: Optional[np.ndarray], U_next: Optional[np.ndarray], iters: int) -> dict[str, Any]:
        """Single-step dynamics snapshot (lattice.py:825-927) computed on the device: step energy through the operator
        kernel, per-node movement and per-edge structural energy flows through the receipt-rows kernel, the coherence
        radius by a level-synchronous BFS over the device graph.  `None` for U_prev / U_next means the device-side
        snapshot taken before the settle / the resident U (what settle() uses: no N x D transfer)."""
        TOP_K = 16
        m2, mx, dH, ft = C.c_double(0.0), C.c_float(0.0), C.c_double(0.0), C.c_double(0.0)
        ti = np.zeros(TOP_K, dtype=np.int32)
        tj = np.zeros(TOP_K, dtype=np.int32)
        tf = np.zeros(TOP_K, dtype=np.float64)
        tn, rad = C.c_int32(0), C.c_int32(0)
        up = None if U_prev is None else np.ascontiguousarray(U_prev, dtype=np.float32)
        un = None if U_next is None else np.ascontiguousarray(U_next, dtype=np.float32)
        self._call("osc_dynamics", None if up is None else nat.f32(up), None if un is None else nat.f32(un),
                   C.byref(m2), C.byref(mx), C.byref(dH), C.byref(ft), TOP_K, nat.i32(ti), nat.i32(tj),
                   tf.ctypes.data_as(nat.c_f64p), C.byref(tn), C.byref(rad))
        dH_step = float(np.float32(dH.value))
        flows = [{"edge": [int(ti[t]), int(tj[t])], "flow": float(tf[t])} for t in range(int(tn.value))]
        temperature = float(np.float32(m2.value))
        return {"temperature": temperature, "step_deltaH": dH_step,
                "viscosity_step": float(iters) / (abs(dH_step) + 1e-12), "flow_total": float(ft.value),
                "top_flows": flows, "radius": int(rad.value),
                "move2_mean": temperature, "move2_max": float(mx.value)}

    def __repr__(self) -> str:  # pragma: no cover
        parts = [f"N={self.N}", f"D={self.D}", f"k={self._kneighbors}", f"lamG={self.lamG}", f"lamC={self.lamC}",
                 f"lamQ={self.lamQ}"]
        if self.lamP > 0 and self._chain_nodes is not None:
            parts += [f"chain_len={len(self._chain_nodes)}", f"lamP={self.lamP}"]
        if self._Ustar_sig is not None:
            parts.append("U*cached")
        return "OscillinkLattice(" + ", ".join(parts) + ")"


def json_line_logger(stream=None):
    """Logger callable writing compact JSON lines (reference lattice.py:995-1014)."""
    import sys

    stream = stream or sys.stderr

    def _emit(ev: str, payload: dict):  # pragma: no cover
        try:
            stream.write(json.dumps({"event": ev, **payload}, separators=(",", ":")) + "\n")
        except Exception:
            pass

    return _emit

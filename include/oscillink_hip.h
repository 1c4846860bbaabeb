/* oscillink_hip.h -- C ABI of liboscillink_hip.so: the MI355X (gfx950) implementation of the
 * Oscillink lattice "settle" hot path.
 *
 * The reference (Maverick0351a/Oscillink v0.1.13) is pure Python + NumPy and has NO native/FFI
 * boundary: its boundary is the Python class `OscillinkLattice` (oscillink/core/lattice.py) calling
 * the NumPy functions in oscillink/core/{graph,solver,receipts}.py.  Every entry point below
 * replaces one of those Python seams 1:1 (file:line cited per function; paths are relative to the
 * reference checkout).  The Python mirror of the class that binds these symbols with ctypes is
 * `oscillink_amd/lattice.py`; INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Conventions
 *   - plain C types only; all host arrays are row-major, contiguous, caller-owned; fp32 / int32 / int64.
 *   - every call returns 0 on success or a negative OSC_E_* code; osc_last_error() gives the text.
 *   - a handle owns one HIP stream and all its device memory; handles are independent and a handle
 *     must not be used from two threads at once (the reference's cloud runs one lattice per request
 *     thread: cloud/app/main.py:1030-1061).  No process-global mutable state except the last-error
 *     string of failed osc_create calls (thread-local).
 *   - there is NO CPU fallback: without a usable gfx950 device osc_create fails with OSC_E_NODEVICE.
 */
#ifndef OSCILLINK_HIP_H
#define OSCILLINK_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct osc_lattice* osc_handle;

enum {
  OSC_OK = 0,
  OSC_E_INVALID = -1,     /* bad argument (the Python layer maps this to ValueError)            */
  OSC_E_NODEVICE = -2,    /* no HIP device / wrong architecture                                  */
  OSC_E_HIP = -3,         /* a HIP runtime call failed                                           */
  OSC_E_STATE = -4,       /* call order problem (e.g. deltaH before any U* solve)                */
  OSC_E_UNSUPPORTED = -5, /* valid request this build cannot serve (e.g. kneighbors > 128)       */
  OSC_E_COMM = -6         /* RCCL failure                                                        */
};

/* precond argument of osc_settle (lattice.py:164,186): "jacobi" -> 1, anything else -> 0 */
enum { OSC_PRECOND_NONE = 0, OSC_PRECOND_JACOBI = 1 };

/* ---- library / device ---------------------------------------------------------------------- */
const char* osc_version(void);
int osc_device_count(int32_t* n);                       /* never initialises a device context     */
int osc_device_name(int32_t device, char* out, int32_t cap);
int osc_device_synchronize(int32_t device);
const char* osc_last_error(osc_handle h);               /* h may be NULL: error of the last failed osc_create on this thread */

/* Pinned host memory for result arrays (what the reference allocates with NumPy for `U`, `Y`, `U*`: lattice.py:54-56,
 * 206, 262-271): a read-back (osc_get_U / osc_get_Y / osc_get_ustar / osc_solve_ustar) into such an array is one DMA at
 * PCIe rate; into ordinary pageable memory it goes through two pinned staging buffers and a threaded host copy.  Freed
 * blocks are parked and reused (pinning is slow).  Needs a HIP runtime, no device context of its own. */
int osc_host_alloc(int64_t bytes, void** out);
int osc_host_free(void* p);

/* ---- construction: OscillinkLattice.__init__ (lattice.py:33-110) ---------------------------- */
/* Copies Y (N x D) to the device, sets U = Y, B = 1, psi = 0, lams = (1.0, 0.5, 4.0).
 * build_graph != 0: builds the mutual-kNN graph on the device -- graph.py:8-66 (mutual_knn_adj),
 * :69-83 (row_sum_cap), :86-93 (normalized_laplacian).  k is clamped to [1, N-1] (lattice.py:60).
 * deterministic != 0 -> ties ordered (similarity desc, index asc) (graph.py:46-49); the
 * non-deterministic reference path leaves ties unspecified (graph.py:59) and this build uses the
 * same total order for it.  seed < 0 means None.  seed >= 0 (`neighbor_seed`): the reference adds a float64
 * uniform(-1e-8, 1e-8) jitter drawn from default_rng(seed) to all N^2 similarities before its argpartition
 * (graph.py:54-58).  fp32 similarities below 0.125 are spaced 7.5e-9 apart (3.7e-9 below 0.0625), so that jitter can
 * reorder exact ties AND candidates within 1-2 ulp of each other at the k-th place; reproducing it bit for bit would
 * need the same N^2 random stream.  This build treats the seed as a tie-break only: the neighbour lists are those of
 * the total order above, i.e. they can differ from the reference's seeded lists only where two candidates for the
 * last list place are 1-2 ulp apart (tests/golden/case_seed_*.npz: identical edge sets on Gaussian anchors).
 * build_graph == 0: no graph yet; call osc_set_csr (from_state / parity tests).
 * Y is read until the call returns and not afterwards.  With build_graph != 0 the anchors of a large lattice (>= 64 MB,
 * unpadded rows; beyond 768 columns from ~130 000 rows) travel to the device in pieces WHILE the build runs on the pieces
 * that have arrived (a copy
 * stream, a second build stream and a few host threads for the duration of the call; OSC_CREATE_STREAM=0: one transfer,
 * then the build): same lattice bit for bit, create 20.8 -> 16.5 ms at N = 100 000, D = 768, k = 32. */
int osc_create(const float* Y, int64_t N, int32_t D, int32_t k, float row_cap, int32_t deterministic,
               int64_t seed, int32_t device, int32_t build_graph, osc_handle* out);
int osc_destroy(osc_handle h);

/* A NEW handle over the rows of `base` (API order) followed by the M rows of Ynew (M x D, host), with base's creation
 * parameters (k as requested, row_cap, deterministic, seed, device) and lambdas; gates, psi, chain and U are those of a
 * newly created handle (U = Y).  base is only read -- its anchors travel device to device, gathered back from its internal
 * row order -- and is left as it was whatever happens; the caller destroys it.  Not in the reference.
 *   mode 0: the planner decides (oscillink_amd/csrc/append_plan.hpp);
 *   mode 1: incremental -- the top-k lists are grown from base's kept lists: the new rows, and the old rows whose lists
 *           cannot be merged (a member clipped at 0, a non-finite row: the redo set), are scored against all N + M columns
 *           in the arithmetic base's list values come from (the score family), every other old row takes the new columns
 *           that beat its worst member, then the graph is assembled from the lists as in any build.  The lists are those of
 *           a build of the N + M anchors in the same score family.  OSC_E_UNSUPPORTED with the reason in
 *           osc_last_error(NULL) when base cannot seed it: no kept lists (osc_set_csr graph), a communicator, an effective
 *           k that changes with the row count, k > 128, N + M >= 2^31, butterfly-scored lists wider than 1536 columns or
 *           mixed with MFMA-scored fallback rows;
 *   mode 2: a plain build of the N + M anchors.
 * Seam: osc_graph.hip build_graph_once takes its seeded branch iff the handle under construction carries a seed; an
 * ordinary osc_create / osc_rebuild_graph never does. */
int osc_create_appended(osc_handle base, const float* Ynew, int64_t M, int32_t mode, osc_handle* out);
/* How a handle came to be: route 0 = not by osc_create_appended, 1 = incremental, 2 = rebuild; new_rows = M; merged_rows = old
 * rows whose lists were merged in place; redo_rows = old rows recomputed; family = score family of the kept lists (1 = fp32
 * MFMA tiles, 2 = fma chains + wave butterfly; valid for every built handle); the incremental route's wall times in ms
 * (scores + selection / merge scan / graph assembly); merge_hits = list members replaced; scan_bytes = bytes of score
 * block the merge scan has to read (its floor); denied = why the planner did not take the incremental route (0 = it did,
 * or mode 2; AppendDenied in append_plan.hpp).  Any pointer may be NULL. */
int osc_append_info(osc_handle h, int32_t* route, int64_t* new_rows, int64_t* merged_rows, int64_t* redo_rows, int32_t* family,
                    double* score_ms, double* merge_ms, double* back_ms, int64_t* merge_hits, int64_t* scan_bytes,
                    int32_t* denied);

/* A NEW handle over the rows of `base` that `ids` (n entries, any order, duplicates allowed, each in [0, N)) does not name,
 * in order and renumbered densely, with base's creation parameters (k as requested, row_cap, deterministic, seed, device)
 * and lambdas; gates, psi, chain and U are those of a newly created handle (U = Y).  It replaces the reference's only way to
 * drop an anchor, a new OscillinkLattice.__init__ (lattice.py:33-110) over the reduced anchors.  base is only read -- the
 * kept anchors travel device to device, gathered from its internal row order, no anchor crosses the bus -- and is left as
 * it was whatever happens; the caller destroys it.  OSC_E_INVALID for an id out of range or ids that name every row.  Not in
 * the reference.
 *   mode 0: the planner decides (oscillink_amd/csrc/remove_plan.hpp);
 *   mode 1: incremental -- a kept row whose list names no removed row keeps its list with the ids renumbered; the rows that
 *           lost a member (and those with a member clipped at 0 or a non-finite row: the redo set) are scored against all
 *           N - M columns in the arithmetic base's list values come from (the score family); then the graph is assembled
 *           from the lists as in any build.  The lists are those of a build of the kept anchors in the same score family.
 *           OSC_E_UNSUPPORTED with the reason in osc_last_error(NULL) when base cannot seed it: no kept lists (osc_set_csr
 *           graph, never built), a communicator, fewer than two rows left, an effective k that changes with the row count,
 *           k > 128, butterfly-scored lists wider than 1536 columns or mixed with MFMA-scored fallback rows;
 *   mode 2: a plain build of the kept anchors.
 * A base with an injected graph (osc_set_csr) is refused in every mode.  Seam: osc_graph.hip build_graph_once takes its
 * removed branch iff the handle under construction carries the seed; an ordinary osc_create / osc_rebuild_graph never
 * does. */
int osc_create_removed(osc_handle base, const int32_t* ids, int64_t n, int32_t mode, osc_handle* out);
/* How a handle came to be: route 0 = not by osc_create_removed, 1 = incremental, 2 = rebuild; removed_rows = M (distinct
 * ids); kept_rows = rows whose lists were kept (renumbered); redo_rows = rows recomputed; family as in osc_append_info; the
 * incremental route's times in ms (scores + selection on the device / graph assembly); denied = why the planner did not
 * take the incremental route (0 = it did, or mode 2; AppendDenied in append_plan.hpp, and 9 = fewer than two rows left).
 * Any pointer may be NULL. */
int osc_remove_info(osc_handle h, int32_t* route, int64_t* removed_rows, int64_t* kept_rows, int64_t* redo_rows, int32_t* family,
                    double* score_ms, double* back_ms, int32_t* denied);

/* A NEW handle over the rows of `base` with row ids[j] replaced by row j of Ynew (M x D, row-major; ids distinct, any order,
 * each in [0, N)), with base's creation parameters (k as requested, row_cap, deterministic, seed, device) and lambdas;
 * gates, psi, chain and U are those of a newly created handle (U = Y).  N, the row pitch and the effective k are base's.
 * It replaces the reference's only way to change an anchor, a new OscillinkLattice.__init__ (lattice.py:33-110) over the
 * changed anchors.  base is only read -- its anchors travel device to device, gathered from its internal row order; only
 * ids and Ynew cross the bus -- and is left as it was whatever happens; the caller destroys it.  OSC_E_INVALID for an id
 * out of range or named twice.  Not in the reference.
 *   mode 0: the planner decides (oscillink_amd/csrc/update_plan.hpp);
 *   mode 1: incremental -- a row whose list names no replaced row keeps its list; the rows that lost a member (and those
 *           with a member clipped at 0 or a non-finite row: the redo set) and the replaced rows are scored against all N
 *           columns in the arithmetic base's list values come from (the score family); every other row takes a replaced
 *           column into its list iff its new score precedes the list's worst member under (score desc, index asc) -- an
 *           equal score wins where the replaced row's id is the lower one; then the graph is assembled from the lists as
 *           in any build.  The lists are those of a build of the changed anchors in the same score family.
 *           OSC_E_UNSUPPORTED with the reason in osc_last_error(NULL) when base cannot seed it: no kept lists (osc_set_csr
 *           graph, never built), a communicator, an effective k other than the lists' length, k > 128, butterfly-scored
 *           lists wider than 1536 columns or mixed with MFMA-scored fallback rows;
 *   mode 2: a plain build of the changed anchors.
 * A base with an injected graph (osc_set_csr) is refused in every mode.  Seam: osc_graph.hip build_graph_once takes its
 * updated branch iff the handle under construction carries the seed; an ordinary osc_create / osc_rebuild_graph never
 * does. */
int osc_create_updated(osc_handle base, const int32_t* ids, const float* Ynew, int64_t M, int32_t mode, osc_handle* out);
/* How a handle came to be: route 0 = not by osc_create_updated, 1 = incremental, 2 = rebuild; replaced_rows = M;
 * merged_rows = rows that kept their lists and scanned the replaced columns; redo_rows = rows recomputed other than the
 * replaced ones; family as in osc_append_info; the incremental route's times in ms (scores + selection on the device /
 * the merge scans / graph assembly); merge_hits = list entries the merge took; denied = why the planner did not take the
 * incremental route (0 = it did, or mode 2; AppendDenied in append_plan.hpp).  Any pointer may be NULL. */
int osc_update_info(osc_handle h, int32_t* route, int64_t* replaced_rows, int64_t* merged_rows, int64_t* redo_rows, int32_t* family,
                    double* score_ms, double* merge_ms, double* back_ms, int64_t* merge_hits, int32_t* denied);

/* The state U of `src` carried onto `dst`, device to device: row a of dst (API ids on both sides) takes U's row
 * src_row_of_dst[a] of src bit for bit, all row-pitch columns of it, or -- entry -1 -- starts at dst's own anchor Y[a].
 * The map has dst.N entries.  Made for a handle that osc_create_appended / osc_create_removed / osc_create_updated built
 * from src: it replaces the host round trip that keeps a settled state over such a change, `U = lat.U` -> the mutation ->
 * `lat.U = U2` (osc_get_U, two N x D host arrays, osc_set_U), which the reference has no counterpart of (its lattice
 * cannot change).  Nothing else of dst changes and src is only read.
 * While src's U still aliases its anchors (never settled, or reset) the carried state is dst's anchors row for row under
 * all three creations: dst is left at U = Y and nothing moves.  Otherwise one kernel writes dst's U in dst's internal row
 * order, ordered behind the work enqueued on src's stream; the call returns when it has finished, so src may be
 * destroyed at once.  OSC_E_INVALID, before any device work and with nothing changed, for a NULL handle or map (message in
 * osc_last_error(NULL) when dst is NULL, else osc_last_error(dst)), dst == src, handles on different devices, differing D
 * or row pitch, a communicator on either handle, a column-sharded U in src, a map entry outside [-1, src.N). */
int osc_carry_state(osc_handle dst, osc_handle src, const int32_t* src_row_of_dst);

/* rebuild_graph (lattice.py:760-801) */
int osc_rebuild_graph(osc_handle h, int32_t k, float row_cap, int32_t deterministic, int64_t seed);

/* nnz = stored directed edges (== count of A > 0), max_deg = widest row, build_ms = wall time of the last graph build
 * (lattice.py:76-77 `_graph_build_ms`); after osc_create it includes the anchors' transfer, which the build overlaps */
int osc_graph_stats(osc_handle h, int64_t* nnz, int32_t* max_deg, double* build_ms);

/* how the last device build ran: prefilter != 0 -> fp16-MFMA prefilter + exact fp32 re-scoring (2 = the
 * register-resident-panel GEMM with sampled thresholds, 1 = the 128 x 128 tile with in-kernel lists); fallback_rows = rows whose
 * candidate list could not be proven and were redone by the all-fp32 kernel; small_solves = solves served by the
 * one-launch small-lattice CG since creation */
int osc_build_info(osc_handle h, int32_t* prefilter, int32_t* fallback_rows, int64_t* small_solves);

/* the one-launch solve's plan for an N x D lattice: cols = columns per workgroup (0: general path), workgroups, LDS bytes per
 * workgroup (both 0 with cols = 0).  Pure: takes no handle and needs no device (csrc/small_plan.hpp).  A handle follows it
 * unless it has a communicator, a padded row pitch (OSC_LD), OSC_SMALL_PATH=0, or the solve asks for more than 4096
 * iterations.  OSC_E_INVALID for N < 1 or D < 1.  Any pointer may be NULL. */
int osc_small_plan(int32_t N, int32_t D, int32_t* cols, int32_t* workgroups, int64_t* lds_bytes);

/* internal row order of the last graph: reordered != 0 -> the rows are stored in BFS (locality-preserving) order, which
 * is invisible at this API (every call speaks the caller's row ids); clustering = sampled local clustering
 * coefficient that decided it (OSC_REORDER=0/1 overrides the automatic choice) */
int osc_order_info(osc_handle h, int32_t* reordered, double* clustering);
/* the internal row order itself (test / diagnostic aid): perm[new] = caller's row id, N entries; the identity when the
 * rows are stored in the caller's order */
int osc_get_row_order(osc_handle h, int32_t* perm);
/* which order the rows are stored in: order_kind 0 = the caller's, 1 = BFS (osc_order_info's reordered), 2 = balanced
 * source blocks -- an unstructured lattice's rows ordered so that every row's neighbours spread over the src_blocks
 * source blocks of the blocked CG matvec with at most 4 in each (chosen without a communicator where the apply plan has
 * source blocks in the wide kernel shapes; OSC_BALANCE=0 never, 1 wherever the plan has source blocks; OSC_REORDER=0
 * keeps the caller's order; OSC_BALANCE_HOST=1 computes the same order on the host).  For order_kind 2: displaced_before /
 * displaced_after = edges beyond the 4 slots a row has per source block in the caller's order / the stored order, rounds =
 * rounds of the search, ms = search + state move, on_device = 1 when the device kernels computed the order, 0 when the host
 * reference did (OSC_BALANCE_HOST=1, or an ELL wider than 255 / lists too large for the device form); 0 otherwise
 * (measurement aid) */
int osc_balance_info(osc_handle h, int32_t* order_kind, int64_t* displaced_before, int64_t* displaced_after, int32_t* rounds,
                     int32_t* src_blocks, double* ms, int32_t* on_device);

/* how one operator apply (the CG matvec over this handle's column window) is launched: launches = kernel launches per
 * apply, slab_cols = columns each launch covers, xs_workgroups = 0 for sequential column slabs swept by the whole
 * chip, > 0 for one launch of XCD-affine 32-column slabs with that many workgroups per XCD (measurement aid) */
int osc_spmm_plan(osc_handle h, int32_t* launches, int32_t* slab_cols, int32_t* xs_workgroups);

/* the CG matvec of the last general-path solve: src_blocks = 0 for the plain apply, else the number of source-row blocks
 * the blocked apply walked (chosen when the 32-column slab an XCD gathers from, N x 128 B, is at least 2 MiB; a chain
 * prior of up to 4096 path rows is applied by a small launch behind it; the block count follows the mean degree;
 * OSC_SPMM_BLOCKED = 0 off / n forces n blocks); blocked_applies = such matvecs enqueued since creation (measurement
 * aid) */
int osc_apply_info(osc_handle h, int32_t* src_blocks, int64_t* blocked_applies);

/* the ring of kept search directions of the last general-path solve: slots = K (1: no ring -- x was updated every
 * iteration; 2..4: the last K directions were kept and x was written by whole passes over them only; OSC_X_RING = 0 off /
 * 2..4 forces K, capped by max_iters), flushes = its passes that ran inside an iteration because a slot was about to be
 * overwritten, passes = all its x passes (one where the solve took at most K iterations), bytes = device memory the
 * handle holds for the ring (measurement aid) */
int osc_x_ring_info(osc_handle h, int32_t* slots, int64_t* flushes, int64_t* passes, int64_t* bytes);

/* the streamed first apply of anchor starts (a solve that starts from the anchors under uniform gates, without a chain
 * prior, on the blocked plan: from the lattice's second such solve on, the cached INIT pass also emits iteration 1's A p from
 * the anchors' second row sums W (W Y) and W 1, and that iteration's gathering matvec is not launched; OSC_ANCHOR_AP = 0 off /
 * 1 wherever the cached INIT pass runs, unset: lattices of at least 96000 rows): streamed_first_applies = such solves since
 * creation, bytes = device memory held for the two arrays (0: not built or dropped), last_solve = whether the last
 * general-path solve took the route, builds = times the arrays were formed (measurement aid) */
int osc_anchor_ap_info(osc_handle h, int64_t* streamed_first_applies, int64_t* bytes, int32_t* last_solve, int64_t* builds);

/* the streamed second apply of anchor starts (on top of the streamed first apply, in a solve of at least two iterations: the
 * cached INIT pass also leaves T = A (A p1), formed from the anchors' third row sums W (W (W Y)) and W (W 1), iteration 2's p
 * update forms A p2 = (1 + beta1) A p1 - m alpha1 T beside p2, and that iteration's gathering matvec is not launched either;
 * OSC_ANCHOR_AP2 = 0 off / 1 wherever the streamed first apply runs, unset: lattices of at least 96000 rows):
 * streamed_second_applies = iterations served so since creation, bytes = device memory held for the two arrays and T (0: not
 * built or dropped), last_solve = whether the last general-path solve took the route, builds = times the arrays were formed
 * (measurement aid) */
int osc_anchor_ap2_info(osc_handle h, int64_t* streamed_second_applies, int64_t* bytes, int32_t* last_solve, int64_t* builds);

/* iterations 1 and 2 of an anchor start inside its INIT pass (further still: the CG scalars of both iterations come from float64
 * Gram sums of the cached row sums, kept per lattice, so neither iteration reads or writes an N x D array of its own;
 * OSC_ANCHOR_GRAM = 0 off / 1 wherever the streamed second apply runs in a ring solve predicted to take three or more
 * iterations, unset: lattices of at least 96000 rows): fused_two_step_solves = solves served so since creation, bytes = device
 * memory held for the sums ((22 ld + 6) doubles; 0: not built or dropped), last_solve = whether the last general-path solve
 * took the route, builds = times the sums were formed, redos = solves that stopped before iteration 3 (or had a column the
 * sums cannot serve) and were run again on the summed route (measurement aid).  OSC_TWO_STEPS = stream (unset) / blocked: the
 * launch geometry of the fused pass -- the update kernels' or the blocked matvec's (the reference form); same bits either way */
int osc_anchor_gram_info(osc_handle h, int64_t* fused_two_step_solves, int64_t* bytes, int32_t* last_solve, int64_t* builds,
                         int64_t* redos);
/* the Gram sums as held (test aid): 22 arrays of ld doubles -- <W^j Y, W^k Y> for j <= k <= 3 in the order (0,0) (0,1) (0,2)
 * (0,3) (1,1) (1,2) (1,3) (2,2) (2,3) (3,3), then <a, W^j Y> for a = 1, W 1, W W 1 and j = 0..3 -- and the six <a, b> in the
 * order (1,1) (1,s) (1,s2) (s,s) (s,s2) (s2,s2); cap = doubles `out` holds; OSC_E_UNSUPPORTED while no sums are held */
int osc_anchor_gram_read(osc_handle h, double* out, int64_t cap);

/* iteration 3 of such a solve in one launch (one step further: alpha3, beta3 and |r3| come from the sums of the two vectors A p3
 * adds to the seven, W W W 1 and W W W W Y, so the iteration's matvec forms r3 and p4 in its epilogue and the alpha reduction, the
 * x-r kernel, the beta reduction and iteration 4's p update are not launched; OSC_ANCHOR_GRAM3 = 0 off / 1 wherever the fused
 * two-step pass runs, unset: lattices of at least 96000 rows): fused_three_step_solves = solves served so since creation, bytes
 * = device memory held ((13 ld + 4) doubles and N floats; 0: not built or dropped), last_solve = whether the last general-path
 * solve took the route, builds = times the sums were formed (measurement aid) */
int osc_anchor_gram3_info(osc_handle h, int64_t* fused_three_step_solves, int64_t* bytes, int32_t* last_solve, int64_t* builds);
/* those sums as held (test aid): 13 arrays of ld doubles -- <W^j Y, W^4 Y> for j = 0..4, then <a, W^4 Y> for a = 1, s, s2, s3 (s
 * = W 1, s2 = W s, s3 = W s2), then <s3, W^j Y> for j = 0..3 -- and the four <a, s3>, a = 1, s, s2, s3; cap = doubles `out`
 * holds; OSC_E_UNSUPPORTED while none are held */
int osc_anchor_gram3_read(osc_handle h, double* out, int64_t cap);

/* a solve of that kind that ends in iteration 4 without a fourth matvec (one level of scalars further: alpha4 and |r4| come from
 * the sums of the two vectors A p4 adds, W W W W 1 and W^5 Y; where the published residuals show the solve to end in iteration 4,
 * iteration 3's matvec writes x4 = x3 + alpha4 p4 from its epilogue and iteration 4 launches nothing; OSC_ANCHOR_GRAM4 = 0 off /
 * 1 wherever the three-step route runs, unset: lattices of at least 96000 rows): fused_four_step_solves = solves that ended so
 * since creation, bytes = device memory held ((16 ld + 5) doubles; 0: not built or dropped), last_solve = whether the last
 * general-path solve ended so, builds = times the sums were formed (measurement aid) */
int osc_anchor_gram4_info(osc_handle h, int64_t* fused_four_step_solves, int64_t* bytes, int32_t* last_solve, int64_t* builds);
/* the form of such a solve's one matvec: folded_four_step_solves = those of fused_four_step_solves whose INIT pass stored x4 less
 * the term in the gathered row sum, so that the matvec reads and writes that one row stream (solves predicted to end in iteration 4); enabled = 0 under OSC_GRAM4_FOLD=0,
 * which keeps the unfolded form (the reference: its results are bit-identical to the route before the fold existed) */
int osc_gram4_fold_info(osc_handle h, int64_t* folded_four_step_solves, int32_t* enabled);
/* such a solve without any matvec (the polynomial last form: x4 = sum_k a_k W^k Y + sum_k q_k W^k 1 per column, one elementwise pass
 * over the lattice's held row sums, W^4 Y among them; OSC_ANCHOR_POLY = 0 off / 1 wherever the folded form would run, unset:
 * lattices of at least 96000 rows): poly_four_step_solves = those of fused_four_step_solves that ran so, bytes = device memory W^4 Y
 * holds (N x ld floats; 0: not kept, denied by the memory rule, or dropped), last_solve = whether the last general-path solve ran
 * so, builds = times W^4 Y was kept, redos = solves predicted to end in iteration 4 whose residuals said otherwise: the pass was
 * gated off and the solve ran again on the folded form's route */
int osc_anchor_poly_info(osc_handle h, int64_t* poly_four_step_solves, int64_t* bytes, int32_t* last_solve, int64_t* builds,
                         int64_t* redos);
/* those sums as held (test aid): 16 arrays of ld doubles -- <W^j Y, W^5 Y> for j = 0..5, then <a, W^5 Y> for a = 1, s, s2, s3, s4
 * (s4 = W s3), then <s4, W^j Y> for j = 0..4 -- and the five <a, s4>, a = 1, s, s2, s3, s4; cap = doubles `out` holds;
 * OSC_E_UNSUPPORTED while none are held */
int osc_anchor_gram4_read(osc_handle h, double* out, int64_t cap);

/* the block-major copy of the graph the blocked matvec walks, built for `nb` source blocks (test / diagnostic aid; no
 * reference counterpart): slot_col / slot_w [nb][N][4] = {neighbour row, W_ij} per (source block, row, slot), unused slots
 * {first row of the block, 0}; rows whose edges exceed 4 nb slots list the rest in over_col / over_w[over_first[i] ..
 * + over_count[i]) (at most over_cap entries in all).  Any output may be NULL.  OSC_E_UNSUPPORTED on a lattice stored in
 * an internal row order. */
int osc_get_blocked_copy(osc_handle h, int32_t nb, int32_t* slot_col, float* slot_w, int32_t* over_first,
                         int32_t* over_count, int32_t* over_col, float* over_w, int32_t over_cap);

/* CSR view of the graph for `.A`, `.L_sym`, `_signature()` (lattice.py:729-744) and export_state
 * (:582-624).  rowptr has N+1 entries; col/a/w have nnz entries, columns ascending within a row;
 * a = capped adjacency A_ij (> 0), w = A_ij / (sqrt_deg_i sqrt_deg_j); sqrt_deg has N entries.
 * Any output pointer may be NULL. */
int osc_get_csr(osc_handle h, int64_t* rowptr, int32_t* col, float* a, float* w, float* sqrt_deg);

/* the first min(cap, nnz) stored edges as int64 (i, j) pairs in row-major order, columns ascending within a row:
 * `argwhere(A > 0)[:cap]` of _signature() (lattice.py:729-744) without moving the whole graph to the host */
int osc_edge_prefix(osc_handle h, int32_t cap, int64_t* pairs, int32_t* n);

/* Inject a (symmetric, zero-diagonal, already capped) adjacency as CSR; recomputes sqrt_deg and W
 * exactly as normalized_laplacian (graph.py:86-93).  Mirrors from_state's `lat.A = A;
 * lat.L_sym, lat.sqrt_deg = normalized_laplacian(lat.A)` (lattice.py:709-713). */
int osc_set_csr(osc_handle h, const int64_t* rowptr, const int32_t* col, const float* a);

/* raw per-row top-k lists of the last device graph build (idx/val: N x k_eff, unsorted within a row;
 * val is the similarity clipped at 0) -- graph.py:59-62.  Test/diagnostic aid. */
int osc_get_knn_lists(osc_handle h, int32_t* idx, float* val, int32_t* k_eff);

/* ---- state setters -------------------------------------------------------------------------- */
/* set_query / set_gates (lattice.py:114-127): psi has D entries; gates (N entries) may be NULL */
int osc_set_query(osc_handle h, const float* psi, const float* gates_or_null);
/* add_chain + build_path_laplacian (lattice.py:129-149, graph.py:96-111); weights may be NULL (all 1) */
int osc_set_chain(osc_handle h, const int32_t* chain, const float* weights_or_null, int32_t len, float lamP);
int osc_clear_chain(osc_handle h);                      /* lattice.py:151-157 */
int osc_set_lams(osc_handle h, float lamG, float lamC, float lamQ);
int osc_get_U(osc_handle h, float* out);                /* N x D */
int osc_get_Y(osc_handle h, float* out);                /* N x D: the device's private copy of the anchors */
int osc_set_U(osc_handle h, const float* U_or_null);    /* NULL -> U = Y (device copy, ordered by the handle's stream: returns without waiting for it) */

/* ---- solves --------------------------------------------------------------------------------- */
/* settle (lattice.py:159-230) + cg_solve (solver.py:6-37): one implicit-Euler step
 * (I + dt M) U+ = U + dt (lamG Y + lamQ B 1 psi^T), Jacobi diagonal 1 + dt (lamG + lamQ B + [lamP]),
 * x0 = Y (warm_start == 0) | U | (1-w) Y + w U with w = clamp(inertia, 0, 1) (lattice.py:751-758).
 * Stop test: max over columns of ||r_c||_2 <= tol, checked before the beta/p update.  Never fails on
 * non-convergence: iters = max_iters and res is the last residual (lattice.py:206-212).
 * ms = host wall time of x0 selection + CG, device-synchronised (the reference's t_ms). */
int osc_settle(osc_handle h, float dt, int32_t max_iters, float tol, int32_t precond, int32_t warm_start,
               float inertia, int32_t* iters, float* res, double* ms);
/* solve_Ustar (lattice.py:232-290): M U* = lamG Y + lamQ B 1 psi^T from x0 = Y, Jacobi lamG + lamQ B + [lamP].
 * U* stays resident on the device for osc_deltaH / receipts; Ustar_out (N x D) may be NULL. */
int osc_solve_ustar(osc_handle h, float tol, int32_t max_iters, float* Ustar_out, int32_t* iters, float* res,
                    double* ms);
/* 1 iff a U* of the current state (graph, psi, gates, lams, chain) is resident on the device */
int osc_has_ustar(osc_handle h, int32_t* yes);
/* copy the resident U* (N x D) to the host; OSC_E_STATE if no solve happened since the last state change */
int osc_get_ustar(osc_handle h, float* out);
/* n selected rows (caller's row ids) of Y (which = 0), U (1) or the resident U* (2) into out (n x D): what
 * chain_receipt (lattice.py:466-528) reads -- the chain nodes and their neighbours -- without moving N x D floats */
int osc_get_rows(osc_handle h, int32_t which, const int32_t* rows, int32_t n, float* out);
/* residual after every iteration of the last solve (solver.py:29), n <= cap entries written */
int osc_residual_history(osc_handle h, float* out, int32_t cap, int32_t* n);

/* screened diffusion solve used by compute_diffusion_gates(method="cg")
 * (preprocess/diffusion.py:130-151): (L_sym + gamma I) h = s, x0 = 0, Jacobi diag(L)+gamma = 1+gamma. */
int osc_cg_single_rhs(osc_handle h, float gamma, const float* s, float tol, int32_t max_iters, float* h_out,
                      int32_t* iters, float* res);
/* cosine of every anchor row with psi (diffusion.py:104-107): out[i] = <Y_i/(|Y_i|+1e-12), psi/(|psi|+1e-12)> */
int osc_cosine_to(osc_handle h, const float* psi, float* out);
/* the same over the rows of the resident U*: bundle()'s alignment term (lattice.py:530-568:
 * align_i = <U*_i / (|U*_i| + 1e-12), psi / (|psi| + 1e-12)>); OSC_E_STATE without a resident U*.  With psi = an
 * anchor row, osc_cosine_to gives the similarity row mmr_diversify needs for one chosen item (graph.py:114-133). */
int osc_ustar_cosine_to(osc_handle h, const float* psi, float* out);
/* out[i] = <Yn_i, Yn_row>: the similarity row of one chosen item for mmr_diversify (graph.py:114-133), from the
 * device's own copy of the anchors */
int osc_cosine_to_row(osc_handle h, int64_t row, float* out);
/* mmr_diversify (graph.py:114-133) over the device's own anchors: greedy selection of min(k, N) rows maximising
 * (1 - lambda_div) * scores[i] - lambda_div * max_{j chosen} cos(Y_i, Y_j), first maximum in row order; scores and
 * out_idx in API row order.  *out_count receives the number of rows written. */
int osc_mmr(osc_handle h, const float* scores, int32_t k, float lambda_div, int32_t* out_idx, int32_t* out_count);

/* ---- multi-query bundles (not in the reference) -------------------------------------------------
 * For the lattice's current graph, gates, chain and lambdas U*(psi) = X + x psi^T with M X = lamG Y (N x D) and
 * M x = lamQ B (N x 1): one basis serves every query.  Batches are processed OSC_QUERY_CHUNK queries at a time. */
#define OSC_QUERY_CHUNK 256
/* Not in the reference (the basis behind solve_Ustar, lattice.py:232-290, for every psi at once).  fresh != 0 solves X
 * (Jacobi-PCG from x0 = Y, stop at max_c |r_c| <= tol / 2) and x; fresh == 0 keeps X and continues x from the resident
 * one.  x is solved to |r_x| <= tol / (2 scale), scale = the largest |psi|_inf it must serve.  iters[2] / res[2] receive
 * X's and x's iterations and final residuals (X: 0 and -1 when kept).  OSC_E_UNSUPPORTED with a communicator. */
int osc_query_basis(osc_handle h, float tol, int32_t max_iters, float scale, int32_t fresh, int32_t* iters, float* res,
                    double* ms);
/* Not in the reference: the resident basis in API row order (X_out N x D, x_out N; either may be NULL).
 * OSC_E_STATE without a basis for the current graph. */
int osc_get_query_basis(osc_handle h, float* X_out, float* x_out);
/* bundle(k, alpha) (lattice.py:530-568) for Q queries psis (Q x D) from the resident basis: per query
 * align_i = cos(U*_i, psi), coh_i (receipts.py:28-38) z-scored, score = alpha z + (1 - alpha) align and
 * mmr_diversify (graph.py:114-133, lambda_div) over the anchors.  ids / score / align are Q x min(k, N), API ids. */
int osc_bundle_many(osc_handle h, const float* psis, int32_t Q, int32_t k, float alpha, float lambda_div, int32_t* ids,
                    float* score, float* align);
/* compute_diffusion_gates (preprocess/diffusion.py:104-124, 130-151: the sources, the screened-diffusion solve, the min-max
 * normalisation and the clip) for Q queries psis (Q x D) on the lattice's graph, as ONE Jacobi-PCG with a right-hand side
 * per query: (L_sym + gamma I) h_q = beta max(0, cos(Y_i, psi_q)).  method 0 ("direct"): every
 * column runs to |r_q| <= 1e-7 max(1, |s_q|), 2048 iterations at most; method 1 ("cg"): to |r_q| <= tol, max_iters at most.
 * A column stops at its own residual and is not touched afterwards, so row q is what the single-query path
 * (osc_cosine_to + osc_cg_single_rhs) gives for psi_q, and is the same to the bit whatever else the batch holds.
 * gates_out is Q x N in API row order (clamp != 0: min-max normalised, ones where max - min < 1e-12; always clipped to
 * [0, 1]); iters_out / res_out (Q each, may be NULL) receive each query's own iteration count and final |r_q|.  Queries run
 * OSC_GATES_CHUNK (read at every call; default and at most 256, a multiple of 32) at a time.  Changes no state of the handle.
 * OSC_E_INVALID for gamma <= 0, max_iters < 1, an unknown method or a non-finite query, OSC_E_STATE without a graph,
 * OSC_E_UNSUPPORTED with a communicator. */
int osc_gates_many(osc_handle h, const float* psis, int32_t Q, float beta, float gamma, int32_t method, float tol,
                   int32_t max_iters, int32_t clamp, float* gates_out, int32_t* iters_out, float* res_out);
/* Not in the reference as one call: set_query(psi_q, gates = g_q); bundle(k, alpha) (lattice.py:114-120, 245-263, 530-568;
 * the second half of examples/rag_replacement.py:159-177) for Q queries psis (Q x D) on the lattice's graph and lambdas
 * (DESIGN.md section 11.2).  With gates M_q = lamG I + lamC L_sym + lamQ diag(g_q) differs per query, so every query gets
 * its own N x D solve of solve_Ustar -- RHS = lamG Y + lamQ g_q psi_q^T, x0 = Y, the Jacobi diagonal lamG + lamQ g_q + 1e-12,
 * alpha / beta per column (solver.py:6-37) -- and the solves of a chunk run as ONE panel PCG over the shared graph.  A query
 * stops at the first iteration where its largest column residual is <= tol, all its columns together, after max_iters at
 * most.  gates is Q x N in API row order; with diffusion != 0 it is an OUTPUT first: osc_gates_many(psis, gate_beta,
 * gate_gamma, gate_method, gate_tol, gate_max_iters, clamp = 1) writes it, then the solves read it.  ids / score / align are
 * osc_bundle_many's (Q x min(k, N) each; k <= 0: not written); iters_out / res_out (Q each, may be NULL) receive each query's
 * iteration count and its largest column residual.  A query's outputs are the same to the bit whatever else the batch holds;
 * a non-finite query or gate row gives that query non-finite answers and changes no other's.  Queries run OSC_GATED_CHUNK
 * (read at every call; default and at most 256) at a time, fewer where one chunk's scratch would pass 1 GiB, never fewer than
 * one.  The lattice's own gates, psi, U, U* and query basis are neither read nor changed.  OSC_E_INVALID for max_iters < 1
 * (and osc_gates_many's with diffusion), OSC_E_STATE without a graph, OSC_E_UNSUPPORTED with a communicator or a chain of the
 * lattice's own. */
int osc_bundle_gated_many(osc_handle h, const float* psis, int32_t Q, float* gates, int32_t diffusion, float gate_beta,
                          float gate_gamma, int32_t gate_method, float gate_tol, int32_t gate_max_iters, float tol,
                          int32_t max_iters, int32_t k, float alpha, float lambda_div, int32_t* ids, float* score, float* align,
                          int32_t* iters_out, float* res_out);
/* The solves of osc_bundle_gated_many alone, read out: U_out is Q x N x D (API row order), U*_q of solve_Ustar under gates
 * g_q (diagnostic; the batched MMR's osc_mmr_many plays the same role). */
int osc_ustar_gated_many(osc_handle h, const float* psis, int32_t Q, const float* gates, float tol, int32_t max_iters,
                         float* U_out, int32_t* iters_out, float* res_out);
/* Not in the reference: the gated flow's set_query(psi_q, gates = g_q); [settle(dt, settle_max_iters, settle_tol);] receipt();
 * [bundle(k, alpha)] (lattice.py:159-230, 298-455, receipts.py:10-83) for Q queries in one call.
 * psis, gates, diffusion and the gate_* arguments are osc_bundle_gated_many's, and so are tol / max_iters of the U* solve,
 * iters_out / res_out and -- with k > 0 -- ids / score / align, bit for bit.  With settle != 0 every query's implicit Euler
 * step starts from the handle's current U (warm_start, no inertia) and stops by solver.py:23-37; settle_iters / settle_res
 * (Q each) report it and deltaH is measured from the query's settled state, which is not written back.  With settle == 0
 * deltaH is measured from U as it is.  dH ... capacity are osc_receipt_many's outputs (detail, z_th, null_cap as there), the
 * energies and null points being those of U*_q under M_q = lamG I + lamC L_sym + lamQ diag(g_q).  settle_ms / solve_ms (Q
 * each): the wall time of the query's chunk in that phase divided by the chunk's queries.  A query's outputs are the same to
 * the bit whatever else the batch holds; queries run OSC_GATED_CHUNK at a time, fewer where a chunk's scratch would pass
 * 1 GiB, never fewer than one.  The handle's U is read; nothing of its state is changed.  Errors as osc_bundle_gated_many;
 * OSC_E_INVALID also for dt <= 0 or settle_max_iters < 1 with settle, or a capacity too small for the null points. */
int osc_receipt_gated_many(osc_handle h, const float* psis, int32_t Q, float* gates, int32_t diffusion, float gate_beta,
                           float gate_gamma, int32_t gate_method, float gate_tol, int32_t gate_max_iters, float tol,
                           int32_t max_iters, int32_t settle, float dt, int32_t settle_max_iters, float settle_tol,
                           int32_t detail, float z_th, int32_t null_cap, int32_t k, float alpha, float lambda_div,
                           int32_t* settle_iters, float* settle_res, double* dH, double* coh_sum, double* anchor_sum,
                           double* query_sum, int32_t* null_total, int64_t* null_offsets, int32_t* i_out, int32_t* j_out,
                           float* z_out, float* r_out, int64_t capacity, int32_t* ids, float* score, float* align,
                           int32_t* iters_out, float* res_out, double* settle_ms, double* solve_ms);
/* Not in the reference: the request sequence with per-query gates AND a per-query chain prior -- add_chain(chain_q, lamP,
 * weights_q); set_query(psi_q, gates = g_q); [settle(...);] receipt(); chain_receipt(chain_q, chain_z_th); [bundle(k, alpha)]
 * (lattice.py:129-149, 159-296, 298-455, 466-528, 530-568) -- for Q queries in one call on a handle without a chain of its
 * own.  Everything but the chain arguments is osc_receipt_gated_many's, with its outputs; the
 * diffusion gates are those of the lattice without the chain.  chain_offsets / chain_nodes are osc_chain_receipt_many's (a chain
 * has 2 to 1024 nodes, repeats allowed, any number of distinct ones); chain_weights is NULL for ones or flat over the chains'
 * edges like the per-edge outputs (build_path_laplacian's rules: the largest weight of a revisited edge, below zero counts as
 * zero).  Query q's operator in the settle, the U* solve and deltaH is M_q = lamG I + lamC L_sym + lamQ diag(g_q) +
 * lamP L_path,q, with the reference's Jacobi diagonal lamG + lamQ g + lamP; lamP == 0 leaves the operator alone, and every
 * receipt and bundle output is then osc_receipt_gated_many's to the bit.  The chain outputs are osc_chain_receipt_many's, of
 * U*_q from the call's own solve, the path residuals on the weighted path of the argument.  A query's outputs are the same to
 * the bit whatever else the batch holds.  Errors as osc_receipt_gated_many; OSC_E_INVALID also for lamP < 0, chains outside
 * the limits or non-finite weights. */
int osc_chain_gated_many(osc_handle h, const float* psis, int32_t Q, float* gates, int32_t diffusion, float gate_beta,
                         float gate_gamma, int32_t gate_method, float gate_tol, int32_t gate_max_iters,
                         const int64_t* chain_offsets, const int32_t* chain_nodes, const float* chain_weights, float lamP,
                         float chain_z_th, float tol, int32_t max_iters, int32_t settle, float dt, int32_t settle_max_iters,
                         float settle_tol, int32_t detail, float z_th, int32_t null_cap, int32_t k, float alpha,
                         float lambda_div, int32_t* settle_iters, float* settle_res, double* dH, double* coh_sum,
                         double* anchor_sum, double* query_sum, int32_t* null_total, int64_t* null_offsets, int32_t* i_out,
                         int32_t* j_out, float* z_out, float* r_out, int64_t capacity, int32_t* ids, float* score, float* align,
                         int32_t* iters_out, float* res_out, double* settle_ms, double* solve_ms, float* chain_z_struct,
                         float* chain_z_path, float* chain_r_struct, float* chain_r_path, double* chain_gain,
                         int32_t* chain_verdict, int32_t* chain_weakest_k, float* chain_weakest_z);
/* Not in the reference: receipt() (lattice.py:298-455, receipts.py:10-83) for Q queries psis (Q x D) with the current U,
 * gates, chain and lambdas held fixed, U*(psi) from the resident basis.  Per query: dH (deltaH_trace
 * of U against U*(psi_q)); with detail != 0 also coh_sum / anchor_sum / query_sum and the null points at z_th (else 0 and
 * none).  null_total[q] counts query q's null points; null_cap > 0 keeps the null_cap highest z of a query that has more
 * (ties in API row order, in that order), else all in API row order.  The kept records of query q are
 * [null_offsets[q], null_offsets[q + 1]) of i_out / j_out / z_out / r_out (capacity entries; OSC_E_INVALID if too few).
 * OSC_E_STATE without a basis, OSC_E_UNSUPPORTED with a communicator. */
int osc_receipt_many(osc_handle h, const float* psis, int32_t Q, int32_t detail, float z_th, int32_t null_cap, double* dH,
                     double* coh_sum, double* anchor_sum, double* query_sum, int32_t* null_total, int64_t* null_offsets,
                     int32_t* i_out, int32_t* j_out, float* z_out, float* r_out, int64_t capacity);
/* Not in the reference: chain_receipt(chain, z_th) (lattice.py:466-528) for Q (query, chain) pairs with the current graph,
 * gates, own chain and lambdas held fixed, U*(psi_q) from the resident basis.  psis is Q x D.
 * chain_offsets holds Q + 1 node offsets from 0 into chain_nodes (API row ids); a chain has 2 to 1024 nodes, repeats allowed.
 * The path residuals use the lattice's own chain (osc_set_chain) with its weights when it has one, else the unit-weight path
 * of the argument (lattice.py:479-483).  A chain of L nodes has L - 1 edges: query q's edge t is entry
 * chain_offsets[q] - q + t of z_struct / z_path / r_struct / r_path (chain_offsets[Q] - Q entries each).  Per query: gain
 * (coherence_gain, added in fp64 in edge order), verdict (1: every edge's max(z_struct, z_path) <= z_th), weakest_k (the
 * first edge whose max(z) is strictly greater than every earlier one, from -1.0; -1 when none is) and weakest_z (that
 * maximum, -1.0 with weakest_k = -1).  A non-finite query gives non-finite answers for that query alone.
 * OSC_E_STATE without a basis, OSC_E_UNSUPPORTED with a communicator, OSC_E_INVALID for a node outside [0, N) or a chain
 * outside 2..1024 nodes. */
int osc_chain_receipt_many(osc_handle h, const float* psis, int32_t Q, const int64_t* chain_offsets,
                           const int32_t* chain_nodes, float z_th, float* z_struct, float* z_path, float* r_struct,
                           float* r_path, double* gain, int32_t* verdict, int32_t* weakest_k, float* weakest_z);
/* Not in the reference: per-query chain priors on a resident lattice.  Query q gets what
 * osc_set_chain(chain_q, weights_q, lamP); osc_set_query(psi_q); chain_receipt(chain_q, z_th) gives, from one basis of the
 * shifted operator M' = M + lamP I and a low-rank update: M + lamP L_path,q = M' - S_q K_q S_q^T over the chain's distinct nodes.
 *
 * osc_query_basis_shifted solves that basis (M' X' = lamG Y, M' x' = lamQ B) into a slot of its own beside osc_query_basis's
 * (one more N x ld array and N x 4 floats); arguments and outputs as osc_query_basis, lamP > 0, res[0] the residual of the
 * stored (scaled) X'.  fresh == 0 keeps X' when the slot holds this lamP for the current graph.  OSC_E_STATE on a lattice
 * with a chain of its own, OSC_E_UNSUPPORTED with a communicator.
 *
 * osc_chain_prior_many: osc_chain_receipt_many's arguments and outputs, and lamP >= 0, chain_weights (flat over the chains'
 * edges like z_struct, or NULL for ones), tol / max_iters of the Green's columns M' g = e_node (one Jacobi-PCG over a panel with
 * a column per distinct chain node, stopped per column at a tolerance derived from tol and the basis), prior_res[q] (the bound
 * |r_basis| + sum_e |r_e| max_c |(T_q V_q)[e, c]| on the residual of the implied U*_q) and prior_iters[q] (the most iterations any
 * of its columns took).  lamP == 0 reads osc_query_basis's basis and solves nothing; only the path weights differ from
 * osc_chain_receipt_many.  A chain has at most 64 distinct nodes.  A query's outputs are the same to the bit whatever else the
 * batch holds.  OSC_E_STATE without the basis (shifted for lamP > 0), OSC_E_UNSUPPORTED with a communicator, OSC_E_INVALID for
 * a lattice with a chain of its own, lamP < 0, a non-finite weight, more than 64 distinct nodes and osc_chain_receipt_many's
 * reasons. */
int osc_query_basis_shifted(osc_handle h, float lamP, float tol, int32_t max_iters, float scale, int32_t fresh, int32_t* iters,
                            float* res, double* ms);
int osc_chain_prior_many(osc_handle h, const float* psis, int32_t Q, const int64_t* chain_offsets, const int32_t* chain_nodes,
                         const float* chain_weights, float lamP, float tol, int32_t max_iters, float z_th, float* z_struct,
                         float* z_path, float* r_struct, float* r_path, double* gain, int32_t* verdict, int32_t* weakest_k,
                         float* weakest_z, float* prior_res, int32_t* prior_iters);
/* Not in the reference as one call: bundle(k, alpha) (lattice.py:530-568) for Q (query, chain) pairs, query q on the stationary
 * state of M + lamP L_path,q -- what add_chain(chain_q, lamP, weights_q) (lattice.py:129-150), set_query(psi_q) and bundle give
 * on a lattice without a chain of its own.  psis, chain_offsets, chain_nodes, chain_weights, lamP, tol,
 * max_iters, prior_res and prior_iters are osc_chain_prior_many's, the shifted basis osc_query_basis_shifted's; k, alpha,
 * lambda_div, ids, score and align are osc_bundle_many's (Q x min(k, N) each).  U*_q is never formed: its alignment and
 * coherence terms are expanded over the shifted basis, the Green's columns of the chain's nodes and T_q V_q.  lamP == 0 is
 * osc_bundle_many on osc_query_basis's basis.  A query's outputs are the same to the bit whatever else the batch holds.
 * OSC_E_STATE without the basis (shifted for lamP > 0), OSC_E_UNSUPPORTED with a communicator, OSC_E_INVALID for a lattice with
 * a chain of its own, a non-finite query and osc_chain_prior_many's reasons. */
int osc_bundle_prior_many(osc_handle h, const float* psis, int32_t Q, const int64_t* chain_offsets, const int32_t* chain_nodes,
                          const float* chain_weights, float lamP, float tol, int32_t max_iters, int32_t k, float alpha,
                          float lambda_div, int32_t* ids, float* score, float* align, float* prior_res, int32_t* prior_iters);
/* Not in the reference as one call: receipt() (lattice.py:298-455, receipts.py:10-83) for Q (query, chain) pairs, query q on the
 * stationary state of M + lamP L_path,q -- what add_chain(chain_q, lamP, weights_q) (lattice.py:129-150), set_query(psi_q) and
 * receipt() give on a lattice without a chain of its own, with the current U, gates and lambdas held fixed (DESIGN.md section
 * 12.3).  psis, chain_offsets, chain_nodes, chain_weights, lamP, tol, max_iters, prior_res and prior_iters are
 * osc_chain_prior_many's, the shifted basis osc_query_basis_shifted's; detail, z_th, null_cap, the four sums, the null-point
 * outputs and capacity are osc_receipt_many's.  The null points run over the graph's edges on U*_q (add_chain does not touch
 * A).  U*_q is never formed: deltaH comes from m rows of U, X' and x' at the chain's nodes, the sums from the moments of the
 * Green's columns, the null points from section 11.1's per-(row, query) expansion.  lamP == 0 is osc_receipt_many on
 * osc_query_basis's basis.  A query's outputs are the same to the bit whatever else the batch holds.
 * OSC_E_INVALID for a NULL handle, a lattice with a chain of its own, a non-finite query, osc_bundle_prior_many's and
 * osc_receipt_many's reasons; OSC_E_STATE without the basis (shifted for lamP > 0); OSC_E_UNSUPPORTED with a communicator. */
int osc_receipt_prior_many(osc_handle h, const float* psis, int32_t Q, const int64_t* chain_offsets,
                           const int32_t* chain_nodes, const float* chain_weights, float lamP, float tol, int32_t max_iters,
                           int32_t detail, float z_th, int32_t null_cap, double* dH, double* coh_sum, double* anchor_sum,
                           double* query_sum, int32_t* null_total, int64_t* null_offsets, int32_t* i_out, int32_t* j_out,
                           float* z_out, float* r_out, int64_t capacity, float* prior_res, int32_t* prior_iters);
/* mmr_diversify (graph.py:114-133) for Q score columns at once: scores N x Q (API row order, queries contiguous per row);
 * out_idx Q x min(k, N) API ids, the same picks as osc_mmr per column up to rounding of the similarities. */
int osc_mmr_many(osc_handle h, const float* scores, int32_t Q, int32_t k, float lambda_div, int32_t* out_idx);

/* ---- corpus refine (not in the reference) ------------------------------------------------------
 * A corpus Y (N x D, D <= 1536) resident on the device as Y and Yn = Y / (|Y_i| + 1e-12) (osc_create's normalisation), both
 * at a row pitch of D rounded up to 32 floats, and nothing else: 8 N ldn bytes.  Queries run OSC_CORPUS_CHUNK (read at
 * creation, default 256) at a time, fewer when one chunk's scratch would pass 1 GiB. */
typedef struct osc_corpus* osc_corpus_handle;
int osc_corpus_create(const float* Y, int64_t N, int32_t D, int32_t device, osc_corpus_handle* out);
int osc_corpus_destroy(osc_corpus_handle h);
const char* osc_corpus_last_error(osc_corpus_handle h);  /* h may be NULL: error of the last failed osc_corpus_create */
/* queries per chunk and one chunk's scratch bytes for a refine of these settings (measurement aid) */
int osc_corpus_info(osc_corpus_handle h, int32_t top_k, int32_t kneighbors, int32_t k, int32_t* chunk, int64_t* bytes);
/* The candidate step of the reference's retrieval loop (scripts/bench_beir.py:84-94 `argpartition` top-K of D @ psi;
 * scripts/real_benchmark.py:328-343, examples/rag_replacement.py:48-66): per query the K = min(top_k, N) corpus rows of the
 * largest cosine Yn_i . psi / (|psi| + 1e-12), ties to the smaller id, in that order.  ids / cos: Q x K.  top_k <= 1024. */
int osc_corpus_search(osc_corpus_handle h, const float* psis, int32_t Q, int32_t top_k, int32_t* ids, float* cos);
/* The whole loop body for Q queries (scripts/bench_beir.py:84-94, scripts/competitor_benchmark.py:236-247):
 * `Oscillink(Y[cand], kneighbors, row_cap, lamG, lamC, lamQ); set_query(psi); bundle(k, alpha)` with U* solved from x0 = Y
 * (lattice.py:245-263; tol / max_iters as solve_Ustar) and mmr lambda 0.5.  cand_in (Q x K) replaces the search when not
 * NULL.  min(kneighbors, K - 1) <= 128 (the dense build route).  Out: cand_out Q x K; local / score / align Q x min(k, K),
 * local = the pick's row in its candidate lattice; iters / res per query (the U* solve's). */
int osc_corpus_refine(osc_corpus_handle h, const float* psis, int32_t Q, int32_t top_k, const int32_t* cand_in,
                      int32_t kneighbors, float row_cap, float lamG, float lamC, float lamQ, float tol, int32_t max_iters,
                      int32_t k, float alpha, int32_t* cand_out, int32_t* local, float* score, float* align, int32_t* iters,
                      float* res);
/* The gates of the reference's hallucination-control loop (examples/rag_replacement.py:159-177, examples/diffusion_gated.py:
 * `compute_diffusion_gates(Y[cand], psi, kneighbors, row_cap_val, beta, gamma, method, tol, max_iters)`,
 * preprocess/diffusion.py:35-124) for Q queries, one single-right-hand-side solve per candidate lattice on the device:
 * s_i = beta max(0, cos(Y_i, psi)), (L_sym + gamma I) h = s by Jacobi-PCG from x0 = 0, min-max to [0, 1] (ones when
 * max h - min h < 1e-12).  method 0 = "direct" (the CG run to 1e-7 max(1, |s|), at most 2048 iterations; tol / max_iters
 * unused), 1 = "cg" (tol / max_iters under solver.py's stop rule).  clamp = 0: the solve's h itself, not normalised and
 * not clipped.  cand_in (Q x K) replaces the search when not NULL.  Out: cand_out / gates_out Q x K (candidate order);
 * iters / res per query. */
int osc_corpus_gates(osc_corpus_handle h, const float* psis, int32_t Q, int32_t top_k, const int32_t* cand_in,
                     int32_t kneighbors, float row_cap, float beta, float gamma, int32_t method, float tol,
                     int32_t max_iters, int32_t clamp, int32_t* cand_out, float* gates_out, int32_t* iters, float* res);
/* osc_corpus_refine with gates (examples/rag_replacement.py:159-177, scripts/benchmark_gating_compare.py:
 * `lat = Oscillink(Y[cand], ...); lat.set_query(psi, gates=g); lat.bundle(k, alpha)`): U* of
 * M = lamG I + lamC L_sym + lamQ diag(g) with right-hand side lamG Y + lamQ g psi^T (lattice.py:245-263).  gates_in (Q x K,
 * finite and >= 0) are used as given; NULL = the diffusion gates of osc_corpus_gates (beta, gamma, method, gate_tol,
 * gate_max_iters; clamped) computed per lattice.  Out as osc_corpus_refine, plus gates_out Q x K (the gates used) and
 * gate_iters / gate_res per query (zeros for given gates).  Gates of exactly 1 give osc_corpus_refine's results bit for bit. */
int osc_corpus_refine_gated(osc_corpus_handle h, const float* psis, int32_t Q, int32_t top_k, const int32_t* cand_in,
                            const float* gates_in, float beta, float gamma, int32_t method, float gate_tol,
                            int32_t gate_max_iters, int32_t kneighbors, float row_cap, float lamG, float lamC, float lamQ,
                            float tol, int32_t max_iters, int32_t k, float alpha, int32_t* cand_out, float* gates_out,
                            int32_t* local, float* score, float* align, int32_t* iters, float* res, int32_t* gate_iters,
                            float* gate_res);
/* The loop body the reference ships with its energy receipt (examples/rag_replacement.py:48-73 and 159-184,
 * examples/diffusion_gated.py, cloud/app/main.py:1043-1063), for Q queries:
 * `lat = Oscillink(Y[cand], ...); lat.set_query(psi[, gates=g]); lat.settle(dt, settle_max_iters, settle_tol);
 *  lat.bundle(k, alpha); lat.receipt()`.  Everything osc_corpus_refine_gated takes and returns, with gate_mode 0 = no gates
 * (gates_out / gate_iters / gate_res may be NULL), 1 = diffusion gates computed per lattice, 2 = gates_in; behind the bundle
 * every lattice is settled (one implicit-Euler step from U = Y, Jacobi-PCG, each lattice stopping on its own) and its
 * receipt is taken on the device.  detail 0 = light (deltaH only; the three sums are zero, no null points), 1 = full.
 * Out per query: settle_iters / settle_res; dH, coh_sum, anchor_sum, query_sum (fp64 sums in row order, not yet rounded to
 * float32 as receipt() reports them); null_total (found) and null_offsets (Q + 1): the kept null points of query q are
 * null_i / null_j / null_z / null_r [null_offsets[q], null_offsets[q + 1]), local row ids of the candidate lattice, in row
 * order -- or, with null_cap > 0 and more found, the null_cap highest z (z descending, then row ascending; selected on the
 * device).  null_capacity >= Q * (null_cap > 0 ? min(null_cap, K) : K) entries in full detail.  z_th: 3.0 in receipt().
 * Optional (NULL skips the download of the chunk's degree and column arrays): nnz_out (Q) the lattice's stored edges,
 * edge_prefix (Q x edge_prefix_cap x 2, int64) its first (i, j) pairs in local ids, row-major, edge_prefix_n (Q) how many. */
int osc_corpus_refine_receipts(osc_corpus_handle h, const float* psis, int32_t Q, int32_t top_k, const int32_t* cand_in,
                               int32_t gate_mode, const float* gates_in, float beta, float gamma, int32_t method,
                               float gate_tol, int32_t gate_max_iters, int32_t kneighbors, float row_cap, float lamG,
                               float lamC, float lamQ, float tol, int32_t max_iters, int32_t k, float alpha, float dt,
                               int32_t settle_max_iters, float settle_tol, int32_t detail, float z_th, int32_t null_cap,
                               int32_t* cand_out, float* gates_out, int32_t* local, float* score, float* align,
                               int32_t* iters, float* res, int32_t* gate_iters, float* gate_res, int32_t* settle_iters,
                               float* settle_res, double* dH, double* coh_sum, double* anchor_sum, double* query_sum,
                               int32_t* null_total, int64_t* null_offsets, int32_t* null_i, int32_t* null_j, float* null_z,
                               float* null_r, int64_t null_capacity, int64_t* nnz_out, int64_t* edge_prefix,
                               int32_t* edge_prefix_n, int32_t edge_prefix_cap);
/* osc_corpus_refine_receipts with a chain prior on the candidate lattices -- the loop with
 * `lat.add_chain(chain, lamP, weights)` after construction and `lat.chain_receipt(chain, chain_z_th)` appended
 * (lattice.py:129-149, 466-528; graph.py:96-111; examples/quickstart.py:14-23, scripts/benchmark.py:60-83).  The superset of
 * the three refine entries: everything osc_corpus_refine_receipts takes and returns, with detail -1 = no settle and no
 * receipt (their outputs may be NULL), and the chain block: query q's chain is chain_nodes[chain_offsets[q],
 * chain_offsets[q + 1]) (chain_offsets Q + 1, from 0), local row ids of its candidate lattice, 2 .. 1024 of them, or an empty
 * range for a lattice without a chain; chain_weights NULL (ones) or one finite weight per chain edge, flat in query order
 * (query q's start at chain_offsets[q] - the number of chains before q).  Repeated nodes, revisited edges (the largest weight
 * is kept) and self-steps mean what they mean in build_path_laplacian.  One lamP >= 0 for the call.  For a lattice with a
 * chain the U* and settle operators gain lamP L_path (while lamP > 0), the Jacobi diagonal gains lamP, deltaH the path term.
 * A lattice without a chain, and one with a chain at lamP = 0, return what osc_corpus_refine_receipts returns, bit for bit.
 * Out, chain receipt from U*: chain_z_struct / chain_z_path / chain_r_struct / chain_r_path per chain edge (flat, laid out as
 * chain_weights); per query chain_gain (fp64, edge order), chain_verdict (all max(z) <= chain_z_th), chain_weakest_k (first
 * edge whose max(z) exceeds every earlier one, from -1; unwritten for a lattice without a chain when no query has one) and
 * chain_weakest_z.  If no query has a chain, the kernels of osc_corpus_refine_receipts run and no chain output is written. */
int osc_corpus_refine_chains(osc_corpus_handle h, const float* psis, int32_t Q, int32_t top_k, const int32_t* cand_in,
                             int32_t gate_mode, const float* gates_in, float beta, float gamma, int32_t method,
                             float gate_tol, int32_t gate_max_iters, int32_t kneighbors, float row_cap, float lamG, float lamC,
                             float lamQ, float tol, int32_t max_iters, int32_t k, float alpha, float dt,
                             int32_t settle_max_iters, float settle_tol, int32_t detail, float z_th, int32_t null_cap,
                             const int64_t* chain_offsets, const int32_t* chain_nodes, const float* chain_weights, float lamP,
                             float chain_z_th, int32_t* cand_out, float* gates_out, int32_t* local, float* score,
                             float* align, int32_t* iters, float* res, int32_t* gate_iters, float* gate_res,
                             int32_t* settle_iters, float* settle_res, double* dH, double* coh_sum, double* anchor_sum,
                             double* query_sum, int32_t* null_total, int64_t* null_offsets, int32_t* null_i, int32_t* null_j,
                             float* null_z, float* null_r, int64_t null_capacity, int64_t* nnz_out, int64_t* edge_prefix,
                             int32_t* edge_prefix_n, int32_t edge_prefix_cap, float* chain_z_struct, float* chain_z_path,
                             float* chain_r_struct, float* chain_r_path, double* chain_gain, int32_t* chain_verdict,
                             int32_t* chain_weakest_k, float* chain_weakest_z);
/* The candidate lattice's graph of one query (mutual_knn_adj + row_sum_cap + normalized_laplacian, graph.py:8-93) as
 * osc_get_csr gives it for `Oscillink(Y[cand])`: rowptr K + 1, col / a / w nnz (<= capacity), sqrt_deg K; local row ids.
 * Test / diagnostic aid. */
int osc_corpus_graph(osc_corpus_handle h, const float* psi, const int32_t* cand_in, int32_t top_k, int32_t kneighbors,
                     float row_cap, int32_t* cand_out, int64_t* rowptr, int32_t* col, float* a, float* w, float* sqrt_deg,
                     int64_t capacity, int64_t* nnz);

/* ---- mutable corpus ------------------------------------------------------------------------
 * Ids are row positions.  Y / Yn are allocated for `capacity` >= N rows; a bitmap of uint32 words (bit i & 31 of word
 * i >> 5 for row i, 1 = live, zero bits beyond N) says which rows take part.  A removed row keeps its id (a tombstone) until
 * osc_corpus_compact.  Everywhere above, K = min(top_k, live rows), a search returns live rows only, cand_in naming a removed
 * row is OSC_E_INVALID (the message names the query and the id), and a corpus without live rows answers every query call
 * and osc_corpus_compact with OSC_E_INVALID.  A corpus without tombstones, called without a filter, launches what it
 * launched before these entry points existed. */
/* Appends M rows (M x D, row-major) as ids N .. N + M - 1, normalised as osc_corpus_create normalises; *first_id = the first
 * new id (N for M = 0).  N + M < 2^31.  When N + M passes the capacity, Y / Yn move to max(N + M, capacity * 3 / 2) rows
 * rounded up to 128; if that allocation fails the corpus is as it was.  Synchronises before it returns. */
int osc_corpus_append(osc_corpus_handle h, const float* Y, int64_t M, int64_t* first_id);
/* Tombstones the n rows ids[]: other rows keep their ids, removed ids are not reused.  An id outside [0, N) is OSC_E_INVALID
 * and nothing changes; an id already removed is ignored.  *newly_removed = how many were live. */
int osc_corpus_remove(osc_corpus_handle h, const int32_t* ids, int64_t n, int64_t* newly_removed);
/* Row ids[j] gets the vector Y[j] (M x D, row-major, finite) for j < M: the rows are uploaded once and one kernel writes
 * Y[ids[j]] and Yn[ids[j]], normalised with osc_corpus_append's arithmetic, so every later answer is byte for byte that of
 * a corpus created over the changed rows.  Ids, tombstones, the capacity and an armed filter's meaning stay.  An id outside
 * [0, N), an id of a removed row, an id named twice or a non-finite row is OSC_E_INVALID and nothing changes.  Synchronises
 * before it returns.   */
int osc_corpus_update(osc_corpus_handle h, const int32_t* ids, const float* Y, int64_t M);
/* Drops the tombstoned rows, keeping the order of the others, and renumbers densely: Y and Yn are gathered (Yn is copied, not
 * recomputed) into fresh buffers of the live rows rounded up to 128.  new_id_of_old_or_null: N entries, the new id or -1.
 * *N_new = the new N (= the live rows).  An armed filter is dropped. */
int osc_corpus_compact(osc_corpus_handle h, int32_t* new_id_of_old_or_null, int64_t* N_new);
/* rows including tombstones, live rows, rows allocated (any may be NULL) */
int osc_corpus_rows(osc_corpus_handle h, int64_t* N, int64_t* live, int64_t* capacity);
/* the live bitmap: ceil(N / 32) words */
int osc_corpus_get_live(osc_corpus_handle h, uint32_t* words);
/* Arms a filter for the NEXT osc_corpus_search / _refine* / _gates / _graph call on this handle, which consumes and clears it
 * whether it succeeds or fails: rows = 0 clears, rows = 1 is one bitmap (the live bitmap's form, words_per_row =
 * ceil(N / 32)) for every query, otherwise rows must equal that call's Q and query q's bitmap is words[q * words_per_row ..].
 * A row is eligible iff it is live and its bit is set; the search ranks eligible rows only (cosine descending, ties to the
 * smaller id).  Every query needs at least K = min(top_k, live rows) eligible rows: otherwise that call returns
 * OSC_E_INVALID with the first such query and its count in the message, before any device work.  A filter together with
 * cand_in is OSC_E_INVALID.  A filter of all ones returns what no filter returns, bit for bit. */
int osc_corpus_filter(osc_corpus_handle h, const uint32_t* words, int32_t rows, int64_t words_per_row);
/* Arms the NEXT osc_corpus_search / _refine* / _gates / _graph call on this handle as ragged; that
 * call spends the arming whether it succeeds or fails, like the filter.  The reference's filtered loop
 * (scripts/proof_hallucination.py:203-221) builds the lattice over whichever rows pass its filter, with
 * kneighbors = min(k, rows - 1): a ragged call gives query q a lattice of n_q rows, 1 <= n_q <= K = min(top_k, live rows), at
 * the front of its K-row slot, and every output keeps its (Q, K) / (Q, min(k, K)) shape.  rows_or_null = NULL: with a filter
 * n_q = min(K, eligible rows of query q) and the candidates are all eligible rows in the search order (zero eligible rows is
 * still OSC_E_INVALID naming the query); with cand_in, row q holds n_q ids in front and -1 behind them; with neither every
 * n_q is K.  rows_or_null = Q counts (copied here): checked against cand_in's padding, or against the eligible rows.  Per query the
 * list length is min(kneighbors, n_q - 1) (a one-row lattice has no edge and sqrt_deg 1e-6), bundle picks are min(k, n_q),
 * gates_in and chain ids are read and checked below n_q only.  Behind n_q (or min(k, n_q)) the outputs hold -1 in ids
 * (cand_out, local, search ids) and 0 in values (cos, gates, score, align).  Everything a lattice returns is, byte for byte,
 * what a call over that lattice alone returns.  When every n_q is K the call runs the kernels of a call that was not armed.
 * Q < 0 clears the arming. */
int osc_corpus_ragged(osc_corpus_handle h, const int32_t* rows_or_null, int32_t Q);
/* One query's operator and solver settings: the values the reference carries per request
 * (cloud/app/models.py:8-23: Params.{lamG, lamC, lamQ, lamP, kneighbors}, SettleOptions.{max_iters, tol, dt, bundle_k}). */
typedef struct osc_corpus_setting {
  float lamG, lamC, lamQ, lamP, alpha, settle_dt, settle_tol;
  int32_t kneighbors, k, settle_max_iters;
} osc_corpus_setting;
/* Arms the NEXT osc_corpus_refine* / _gates / _graph call on this handle with one settings record per query (copied here); that
 * call spends the arming whether it succeeds or fails, like the filter and the ragged arming.  The reference builds every
 * request's lattice from the request's own settings (_build_lattice, cloud/app/main.py:887-947), overrides them per API key
 * and jitters them per request while exploring (cloud/app/learners.py:148-192), and sweeps them per query when tuning
 * (scripts/benchmark_adaptive.py:186-232): armed, any set of requests over one corpus is one batch.  Q must equal the armed
 * call's Q (otherwise that call returns OSC_E_INVALID), and the armed call ignores its own scalar arguments of the record's
 * names (lamG, lamC, lamQ, lamP, alpha, dt, settle_max_iters, settle_tol, kneighbors, k).  Per lattice of n_q rows the list
 * length is min(kneighbors[q], n_q - 1) (0 for one row) and the picks are min(k[q], n_q); the (Q, .) pick outputs are
 * max_q min(k[q], K) wide, with -1 in local and 0 in score and align behind a query's own picks.  Every record gets the
 * scalars' checks here -- lamG > 0; lamC, lamQ, lamP >= 0 and finite; kneighbors >= 1; settle_dt finite and > 0;
 * settle_max_iters >= 1; settle_tol and alpha finite -- and min(kneighbors[q], K - 1) <= 128 in the armed call, each
 * OSC_E_INVALID with the first offending query in the message.  Everything returned for query q is byte for byte what the same
 * call returns for that query alone with its settings as scalars; the per-lattice reads run even when all records are equal.
 * Q = 0 or per_query = NULL clears the arming. */
int osc_corpus_settings(osc_corpus_handle h, const osc_corpus_setting* per_query, int32_t Q);
/* the n_q of the last call on this handle that was armed by osc_corpus_ragged (proof_hallucination.py:203-221: the size is
 * whatever the filter leaves); Q must be that call's Q */
int osc_corpus_ragged_rows(osc_corpus_handle h, int32_t* rows, int32_t Q);

/* ---- receipts ------------------------------------------------------------------------------- */
/* deltaH_trace (receipts.py:10-25) on the resident U and U* */
int osc_deltaH(osc_handle h, double* dH);
/* per_node_components (receipts.py:28-60): three arrays of N entries (any may be NULL) */
int osc_receipt_components(osc_handle h, float* coh_drop, float* anchor_pen, float* query_term);
/* null_points (receipts.py:63-83), sparse restatement: per row the first argmax edge, reported iff
 * residual > 0 and z > z_th.  Output arrays hold N entries; *count rows are written in row order. */
int osc_null_points(osc_handle h, float z_th, int32_t* i_out, int32_t* j_out, float* z_out, float* r_out,
                    int32_t* count);

/* components + null points in ONE pass over the edges (what receipt() in "full" detail needs; lattice.py:320-332) */
int osc_receipt_rows(osc_handle h, float z_th, float* coh_drop, float* anchor_pen, float* query_term, int32_t* i_out,
                     int32_t* j_out, float* z_out, float* r_out, int32_t* count);

/* ---- dynamics snapshot: _compute_dynamics (lattice.py:825-927, env-gated OSCILLINK_RECEIPT_DYNAMICS) -------------- */
/* U_prev <- U on the device; call right before osc_settle (replaces the reference's `U_prev = self.U.copy()`,
 * lattice.py:213-216, without moving N x D floats to the host) */
int osc_dynamics_snapshot(osc_handle h);
/* Metrics of the step U_prev -> U_next, all on the device.  U_prev / U_next: host N x D arrays, or NULL for the
 * snapshot taken by osc_dynamics_snapshot / the resident U.
 *   move2_mean, move2_max : mean and max over nodes of ||U_next_i - U_prev_i||^2 (temperature = move2_mean)
 *   step_deltaH           : deltaH_trace(U_prev, U_next, ...) (receipts.py:10-25), chain term at any N
 *   flow_total, top_*     : per directed edge f = max(0, 0.5 lamC A_ij (||Up_i-Up_j||^2 - ||Un_i-Un_j||^2)) with
 *                           Up = U_prev/(sqrt_deg+1e-12), Un likewise; their sum and the top_cap (<= 32; the reference
 *                           keeps 16) largest in the reference's order (flow desc, then (i, j) asc)
 *   radius                : largest BFS hop distance over the lattice graph from the nodes with
 *                           sqrt(move2 + 1e-12) >= 0.1 * max (0 when nothing moved)
 * Any output pointer may be NULL. */
int osc_dynamics(osc_handle h, const float* U_prev_or_null, const float* U_next_or_null, double* move2_mean,
                 float* move2_max, double* step_deltaH, double* flow_total, int32_t top_cap, int32_t* top_i,
                 int32_t* top_j, double* top_flow, int32_t* top_n, int32_t* radius);

/* ---- measurement ---------------------------------------------------------------------------- */
/* Per-kernel HIP-event timing on the handle's own stream.  which: 0 = operator apply inside the CG loop (SpMM, the
 * CG matvec; one sample per apply = all its launches), 1 = fused x/r update, 2 = p update, 3 = kNN GEMM+top-k,
 * 4 = the initial-residual apply of a solve (same gather plus the rhs / r / p streams).  Returns samples and the
 * summed device time since the last reset.  Enabling adds two event records per sample. */
int osc_profile_enable(osc_handle h, int32_t on);
int osc_profile_reset(osc_handle h);
int osc_profile_get(osc_handle h, int32_t which, int64_t* launches, double* total_ms);

/* Counters of the handle's device paths (not timings): what the last build and the solves so far did, so that tests can
 * assert the presence or the absence of a piece of work. */
typedef struct osc_counters {
  /* the kernel shape the last blocked matvec ran with (0 = two 8-wave workgroups per CU, one gather round in flight;
   * 1..6 = one workgroup per CU, four rounds in flight, 8 / 12 / 16 / 20 / 24 / 28 row groups per wave; OSC_BLK_VARIANT
   * forces one) */
  int64_t blocked_shape;
  /* the pieces the last graph build received its anchors in (0: they were resident before it started; negative: a
   * streamed build gave up on overflowing hit lists and the whole-array build ran instead) */
  int64_t create_pieces;
  /* the main sweep of the last build's thresholds-and-hits prefilter (0: another route built the lists; 1: every rank
   * swept every column tile for its row blocks; 2: the symmetric half sweep, ONE per build whatever the world size -- the
   * ranks of a sharded build split its work items) */
  int64_t knn_sweep;
  /* the whole-array Y -> U copies made for this handle since creation (none on one GPU: U aliases Y until a settle
   * writes it) */
  int64_t y_to_u_copies;
  /* the rows -> slab-major transposes launched (k_rows_to_slab) */
  int64_t rows_to_slab_launches;
  /* the bytes the slab-major image of the anchors holds (0: not built, or dropped with the anchors, the row order or the
   * column window; OSC_ANCHOR_SLAB=0: never) */
  int64_t anchor_slab_bytes;
  /* the bytes the anchors' cached row sums W.Y hold (as many as the image once built; 0: not built, or dropped with the
   * image or the graph; OSC_ANCHOR_WY=0 or OSC_ANCHOR_SLAB=0: never) */
  int64_t anchor_wy_bytes;
  /* the INIT passes of solves from the anchors that streamed those sums instead of gathering them */
  int64_t cached_inits;
  /* 1: the rows are stored in a breadth-first order that the device kernels computed (bfs_order.hip); 0: no breadth-first
   * order, OSC_BFS_HOST=1, or the device form declined the graph (too deep for its key layout) and the host walked it */
  int64_t bfs_on_device;
} osc_counters;
int osc_counters_get(osc_handle h, osc_counters* out);

/* ---- multi-GPU (one process per GPU, RCCL over xGMI) ---------------------------------------- */
/* Column-sharded CG: every rank holds the whole graph and the column slab [c0, c1) of the N x D state;
 * alpha/beta are per column (solver.py:22-36) so the only exchange per iteration is one
 * all-reduce(max) of the stop-test residual.  id is an ncclUniqueId (128 bytes) made by rank 0
 * with osc_comm_unique_id and distributed by the caller. */
int osc_comm_unique_id(char id_out[128]);
/* version code of the RCCL this library is linked against (ncclGetVersion, e.g. 22203 = 2.22.3); touches no device.
 * A bench line carries it so that a scaling record says which collective library produced it. */
int osc_comm_backend_version(int32_t* version);
/* An id for the in-process LOOPBACK backend instead: the ranks are threads of ONE process, each with its own handle on
 * the same GPU, and every collective is device-to-device copies between host barriers.  It runs the multi-rank code
 * paths (unequal column slabs, row-block / halo exchanges, the sharded kNN list all-gather, speculative iterations
 * around collectives) at world > 1 on a single MI355X, where RCCL refuses two ranks on one device.  Test backend:
 * every collective blocks the calling thread until all ranks of the group have entered it (60 s limit, then
 * OSC_E_COMM on every rank; OSC_LOOPBACK_TIMEOUT_S overrides). */
int osc_comm_loopback_id(char id_out[128]);
/* Joins the communicator the id names (RCCL or loopback).  Sets this rank's column window (column-sharded CG, the
 * default) or keeps all columns (OSC_SHARD=row: row-sharded CG).  Collective for RCCL ids. */
int osc_comm_init(osc_handle h, const char id[128], int32_t rank, int32_t world);
int osc_comm_shard(osc_handle h, int32_t* c0, int32_t* c1);
/* rank / world (0 / 1 without a communicator), shard_mode 0 = column-sharded CG, 1 = row-sharded; kind_out receives
 * "none", "rccl" or "loopback" */
int osc_comm_info(osc_handle h, int32_t* rank, int32_t* world, int32_t* shard_mode, char* kind_out, int32_t cap);
/* Row-sharded CG only (OSC_SHARD=row): the halo of this rank -- need_rows = off-partition rows its lattice rows (and
 * chain) reference, i.e. the rows of the search direction it receives every iteration; need_rows_max = the largest
 * such count over the ranks; remote_rows = N - own rows; bytes_per_iteration = inbound bytes of one exchange;
 * full_exchange != 0: the lists cover more than 70 % of the remote rows on some rank (unstructured graph), so whole
 * row blocks are exchanged instead (OSC_HALO=lists|full forces either).  Builds the plan on first use per graph:
 * COLLECTIVE (every rank must call it), OSC_E_STATE without a row-sharded communicator. */
int osc_halo_info(osc_handle h, int64_t* need_rows, int64_t* need_rows_max, int64_t* remote_rows,
                  int64_t* bytes_per_iteration, int32_t* full_exchange);
/* Drains the handle's stream, then all-reduces n host doubles in place over the handle's communicator (op 0 = sum,
 * 1 = max); n = 0 is a pure barrier.  Without a communicator: stream drain only.  What a benchmark harness needs for
 * "barrier + max over ranks" without any other distributed runtime. */
int osc_comm_allreduce_f64(osc_handle h, double* vals, int32_t n, int32_t op);

#ifdef __cplusplus
}
#endif
#endif /* OSCILLINK_HIP_H */

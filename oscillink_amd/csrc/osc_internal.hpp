// Internal header of liboscillink_hip.so's host side: the handle (struct osc_lattice), the error types the C ABI maps to
// status codes, and the functions the translation units share.  Round 5 cut osc_api.hip (3 500 lines) along its seams:
//   osc_runtime.hip : process-wide pools (streams, device and pinned host memory, staging buffers, control blocks),
//                     host <-> device transfers, profiling events, per-handle scratch
//   osc_graph.hip   : lattice build orchestration (graph.py:8-93 on the device), chain prior, internal row order
//   osc_solve.hip   : operator parameters, apply plans, the CG drivers (one GPU, column windows, row-sharded + halo lists)
//   osc_anchor_build.hip : the builders of the anchor-start chain's levels (derived_state.hpp: Level)
//   osc_api.hip     : environment switches and the extern "C" entry points of include/oscillink_hip.h
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/oscillink_hip.h"
#include "common.hpp"
#include "host_logic.hpp"
#include "derived_state.hpp"
#include "comm.hpp"
#include "knn.hpp"
#include "knn_gemm.hpp"
#include "append.hpp"
#include "append_plan.hpp"
#include "remove.hpp"
#include "remove_plan.hpp"
#include "update.hpp"
#include "update_plan.hpp"
#include "receipts.hpp"
#include "perm.hpp"
#include "dynamics.hpp"
#include "small.hpp"
#include "query.hpp"
#include "gates_many.hpp"
#include "bundle_gated.hpp"
#include "receipt_gated.hpp"
#include "chain_gated.hpp"
#include "chain_prior_plan.hpp"
#include "bundle_prior_plan.hpp"
#include "receipt_prior_plan.hpp"

using namespace osc;

struct ProfSlot {
  hipEvent_t a, b;
  int which;
  int iter;  // CG iteration the launch belongs to (0 = not part of a CG loop); speculative no-ops are dropped
};

struct Invalid : std::runtime_error {
  using std::runtime_error::runtime_error;
};
struct StateError : std::runtime_error {
  using std::runtime_error::runtime_error;
};
struct Unsupported : std::runtime_error {
  using std::runtime_error::runtime_error;
};

// per device like the streams
struct CtrlBlock {
  float* res_host = nullptr;
  size_t res_host_n = 0;
  std::vector<hipEvent_t> events;
};

hipStream_t acquire_stream(int device);
void release_stream(int device, hipStream_t s);
double now_ms();

struct osc_lattice {
  int device = 0;
  hipStream_t stream = nullptr;
  int64_t N = 0;
  int32_t D = 0, ld = 0;
  // state (N x ld, row-major)
  DevBuf<float> Y, U, X, R, P, AP, Ustar;
  // U is bit-for-bit Y and U's buffer holds nothing yet (the state right after construction and after osc_set_U(NULL)):
  // readers go through u_read(), the first settle writes U.  Cleared by osc_set_U(ptr) and at the successful end of a settle.
  bool u_is_y = false;
  // slab-major image of the anchors over the handle's window (the layout launch_rows_to_slab writes), built on first use
  // by a blocked INIT pass that starts from Y and kept until Y's device copy, the row order or the window changes (OSC_ANCHOR_SLAB=0: never built)
  DevBuf<float> Ys;
  bool anchor_slab = true;
  // The anchors' row sums W.Y, slab-major like Ys: exactly what the gathering INIT pass of a solve that starts from Y has in
  // hand when its rows are complete.  Written by that pass as a by-product (run_cg), then every later anchor start on this
  // graph copy streams its INIT pass (k_init_cached) instead of gathering.  The sums depend on Y, the graph and the slot
  // placement of the block-major copy (derived_state.hpp: anchor_wy).  OSC_ANCHOR_WY=0 or OSC_ANCHOR_SLAB=0: never built.
  DevBuf<float> WYs;
  bool anchor_wy = true;
  int64_t cached_inits = 0;  // INIT passes served from WYs (osc_counters::cached_inits)
  // The anchors' second row sums W.(W.Y) (row-major) and the rows' weight sums W.1: with them the cached INIT pass of an anchor
  // start under uniform gates also emits iteration 1's A p (k_init_cached_ap) and that iteration's gathering matvec is not
  // launched.  Built from WYs on the first solve that takes the route (a lattice's second anchor start), valid exactly as
  // long as WYs (Level::wwy).  OSC_ANCHOR_AP: 0 never, 1 wherever the cached INIT runs, unset: by the lattice's rows
  // (host_logic.hpp: anchor_ap_route).
  DevBuf<float> WWs, Wsum;
  bool gates_uniform = true;      // B holds one value (osc_set_query scans the gates it is handed)
  // One level further (host_logic.hpp: anchor_ap2_route): the anchors' third row sums W.(W.(W.Y)) (row-major), W.(W.1) and the
  // scratch array T = A (A p1) the INIT pass fills; iteration 2's p update then forms A p2 and that iteration launches no
  // matvec either.  Built from WWs / Wsum on the first solve that takes the route -- the anchor start that built WWs, or the
  // first one after OSC_ANCHOR_AP2 allows it -- and valid exactly as long as they are (Level::w3).  OSC_ANCHOR_AP2: 0
  // never, 1 wherever the depth-1 route runs, unset: by the lattice's rows.
  DevBuf<float> W3s, Wsum2, Tap;
  // Further still (host_logic.hpp: anchor_gram_route): the float64 Gram sums of the seven vectors iterations 1 and 2 are
  // combinations of (anchor_gram.hpp; (22 ld + 6) doubles).  With them k_anchor_gram_scalars has both iterations' alpha, beta
  // and residuals before any N x D pass, and k_init_two_steps runs both iterations inside the INIT pass.  Built by the first
  // solve that takes the route, valid exactly as long as W3s (Level::gram).  OSC_ANCHOR_GRAM: 0 never, 1 wherever the
  // depth-2 route runs, unset: by the lattice's rows.
  DevBuf<double> gram;
  DevBuf<uint32_t> gram_go;  // the fused pass's gate word, iteration 3's and the folded last form's (GramScalarArgs::go)
  // The form of that pass (launch_init_two_steps), same bits either way.  OSC_TWO_STEPS: stream (unset) -- the update kernels'
  // launch geometry -- or blocked, the matvec's: the reference form.
  bool two_steps_stream = true;
  // One iteration further (host_logic.hpp: anchor_gram3_route): the sums of the two vectors A p3 adds to the seven -- psi s3, s3 =
  // W.(W.(W.1)), and W.(W3s), formed once into the solve's AP scratch array, summed against and dropped (anchor_gram.hpp; (13 ld +
  // 4) doubles and the N floats of s3 are held).  With them k_anchor_gram_scalars also has alpha3, beta3 and |r3|, and iteration 3
  // is one launch (k_apply_blocked's FUSED form).  Built by the first solve that takes the route, valid exactly as long as gram
  // (Level::gram3).  OSC_ANCHOR_GRAM3: 0 never, 1 wherever the Gram route runs, unset: by the lattice's rows.
  DevBuf<double> gram3;
  DevBuf<float> Wsum3;
  // One level of scalars further (host_logic.hpp: anchor_gram4_route): the sums of the two vectors A p4 adds -- psi s4, s4 = W s3,
  // and W^5 Y; W^4 Y and W^5 Y are formed once into two of the solve's scratch arrays, summed against and dropped (anchor_gram.hpp;
  // (16 ld + 5) doubles are held).  With them k_anchor_gram_scalars also has alpha4 and |r4|, and a solve that ends in iteration 4
  // writes x4 in iteration 3's fused matvec (FUSED_LAST) and launches nothing for iteration 4.  Built by the first solve that plans
  // the route, valid exactly as long as gram3 (Level::gram4).  OSC_ANCHOR_GRAM4: 0 never, 1 wherever the three-step route
  // runs, unset: by the lattice's rows.
  DevBuf<double> gram4;
  // The form of such a solve's one matvec.  Folded (unset): the INIT pass, which runs behind alpha3, beta3 and alpha4, stores e = x4
  // less the term in the gathered row sum in x's place and no r2, and the matvec's epilogue is one fmaf on the row of e
  // (k_apply_blocked, FMODE == 3).  OSC_GRAM4_FOLD=0: the INIT pass stores x3, r2, p3 and the epilogue forms r3, p4 and x4
  // (FUSED_LAST), the reference form -- also the form of a solve that ends in iteration 4 behind another prediction (run_cg:
  // two_steps).  After a folded solve the R array holds nothing defined.
  bool gram4_fold = true;
  int64_t folded_four_step_solves = 0;
  // The polynomial last form (host_logic.hpp: anchor_poly_route): W^4 Y, which the pass that forms gram4 computes anyway, is kept
  // (row-major N x ld like W3s; the memory rule of WWs, a denial remembered until WYs is formed anew; Level::w4),
  // and a solve predicted and shown to end in iteration 4 is the scalars kernel and one elementwise pass over Ys, WYs, WWs, W3s and
  // W4s with nine coefficients a column (poly_coef).  After such a solve R, P and AP hold nothing defined.  OSC_ANCHOR_POLY: 0
  // never, 1 wherever the folded form would run, unset: by the lattice's rows.
  DevBuf<float> W4s, poly_coef;
  int anchor_poly_max_mb = -1;  // OSC_ANCHOR_POLY_MAX_MB: W4s is kept only if it is no larger than this many MiB (unset: the free memory alone decides)
  // What the handle keeps per level of that chain (derived_state.hpp: Level; wy's record stays unused: anchor_wy and cached_inits
  // above).  mode: the level's OSC_ANCHOR_* switch (0 never, 1 wherever the level below runs, < 0 by the lattice's rows); denied:
  // its arrays did not fit (asked again once WYs is formed anew); last: the last general-path solve took its route; solves: the
  // solves that took it (wwy: streamed first applies, w3: streamed second applies, gram / gram3 / gram4: fused two- / three- /
  // four-step solves, w4: polynomial four-step solves); builds, redos: times its arrays were formed / a solve on its route was
  // gated off and run again.
  struct AnchorLevel {
    int mode = -1;
    bool denied = false, last = false;
    int64_t solves = 0, builds = 0, redos = 0;
  };
  AnchorLevel anchor[host::kLevels];
  AnchorLevel& at(host::Level l) { return anchor[(unsigned)l]; }
  const AnchorLevel& at(host::Level l) const { return anchor[(unsigned)l]; }
  int64_t yu_copies = 0;    // whole-array Y -> U copies made for this handle (osc_counters::y_to_u_copies)
  int64_t slab_launches = 0;  // k_rows_to_slab launches (osc_counters::rows_to_slab_launches)
  // Which of the arrays computed from other state (ell_col_t / ell_w_t, blk_*, Ys, WYs, Ustar; by epoch: halo, query) are
  // current.  Dropped by host::changed(derived, <what changed>) alone (derived_state.hpp has the dependency table).
  host::Derived derived;
  DevBuf<float> Uprev;  // state before the last settle (dynamics snapshot, lattice.py:825-927); allocated on first use
  bool have_uprev = false;
  DevBuf<float> B, psi;
  float lamG = 1.0f, lamC = 0.5f, lamQ = 4.0f;
  // graph (ELL)
  int32_t k_eff = 0;
  float row_cap = 1.0f;
  int deterministic = 0;
  int64_t seed = -1;
  bool have_graph = false;
  int32_t width = 0;
  DevBuf<int32_t> ell_col, deg;
  DevBuf<float> ell_a, ell_w, sqrt_deg;
  DevBuf<float> knn_val;
  DevBuf<int32_t> knn_idx;
  int32_t knn_k = 0;
  int32_t knn_fallback_rows = 0;  // rows of the last build the prefilter could not prove and the exact kernel redid
  KnnBuildPlan knn_last;          // the route of the last build (knn_plan.hpp: plan_knn_build)
  // The builds seeded from a base's kept lists: osc_create_appended, osc_create_removed, osc_create_updated (DESIGN.md
  // sections 14.1, 14-16).  k_requested: k as asked for at creation / the last rebuild, before the clamp to N - 1.
  // score_family: which arithmetic the kept lists' values come from (host::AppendFamily; from the build's route, inherited by
  // a seeded handle).  list_seed: set only while a handle is being built from a base's lists (build_graph_once takes its seeded
  // branch then; create_handle alone sets it).  made: how the handle came to be, what osc_append_info / osc_remove_info /
  // osc_update_info report -- each its own kind, zeros otherwise.
  int32_t k_requested = 0;
  int32_t score_family = 0;
  enum class SeedKind : int32_t { none = 0, append, remove, update };
  struct Seed {
    SeedKind kind = SeedKind::none;
    const osc_lattice* base = nullptr;  // its anchors and lists are read, nothing of it is written
    bool forced = false;                // mode 1: the planner's thresholds do not apply
    bool seed_lists = false;            // the base's lists seed the build (else only its anchors are taken over)
    int64_t n_old = 0;                  // rows of the base
    std::vector<int32_t> row_map;       // per base row.  remove: its row here, -1 for a removed row (host::remove_map);
                                        // update: its own id, -1 for a replaced row (host::update_ids)
    std::vector<int32_t> old_of_new;    // remove: per row here, its base row
    std::vector<int32_t> fresh;         // ascending: the appended rows n_old .. N - 1, none, the replaced rows
    const int32_t* ids_as_given = nullptr;  // update: the replaced rows in the order of the new vectors (the caller's array)
  };
  const Seed* list_seed = nullptr;
  int64_t append_scratch_bytes = host::kAppendScratchBytes;  // budget of one chunk's score block (OSC_APPEND_SCRATCH_MB)
  struct SeedInfo {
    SeedKind kind = SeedKind::none;
    int32_t route = 0;  // host::AppendRoute
    int64_t fresh_rows = 0;    // rows appended / replaced
    int64_t removed_rows = 0;
    int64_t kept_rows = 0;     // listed rows that neither were recomputed nor are fresh: append's and update's merged rows
    int64_t redo_rows = 0, merge_hits = 0, scan_bytes = 0;
    int32_t denied = 0;
    double score_ms = 0, merge_ms = 0, back_ms = 0;
  } made;
  double build_ms = 0.0;
  int64_t nnz = 0;
  int32_t max_deg = 0;
  // internal row order (empty = identity): API row i lives at device row inv_h[i]; perm_h[new] = old
  int reorder = -1;        // OSC_REORDER: 0 never, 1 always, unset = auto (when the graph is clustered enough to pay)
  double clustering = 0.0;  // sampled local clustering coefficient of the last graph
  bool reordered = false;   // the stored order is the BFS order (selects the deep kernels and the BFS block rule; order_kind == 1)
  // Which order the rows are stored in: 0 the API's, 1 BFS, 2 balanced source blocks (block_balance.hpp: every row's
  // neighbours spread over the blocked matvec's source blocks; the graph keeps no locality, so nothing BFS-specific applies).
  int order_kind = 0;
  bool bfs_on_device = false;  // order_kind == 1 and the device kernels computed that order (osc_counters::bfs_on_device)
  int balance = -1;        // OSC_BALANCE: 0 never, 1 wherever the apply plan has source blocks, unset = auto (maybe_reorder)
  bool balance_host = false;  // OSC_BALANCE_HOST=1: the host reference computes the order (A/B, tests)
  int64_t displaced_before = 0, displaced_after = 0;  // displaced edges of the last balanced order: API order / stored order
  int32_t balance_rounds = 0, balance_nb = 0;
  bool balance_on_device = false;  // the device kernels computed the last balanced order (false: the host reference did)
  double balance_ms = 0.0;  // search + state move of the last balanced order
  std::vector<int32_t> perm_h, inv_h;
  DevBuf<int32_t> perm_d, inv_d;
  // chain prior (kept in API ids on the host so it can be re-installed after a re-order)
  std::vector<int32_t> chain_nodes;
  std::vector<float> chain_w;
  bool chain_present = false;
  float lamP = 0.0f;
  int32_t prows = 0, pwidth = 0;
  DevBuf<int32_t> path_slot, pcol, pdeg, prow;  // prow: lattice row of path row s (inverse of path_slot)
  DevBuf<float> pw;
  // CG scratch
  int grid_cap = 1024;
  DevBuf<float> vec_q, vec_n;  // query / per-row result scratch of the cosine calls
  int32_t dcols = 0;      // D rounded up to 4: the columns the kernels work on (ld >= dcols is the row pitch)
  // the operator-apply plan's forcing switches (host_logic.hpp: plan_apply)
  int spmm_xs = -1;        // XCD-affine narrow slabs: -1 auto, 0 off, 1 on (OSC_SPMM_XS)
  int xs_nb = 0;           // workgroups per XCD in that mode; 0 = automatic (OSC_XS_NB)
  DevBuf<float> part0, part1, alpha, beta;
  DevBuf<double> rz, colsum;
  DevBuf<uint32_t> res_bits;  // residual slots of the row-sharded solve
  // Zeroed control words of the solves (residual slots, arrival counters): a ring of segments, one per solve, cleared all
  // at once when it wraps -- hipMemsetAsync costs ~15 us of HOST time per call on this stack, during which the device
  // sits idle at the start of a solve (7 % of a settle at N = 20000, D = 128; a quarter of one at N = 80)
  DevBuf<uint32_t> ctrl_ring;
  size_t ctrl_seg = 0;   // words per segment
  int ctrl_next = 0;     // next free segment
  bool small_path = true;             // OSC_SMALL_PATH=0 disables the one-launch CG for small lattices
  bool fake_window = false;  // OSC_FAKE_COL_SHARD under a one-rank communicator (measurement hook; reported by osc_comm_info)
  // build-route switches (read_env): every OSC_* variable the library reads per handle is read in ONE place, at
  // osc_create and again at osc_rebuild_graph (INTEGRATION.md has the table)
  KnnBuildInputs knn_env;      // OSC_KNN_* / OSC_CREATE_*: the kNN planner's switch inputs (knn_plan.hpp)
  bool receipt_pair = true;  // OSC_RECEIPT_PAIR=0: the receipt's per-edge pass from both ends of every edge (one launch)
  bool create_force_retry = false;  // OSC_CREATE_FORCE_RETRY (test hook): a streamed build always hands over to the whole-array one
  int32_t create_pieces = 0;   // pieces the last build received its anchors in (0: they were on the device before it started)
  int halo_force = 0;          // OSC_HALO: 1 full, 2 lists
  bool bfs_host = false;       // OSC_BFS_HOST=1: the breadth-first row order is walked on the host (A/B, tests)
  int fake_col_r = 0, fake_col_w = 0;  // OSC_FAKE_COL_SHARD "r/w"
  int predicted_iters[3] = {0, 0, 0};  // iterations the last general-path solve of each kind (CgBuffers::kind) took (0 = unknown)
  bool x_defer = true;                // the x update rides in the next iteration's p update (run_cg; OSC_X_DEFER=0: beside the r update)
  bool x_last_form = true;            // ... and the expected last iteration finishes x itself without storing r (OSC_X_DEFER=2: off)
  // The ring of kept search directions (run_cg; host_logic.hpp: plan_x_ring): up to three arrays beside P, and the alpha
  // vectors of the kept iterations.  Scratch like P and AP: nothing in them outlives a solve, they stay with the handle.
  DevBuf<float> xring[3], alpha_ring;
  int x_ring_force = -1;              // OSC_X_RING: 0 off, 2..4 that many slots, unset: by the planner
  int x_ring_k = 1;                   // slots of the last general-path solve (1: no ring), its gated flushes and all its x passes
  int64_t x_ring_flushes = 0, x_ring_passes = 0;
  DevBuf<int32_t> ell_col_t;          // transposed ELL for the one-launch path (built on first use per graph)
  DevBuf<float> ell_w_t;
  // block-major copy of the graph for the source-blocked CG matvec (k_spmm_blocked), built on first use per graph
  DevBuf<int2> blk_slots, blk_rest, blk_over;
  int spmm_blocked = -1;   // < 0 by lattice size, 0 off, > 0 = that many source blocks (OSC_SPMM_BLOCKED)
  int blk_variant = -1;    // kernel shape of the blocked matvec (kBlkShapes); -1 = by geometry, OSC_BLK_VARIANT forces one
  mutable int blk_resident[kBlkShapeCount] = {-1};  // workgroups per XCD each shape gets resident ([0] < 0: not queried yet)
  host::ApplyPlan last_plan;  // the apply plan of the last general-path solve (osc_apply_info, osc_counters::blocked_shape)
  double temporal_mb = 200.0;  // largest solve (5 arrays x N x window) whose update kernels use ordinary instead of nontemporal accesses
  bool spmm_deep = true;   // re-ordered lattices: the operator apply with 8 gathers in flight per row (OSC_SPMM_DEEP=0: the usual 2)
  bool blk_init = true;    // the initial residual goes through the blocked matvec as well (OSC_BLK_INIT=0: plain INIT apply)
  bool blk_init_fused = true;  // ... and is formed in that launch's epilogue where it can be (OSC_BLK_INIT=2: separate finish pass)
  int64_t blk_applies = 0; // blocked matvecs enqueued since creation
  int64_t small_solves = 0;
  float* res_host = nullptr;  // pinned, host-mapped mirror of res_bits for the per-iteration read-back
  float* res_host_dev = nullptr;  // the device's address of it
  size_t res_host_n = 0;
  std::vector<hipEvent_t> iter_events;
  // sharded solves: the stop test's all-reduce runs on a second stream beside the next iteration's p update and matvec
  // (run_cg); step_events[it] = "iteration it's local residual is out" (OSC_COMM_OVERLAP=0: all-reduce in the solve's stream)
  hipStream_t comm_stream = nullptr;
  std::vector<hipEvent_t> step_events;
  int comm_overlap = -1;  // 1 / 0: always / never; -1: from four ranks on (run_cg)
  bool comm_stream_busy = false;  // a solve left work on comm_stream (at most a speculative iteration's all-reduce + publish)
  std::vector<float> history;
  // column shard (multi-GPU, column-sharded CG); single GPU: [0, ld)
  int32_t c0 = 0, c1 = 0;
  std::unique_ptr<Comm> comm;  // RCCL (one process per GPU) or the in-process loopback (comm.hpp)
  int rank = 0, world = 1;
  bool u_sharded = false;  // U holds only this rank's columns (after a sharded settle)
  int shard_mode = 0;      // 0 = column-sharded CG (default), 1 = row-sharded CG (north-star wording; OSC_SHARD=row)
  int fake_row_shards = 0; // test hook (OSC_ROW_FAKE_SHARDS=V): V row shards on this one GPU, collectives local
  DevBuf<double> sums;     // [2][ld] completed column sums of the row-sharded CG
  DevBuf<float> comm_buf;
  // halo plan of the row-sharded CG (built on first use per graph / chain / communicator: derived.epoch)
  struct HaloPlan {
    uint64_t epoch = 0;                      // derived.epoch it was built for (0 = none)
    bool full = false;                       // halo ~ everything: exchange whole row blocks instead (all-gather)
    std::vector<int64_t> give_off, need_off; // [world + 1] offsets of each peer's slice in give_idx / need_idx
    DevBuf<int32_t> give_idx, need_idx;      // my rows each peer needs (sorted) / the peers' rows I need (sorted)
    DevBuf<float> send, recv;                // packed rows
    int64_t need_rows = 0, give_rows = 0;    // this rank
    int64_t need_rows_max = 0;               // max over ranks
  } halo;
  // profiling
  bool prof_on = false;
  std::vector<ProfSlot> prof_pending;
  std::vector<hipEvent_t> prof_pool;
  int64_t prof_count[5] = {0, 0, 0, 0, 0};
  double prof_ms[5] = {0, 0, 0, 0, 0};
  // multi-query bundles (osc_query.hip): the query basis M X = lamG Y, M x = lamQ B of the graph / gates / chain / lams it
  // was solved for (the caller keys it; a new derived.epoch drops it), its per-row constants and the batch scratch
  struct QueryState {
    bool have = false;
    uint64_t epoch = 0;        // derived.epoch of the basis
    float scale = 0.f;         // |psi|_inf the x part was solved for (its residual target is tol / (2 scale))
    DevBuf<float> X, x4;       // N x ld, N x 4 (column 0 = x)
    DevBuf<double> s;          // [N] x / (sd + 1e-12)
    DevBuf<double> xn2, c0, c2;
    DevBuf<float> Yn;          // row-normalised anchors (the MMR's representers)
    uint64_t yn_epoch = 0;
    DevBuf<float> zero_psi;    // [ld] zeros: the psi of the X solve
    DevBuf<float> Bt;          // [query_qpad(chunk) x kpad] GEMM operand
    DevBuf<float> align, pm, cs;  // N x qs: alignment; p, then the MMR's running maxima; coh, then the score
    DevBuf<double> pn2, pinv, pval;
    DevBuf<double2> part, stats;
    DevBuf<int32_t> pid, prow, chosen_api, chosen_row;
    DevBuf<float> out_score, out_align;
    // receipt_many: per-basis terms, kept until the next basis solve or extension (gen)
    uint64_t gen = 0;            // bumped by every basis solve
    uint64_t rm_gen = 0;         // gen of Mx and the per-basis sums below
    uint64_t rd_gen = 0;         // gen of dslot
    DevBuf<double> Mx;           // [N] M x
    DevBuf<float> dslot;         // [N * width] |P_i - P_j|^2 per ELL slot
    std::vector<double> rm_vec;  // 4 x D: sum x_i (X_i - Y_i), sum B_i (x_i - 1) X_i, then the column sums of a0 and b0
    double rm_a0 = 0, rm_b0 = 0, rm_a2 = 0, rm_b2 = 0, rm_h2 = 0;
    DevBuf<double> rpart, rspart, rsum, rfin, cohpart, cohfin;
    DevBuf<float> U0, rz, rr, zt, roz, ror;  // U0: X + x psi0^T; rz / rj / rr: N x qs candidates; zt: qs x N
    DevBuf<int32_t> rj, rtot, rsel, roi, roj;
    DevBuf<int64_t> roff;
    // chain_receipt_many: one chunk's queries, units, path entries and results; nothing is kept
    DevBuf<float> cm_psi, cm_pa, cm_edge, cm_wz;
    DevBuf<host::ChainManyUnit> cm_units;
    DevBuf<int32_t> cm_pcol, cm_eoff, cm_verdict, cm_wk;
    DevBuf<double> cm_term, cm_gain;
    // osc_chain_prior_many.  res_X / res_x: the resident basis's residuals, |r_X| and |r_x| of the
    // unscaled x.  shifted: the basis of M + lamP I in a slot of its own, X' stored scaled by lamG / (lamG + lamP); epoch-keyed
    // like the first, and by lamP; max_X / max_x = max |X'| / max |x'| (the Green's columns' stop is derived from them).
    float res_X = 0.f, res_x = 0.f;
    struct Shifted {
      bool have = false;
      uint64_t epoch = 0;
      float lamP = 0.f, scale = 0.f;
      DevBuf<float> X, x4;
      float res_X = 0.f, res_x = 0.f, max_X = 0.f, max_x = 0.f;
      // osc_bundle_prior_many: k_query_basis_stats of (X', x'), kept until the next solve (gen).
      // gen is bumped by every shifted solve or extension; a new epoch or lamP forces a solve first, so it keys the constants
      // as (epoch, lamP) would -- at the cost that an x-only extension also recomputes c0 and |X'|^2, which did not change.
      uint64_t gen = 0, stats_gen = 0;
      DevBuf<double> s;
      DevBuf<double> xn2, c0, c2;
      // osc_receipt_prior_many: section 12's per-basis terms on (X', x') and M', under the same gen
      uint64_t rm_gen = 0, rd_gen = 0;
      DevBuf<double> Mx;           // [N] M' x'
      DevBuf<float> dslot;         // [N * width] |P'_i - P'_j|^2 per ELL slot
      std::vector<double> rm_vec;  // 4 x D, as QueryState's
      double rm_a0 = 0, rm_b0 = 0, rm_a2 = 0, rm_b2 = 0, rm_h2 = 0;
      DevBuf<double> rp_base;      // one call's [8 scalars | h1' | a1 | b1] for k_rp_scalars
    } shifted;
    DevBuf<char> cp_scratch;     // one pass's panels and per-column scalars (chain_prior_plan.hpp: ChainPriorLayout)
    DevBuf<float> cp_diag;       // [N] d_i = lamG + lamP + lamC + lamQ B_i
    DevBuf<int32_t> cp_ints;     // one pass's systems and per-query indices
    DevBuf<int64_t> cp_longs;
    DevBuf<float> cp_flts, cp_tv;
    DevBuf<double> cp_T;
  } query;
  std::string err;

  ~osc_lattice() {
    for (auto& s : prof_pending) {
      (void)hipEventDestroy(s.a);
      (void)hipEventDestroy(s.b);
    }
    for (auto e : prof_pool) (void)hipEventDestroy(e);
    if (comm_stream && comm_stream_busy) (void)hipStreamSynchronize(comm_stream);
    for (auto e : step_events) (void)hipEventDestroy(e);
    park_ctrl();
    release_stream(device, comm_stream);
    release_stream(device, stream);
  }
  void park_ctrl();
};

using L = osc_lattice;

constexpr size_t kStageBytes = (size_t)32 << 20;  // one pinned staging buffer (two per StagePair)
struct StagePair {
  void* buf[2] = {nullptr, nullptr};
  hipEvent_t ev[2] = {nullptr, nullptr};
};

struct CgBuffers {  // the arrays one solve works on (all N x ld)
  const float* x0;  // gathered in INIT
  float* X;
  float* R;
  float* P;
  float* AP;
  const float* rhsU;
  const float* rhsY;
  const float* B;
  const float* psi;
  int32_t ld, c0, c1;
  // When X aliases x0 / rhsU (the in-place warm-started settle), a path that cannot guarantee it completes -- the
  // one-launch small kernel may give up at its barrier -- writes here instead and reports it in CgResult::sol, so a
  // failed attempt never leaves the caller's state partly advanced.  nullptr: X is never aliased.
  float* Xalt = nullptr;
  // x0 is the anchors and X holds nothing yet (the settle from an aliased U): the INIT pass of the general path writes
  // no copy of x0 into X; the launch that applies iteration 1's x update reads x from x0 instead (run_cg)
  bool defer_x0 = false;
  int kind = 0;  // 0 settle, 1 U*, 2 single right-hand side: repeated solves of one kind take the same iteration count
};

struct CgResult {
  int iters;
  float res;
  float* sol = nullptr;  // the buffer that holds the solution (b.X, or b.Xalt)
};

struct RowShard {
  int64_t r0, r1;
};

hipEvent_t prof_event(L& h);
void prof_drain(L& h, bool nothrow = false);
void use_device(L& h);
void sync(L& h);
int64_t device_free_bytes();  // of the current device
void upload_rows(L& h, float* dst, const float* src);
StagePair acquire_stage(int device);
void release_stage(int device, const StagePair& sp);
void* host_pool_alloc(size_t bytes);
bool host_pool_free(void* p);
bool host_pool_owns(const void* p, size_t bytes);
void parallel_copy(char* dst, const char* src, size_t bytes, int threads);
void download_contiguous(L& h, char* dst, const char* src, size_t bytes);
void download_rows(L& h, float* dst, const float* src);
void to_api_order(const L& h, float* v);
void download_api_order(L& h, float* dst, const float* src);
void drain_comm_stream(L& h);
uint32_t* ctrl_segment(L& h, size_t words);
void ensure_ctrl(L& h, size_t slots);
// A word of the host-mapped mirror (L::res_host) the device has yet to publish: never a residual (those are sqrt(...) >= 0
// or a canonical NaN) nor a status.  poll_host_word spins on such a word and returns its first other value; `second`:
// nullptr, or the stream the word comes out of where that is not the handle's (queried as well); `what` names the word in
// the errors (HipError: the streams finished without publishing it, or 120 s passed).
constexpr uint32_t kCtrlPending = 0xFFFFFFFFu;
uint32_t poll_host_word(L& h, volatile uint32_t* word, hipStream_t second, const char* what);
void ensure_cg_scratch(L& h, int max_iters);
int cg_grid(const L& h);
int blocked_quad_form(L& h, const host::ApplyPlan& plan, const OpParams& op, const float* x_rows, float* scratch_slab,
                      float* scratch_out, bool with_path, const float* x_sub = nullptr);  // x_sub: the form of x_rows - x_sub
GraphView graph_view(L& h, bool with_path);
void graph_counts(L& h);
void alloc_ell(L& h, int32_t width);
bool permuted(const L& h);
void install_chain(L& l);
void move_state(L& l, const int32_t* from_d, const int32_t* relabel_d);
void drop_order(L& l);
void apply_order(L& l, const std::vector<int32_t>& perm);
std::vector<int32_t> bfs_order(L& l);
void maybe_reorder(L& l);
void exchange_buckets(L& h, const KnnPanelPlan& pp, const KnnPanelSymDev& sd, int rb_per);
void build_graph(L& h, const float* host_Y = nullptr);
bool path_active(const L& h);
OpParams settle_op(const L& h, float dt, int precond);
OpParams ustar_op(const L& h);
host::ApplyPlan apply_plan(const L& h, int32_t c0, int32_t c1, int32_t ld, bool with_path);
BlockedView blocked_view(L& h, int nb);
void spmm_slabbed(L& h, const host::ApplyPlan& plan, int mode, SpmmArgs sa, int grid, int iter = 0);
bool run_cg_small(L& h, const OpParams& op, const CgBuffers& b, bool with_path, int max_iters, float tol,
                  CgResult& out);
CgResult run_cg(L& h, const OpParams& op, const CgBuffers& b, bool with_path, int max_iters, float tol);
void gather_columns(L& h, float* arr);
std::vector<RowShard> row_shards(const L& h);
void exchange_rows(L& h, float* arr, int32_t ld);
void allreduce_sums(L& h, double* buf, size_t n);
void build_halo_plan(L& h);
void halo_exchange(L& h, float* arr, int32_t ld);
CgResult run_cg_rows(L& h, const OpParams& op, const CgBuffers& b, bool with_path, int max_iters, float tol);
bool row_mode(const L& h);
// U as readers see it: the anchors while U aliases them
inline const float* u_read(const L& h) { return h.u_is_y ? h.Y.p : h.U.p; }
bool u_alias_ok(const L& h);
void reset_u_to_y(L& h);
void materialise_u(L& h);
void rows_to_slab(L& h, const float* src, float* dst, int32_t ld, int32_t c0, int32_t c1, int grid, const float* sub = nullptr);
// osc_anchor_build.hip: a level of the anchor-start chain formed where it is not held (derived_state.hpp: Level; wwy to gram4 --
// wy is a by-product of the gathering INIT pass, w4 of gram4's build).  False: not held and not to be had, the solve stays on the
// route of the level below.  What a solve lends the builders: its blocked-matvec arguments, kernel shape and grid, its window and
// pitch, and two N x ld arrays that are free until its INIT pass (gram3 borrows the first, gram4 both).
struct AnchorBuild {
  L& h;
  const BlkArgs& ba;
  int shape, grid;
  int32_t ld, c0, c1;
  float *scratch0, *scratch1;
};
bool ensure_anchor(const AnchorBuild& c, host::Level level);
int64_t anchor_level_bytes(const L& h, host::Level level);  // what the level holds on the device, 0 while it is not held
bool env_num(const char* name, int& out);
void read_env_solver(L& h);
void read_env_build(L& h);
void read_env(L& h);
void require_graph(L& h);
// osc_query.hip (include/oscillink_hip.h: osc_query_basis, osc_get_query_basis, osc_bundle_many, osc_mmr_many)
void query_basis_solve(L& l, float tol, int32_t max_iters, float scale, bool fresh, int32_t* iters, float* res, double* ms);
void query_basis_download(L& l, float* X_out, float* x_out);
// the caller's arrays of a receipt batch (osc_receipt_many's outputs): four sums and the null-point count per query, then the
// kept null points of all queries at null_offsets, `capacity` of them at most
struct ReceiptManyOut {
  double *dH, *coh_sum, *anchor_sum, *query_sum;
  int32_t* null_total;
  int64_t* null_offsets;
  int32_t *i, *j;
  float *z, *r;
  int64_t capacity;
};
// the caller's arrays of a chain-receipt batch (osc_chain_receipt_many's outputs): four values per chain edge, four per query
struct ChainManyOut {
  float *z_struct, *z_path, *r_struct, *r_path;
  double* gain;
  int32_t *verdict, *weakest_k;
  float* weakest_z;
};
void query_receipt_many(L& l, const float* psis, int32_t Q, int32_t detail, float z_th, int32_t null_cap, const ReceiptManyOut& o);
void query_chain_receipt_many(L& l, const float* psis, int32_t Q, const int64_t* chain_offsets, const int32_t* chain_nodes,
                              float z_th, const ChainManyOut& o);
// osc_query_basis_shifted / osc_chain_prior_many
void query_basis_shifted_solve(L& l, float lamP, float tol, int32_t max_iters, float scale, bool fresh, int32_t* iters,
                               float* res, double* ms);
void query_chain_prior_many(L& l, const float* psis, int32_t Q, const int64_t* chain_offsets, const int32_t* chain_nodes,
                            const float* chain_weights, float lamP, float tol, int32_t max_iters, float z_th,
                            const ChainManyOut& o, float* prior_res, int32_t* prior_iters);
// sum (A - B) . M (A - B) with the stationary operator (osc_api.hip; receipts.py:21-25)
double quad_form_of_difference(L& l, const float* A, const float* B);
// osc_bundle_prior_many
void query_bundle_prior_many(L& l, const float* psis, int32_t Q, const int64_t* chain_offsets, const int32_t* chain_nodes,
                             const float* chain_weights, float lamP, float tol, int32_t max_iters, int32_t k, float alpha,
                             float lambda_div, int32_t* ids, float* score, float* align, float* prior_res,
                             int32_t* prior_iters);
// osc_receipt_prior_many
void query_receipt_prior_many(L& l, const float* psis, int32_t Q, const int64_t* chain_offsets, const int32_t* chain_nodes,
                              const float* chain_weights, float lamP, float tol, int32_t max_iters, int32_t detail, float z_th,
                              int32_t null_cap, const ReceiptManyOut& o, float* prior_res, int32_t* prior_iters);
void query_bundle_many(L& l, const float* psis, int32_t Q, int32_t k, float alpha, float lambda_div, int32_t* ids,
                       float* score, float* align);
void query_mmr_many(L& l, const float* scores, int32_t Q, int32_t k, float lambda_div, int32_t* ids);
// osc_gates_many (gates_many.hpp)
void query_gates_many(L& l, const float* psis, int32_t Q, float beta, float gamma, int32_t method, float tol, int32_t max_iters,
                      int32_t clamp, float* gates_out, int32_t* iters_out, float* res_out);
// osc_bundle_gated_many / osc_ustar_gated_many (bundle_gated.hpp)
void query_bundle_gated_many(L& l, const float* psis, int32_t Q, float* gates, int32_t diffusion, float gate_beta,
                             float gate_gamma, int32_t gate_method, float gate_tol, int32_t gate_max_iters, float tol,
                             int32_t max_iters, int32_t k, float alpha, float lambda_div, int32_t* ids, float* score,
                             float* align, int32_t* iters_out, float* res_out, float* U_out);
// osc_receipt_gated_many (receipt_gated.hpp)
void query_receipt_gated_many(L& l, const float* psis, int32_t Q, float* gates, int32_t diffusion, float gate_beta,
                              float gate_gamma, int32_t gate_method, float gate_tol, int32_t gate_max_iters, float tol,
                              int32_t max_iters, int32_t settle, float dt, int32_t settle_max_iters, float settle_tol,
                              int32_t detail, float z_th, int32_t null_cap, int32_t k, float alpha, float lambda_div,
                              int32_t* settle_iters, float* settle_res, const ReceiptManyOut& o, int32_t* ids, float* score,
                              float* align, int32_t* iters_out, float* res_out, double* settle_ms, double* solve_ms);
// osc_chain_gated_many (chain_gated.hpp)
void query_chain_gated_many(L& l, const float* psis, int32_t Q, float* gates, int32_t diffusion, float gate_beta,
                            float gate_gamma, int32_t gate_method, float gate_tol, int32_t gate_max_iters,
                            const int64_t* chain_offsets, const int32_t* chain_nodes, const float* chain_weights, float lamP,
                            float chain_z_th, float tol, int32_t max_iters, int32_t settle, float dt,
                            int32_t settle_max_iters, float settle_tol, int32_t detail, float z_th, int32_t null_cap,
                            int32_t k, float alpha, float lambda_div, int32_t* settle_iters, float* settle_res,
                            const ReceiptManyOut& o, const ChainManyOut& co, int32_t* ids, float* score, float* align,
                            int32_t* iters_out, float* res_out, double* settle_ms, double* solve_ms);

struct ProfScope {
  L& h;
  ProfSlot s{};
  bool on;
  ProfScope(L& h_, int which, int iter = 0) : h(h_), on(h_.prof_on) {
    if (on) {
      s.which = which;
      s.iter = iter;
      s.a = prof_event(h);
      s.b = prof_event(h);
      HIP_CHECK(hipEventRecord(s.a, h.stream));
    }
  }
  ~ProfScope() {
    if (on) {
      (void)hipEventRecord(s.b, h.stream);
      h.prof_pending.push_back(s);
      if (h.prof_pending.size() > 8192) prof_drain(h, true);
    }
  }
};

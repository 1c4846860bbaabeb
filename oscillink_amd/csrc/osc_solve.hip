// Operator parameters, apply plans and the CG drivers of liboscillink_hip.so (see osc_internal.hpp).
#include "osc_internal.hpp"
#include "anchor_gram.hpp"

#include <limits>

// ---- operators ------------------------------------------------------------------------------------
bool path_active(const L& h) { return h.chain_present && h.lamP > 0.0f; }

OpParams settle_op(const L& h, float dt, int precond) {
  OpParams o{};
  const float lp_op = path_active(h) ? h.lamP : 0.0f;
  o.cs_const = 1.0f + dt * (h.lamG + h.lamC + lp_op);  // X + dt (lamG X + lamC (X - W X) + lamP (X - Wp X))
  o.cs_B = dt * h.lamQ;
  o.cW = dt * h.lamC;
  o.cP = dt * lp_op;
  o.md_const = 1.0f + dt * (h.lamG + (h.chain_present ? h.lamP : 0.0f));  // lattice.py:187-192
  o.md_B = dt * h.lamQ;
  o.precond = precond;
  o.rbU = 1.0f;
  o.rbY = dt * h.lamG;
  o.rbB = dt * h.lamQ;
  return o;
}
OpParams ustar_op(const L& h) {
  OpParams o{};
  const float lp_op = path_active(h) ? h.lamP : 0.0f;
  o.cs_const = h.lamG + h.lamC + lp_op;
  o.cs_B = h.lamQ;
  o.cW = h.lamC;
  o.cP = lp_op;
  o.md_const = h.lamG + (h.chain_present ? h.lamP : 0.0f);  // lattice.py:257-259
  o.md_B = h.lamQ;
  o.precond = 1;
  o.rbU = 0.0f;
  o.rbY = h.lamG;
  o.rbB = h.lamQ;
  return o;
}

// The apply plan of a solve over columns [c0, c1) of N x ld buffers: host_logic.hpp, plan_apply, decides; this fills its
// inputs from the handle.  Row-sharded solves plan for the whole lattice.
host::ApplyPlan apply_plan(const L& h, int32_t c0, int32_t c1, int32_t ld, bool with_path) {
  if (h.blk_resident[0] < 0) {  // workgroups per XCD each shape of the blocked matvec gets resident (queried once)
    hipDeviceProp_t prop;
    HIP_CHECK(hipGetDeviceProperties(&prop, h.device));
    for (int v = 0; v < kBlkShapeCount; ++v) h.blk_resident[v] = blocked_resident_per_cu(v) * std::max(1, prop.multiProcessorCount / 8);
  }
  host::ApplyInputs in;
  in.N = h.N;
  in.nnz = h.nnz;
  in.width = h.width;
  in.ld = h.ld;
  in.c0 = h.c0;
  in.c1 = h.c1;
  in.reordered = h.reordered;
  in.prows = h.prows;
  in.sc0 = c0;
  in.sc1 = c1;
  in.sld = ld;
  in.with_path = with_path;
  in.grid = cg_grid(h);
  std::copy(h.blk_resident, h.blk_resident + kBlkShapeCount, in.resident);
  in.spmm_xs = h.spmm_xs;
  in.xs_nb = h.xs_nb;
  in.spmm_blocked = h.spmm_blocked;
  in.blk_variant = h.blk_variant;
  in.spmm_deep = h.spmm_deep;
  return host::plan_apply(in);
}

BlockedView blocked_view(L& h, int nb) {
  if (h.derived.blk_nb != nb) {
    DevBuf<unsigned> cnt;
    cnt.alloc(1);
    HIP_CHECK(hipMemsetAsync(cnt.p, 0, 4, h.stream));
    launch_blocked_count(h.ell_col.p, h.deg.p, h.width, (int32_t)h.N, nb, cnt.p, h.stream);
    unsigned over = 0;
    HIP_CHECK(hipMemcpyAsync(&over, cnt.p, 4, hipMemcpyDeviceToHost, h.stream));
    sync(h);
    // the apply's list wave copies whole row groups: up to 8 x gather-waves slot rows past the lattice's end
    // (host_logic.hpp: blocked_list_extent <= N - 1 + 8 x gather waves, swept in tests/host_logic)
    constexpr size_t kPadRows = 8192;
    for (const BlkShape& sh : kBlkShapes)
      if ((size_t)sh.cw * 8 > kPadRows) throw std::runtime_error("blocked graph copy: padding too small");
    const size_t nslots = (size_t)nb * h.N * OSC_BLK_SLOTS, npad = kPadRows * OSC_BLK_SLOTS;
    h.blk_slots.alloc(nslots + npad);
    HIP_CHECK(hipMemsetAsync(h.blk_slots.p + nslots, 0, npad * sizeof(int2), h.stream));  // {row 0, 0.0f}
    h.blk_over.alloc((size_t)over + 1);
    h.blk_rest.alloc((size_t)h.N);
    HIP_CHECK(hipMemsetAsync(cnt.p, 0, 4, h.stream));
    launch_blocked_fill(h.ell_col.p, h.ell_w.p, h.deg.p, h.width, (int32_t)h.N, nb, h.blk_slots.p, h.blk_rest.p, h.blk_over.p, cnt.p,
                        h.stream);
    sync(h);  // cnt goes out of scope
    h.derived.blk_nb = nb;
  }
  BlockedView v{};
  v.slots = h.blk_slots.p;
  v.rest = h.blk_rest.p;
  v.over = h.blk_over.p;
  v.nb = nb;
  return v;
}

// the plain operator apply over sa's column window, which is the plan's
void spmm_slabbed(L& h, const host::ApplyPlan& plan, int mode, SpmmArgs sa, int grid, int iter) {
  const int32_t c0 = sa.c0, c1 = sa.c1;
  sa.deep = plan.deep ? 1 : 0;
  ProfScope ps(h, mode == SPMM_INIT ? 4 : 0, iter);  // slot 0: AP applies (the CG matvec); slot 4: the INIT apply
  if (plan.xs) {
    sa.xs = sa.xblk != 0 ? plan.xs_pmajor : plan.xs;
    sa.xs_groups = plan.xs_groups;
    launch_spmm(mode, sa, grid, h.stream);
    return;
  }
  for (int32_t s0 = c0; s0 < c1; s0 += plan.slab) {
    sa.c0 = s0;
    sa.c1 = std::min(c1, s0 + plan.slab);
    launch_spmm(mode, sa, grid, h.stream);
  }
}

// elementwise CG kernels cover at most 2048 columns per launch: wider states run as several column windows
template <typename Args, typename F>
void for_windows(Args a, F&& launch) {
  const int32_t c0 = a.c0, c1 = a.c1;
  for (int32_t s0 = c0; s0 < c1; s0 += 2048) {
    a.c0 = s0;
    a.c1 = std::min(c1, s0 + 2048);
    launch(a);
  }
}

// The CG drivers.  The host enqueues iteration it+1 before it reads iteration it's residual.  On one GPU every kernel of a
// speculative iteration carries a gate (residual of the previous iteration, tol) and is a no-op once the CG has converged;
// under a communicator it carries none and writes scratch arrays only (the x update of an iteration is applied by its
// successor's p update or by the host's order, never speculatively).  Either way the reference's "stop before the
// beta/p update" semantics hold exactly while the stream never drains between iterations.
// Small lattices: the whole solve in ONE launch with the state in LDS (small_kernels.hip).  Returns false when the
// lattice does not fit that path (or its barrier timed out) and the general path must run.
bool run_cg_small(L& h, const OpParams& op, const CgBuffers& b, bool with_path, int max_iters, float tol,
                  CgResult& out) {
  if (!h.small_path || h.comm != nullptr || b.c0 != 0 || b.c1 != h.dcols || b.ld != h.dcols || max_iters > host::kSmallMaxIters)
    return false;
  const int C = host::small_pick_cols((int32_t)h.N, b.ld);
  if (C <= 0) return false;
  const size_t nslots = (size_t)max_iters + 2;
  const size_t nctl = 2 * nslots + 2;  // [residual slots | arrival counters | status | finish counter]
  ensure_ctrl(h, nctl);
  uint32_t* ctl = ctrl_segment(h, nctl);
  // the kernel's last workgroup publishes residuals + a "done" word into host-mapped memory and the host polls that
  // word
  volatile uint32_t* host_words = reinterpret_cast<volatile uint32_t*>(h.res_host);
  host_words[nslots] = kCtrlPending;
  SmallArgs a{};
  if (!h.derived.ell_t) {
    h.ell_col_t.alloc((size_t)h.N * h.width);
    h.ell_w_t.alloc((size_t)h.N * h.width);
    launch_transpose_ell(h.ell_col.p, h.ell_w.p, (int32_t)h.N, h.width, h.ell_col_t.p, h.ell_w_t.p, h.stream);
    h.derived.ell_t = true;
  }
  a.g = graph_view(h, with_path);
  a.col_t = h.ell_col_t.p;
  a.w_t = h.ell_w_t.p;
  a.op = op;
  float* xout = b.X;
  if (b.X == b.x0 || b.X == b.rhsU || b.X == b.rhsY) {  // never hand the one-launch kernel an aliased output
    if (!b.Xalt) return false;
    xout = b.Xalt;
  }
  a.x0 = b.x0;
  a.X = xout;
  a.U = b.rhsU;
  a.Y = b.rhsY;
  a.B = b.B;
  a.psi = b.psi;
  a.res_bits = ctl;
  a.arrive = ctl + nslots;
  a.status = ctl + 2 * nslots;
  a.finish = ctl + 2 * nslots + 1;
  a.host_words = reinterpret_cast<uint32_t*>(h.res_host_dev);
  a.N = (int32_t)h.N;
  a.ld = b.ld;
  a.max_iters = max_iters;
  a.tol = tol;
  launch_settle_small(a, C, h.stream);
  if (poll_host_word(h, host_words + nslots, nullptr, "the one-launch solve's done word") != 0u) {
    sync(h);       // (the kernel's other workgroups are on their way out)
    return false;  // barrier timeout (GPU shared with other persistent work): take the general path
  }
  h.history.clear();
  out = CgResult{max_iters, 0.f, xout};
  for (int it = 1; it <= max_iters; ++it) {
    const float res = h.res_host[it];
    h.history.push_back(res);
    out.res = res;
    if ((double)res <= (double)tol) {
      out.iters = it;
      break;
    }
  }
  h.small_solves += 1;
  return true;
}

// rows -> slab-major over [c0, c1) (k_rows_to_slab), counted per handle (osc_counters::rows_to_slab_launches)
void rows_to_slab(L& h, const float* src, float* dst, int32_t ld, int32_t c0, int32_t c1, int grid, const float* sub) {
  launch_rows_to_slab(src, dst, h.N, ld, c0, c1, grid, h.stream, sub);
  h.slab_launches += (c1 - c0 + 2047) / 2048;
}

// The slab-major operand of a blocked INIT pass that starts from x0: the anchors' image where x0 IS the anchors (built on
// first use, the same bits for every solve that starts from Y: the first settle of a lattice, every settle after a reset,
// the U* solve, the query basis), else x0 transposed into `scratch`.
static const float* init_operand(L& h, const CgBuffers& b, float* scratch, int grid) {
  if (h.anchor_slab && b.x0 == h.Y.p && b.ld == h.ld && b.c0 == h.c0 && b.c1 == h.c1) {
    if (!h.derived.ys) {
      h.Ys.alloc((size_t)h.N * h.ld);
      rows_to_slab(h, h.Y.p, h.Ys.p, h.ld, h.c0, h.c1, grid);
      h.derived.ys = true;
    }
    return h.Ys.p;
  }
  rows_to_slab(h, b.x0, scratch, b.ld, b.c0, b.c1, grid);
  return scratch;
}

// Arguments of the source-blocked matvec (k_apply_blocked) for the handle's whole column window: X = slab-major input, OUT =
// row-major output, column sums of X . OUT into h.part0 (grid rows, + the chain fix-up's chunks behind them).  For a plan
// with source blocks.
void blocked_setup(L& h, const host::ApplyPlan& plan, const OpParams& op, const float* X, float* OUT, const float* B, int32_t ld,
                   bool with_path, int grid, BlkArgs& ba, ChainFixArgs& cf) {
  const int nb = plan.src_blocks;
  const BlockedView bv = blocked_view(h, nb);
  ba.X = X;
  ba.OUT = OUT;
  ba.B = B;
  ba.part = h.part0.p;
  ba.slots = bv.slots;
  ba.rest = bv.rest;
  ba.over = bv.over;
  ba.cs_const = op.cs_const;
  ba.cs_B = op.cs_B;
  ba.cW = op.cW;
  ba.N = (int32_t)h.N;
  ba.ld = ld;
  ba.c0 = h.c0;
  ba.c1 = h.c1;
  ba.nb = nb;
  // workgroups per XCD (what is resident at once), slab groups, row groups per wave, destination slices
  ba.xs = plan.geom.xs;
  ba.xs_groups = plan.geom.xs_groups;
  ba.slices = plan.geom.slices;
  ba.groups = plan.geom.groups;
  if (with_path && op.cP != 0.f) {  // the chain prior's few rows: a small launch behind every blocked apply
    cf.X = X;
    cf.OUT = OUT;
    cf.part = h.part0.p;
    cf.prow = h.prow.p;
    cf.pcol = h.pcol.p;
    cf.pw = h.pw.p;
    cf.pdeg = h.pdeg.p;
    cf.cP = op.cP;
    cf.prows = h.prows;
    cf.pwidth = h.pwidth;
    cf.N = (int32_t)h.N;
    cf.ld = ld;
    cf.c0 = h.c0;
    cf.c1 = h.c1;
    cf.part_row0 = grid;
    cf.chunks = chain_fix_chunks(h.prows);
  }
}

// k_apply_blocked over ba and, where the lattice has a chain prior (cf.chunks > 0), the chain fix-up behind it, both under the
// gate g.  The caller counts the launch where osc_counters::blocked_applies counts it (the INIT passes of a solve do not).
static void apply_blocked(L& h, const host::ApplyPlan& plan, BlkArgs& ba, ChainFixArgs& cf, int grid, Gate g) {
  ba.gate = g.p;
  ba.gate_tol = g.tol;
  launch_apply_blocked(ba, grid, h.stream, nullptr, plan.shape);
  if (cf.chunks > 0) {
    cf.gate = g.p;
    cf.gate_tol = g.tol;
    launch_chain_fix(cf, h.stream);
  }
}

// launches of iterations behind the one a solve stopped in (speculative, gated off) are not profile samples
static void drop_speculative_samples(L& h, size_t mark, int iters) {
  for (size_t i = mark; i < h.prof_pending.size(); ++i)
    if (h.prof_pending[i].iter > iters) h.prof_pending[i].which = -1;
}

// x . (op x) summed per column into h.part0 for a ROW-major x (N x ld, the handle's whole window) through the blocked matvec:
// x -> slab-major (scratch_slab), one launch (+ the chain fix-up), op x -> scratch_out.  Returns the rows of partial sums
// h.part0 holds, 0 where the blocked matvec does not serve this lattice (the caller takes the plain apply's DOT form).
// plan: the handle's window at its pitch.
int blocked_quad_form(L& h, const host::ApplyPlan& plan, const OpParams& op, const float* x_rows, float* scratch_slab,
                      float* scratch_out, bool with_path, const float* x_sub) {
  if (plan.src_blocks == 0) return 0;
  const int grid = cg_grid(h);
  BlkArgs ba{};
  ChainFixArgs cf{};
  blocked_setup(h, plan, op, scratch_slab, scratch_out, h.B.p, h.ld, with_path, grid, ba, cf);
  rows_to_slab(h, x_rows, scratch_slab, h.ld, h.c0, h.c1, grid, x_sub);
  apply_blocked(h, plan, ba, cf, grid, Gate{nullptr, 0.f});
  h.blk_applies += 1;
  return grid + cf.chunks;
}

namespace {

using host::Level;

// One general-path solve: the host side of cg_solve (solver.py:6-37) as run_cg stages it -- construction (control words, stop
// test route, the arguments that hold for the whole solve), init() (r = b - A x0, z, p, r . z), plan_ring(), the loop methods
// host::cg_host_loop drives (host_logic.hpp), finish().
struct CgSolve {
  // ---- fixed for the solve ------------------------------------------------------------------------------------------
  L& h;
  const OpParams& op;
  const CgBuffers& b;
  const bool with_path;
  const int max_iters;
  const float tol;
  const int grid;
  const host::ApplyPlan plan;
  const size_t nslots;
  // Single GPU: the last workgroup of each iteration's beta reduction writes the residual into host-mapped memory and
  // the host polls that word (no 4-byte copy, event record and event wait per iteration).  Under a communicator the
  // residual first goes through the all-reduce (publish_residual; OSC_COMM_OVERLAP=0: in the solve's stream, read back by
  // copy + event).
  const bool mapped;
  // Sharded (column windows): the stop test needs max over the ranks of the residual -- a 4-byte all-reduce per iteration,
  // tens of microseconds of latency on xGMI next to ~180 us of kernels per iteration in an 8-rank window of config 3.
  // With the x update deferred a speculative iteration writes scratch arrays only (r, p, Ap, alpha, beta), so it needs no
  // gate and the solve's stream never waits for the all-reduce: that goes to a second stream behind an event per iteration,
  // followed by a one-thread kernel that publishes the reduced word into the host-mapped slot the host polls, as on one
  // GPU.  The host alone decides when to stop; a wrong guess of the last iteration costs one iteration of device time
  // instead of five gated-off launches.
  // What it costs (one-rank RCCL communicator, all-reduce latency ~0: docs/DESIGN_HISTORY.md section 6): ~17 us once per
  // solve for the second stream's hand-over at the last iteration, and the expected last iteration's own form (an ungated
  // speculative iteration must not touch x): 47 us at 768 columns, 6 at 96.  What it saves: every all-reduce latency but
  // the last.  Hence by default from four ranks on (narrow windows, 15-30 us per all-reduce); OSC_COMM_OVERLAP=1 / 0 force it.
  const bool overlap;
  const bool polled;  // the host reads residuals from the host-mapped words (false: copy + event per iteration)
  uint32_t* res_slots = nullptr;  // zeroed: [residual per iteration | arrival counter per iteration]
  uint32_t* done_ctr = nullptr;
  // The settle from an aliased U (b.defer_x0: x0 = the anchors, X = U's empty buffer): no INIT form writes a copy of x0
  // into X -- each is told that x0 IS its solution array, as in an in-place solve -- and the one launch that applies
  // iteration 1's x update reads x from x0 and writes it to X (UpdateArgs::Xin).
  const float* const x1_in;
  float* const x_init;  // (only compared with x0, never written, then)
  const int stop_guess;  // the count of the handle's previous solve of this kind (0: unknown)
  float* Pbuf;   // search direction / operator output: the fused INIT pass leaves p in the AP array and swaps the two for
  float* APbuf;  // the rest of the solve (init() alone changes them)
  size_t prof_mark = 0;  // the handle's pending profile samples when the loop started
  // The INIT pass also left iteration 1's A p (in the AP array) and its p . Ap partials (in part1): init_fused, the anchor
  // start under uniform gates.  enqueue(1) then launches no matvec and forms alpha from those partials.
  bool first_ap_done = false;
  // ... and T = A (A p1) (in the handle's Tap array): iteration 2's p update then forms A p2 over A p1 and leaves the
  // p . Ap partials in part0 (k_update_p_ap2), and enqueue(2) launches no matvec either.
  bool second_ap_ready = false;
  // Iterations 1 and 2 ran inside the INIT pass, with their scalars from the lattice's Gram sums (init_fused; host_logic.hpp:
  // anchor_gram_route): r2, p3 (in dir(3)) and x2 are in place, alpha_of(1), alpha_of(2), h.beta and h.rz hold what the two
  // iterations' reductions would have left, residual slots 1 and 2 are published.  enqueue(1) and enqueue(2) launch nothing,
  // enqueue(3) launches no p update, and the ring starts with two directions applied.
  const bool allow_gram;  // (false: the solve run again after a fused pass that was gated off)
  const bool allow_poly;  // (false: the solve run again after a polynomial pass that was gated off)
  bool gram_route = false;
  // ... and iteration 3's scalars are known as well (anchor_gram3_route): alpha_of(3) holds alpha3, h.beta beta3, h.rz r3 . z3,
  // residual slot 3 is published.  enqueue(3) launches the matvec's fused form alone -- r3 over r2, p4 into dir(4), under its own
  // gate word --, enqueue(4) launches no p update.  The INIT pass has alpha3 and p3 in hand and runs only if iteration 3 is a real
  // one: it leaves x3 instead of x2, and the ring starts with three directions applied.
  bool gram3_route = false;
  // ... and alpha4 and |r4| too (anchor_gram4_route): alpha_of(4) holds alpha4 and host word 4 is published (the device's slot 4 is not).
  // enqueue(3) reads the four published words -- cg_host_loop calls it behind wait(1), and word 1 is the last to go out -- and
  // where they say the solve ends in iteration 4 it launches the matvec's last form (x4 over x3, nothing else) and sets
  // gram4_taken: no launch belongs to iteration 4 or to one behind it, and x is complete.  Otherwise it takes word 4 back
  // (iteration 4's beta reduction publishes it anew) and everything is the three-step route's.
  bool gram4_planned = false, gram4_taken = false;
  bool gram4_fold = false;  // ... and the INIT pass was given go[2]: a solve that ends so takes the folded last form (OSC_GRAM4_FOLD)
  // The polynomial last form (host_logic.hpp: anchor_poly_route): in the INIT pass's place the scalars kernel and k_settle_poly are
  // enqueued, both acting on go[2], and nothing else: run_cg reads the four words (poly_done) instead of running the host loop.
  bool poly_pending = false;
  float fused_md_B = 0.f, fused_md_const = 1.f;  // (BlkInit's, for the fused launch)
  bool ring_planned = false;

  // ---- where x is updated ---------------------------------------------------------------------------------------------
  // Deferred x update: iteration it's x += alpha p is applied by iteration it + 1's p update, which reads p anyway (x, r,
  // p in / x, p out there, r, Ap in / r out in the x-r kernel: 8 array passes per iteration instead of 9), or by
  // finish_x behind an iteration that has no successor enqueued.  The iteration expected to be the last (stop_guess, or
  // max_iters) takes k_update_xr's "last" form instead: x finished next to the r update, the new r not stored (five passes
  // instead of three there and three in finish_x).  Which launch carries which update is decided by host::CgXSchedule
  // (host_logic.hpp; swept against a model of the device's gating on the CPU box, tests/host_logic/sweep_host_logic.cpp).
  host::CgXSchedule xs;
  // The ring of kept directions (host_logic.hpp: plan_x_ring, CgXRing): K >= 2 slots -- direction `it` in slot it % K, its
  // alpha in the same slot of h.alpha_ring -- and x is written by k_update_x_ring alone: once per solve where the solve
  // takes at most K iterations.  K = 1: everything runs as CgXSchedule says.
  host::CgXRing ring;
  float* slot[host::kXRingMax] = {nullptr, nullptr, nullptr, nullptr};
  float* aslot[host::kXRingMax] = {nullptr, nullptr, nullptr, nullptr};

  // ---- kernel arguments: members, edited launch by launch --------------------------------------------------------------
  // Every launch site sets each field that differs between launch kinds; the rest is set once, here said where.
  // sa (k_spmm): the constructor sets g, op, B, psi, N, ld, c0, c1, part, R, P, U, Y (the INIT outputs and rhs: the AP mode
  //   reads none of them); per launch: X, OUT, xblk, pblk, gate, gate_tol (spmm_slabbed sets deep, xs, xs_groups and the slab).
  // ua (k_update_p / _xr / _x): the constructor sets X, R, B, beta, part_rr, part_rz, op, N, ld, c0, c1, pblk, temporal,
  //   init() sets AP; per launch (set_update): gate, gate_tol, xmode, Xin, alpha, P, Pout (for_windows sets the window).
  // ba (k_apply_blocked), cf (k_chain_fix): blocked_setup sets everything but X, OUT, gate, gate_tol, which are per launch.
  SpmmArgs sa{};
  UpdateArgs ua{};
  BlkArgs ba{};
  ChainFixArgs cf{};

  CgSolve(L& h_, const OpParams& op_, const CgBuffers& b_, bool with_path_, int max_iters_, float tol_, bool allow_gram_, bool allow_poly_)
      : h(h_), op(op_), b(b_), with_path(with_path_), max_iters(max_iters_), tol(tol_), grid(cg_grid(h_)),
        plan(apply_plan(h_, b_.c0, b_.c1, b_.ld, with_path_)), nslots((size_t)max_iters_ + 2), mapped(h_.comm == nullptr),
        overlap(h_.comm != nullptr && (h_.comm_overlap == 1 || (h_.comm_overlap < 0 && h_.world >= 4)) && h_.x_defer),
        polled(mapped || overlap), x1_in(b_.defer_x0 && b_.X != b_.x0 && !overlap ? b_.x0 : nullptr),
        x_init(x1_in != nullptr ? const_cast<float*>(b_.x0) : b_.X), stop_guess(h_.predicted_iters[b_.kind]), Pbuf(b_.P),
        APbuf(b_.AP), allow_gram(allow_gram_), allow_poly(allow_poly_) {
    ensure_ctrl(h, nslots);
    res_slots = ctrl_segment(h, 2 * nslots);
    done_ctr = res_slots + nslots;
    if (overlap) {
      if (!h.comm_stream) h.comm_stream = acquire_stream(h.device);
      while (h.step_events.size() < nslots) {
        hipEvent_t e;
        HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        h.step_events.push_back(e);
      }
      h.comm_stream_busy = true;  // from here on (also if the solve is abandoned half way): drained before the slots are reused
    }
    if (polled)  // (kCtrlPending is never a residual: those are sqrt(...) >= 0 or a canonical NaN)
      for (size_t i = 0; i < nslots; ++i) reinterpret_cast<volatile uint32_t*>(h.res_host)[i] = kCtrlPending;
    sa.g = graph_view(h, with_path);
    sa.op = op;
    sa.B = b.B;
    sa.psi = b.psi;
    sa.N = h.N;
    sa.ld = b.ld;
    sa.c0 = b.c0;
    sa.c1 = b.c1;
    sa.part = h.part0.p;
    sa.R = b.R;
    sa.P = b.P;
    sa.U = b.rhsU;
    sa.Y = b.rhsY;
    // source-blocked CG matvec (k_apply_blocked) where the slab an XCD gathers from is far larger than its L2
    if (plan.src_blocks > 0) blocked_setup(h, plan, op, b.P, b.AP, b.B, b.ld, with_path, grid, ba, cf);
    // slab-major search direction: only where the XCD-affine slab apply runs (its gathers then read contiguous slabs)
    ua.pblk = plan.pblk ? h.N : 0;
    ua.temporal = 5.0 * (double)h.N * (double)(b.c1 - b.c0) * 4.0 <= h.temporal_mb * 1048576.0;
    ua.X = b.X;
    ua.R = b.R;
    ua.B = b.B;
    ua.beta = h.beta.p;
    ua.part_rr = h.part0.p;
    ua.part_rz = h.part1.p;
    ua.op = op;
    ua.N = h.N;
    ua.ld = b.ld;
    ua.c0 = b.c0;
    ua.c1 = b.c1;
    xs.xdefer = h.x_defer;
    xs.last_form = h.x_last_form;
    xs.ungated = overlap;
    xs.stop_guess = stop_guess;
    xs.max_iters = max_iters;
    ring.K = 1;  // (until plan_ring)
  }

  // what the builders of the anchor-start chain borrow (osc_anchor_build.hip): AP and R hold nothing before the INIT pass
  AnchorBuild builder() { return AnchorBuild{h, ba, plan.shape, grid, b.ld, b.c0, b.c1, b.AP, b.R}; }
  bool ringed() const { return ring.K > 1; }
  float* dir(int it) const { return ringed() ? slot[it % ring.K] : Pbuf; }  // where direction `it` lives
  float* alpha_of(int it) const { return ringed() ? aslot[it % ring.K] : h.alpha.p; }

  // r = b - A x0 ; z ; p ; rz.  Returns the rows of r . z partials the pass left (+ the chain fix-up's behind the fused pass).
  int init() {
    int part_rows = grid;
    for (const Level l : {Level::gram, Level::gram3, Level::gram4, Level::w4}) h.at(l).last = false;
    // (the rhs rows the fused pass can take besides x0 itself: one -- the state term must be x0 or absent, and if y is a
    // third array the solution array must be x0)
    const bool fuse_u = b.rhsU == b.x0 || op.rbU == 0.f;
    const bool fuse_y = b.rhsY == b.x0 || x_init == b.x0;
    // (an inertia start hands over x0 IN the AP array, which the blocked matvec would overwrite with A x0 before
    // init_finish has read x0: such a solve keeps the gathering INIT kernel, which reads x0 completely first)
    if (ba.nb > 0 && h.blk_init && h.blk_init_fused && fuse_u && fuse_y && b.x0 != b.AP) {
      part_rows = init_fused();
    } else if (ba.nb > 0 && h.blk_init && b.x0 != b.AP) {
      // r = b - A x0 around the blocked matvec: x0 slab-major (into P, or the anchors' image), A x0 -> AP, then r, z, p = z, r . z
      ProfScope ps(h, 4, 0);
      ba.X = cf.X = init_operand(h, b, b.P, grid);
      ba.OUT = cf.OUT = b.AP;
      apply_blocked(h, plan, ba, cf, grid, Gate{nullptr, 0.f});  // (an INIT pass: not counted in blk_applies)
      InitFinishArgs fa{};
      fa.AP = b.AP;
      fa.X0 = b.x0;
      fa.X = x_init;
      fa.R = b.R;
      fa.P = b.P;
      fa.U = b.rhsU;
      fa.Y = b.rhsY;
      fa.B = b.B;
      fa.psi = b.psi;
      fa.part = h.part0.p;
      fa.op = op;
      fa.N = h.N;
      fa.pblk = h.N;
      fa.ld = b.ld;
      fa.c0 = b.c0;
      fa.c1 = b.c1;
      for_windows(fa, [&](const InitFinishArgs& w) { launch_init_finish(w, grid, h.stream); });
    } else {
      sa.X = b.x0;
      sa.OUT = x_init;
      sa.xblk = 0;
      sa.pblk = plan.pblk ? h.N : 0;
      sa.gate = nullptr;
      sa.gate_tol = 0.f;
      spmm_slabbed(h, plan, SPMM_INIT, sa, grid);
    }
    if (!gram_route) launch_reduce_init(h.part0.p, part_rows, b.ld, b.c0, b.c1, h.rz.p, h.stream);
    ua.AP = APbuf;
    h.last_plan = plan;
    h.at(Level::wwy).last = first_ap_done;
    h.at(Level::w3).last = second_ap_ready;
    return part_rows;
  }

  // r = b - A x0 INSIDE the blocked matvec (the in-place warm-started settle: x0 is also the rhs state term and the
  // solution array; the U* solve: x0 is Y, no state term): x0 slab-major (into P, or the anchors' image), then one launch
  // gathers A x0 and leaves r, z (slab-major, in the AP array), x0 in the solution array and the r . z column sums.
  int init_fused() {
    ProfScope ps(h, 4, 0);
    ba.X = cf.X = init_operand(h, b, b.P, grid);
    ba.OUT = nullptr;
    ba.gate = nullptr;
    ba.gate_tol = 0.f;
    BlkInit bi{};
    bi.Y = b.rhsY == b.x0 ? nullptr : b.rhsY;
    bi.Xcopy = x_init == b.x0 ? nullptr : b.X;
    bi.R = b.R;
    bi.Z = b.AP;
    bi.psi = b.psi;
    bi.rbU = b.rhsU == b.x0 ? op.rbU : 0.f;
    bi.rbY = op.rbY;
    bi.rbB = op.rbB;
    bi.md_B = op.precond ? op.md_B : 0.f;
    bi.md_const = op.precond ? op.md_const : 1.f;
    // From the anchors' resident image: their row sums W.Y are the same for every such solve on this graph copy.  The first
    // one gathers them and leaves them behind (one more store per row), the later ones stream them (k_init_cached: the
    // same r, z and r . z sums to the bit).  (INIT passes are not counted in blk_applies.)
    const bool wy_route = h.anchor_wy && h.anchor_slab && ba.X == h.Ys.p && bi.Y == nullptr;
    if (wy_route && host::held(h.derived, Level::wy, ba.nb)) {
      bi.WY = h.WYs.p;
      host::AnchorApInputs ai;
      ai.mode = h.at(Level::wwy).mode;
      ai.N = h.N;
      ai.cached_init = true;
      ai.gates_uniform = h.gates_uniform && b.B == h.B.p;
      ai.chain_rows = cf.chunks > 0;
      if (host::anchor_ap_route(ai) && ensure_anchor(builder(), Level::wwy)) {
        // ... and iteration 1's A p with its p . Ap sums: p1 = z0 goes to the AP array (the swap below), A p1 to the P array
        BlkInitAp ap{h.WWs.p, h.Wsum.p, b.P, h.part1.p};
        host::AnchorAp2Inputs a2;
        a2.mode = h.at(Level::w3).mode;
        a2.N = h.N;
        a2.depth1 = true;
        a2.max_iters = max_iters;
        if (host::anchor_ap2_route(a2) && ensure_anchor(builder(), Level::w3)) {  // ... and T = A (A p1) for iteration 2's p update
          BlkInitAp2 ap2{h.W3s.p, h.Wsum2.p, h.Tap.p};
          if (two_steps(bi, ap, ap2)) return grid;  // ... or both iterations here and now
          launch_init_cached(ba, grid, h.stream, bi, plan.shape, &ap, &ap2);
          second_ap_ready = true;
        } else {
          launch_init_cached(ba, grid, h.stream, bi, plan.shape, &ap);
        }
        first_ap_done = true;
        h.at(Level::wwy).solves += 1;
      } else {
        launch_init_cached(ba, grid, h.stream, bi, plan.shape);
      }
      h.cached_inits += 1;
    } else if (wy_route) {
      host::begin_build(h.derived, Level::wy);  // (not current while this launch rewrites them)
      for (L::AnchorLevel& a : h.anchor) a.denied = false;
      h.WYs.alloc((size_t)h.N * h.ld);
      bi.WY = h.WYs.p;
      launch_apply_blocked(ba, grid, h.stream, &bi, plan.shape, true);
      host::built(h.derived, Level::wy, ba.nb);
    } else {
      launch_apply_blocked(ba, grid, h.stream, &bi, plan.shape);
    }
    int part_rows = grid;
    if (cf.chunks > 0) {  // the chain prior's rows: their r, z and r . z still lack the chain term
      ChainFixArgs ci = cf;
      ci.OUT = b.AP;  // (not written in this form: what blocked_setup left there)
      ci.gate = nullptr;
      ci.gate_tol = 0.f;
      ci.initR = b.R;
      ci.initZ = b.AP;
      ci.B = b.B;
      ci.md_B = bi.md_B;
      ci.md_const = bi.md_const;
      launch_chain_fix(ci, h.stream);
      part_rows = grid + cf.chunks;
    }
    if (!ring_planned) std::swap(Pbuf, APbuf);  // z, the first direction, lies in the AP array (two_steps has swapped them already)
    return part_rows;
  }

  // Iterations 1 and 2 inside the cached INIT pass (anchor_gram_route).  The ring has to be planned first -- p3 goes to its slot
  // -- hence with the P and AP arrays swapped as every fused INIT pass leaves them.  False: the route does not hold (the ring
  // stays planned), and the depth-2 pass runs.
  bool two_steps(BlkInit& bi, const BlkInitAp& ap, const BlkInitAp2& ap2) {
    if (!allow_gram || h.at(Level::gram).mode == 0 || b.X == b.x0 || b.X == h.Ys.p) return false;
    std::swap(Pbuf, APbuf);
    plan_ring();
    host::AnchorGramInputs gi;
    gi.mode = h.at(Level::gram).mode;
    gi.N = h.N;
    gi.depth2 = true;
    gi.comm = h.comm != nullptr;
    gi.ring_slots = ring.K;
    gi.max_iters = max_iters;
    gi.predicted = stop_guess;
    if (!host::anchor_gram_route(gi) || !ensure_anchor(builder(), Level::gram)) return false;
    host::AnchorGram3Inputs g3;
    g3.mode = h.at(Level::gram3).mode;
    g3.N = h.N;
    g3.gram_route = true;
    g3.comm = gi.comm;
    g3.ring_slots = ring.K;
    g3.max_iters = max_iters;
    g3.predicted = stop_guess;
    const bool three = host::anchor_gram3_route(g3) && ensure_anchor(builder(), Level::gram3);
    host::AnchorGram4Inputs g4;
    g4.mode = h.at(Level::gram4).mode;
    g4.N = h.N;
    g4.gram3_route = three;
    g4.max_iters = max_iters;
    const bool four = host::anchor_gram4_route(g4) && ensure_anchor(builder(), Level::gram4);
    GramScalarArgs ga{};
    ga.gram = h.gram.p;
    ga.psi = b.psi;
    ga.B = b.B;
    ga.cs_const = ba.cs_const;
    ga.cs_B = ba.cs_B;
    ga.cW = ba.cW;
    ga.rbU = bi.rbU;
    ga.rbY = bi.rbY;
    ga.rbB = bi.rbB;
    ga.md_B = bi.md_B;
    ga.md_const = bi.md_const;
    ga.tol = tol;
    ga.ld = b.ld;
    ga.c0 = b.c0;
    ga.c1 = b.c1;
    ga.alpha1 = alpha_of(1);
    ga.alpha2 = alpha_of(2);
    ga.beta1 = h.part1.p;  // (beta1 has no array of its own on the summed route either: the r . z partials' first row is free here)
    ga.beta2 = h.beta.p;
    ga.rz = h.rz.p;
    ga.res_slots = res_slots;
    ga.host_words = reinterpret_cast<uint32_t*>(h.res_host_dev);
    if (h.gram_go.n < 3) h.gram_go.alloc(3);
    ga.go = h.gram_go.p;
    if (three) {
      // beta3 takes h.beta, where iteration 4 would look for it, and with two ring slots alpha3 takes alpha1's: the INIT pass,
      // their only reader, finds beta2 and alpha1 in further free rows of the r . z partials
      ga.gram3 = h.gram3.p;
      ga.alpha3 = alpha_of(3);
      ga.beta3 = h.beta.p;
      ga.beta2 = h.part1.p + (size_t)b.ld;
      if (ga.alpha1 == ga.alpha3) ga.alpha1 = h.part1.p + 2 * (size_t)b.ld;
    }
    if (four) {  // alpha4 takes alpha1's slot in a ring of three and alpha2's in one of two: the same way out
      ga.gram4 = h.gram4.p;
      ga.alpha4 = alpha_of(4);
      if (ga.alpha1 == ga.alpha4) ga.alpha1 = h.part1.p + 2 * (size_t)b.ld;
      if (ga.alpha2 == ga.alpha4) ga.alpha2 = h.part1.p + 3 * (size_t)b.ld;
    }
    const bool fold = four && h.gram4_fold && stop_guess == 4;
    if (fold && allow_poly && poly_pass(ga)) return true;
    launch_anchor_gram_scalars(ga, h.stream);
    BlkInit ti = bi;
    ti.Z = dir(3);
    ti.Xcopy = b.X;
    // (three steps: alpha3 is out as well, the pass has p3 in hand and runs only if iteration 3 is a real one: it leaves x3)
    BlkTwoSteps ts{ga.alpha1, ga.alpha2, ga.beta1, ga.beta2, ga.go, 0, three ? ga.alpha3 : nullptr, nullptr, nullptr, nullptr};
    // (four steps: beta3 and alpha4 are out too, and where go[2] says that the solve ends in iteration 4 the pass leaves e for the
    // matvec's folded last form instead of x3 and r2.  Only behind a prediction of 4: the pass's foldable form holds a wave per SIMD
    // less, which a solve that runs on past iteration 4 pays for nothing -- 0.18 ms of a 14.4 ms settle at 1 M rows.  A solve that
    // ends in iteration 4 unannounced takes the unfolded form once and leaves the prediction.)
    if (fold) ts.beta3 = ga.beta3, ts.alpha4 = ga.alpha4, ts.go_fold = ga.go + 2;
    launch_init_two_steps(ba, grid, h.stream, ti, plan.shape, ap, ap2, ts, h.two_steps_stream);
    gram_route = true;
    gram3_route = three;
    gram4_planned = four;
    gram4_fold = fold;
    fused_md_B = bi.md_B;
    fused_md_const = bi.md_const;
    ring.applied = three ? 3 : 2;  // directions 1 and 2 (and 3) are in what the pass left in x
    h.at(Level::gram).solves += 1;
    h.at(Level::gram).last = true;
    if (three) h.at(Level::gram3).solves += 1;
    h.at(Level::gram3).last = three;
    h.cached_inits += 1;
    return true;
  }

  // The polynomial last form in the INIT pass's place: the scalars kernel, which also leaves the nine coefficients a column, and the one
  // elementwise pass that writes x4, gated by go[0] and go[2].  False: the route does not hold, nothing was enqueued.
  bool poly_pass(GramScalarArgs& ga) {
    host::AnchorPolyInputs pi;
    pi.mode = h.at(Level::w4).mode;
    pi.N = h.N;
    pi.fold = true;
    pi.w4_held = host::held(h.derived, Level::w4, ba.nb) && h.Wsum3.n == (size_t)h.N;
    if (!host::anchor_poly_route(pi) || !polled) return false;
    SettlePolyArgs pa{};
    pa.Ys = h.Ys.p;
    pa.WYs = h.WYs.p;
    pa.WW = h.WWs.p;
    pa.W3 = h.W3s.p;
    pa.W4 = h.W4s.p;
    pa.wsum = h.Wsum.p;
    pa.wsum2 = h.Wsum2.p;
    pa.wsum3 = h.Wsum3.p;
    pa.X = b.X;
    pa.N = (int32_t)h.N;
    pa.ld = b.ld;
    pa.c0 = b.c0;
    pa.c1 = b.c1;
    if (!settle_poly_supported(pa)) return false;
    const size_t nc = (size_t)gram::kPolyCoeffs * b.ld;
    try {
      if (h.poly_coef.n < nc) h.poly_coef.alloc(nc);
    } catch (const HipError&) {
      (void)hipGetLastError();
      h.poly_coef.release();
      return false;
    }
    ga.poly = h.poly_coef.p;
    pa.coef = h.poly_coef.p;
    pa.go = ga.go;
    pa.go_fold = ga.go + 2;
    launch_anchor_gram_scalars(ga, h.stream);
    launch_settle_poly(pa, grid, h.stream);
    poly_pending = true;
    gram_route = true;  // (every scalar comes from the sums: init() launches no reduction)
    return true;
  }
  // ... and its end: word 1 is the last the scalars kernel publishes.  True: the four words say what go[2] said, x4 is written (or
  // about to be: finish waits) and the solve is over -- iterations, residuals and every counter but blk_applies as the folded form
  // leaves them.  False: the pass was gated off and wrote nothing (U still aliases Y); run_cg solves again without this form.
  bool poly_done() {
    (void)poll_host_word(h, reinterpret_cast<volatile uint32_t*>(h.res_host) + 1, nullptr, "the polynomial settle's residuals");
    const volatile float* words = reinterpret_cast<const volatile float*>(h.res_host);
    const float r1 = words[1], r2 = words[2], r3 = words[3], r4 = words[4];
    if (!host::anchor_gram4_last_form(r1, r2, r3, r4, (double)tol)) return false;
    for (const float r : {r1, r2, r3, r4}) h.history.push_back(r);
    gram_route = gram3_route = gram4_planned = gram4_fold = gram4_taken = true;
    ring.applied = 4;  // (x is complete: no pass is left)
    for (const Level l : {Level::gram, Level::gram3, Level::gram4, Level::w4}) {
      h.at(l).solves += 1;
      h.at(l).last = true;
    }
    h.folded_four_step_solves += 1;
    h.cached_inits += 1;
    return true;
  }

  // How many directions the solve keeps (plan_x_ring) and where: only a solve that wants more slots than the handle holds at
  // this size asks the device what is free; no solve fails over its ring.
  void plan_ring() {
    if (ring_planned) return;
    ring_planned = true;
    host::XRingInputs ri;
    ri.predicted = stop_guess;
    ri.max_iters = max_iters;
    ri.array_bytes = (int64_t)h.N * b.ld * 4;
    ri.ungated = overlap;
    ri.xdefer = h.x_defer;
    ri.forced = h.x_ring_force;
    const size_t ring_n = (size_t)h.N * b.ld;
    int held = 0;
    while (held < host::kXRingMax - 1 && h.xring[held].n >= ring_n) ++held;
    ri.free_bytes = std::numeric_limits<int64_t>::max();
    if (host::plan_x_ring(ri) - 1 > held) ri.free_bytes = device_free_bytes() + ri.array_bytes * held;
    ring.K = host::plan_x_ring(ri);
    ring.last_form = h.x_last_form;
    ring.stop_guess = stop_guess;
    ring.max_iters = max_iters;
    if (ring.K > 1) {
      try {
        for (int j = 0; j < ring.K - 1; ++j)
          if (h.xring[j].n < ring_n) h.xring[j].alloc(ring_n);
        const size_t an = (size_t)std::max(h.ld, b.ld);
        if (h.alpha_ring.n < an * host::kXRingMax) h.alpha_ring.alloc(an * host::kXRingMax);
        for (int i = 0; i < ring.K; ++i) aslot[i] = h.alpha_ring.p + (size_t)i * an;
      } catch (const HipError&) {
        (void)hipGetLastError();
        for (DevBuf<float>& r : h.xring) r.release();
        ring.K = 1;
      }
    }
    if (ring.K > 1) {
      slot[1 % ring.K] = Pbuf;  // direction 1 is where the INIT pass left z (behind the fused pass: the AP array)
      for (int i = 0, j = 0; i < ring.K; ++i)
        if (i != 1 % ring.K) slot[i] = h.xring[j++].p;
    }
  }

  // the per-launch fields of ua, all of them
  void set_update(const float* gate, int32_t xmode, const float* Xin, const float* alpha, float* P, float* Pout) {
    ua.gate = gate;
    ua.gate_tol = tol;
    ua.xmode = xmode;
    ua.Xin = Xin;
    ua.alpha = alpha;
    ua.P = P;
    ua.Pout = Pout;
  }
  void update_p() { for_windows(ua, [&](const UpdateArgs& w) { launch_update_p(w, grid, h.stream); }); }
  void update_xr() { for_windows(ua, [&](const UpdateArgs& w) { launch_update_xr(w, grid, h.stream); }); }
  // P / Pout of iteration it's x-r kernel and of the redone r update behind it: what that iteration's p update left there.
  // No form of k_update_xr a ring solve launches reads them (x is left alone); they keep the values they always had.
  float* xr_p(int it) const { return dir(std::max(it - 1, 1)); }
  float* xr_pout(int it) const { return ringed() && it > 1 ? dir(it) : nullptr; }

  void ring_pass(host::CgXRing::Pass ps, const float* gate) {
    if (ps.count <= 0) return;
    XRingArgs xa{};
    xa.X = b.X;
    xa.Xin = ps.first == 1 ? x1_in : nullptr;  // (nothing applied yet: x is still x0, the anchors of an aliased start)
    xa.M = ps.count;
    for (int m = 0; m < ps.count; ++m) {
      xa.P[m] = dir(ps.first + m);
      xa.alpha[m] = alpha_of(ps.first + m);
    }
    xa.N = h.N;
    xa.ld = b.ld;
    xa.gate = gate;
    xa.gate_tol = tol;
    xa.pblk = ua.pblk;
    xa.temporal = ua.temporal;
    xa.c0 = b.c0;
    xa.c1 = b.c1;
    for_windows(xa, [&](const XRingArgs& w) { launch_update_x_ring(w, grid, h.stream); });
  }
  void finish_x(int it) {  // iteration it's x += alpha p on its own, ungated (not in a ring solve)
    set_update(nullptr, OSC_XMODE_XR_SKIPS_X | OSC_XMODE_P_APPLIES_X, it == 1 ? x1_in : nullptr, h.alpha.p, Pbuf, nullptr);
    for_windows(ua, [&](const UpdateArgs& w) { launch_update_x(w, grid, h.stream); });
    xs.finished(it);
  }

  // everything of iteration `it` up to its residual, gated on iteration it - 1
  // (overlap: no gates -- an iteration writes scratch arrays only until the host has seen its predecessor unconverged)
  void enqueue(int it, bool speculative) {
    if (gram_route && it <= 2) return;  // (both ran inside the INIT pass; their residuals are out)
    if (gram4_taken && it >= 4) return;  // (x4 is written and the solve is known to end in iteration 4: nothing is left to launch)
    const Gate g{it > 1 && !overlap ? reinterpret_cast<const float*>(res_slots) + (it - 1) : nullptr, tol};
    host::CgXSchedule::IterForm form{false, host::CgXSchedule::XR_SKIPS_X};
    if (!ringed()) form = xs.enqueue(it, speculative);
    if (gram4_planned && it == 3) {
      // All four residuals are out (the host has read word 1, the last the scalars kernel publishes).  A solve they show to end in
      // iteration 4 needs no A p4: the matvec's last form writes x4 = x3 + alpha4 p4 from its epilogue, and that is the solve's
      // one operator apply (profile slot 0).
      const volatile float* words = reinterpret_cast<const volatile float*>(h.res_host);
      if (host::anchor_gram4_last_form(words[1], words[2], words[3], words[4], (double)tol)) {
        ProfScope ps(h, 0, 4);
        BlkArgs fa = ba;
        fa.X = dir(3);
        fa.OUT = nullptr;
        fa.gate = nullptr;
        fa.gate_tol = 0.f;
        BlkFused f{b.R, nullptr, alpha_of(3), h.beta.p, h.gram_go.p + 1, fused_md_B, fused_md_const};
        f.X = b.X;
        f.alpha_last = alpha_of(4);
        // (go[2] is this predicate on the same bits: the INIT pass left e in x and no r2, and the folded form is the one to run)
        if (gram4_fold) f.go_fold = h.gram_go.p + 2;
        launch_apply_blocked_fused(fa, grid, h.stream, f, plan.shape);
        h.blk_applies += 1;
        gram4_taken = true;
        ring.applied = 4;  // (directions 3 and 4 are in x: no pass is left)
        h.at(Level::gram4).solves += 1;
        if (gram4_fold) h.folded_four_step_solves += 1;
        h.at(Level::gram4).last = true;
        return;
      }
      // (iteration 4 runs on the summed route and publishes its own residual: the word is pending again)
      reinterpret_cast<volatile uint32_t*>(h.res_host)[4] = kCtrlPending;
    }
    if (gram3_route && it == 3) {
      // The whole iteration in the matvec's fused form: r3 over r2, p4 into dir(4); alpha3, beta3, r3 . z3 and the residual are
      // out already.  (A sample of iteration 4: a solve that stops in 3 had the launch gated off.)
      ProfScope ps(h, 4, 4);
      BlkArgs fa = ba;
      fa.X = dir(3);
      fa.OUT = nullptr;
      fa.gate = nullptr;
      fa.gate_tol = 0.f;
      const BlkFused f{b.R, dir(4), alpha_of(3), h.beta.p, h.gram_go.p + 1, fused_md_B, fused_md_const};
      launch_apply_blocked_fused(fa, grid, h.stream, f, plan.shape);
      h.blk_applies += 1;
      return;
    }
    const host::ApSource ap_src = host::cg_ap_source(it, first_ap_done, second_ap_ready);
    if (it > 1 && !(gram_route && it == 3) && !(gram3_route && it == 4)) {  // (the fused INIT pass left p3 in dir(3), the fused matvec p4 in dir(4))
      ProfScope ps(h, 2, it);
      if (ringed()) {
        // the slot p_it goes to still holds a direction x lacks: this iteration's flush, then p_it = z + beta p_{it-1}
        // (alpha: iteration it - 1's, as its x-r kernel left it; a p update that applies no x update does not read it)
        ring_pass(ring.flush_before_p(it), g.p);
        set_update(g.p, 0, nullptr, alpha_of(it - 1), dir(it - 1), dir(it));
      } else {
        // p = z + beta p (solver.py:32-36), and iteration it - 1's x += alpha p (solver.py:27) with the p it replaces
        // (Xin: this launch applies iteration it - 1's x update)
        set_update(g.p, form.p_applies_x ? OSC_XMODE_P_APPLIES_X : 0, it == 2 ? x1_in : nullptr, h.alpha.p, Pbuf, nullptr);
      }
      if (ap_src == host::ApSource::p_update) {  // ... and A p2 over A p1, with the p . Ap partials (k_update_p_ap2; alpha: iteration 1's)
        ua.T = h.Tap.p;
        ua.APout = APbuf;
        for_windows(ua, [&](const UpdateArgs& w) { launch_update_p_ap2(w, grid, h.stream); });
        ua.T = nullptr;
        ua.APout = nullptr;
      } else {
        update_p();
      }
    }
    if (ap_src == host::ApSource::p_update) {
      // (the p update left A p2 in the AP array and the p . Ap partials in part0, which this iteration's x-r kernel overwrites)
      launch_reduce_alpha(h.part0.p, grid, b.ld, b.c0, b.c1, h.rz.p, alpha_of(it), g, h.stream);
      h.at(Level::w3).solves += 1;
    } else if (ap_src == host::ApSource::init_pass) {
      // (the INIT pass left A p1 in the AP array and the p . Ap partials in part1, which this iteration's x-r kernel overwrites)
      launch_reduce_alpha(h.part1.p, grid, b.ld, b.c0, b.c1, h.rz.p, alpha_of(it), g, h.stream);
    } else if (ba.nb > 0) {  // Ap and column sums of p.Ap
      ProfScope ps(h, 0, it);
      ba.X = cf.X = dir(it);
      ba.OUT = cf.OUT = APbuf;
      apply_blocked(h, plan, ba, cf, grid, g);
      h.blk_applies += 1;
    } else {
      sa.X = dir(it);
      sa.OUT = APbuf;
      sa.xblk = plan.pblk ? h.N : 0;
      sa.pblk = 0;
      sa.gate = g.p;
      sa.gate_tol = tol;
      spmm_slabbed(h, plan, SPMM_AP, sa, grid, it);
    }
    if (ap_src == host::ApSource::matvec)
      launch_reduce_alpha(h.part0.p, grid + (ba.nb > 0 ? cf.chunks : 0), b.ld, b.c0, b.c1, h.rz.p, alpha_of(it), g, h.stream);
    {
      ProfScope ps(h, 1, it);
      if (ringed()) {
        set_update(g.p, OSC_XMODE_XR_SKIPS_X | (ring.xr_last(it) ? OSC_XMODE_XR_BARE : 0), nullptr, alpha_of(it), xr_p(it), xr_pout(it));
      } else {  // (Xin: the forms that carry an x update here carry iteration it's)
        const int32_t xmode = form.xr == host::CgXSchedule::XR_LAST ? OSC_XMODE_XR_LAST : form.xr == host::CgXSchedule::XR_SKIPS_X ? OSC_XMODE_XR_SKIPS_X : 0;
        set_update(g.p, xmode, it == 1 ? x1_in : nullptr, h.alpha.p, Pbuf, nullptr);
      }
      update_xr();
    }
    publish_residual(it, g);
  }

  // beta, the residual of iteration `it` and its way to the host: mapped, overlap via the second stream, copy + event
  void publish_residual(int it, Gate g) {
    if (mapped) {
      launch_reduce_beta(h.part0.p, h.part1.p, grid, b.ld, b.c0, b.c1, h.rz.p, h.beta.p, res_slots + it, g, h.stream,
                         done_ctr + it, h.res_host_dev + it);
      return;
    }
    launch_reduce_beta(h.part0.p, h.part1.p, grid, b.ld, b.c0, b.c1, h.rz.p, h.beta.p, res_slots + it, g, h.stream);
    if (overlap) {  // max over the shards (solver.py:29) and its way to the host, beside the next iteration's first kernels
      HIP_CHECK(hipEventRecord(h.step_events[(size_t)it], h.stream));
      HIP_CHECK(hipStreamWaitEvent(h.comm_stream, h.step_events[(size_t)it], 0));
      h.comm->allreduce(res_slots + it, 1, COMM_F32, COMM_MAX, h.comm_stream);
      launch_publish_word(res_slots + it, reinterpret_cast<uint32_t*>(h.res_host_dev + it), h.comm_stream);
      return;
    }
    // column-sharded (not mapped: there is a communicator): the stop test is the max over all shards (solver.py:29)
    h.comm->allreduce(res_slots + it, 1, COMM_F32, COMM_MAX, h.stream);
    HIP_CHECK(hipMemcpyAsync(h.res_host + it, res_slots + it, 4, hipMemcpyDeviceToHost, h.stream));
    HIP_CHECK(hipEventRecord(h.iter_events[(size_t)it], h.stream));
  }

  void idle_before_wait(int it) {
    if (gram4_taken) return;  // (x is complete)
    if (ringed()) {
      // the pending directions up to `it` go into x behind its x-r kernel, while the host waits for its residual
      ring_pass(ring.pass_before_wait(it), nullptr);
    } else if (xs.finish_before_wait(it)) {
      finish_x(it);  // (the expected last one): its x update goes out at once
    }
  }
  float wait(int it) {  // iteration it's residual, into the handle's history
    float res;
    if (polled) {  // (overlap: the word comes out of the second stream)
      const uint32_t bits = poll_host_word(h, reinterpret_cast<volatile uint32_t*>(h.res_host) + it,
                                           overlap ? h.comm_stream : nullptr, "a CG iteration's residual");
      std::memcpy(&res, &bits, 4);
    } else {
      HIP_CHECK(hipEventSynchronize(h.iter_events[(size_t)it]));
      res = h.res_host[it];
    }
    h.history.push_back(res);
    return res;
  }
  void go_on(int it) {  // the solve goes on behind `it` ... from the r this iteration computed but did not keep
    if (ringed() ? ring.restore_r(it) : xs.restore_r(it)) {
      set_update(nullptr, OSC_XMODE_XR_SKIPS_X, nullptr, alpha_of(it), xr_p(it), xr_pout(it));
      update_xr();
    }
  }

  CgResult finish(int iters) {
    h.predicted_iters[b.kind] = iters;
    // the last iteration's x update rode in a gated p update that did not run (the solve converged under a speculative
    // iteration): alpha and p are still that iteration's
    if (gram4_taken) {
      // (x4 was written by iteration 3's launch; the ring holds nothing)
    } else if (ringed()) {  // what the ring still holds for x: with at most K iterations the solve's only x pass
      ring_pass(ring.final_pass(iters), nullptr);
    } else if (xs.finish_at_end(iters)) {
      finish_x(iters);
    }
    h.x_ring_k = ring.K;
    h.x_ring_flushes = ringed() ? ring.flushes : 0;
    h.x_ring_passes = ringed() ? ring.passes : 0;
    // The solution is complete once the last residual is out; what may still be queued are the gated-off launches of
    // the speculative iteration (they return at once and write nothing).  With the polled read-back the stream is left
    // to drain on its own -- later calls are ordered behind it anyway; the copy + event path keeps its full wait.
    // (overlap: the same; the second stream is drained by whoever next touches the residual slots it writes -- drain_comm_stream)
    // (the route without a fourth matvec has every residual before its first N x D pass: what is queued then is the solve itself,
    // and it is waited for, so that the caller's time is the solve's)
    if (!polled || h.prof_on || gram4_taken) sync(h);
    drop_speculative_samples(h, prof_mark, iters);
    return CgResult{iters, h.history.empty() ? 0.f : h.history.back(), b.X};
  }
};

}  // namespace

// cg_solve (solver.py:6-37) on the device; returns once the last residual is out (what may still be queued then touches
// scratch arrays only, or is the ring's last x pass, and later calls are ordered behind it by the stream; a solve on the route
// without a fourth matvec, whose residuals are out before its first pass, returns when its last launch has finished).  Which iteration is enqueued when is
// host::cg_host_loop's business (host_logic.hpp; the sweeps under tests/host_logic run that same function against a model
// of the device's gating); CgSolve is what it drives.
CgResult run_cg(L& h, const OpParams& op, const CgBuffers& b, bool with_path, int max_iters, float tol) {
  if (row_mode(h) && b.ld == h.ld) return run_cg_rows(h, op, b, with_path, max_iters, tol);
  {
    CgResult one{};
    if (run_cg_small(h, op, b, with_path, max_iters, tol, one)) return one;
  }
  bool allow_gram = true, allow_poly = true;
  for (int attempt = 0; attempt < 3; ++attempt) {
    CgSolve s(h, op, b, with_path, max_iters, tol, allow_gram, allow_poly);
    s.init();
    s.plan_ring();
    h.history.clear();
    s.prof_mark = h.prof_pending.size();
    if (s.poly_pending) {
      if (s.poly_done()) return s.finish(4);
      // The solve does not end in iteration 4 after all (or a column's sums were unusable): the pass was gated off and nothing but
      // scratch scalars was written.  The same solve again on the folded form's route, which takes it from there as it always did.
      h.at(Level::w4).redos += 1;
      allow_poly = false;
      continue;
    }
    const int iters = host::cg_host_loop(max_iters, s.stop_guess, (double)tol, s);
    if (s.gram_route && iters < 3) {
      // The solve stopped before iteration 3 (or a column's sums were unusable): the fused pass was gated off, nothing but
      // scratch scalars was written.  The same solve again, on the depth-2 route; its count keeps the next one off the route.
      h.at(Level::gram).redos += 1;
      h.at(Level::gram).solves -= 1;
      if (s.gram3_route) h.at(Level::gram3).solves -= 1;
      if (s.gram4_taken) h.at(Level::gram4).solves -= 1;
      if (s.gram4_taken && s.gram4_fold) h.folded_four_step_solves -= 1;
      h.cached_inits -= 1;  // (the solve counts once, where it ends)
      allow_gram = false;
      continue;
    }
    return s.finish(iters);
  }
  throw std::runtime_error("run_cg: the summed route did not finish");
}

// Column-sharded runs: every rank owns columns [c0, c1) of an N x ld array.  Make the whole array valid on every
// rank: one ncclBroadcast of each rank's packed slab (slab widths may differ by 4 columns, so not an all-gather).
// Collective: every rank must call it.
void gather_columns(L& h, float* arr) {
  if (!h.comm || h.world <= 1) return;
  const int32_t q = h.dcols / 4;
  int32_t wmax = 0;
  for (int r = 0; r < h.world; ++r) wmax = std::max(wmax, (int32_t)(((int64_t)q * (r + 1) / h.world - (int64_t)q * r / h.world) * 4));
  h.comm_buf.alloc((size_t)h.N * wmax);
  for (int r = 0; r < h.world; ++r) {
    const int32_t lo = (int32_t)((int64_t)q * r / h.world) * 4, hi = (int32_t)((int64_t)q * (r + 1) / h.world) * 4;
    const int32_t w = hi - lo;
    if (w <= 0) continue;
    if (r == h.rank)
      HIP_CHECK(hipMemcpy2DAsync(h.comm_buf.p, (size_t)w * 4, arr + lo, (size_t)h.ld * 4, (size_t)w * 4, (size_t)h.N,
                                 hipMemcpyDeviceToDevice, h.stream));
    h.comm->broadcast_group({CommXfer{h.comm_buf.p, (size_t)h.N * w * 4, r}}, h.stream);
    if (r != h.rank)
      HIP_CHECK(hipMemcpy2DAsync(arr + lo, (size_t)h.ld * 4, h.comm_buf.p, (size_t)w * 4, (size_t)w * 4, (size_t)h.N,
                                 hipMemcpyDeviceToDevice, h.stream));
  }
}

// ---- row-sharded CG (BASELINE north_star wording) --------------------------------------------------------------
// Rank r owns rows [N r/G, N (r+1)/G) of every N x D array and of the lattice graph.  Per iteration: the local rows of
// the search direction p are exchanged so every rank holds all of p for the neighbour gathers ("halo": on i.i.d.
// anchors ~all rows are somebody's neighbour, so the halo is the whole array), and the column sums (p.Ap, then
// [r.r, r.z]) are completed with all-reduces of fp64 D-vectors before alpha / beta / the residual are formed.

std::vector<RowShard> row_shards(const L& h) {
  std::vector<RowShard> v;
  if (h.comm) {
    v.push_back({h.N * h.rank / h.world, h.N * (h.rank + 1) / h.world});
  } else {
    const int V = std::max(1, h.fake_row_shards);
    for (int s = 0; s < V; ++s) v.push_back({h.N * s / V, h.N * (s + 1) / V});
  }
  return v;
}

// make every rank's copy of `arr` complete: each rank broadcasts its own row block (grouped, in place)
void exchange_rows(L& h, float* arr, int32_t ld) {
  if (!h.comm) return;  // (a 1-rank communicator still runs the calls: that is how one GPU exercises this path)
  std::vector<CommXfer> pieces;
  for (int r = 0; r < h.world; ++r) {
    const int64_t a = h.N * r / h.world, b = h.N * (r + 1) / h.world;
    pieces.push_back(CommXfer{arr + (size_t)a * ld, (size_t)(b - a) * ld * 4, r});
  }
  h.comm->broadcast_group(pieces, h.stream);
}

void allreduce_sums(L& h, double* buf, size_t n) {
  if (!h.comm) return;
  h.comm->allreduce(buf, n, COMM_F64, COMM_SUM, h.stream);
}


// ---- halo lists ---------------------------------------------------------------------------------------------------
// Which rows of the search direction a rank needs from its peers: the off-partition column ids its ELL rows (and its
// rows of the chain's path graph) reference.  The adjacency is symmetric (by construction of the build, enforced on
// injection), so "peer q needs my row i" == "my row i has a neighbour in q's row block": both lists of a pair of
// ranks follow from each rank's OWN rows, sorted by row id on both sides, and no index lists are exchanged -- only the
// counts, once, as a consistency check and to take the same full-exchange decision everywhere.
void build_halo_plan(L& h) {
  L::HaloPlan& hp = h.halo;
  const int G = h.world, me = h.rank;
  auto lo = [&](int r) { return host::row_lo(h.N, G, r); };
  const int64_t r0 = lo(me), r1 = lo(me + 1), nloc = r1 - r0;
  std::vector<int32_t> col((size_t)nloc * h.width), deg((size_t)nloc);
  if (nloc > 0) {
    HIP_CHECK(hipMemcpyAsync(col.data(), h.ell_col.p + (size_t)r0 * h.width, col.size() * 4, hipMemcpyDeviceToHost, h.stream));
    HIP_CHECK(hipMemcpyAsync(deg.data(), h.deg.p + r0, (size_t)nloc * 4, hipMemcpyDeviceToHost, h.stream));
  }
  sync(h);
  std::vector<std::pair<int64_t, int64_t>> chain_edges;  // path graph: consecutive chain nodes (graph.py:96-111), device row ids
  if (h.chain_present && h.lamP > 0.0f) {
    auto id = [&](int32_t v) { return permuted(h) ? h.inv_h[(size_t)v] : v; };
    for (size_t t = 0; t + 1 < h.chain_nodes.size(); ++t) chain_edges.emplace_back(id(h.chain_nodes[t]), id(h.chain_nodes[t + 1]));
  }
  host::HaloLists hl = host::build_halo_lists(h.N, G, me, h.width, col.data(), deg.data(), chain_edges);
  hp.give_off = hl.give_off;
  hp.need_off = hl.need_off;
  const std::vector<int32_t>&gi = hl.give_idx, &ni = hl.need_idx;
  hp.give_rows = (int64_t)gi.size();
  hp.need_rows = (int64_t)ni.size();
  // counts of every (rank, peer) pair, all-gathered: row r = [need from 0..G-1 | give to 0..G-1] of rank r
  DevBuf<int32_t> cnt_d;
  cnt_d.alloc((size_t)G * 2 * G);
  std::vector<int32_t> mine((size_t)2 * G), all((size_t)G * 2 * G);
  for (int q = 0; q < G; ++q) {
    mine[(size_t)q] = (int32_t)(hp.need_off[(size_t)q + 1] - hp.need_off[(size_t)q]);
    mine[(size_t)G + q] = (int32_t)(hp.give_off[(size_t)q + 1] - hp.give_off[(size_t)q]);
  }
  HIP_CHECK(hipMemcpyAsync(cnt_d.p + (size_t)me * 2 * G, mine.data(), (size_t)2 * G * 4, hipMemcpyHostToDevice, h.stream));
  h.comm->allgather(cnt_d.p, (size_t)2 * G * 4, h.stream);
  HIP_CHECK(hipMemcpyAsync(all.data(), cnt_d.p, all.size() * 4, hipMemcpyDeviceToHost, h.stream));
  sync(h);
  const host::HaloDecision dec = host::halo_decide(h.N, G, all);
  if (!dec.consistent) throw CommError("halo plan: need / give counts of a rank pair differ (asymmetric lattice graph?)");
  hp.need_rows_max = dec.need_rows_max;
  bool full = dec.full;
  const int force = h.halo_force;  // OSC_HALO = full | lists: force one exchange form (tests, A/B); same on every rank
  if (force == 1) full = true;
  if (force == 2) full = false;
  hp.full = full;
  hp.give_idx.alloc(std::max<size_t>(1, gi.size()));
  hp.need_idx.alloc(std::max<size_t>(1, ni.size()));
  if (!gi.empty()) HIP_CHECK(hipMemcpyAsync(hp.give_idx.p, gi.data(), gi.size() * 4, hipMemcpyHostToDevice, h.stream));
  if (!ni.empty()) HIP_CHECK(hipMemcpyAsync(hp.need_idx.p, ni.data(), ni.size() * 4, hipMemcpyHostToDevice, h.stream));
  if (!full) {
    hp.send.alloc(std::max<size_t>(1, gi.size() * (size_t)h.ld));
    hp.recv.alloc(std::max<size_t>(1, ni.size() * (size_t)h.ld));
  }
  sync(h);
  hp.epoch = h.derived.epoch;
}

// the per-iteration halo exchange of `arr` (N x ld, every rank's own row block current): afterwards the rows this
// rank's operator gathers from are current too
void halo_exchange(L& h, float* arr, int32_t ld) {
  if (!h.comm) return;
  if (h.halo.epoch != h.derived.epoch) build_halo_plan(h);
  L::HaloPlan& hp = h.halo;
  if (hp.full || ld != h.ld) {
    exchange_rows(h, arr, ld);
    return;
  }
  if (hp.give_rows > 0) launch_move_rows(hp.send.p, arr, hp.give_idx.p, hp.give_rows, ld, false, h.stream);  // pack
  std::vector<CommXfer> sends, recvs;
  for (int q = 0; q < h.world; ++q) {
    const int64_t g0 = hp.give_off[(size_t)q], g1 = hp.give_off[(size_t)q + 1];
    const int64_t n0 = hp.need_off[(size_t)q], n1 = hp.need_off[(size_t)q + 1];
    if (g1 > g0) sends.push_back(CommXfer{hp.send.p + (size_t)g0 * ld, (size_t)(g1 - g0) * ld * 4, q});
    if (n1 > n0) recvs.push_back(CommXfer{hp.recv.p + (size_t)n0 * ld, (size_t)(n1 - n0) * ld * 4, q});
  }
  h.comm->exchange(sends, recvs, h.stream);
  if (hp.need_rows > 0) launch_move_rows(arr, hp.recv.p, hp.need_idx.p, hp.need_rows, ld, true, h.stream);  // unpack
}

CgResult run_cg_rows(L& h, const OpParams& op, const CgBuffers& b, bool with_path, int max_iters, float tol) {
  const std::vector<RowShard> shards = row_shards(h);
  const int V = (int)shards.size();
  const int grid = cg_grid(h);
  const host::ApplyPlan plan = apply_plan(h, b.c0, b.c1, b.ld, with_path);
  const size_t pn = (size_t)V * grid * b.ld;  // one block of partial rows per local shard
  if (h.part0.n < pn) h.part0.alloc(pn);
  if (h.part1.n < pn) h.part1.alloc(pn);
  h.sums.alloc((size_t)2 * b.ld);
  double* s0 = h.sums.p;
  double* s1 = h.sums.p + b.ld;
  ensure_ctrl(h, (size_t)max_iters + 2);  // (every caller has sized them already, ensure_cg_scratch: nothing grows here)
  HIP_CHECK(hipMemsetAsync(h.res_bits.p, 0, ((size_t)max_iters + 2) * 4, h.stream));
  const float* res_dev = reinterpret_cast<const float*>(h.res_bits.p);
  SpmmArgs sa{};
  sa.g = graph_view(h, with_path);
  sa.op = op;
  sa.B = b.B;
  sa.psi = b.psi;
  sa.ld = b.ld;
  sa.c0 = b.c0;
  sa.c1 = b.c1;
  UpdateArgs ua{};
  ua.X = b.X;
  ua.R = b.R;
  ua.P = b.P;
  ua.AP = b.AP;
  ua.B = b.B;
  ua.alpha = h.alpha.p;
  ua.beta = h.beta.p;
  ua.op = op;
  ua.ld = b.ld;
  ua.c0 = b.c0;
  ua.c1 = b.c1;
  auto for_shards_spmm = [&](int mode, int iter) {
    for (int s = 0; s < V; ++s) {
      sa.row0 = shards[(size_t)s].r0;
      sa.N = shards[(size_t)s].r1;
      sa.part = h.part0.p + (size_t)s * grid * b.ld;
      spmm_slabbed(h, plan, mode, sa, grid, iter);
    }
  };
  // r = b - A x0 ; z ; p ; rz
  sa.X = b.x0;
  sa.OUT = b.X;
  sa.R = b.R;
  sa.P = b.P;
  sa.U = b.rhsU;
  sa.Y = b.rhsY;
  sa.gate = nullptr;
  for_shards_spmm(SPMM_INIT, 0);
  launch_reduce_sum(h.part0.p, V * grid, b.ld, b.c0, b.c1, s0, h.stream);
  allreduce_sums(h, s0 + b.c0, (size_t)(b.c1 - b.c0));
  launch_finish_init(s0, b.c0, b.c1, h.rz.p, h.stream);
  halo_exchange(h, b.P, b.ld);
  sa.X = b.P;
  sa.OUT = b.AP;

  auto enqueue_iter = [&](int it) {
    const Gate g{it > 1 ? res_dev + (it - 1) : nullptr, tol};
    sa.gate = g.p;
    sa.gate_tol = tol;
    ua.gate = g.p;
    ua.gate_tol = tol;
    if (it > 1) {
      for (int s = 0; s < V; ++s) {
        ua.row0 = shards[(size_t)s].r0;
        ua.N = shards[(size_t)s].r1;
        ProfScope ps(h, 2, it);
        for_windows(ua, [&](const UpdateArgs& w) { launch_update_p(w, grid, h.stream); });
      }
      halo_exchange(h, b.P, b.ld);  // the halo exchange of this iteration
    }
    for_shards_spmm(SPMM_AP, it);
    launch_reduce_sum_gated(h.part0.p, V * grid, b.ld, b.c0, b.c1, s0, g, h.stream);
    allreduce_sums(h, s0 + b.c0, (size_t)(b.c1 - b.c0));
    launch_finish_alpha(s0, b.c0, b.c1, h.rz.p, h.alpha.p, g, h.stream);
    for (int s = 0; s < V; ++s) {
      ua.row0 = shards[(size_t)s].r0;
      ua.N = shards[(size_t)s].r1;
      ua.part_rr = h.part0.p + (size_t)s * grid * b.ld;
      ua.part_rz = h.part1.p + (size_t)s * grid * b.ld;
      ProfScope ps(h, 1, it);
      for_windows(ua, [&](const UpdateArgs& w) { launch_update_xr(w, grid, h.stream); });
    }
    launch_reduce_sum_gated(h.part0.p, V * grid, b.ld, b.c0, b.c1, s0, g, h.stream);
    launch_reduce_sum_gated(h.part1.p, V * grid, b.ld, b.c0, b.c1, s1, g, h.stream);
    allreduce_sums(h, s0, (size_t)2 * b.ld);  // [r.r | r.z] in one message
    launch_finish_beta(s0, s1, b.c0, b.c1, h.rz.p, h.beta.p, h.res_bits.p + it, g, h.stream);
    HIP_CHECK(hipMemcpyAsync(h.res_host + it, h.res_bits.p + it, 4, hipMemcpyDeviceToHost, h.stream));
    HIP_CHECK(hipEventRecord(h.iter_events[(size_t)it], h.stream));
  };

  h.history.clear();
  CgResult out{max_iters, 0.f, b.X};
  const size_t prof_mark = h.prof_pending.size();
  enqueue_iter(1);
  for (int it = 1; it <= max_iters; ++it) {
    if (it < max_iters) enqueue_iter(it + 1);
    HIP_CHECK(hipEventSynchronize(h.iter_events[(size_t)it]));
    const float res = h.res_host[it];
    h.history.push_back(res);
    out.res = res;
    if ((double)res <= (double)tol) {
      out.iters = it;
      break;
    }
  }
  exchange_rows(h, b.X, b.ld);  // every rank leaves with the whole solution
  sync(h);
  drop_speculative_samples(h, prof_mark, out.iters);
  return out;
}

bool row_mode(const L& h) { return h.shard_mode == 1 && (h.comm != nullptr || h.fake_row_shards > 1); }

// The ONE place the per-handle OSC_* switches are read (osc_create, osc_rebuild_graph).  Process-wide ones are read where
// the process-wide object is made: OSC_POOL_MB (device memory pool), OSC_PINNED_DL / OSC_COPY_THREADS (read-back staging),
// OSC_LOOPBACK_TIMEOUT_S / OSC_RCCL_PROXY (communicator backends, comm.hip), OSC_LD (osc_create, before the arrays are sized).

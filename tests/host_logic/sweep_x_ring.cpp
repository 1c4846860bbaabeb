// Sweep of the direction ring's host logic (oscillink_amd/csrc/host_logic.hpp: plan_x_ring, CgXRing) against a model of
// the device, built with a plain host compiler by tests/test_x_ring_host.py (once plain, once under
// -fsanitize=address,undefined).  The host loop of run_cg (osc_solve.hip) -- the library's loop, cg_host_loop -- runs
// for every (predicted iterations, stopping iteration, max_iters <= 12, K, last-form switch); which iterations are
// enqueued speculatively follows from the prediction, as in run_cg.  The "device" executes the launches in order with
// the gating rule of the kernels (a gated launch of iteration it runs iff iteration it - 1 did not converge; an ungated
// one always runs) and tracks which iteration's direction and alpha each slot holds.  Checked: every real iteration's
// direction is applied exactly once, in ascending order, with its own alpha, before its slot is overwritten; none
// behind the stop; a pass holds 1..K directions; the first pass, and only it, starts from x0; every kernel that reads r
// finds the r it expects.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <utility>
#include <vector>

#include "../../oscillink_amd/csrc/host_logic.hpp"
#include "cg_loop_model.hpp"

using namespace osc::host;

static int g_fail = 0;
static long g_cases = 0;
#define CHECK(cond, ...)                                                  \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::fprintf(stderr, "FAIL %s:%d %s  ", __FILE__, __LINE__, #cond); \
      std::fprintf(stderr, __VA_ARGS__);                                  \
      std::fprintf(stderr, "\n");                                         \
      if (++g_fail > 20) std::exit(1);                                    \
    }                                                                     \
  } while (0)

static void check_ring(int K, int max_iters, int stop_guess, int converge_at, bool last_form) {
  ++g_cases;
  CgXRing ring;
  ring.K = K, ring.last_form = last_form, ring.stop_guess = stop_guess, ring.max_iters = max_iters;
  std::vector<int> slot_dir((size_t)K, 0), slot_alpha((size_t)K, 0);  // the iteration whose p / alpha a slot holds
  slot_dir[(size_t)(1 % K)] = 1;                                       // the INIT pass leaves direction 1
  int r_ver = 0, x_upto = 0;  // r of iteration r_ver; x holds directions 1 .. x_upto
  bool x_in_X = false;        // a pass has written X (before that x is x0, wherever that lives)
  std::vector<int> applied((size_t)max_iters + 3, 0);
  auto converged = [&](int it) { return converge_at > 0 && it == converge_at; };
  auto runs = [&](int it, bool gated) { return !gated || it == 1 || !converged(it - 1); };
  auto tag = [&]() {
    static char buf[160];
    std::snprintf(buf, sizeof buf, "K %d max_iters %d guess %d converge_at %d last %d", K, max_iters, stop_guess, converge_at, (int)last_form);
    return buf;
  };
  auto pass = [&](CgXRing::Pass ps, int gate_iter /* 0: ungated */) {
    if (ps.count <= 0) return;
    CHECK(ps.count <= K && ps.count <= kXRingMax, "%s: pass of %d directions", tag(), ps.count);
    if (gate_iter != 0 && !runs(gate_iter, true)) return;
    CHECK((ps.first == 1) == !x_in_X, "%s: pass from direction %d, x %s", tag(), ps.first, x_in_X ? "already in X" : "still x0");
    for (int j = ps.first; j < ps.first + ps.count; ++j) {
      CHECK(j == x_upto + 1, "%s: direction %d applied behind %d", tag(), j, x_upto);
      CHECK(slot_dir[(size_t)(j % K)] == j, "%s: slot of direction %d holds %d", tag(), j, slot_dir[(size_t)(j % K)]);
      CHECK(slot_alpha[(size_t)(j % K)] == j, "%s: alpha slot of iteration %d holds %d", tag(), j, slot_alpha[(size_t)(j % K)]);
      ++applied[(size_t)j];
      x_upto = j;
    }
    x_in_X = true;
  };
  auto enqueue_iter = [&](int it, bool /*speculative*/) {
    if (it > 1) {
      pass(ring.flush_before_p(it), it);
      if (runs(it, true)) {  // p_it = z(r_{it-1}) + beta p_{it-1} into slot it % K
        CHECK(r_ver == it - 1, "%s: p update of iteration %d reads r of %d", tag(), it, r_ver);
        CHECK(slot_dir[(size_t)((it - 1) % K)] == it - 1, "%s: p update of %d reads direction %d", tag(), it, slot_dir[(size_t)((it - 1) % K)]);
        const int old = slot_dir[(size_t)(it % K)];
        CHECK(old == 0 || old <= x_upto, "%s: direction %d overwritten before it is in x (x holds up to %d)", tag(), old, x_upto);
        slot_dir[(size_t)(it % K)] = it;
      }
    }
    if (runs(it, true)) {  // matvec, reduce_alpha, x-r kernel
      CHECK(slot_dir[(size_t)(it % K)] == it, "%s: matvec of iteration %d gathers direction %d", tag(), it, slot_dir[(size_t)(it % K)]);
      const int olda = slot_alpha[(size_t)(it % K)];
      CHECK(olda == 0 || olda <= x_upto, "%s: alpha of iteration %d overwritten before use", tag(), olda);
      slot_alpha[(size_t)(it % K)] = it;
      CHECK(r_ver == it - 1, "%s: x-r kernel of iteration %d reads r of %d", tag(), it, r_ver);
      if (!ring.xr_last(it)) r_ver = it;
    } else {
      (void)ring.xr_last(it);  // (the host calls it whether or not the launch runs)
    }
  };
  auto idle_before_wait = [&](int it) { pass(ring.pass_before_wait(it), 0); };
  auto wait = [&](int it) { return converged(it) ? 0.f : 1.f; };  // (against tol 0.5)
  auto go_on = [&](int it) {
    if (ring.restore_r(it)) {
      CHECK(r_ver == it - 1, "%s: redoing the r update of iteration %d from r of %d", tag(), it, r_ver);
      CHECK(slot_alpha[(size_t)(it % K)] == it, "%s: redoing the r update of %d with alpha of %d", tag(), it, slot_alpha[(size_t)(it % K)]);
      r_ver = it;
    }
  };
  auto ops = cg_loop_model(enqueue_iter, idle_before_wait, wait, go_on);
  const int iters = cg_host_loop(max_iters, stop_guess, 0.5, ops);  // the library's loop
  pass(ring.final_pass(iters), 0);
  for (int it = 1; it <= max_iters + 1; ++it)
    CHECK(applied[(size_t)it] == (it <= iters ? 1 : 0), "%s: direction %d applied %d times (solve stopped in %d)", tag(), it,
          applied[(size_t)it], iters);
  CHECK(ring.flushes <= ring.passes && ring.passes >= 1, "%s: %d flushes, %d passes", tag(), ring.flushes, ring.passes);
  if (iters <= K && (stop_guess == iters || (iters == max_iters && (stop_guess <= 0 || stop_guess > iters))))
    CHECK(ring.passes == 1 && ring.flushes == 0, "%s: a right guess within the ring takes %d passes", tag(), ring.passes);
}

static void check_planner() {
  const int64_t arr = 300ll << 20;
  for (int pred = 0; pred <= 13; ++pred)
    for (int mi = 1; mi <= 12; ++mi)
      for (int forced : {-1, 0, 1, 2, 3, 4, 7})
        for (int m = 0; m < 8; m += 2)
          for (int64_t free_b : {(int64_t)0, arr, 4 * arr, 4 * arr + 1, 8 * arr, 12 * arr, (int64_t)200 << 30}) {
            XRingInputs in;
            in.predicted = pred, in.max_iters = mi, in.array_bytes = arr, in.free_bytes = free_b;
            in.ungated = (m & 2) != 0, in.xdefer = (m & 4) == 0, in.forced = forced;
            const int K = plan_x_ring(in);
            CHECK(K >= 1 && K <= kXRingMax && K <= std::max(1, mi), "K %d", K);
            CHECK((int64_t)(K - 1) * arr <= free_b / 4, "K %d does not fit %lld", K, (long long)free_b);
            if (in.ungated || !in.xdefer || forced == 0) CHECK(K == 1, "ring on where it must be off: K %d", K);
            if (forced < 0 && pred <= 0) CHECK(K == 1, "no prediction: K %d", K);
            if (forced < 0 && !in.ungated && in.xdefer && pred > 0 && free_b >= 12 * arr)
              CHECK(K == std::min({pred, kXRingMax, mi}), "pred %d max_iters %d: K %d", pred, mi, K);
            if (forced > 0 && !in.ungated && in.xdefer && free_b >= 12 * arr)
              CHECK(K == std::min({forced, kXRingMax, mi}), "forced %d max_iters %d: K %d", forced, mi, K);
          }
}

int main() {
  for (int K = 2; K <= kXRingMax; ++K)
    for (int max_iters = 1; max_iters <= 12; ++max_iters)
      for (int guess = 0; guess <= max_iters + 2; ++guess)        // 0: no prediction (every iteration speculates ahead)
        for (int conv = 0; conv <= max_iters + 1; ++conv)         // 0 / beyond max_iters: never converges
          for (int last = 0; last < 2; ++last) check_ring(K, max_iters, guess, conv > max_iters ? 0 : conv, last != 0);
  check_planner();
  if (g_fail) {
    std::fprintf(stderr, "%d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("x ring sweep ok: %ld schedules\n", g_cases);
  return 0;
}

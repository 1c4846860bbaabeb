// Sweep of the streamed second apply's host logic (host_logic.hpp: anchor_ap2_route, cg_ap_source) on the CPU, built by
// tests/test_anchor_ap2_host.py (once plain, once under -fsanitize=address,undefined).
// 1. The route's truth table against rules written out here: only on top of the depth-1 route, only in a solve that may run a
//    second iteration, and where the switch allows it (0 never, 1 always, unset from 96 000 rows on).
// 2. The library's host loop, cg_host_loop, against a model of the launches CgSolve::enqueue makes, for every (prediction,
//    stopping iteration, max_iters <= 12, K; K = 1: CgXSchedule, K >= 2: the direction ring) and every depth the INIT pass can
//    leave (0: nothing, 1: A p1, 2: A p1 and T).  The "device" runs the launches in order under the kernels' gating rule and
//    tracks what the AP array, the two partial arrays and r hold.  Checked: every real iteration has exactly one A p, from
//    exactly one source (INIT pass, p update, matvec), and no iteration behind the stop has any; the alpha reduction of an
//    iteration reads that iteration's p . Ap partials, and iteration 2's are read before anything overwrites them; the p
//    update that forms A p2 finds A p1 and T; every kernel that reads r or A p finds the one it expects; nothing runs behind
//    the stop.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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

static void check_route() {
  const int modes[] = {-1, 0, 1, -7, 5};
  const int64_t rows[] = {0, 1, 20000, 95999, 96000, 96001, 100000, 1000000, (int64_t)1 << 40};
  for (int mode : modes)
    for (int64_t N : rows)
      for (int d1 = 0; d1 < 2; ++d1)
        for (int mi = -1; mi <= 5; ++mi) {
          AnchorAp2Inputs in;
          in.mode = mode, in.N = N, in.depth1 = d1 != 0, in.max_iters = mi;
          bool want = d1 != 0 && mi >= 2;
          if (mode == 0) want = false;
          if (mode < 0 && N < 96000) want = false;
          CHECK(anchor_ap2_route(in) == want, "route: mode %d N %lld depth1 %d max_iters %d", mode, (long long)N, d1, mi);
          ++g_cases;
        }
  CHECK(!anchor_ap2_route(AnchorAp2Inputs{}), "default inputs take the route");
  for (int it = -1; it <= 14; ++it)
    for (int f = 0; f < 2; ++f)
      for (int s = 0; s < 2; ++s) {
        ApSource want = ApSource::matvec;
        if (it == 1 && f) want = ApSource::init_pass;
        if (it == 2 && f && s) want = ApSource::p_update;
        CHECK(cg_ap_source(it, f != 0, s != 0) == want, "source: it %d first %d second %d", it, f, s);
        ++g_cases;
      }
}

// what a partial array holds: 0 nothing, RZ0 the INIT pass's r . z, PAP + it iteration it's p . Ap, RES + it its r . r / r . z
enum { RZ0 = 1, PAP = 100, RES = 200 };

static void check_loop(int K, int max_iters, int stop_guess, int converge_at, int depth_asked) {
  ++g_cases;
  AnchorAp2Inputs a2;
  a2.mode = 1, a2.N = 1000, a2.depth1 = depth_asked >= 1, a2.max_iters = max_iters;
  const bool first = depth_asked >= 1, second = depth_asked >= 2 && anchor_ap2_route(a2);
  if (depth_asked >= 2 && max_iters == 1) CHECK(!second, "max_iters 1 takes depth 2");
  CgXSchedule xs;
  xs.stop_guess = stop_guess, xs.max_iters = max_iters;
  CgXRing ring;
  ring.K = K, ring.last_form = true, ring.stop_guess = stop_guess, ring.max_iters = max_iters;
  const bool ringed = K > 1;
  // after the INIT pass
  int ap_holds = first ? 1 : 0;  // the iteration whose A p the AP array holds
  bool t_valid = second;
  int part0 = RZ0, part1 = first ? PAP + 1 : 0;
  bool part0_read = false;  // the p . Ap partials in part0 have been reduced
  int r_ver = 0;
  std::vector<int> n_ap((size_t)max_iters + 3, 0), src_mask((size_t)max_iters + 3, 0);
  if (first) n_ap[1] = 1, src_mask[1] = 1 << (int)ApSource::init_pass;
  part0_read = true;  // (reduce_init has read the r . z partials)
  auto converged = [&](int it) { return converge_at > 0 && it == converge_at; };
  auto runs = [&](int it) { return it == 1 || !converged(it - 1); };
  char tag[160];
  std::snprintf(tag, sizeof tag, "K %d max_iters %d guess %d converge_at %d depth %d", K, max_iters, stop_guess, converge_at, depth_asked);
  auto enqueue_iter = [&](int it, bool speculative) {
    const bool run = runs(it);
    CHECK(!(run && converge_at > 0 && it > converge_at), "%s: iteration %d runs behind the stop", tag, it);
    CgXSchedule::IterForm form{false, CgXSchedule::XR_SKIPS_X};
    if (!ringed) form = xs.enqueue(it, speculative);
    const ApSource src = cg_ap_source(it, first, second);
    if (it > 1) {
      if (ringed) (void)ring.flush_before_p(it);
      if (run) {
        CHECK(r_ver == it - 1, "%s: p update of iteration %d reads r of %d", tag, it, r_ver);
        if (src == ApSource::p_update) {
          CHECK(it == 2 && t_valid, "%s: p update of %d forms A p without T", tag, it);
          CHECK(ap_holds == 1, "%s: p update of 2 finds A p of %d", tag, ap_holds);
          CHECK(part0_read, "%s: p update of 2 overwrites partials nobody read (%d)", tag, part0);
          ap_holds = 2, n_ap[2] += 1, src_mask[2] |= 1 << (int)src;
          part0 = PAP + 2, part0_read = false;
        }
      }
    }
    if (run) {
      if (src == ApSource::init_pass) {
        CHECK(ap_holds == 1 && part1 == PAP + 1, "%s: iteration 1 finds A p of %d, partials %d", tag, ap_holds, part1);
      } else if (src == ApSource::p_update) {
        CHECK(part0 == PAP + 2 && !part0_read, "%s: alpha of 2 reads partials %d", tag, part0);
        part0_read = true;
      } else {
        CHECK(part0_read, "%s: matvec of %d overwrites partials nobody read (%d)", tag, it, part0);
        ap_holds = it, n_ap[(size_t)it] += 1, src_mask[(size_t)it] |= 1 << (int)src;
        part0 = PAP + it, part0_read = true;  // (reduced right behind the matvec)
      }
      // the x-r kernel: r -= alpha A p, r . r -> part0, r . z -> part1
      CHECK(ap_holds == it, "%s: x-r kernel of %d reads A p of %d", tag, it, ap_holds);
      CHECK(r_ver == it - 1, "%s: x-r kernel of %d reads r of %d", tag, it, r_ver);
      CHECK(part0_read, "%s: x-r kernel of %d overwrites partials nobody read (%d)", tag, it, part0);
      part0 = part1 = RES + it;
      const bool keeps_r = ringed ? !ring.xr_last(it) : form.xr != CgXSchedule::XR_LAST;
      if (keeps_r) r_ver = it;
    } else if (ringed) {
      (void)ring.xr_last(it);
    }
  };
  auto idle_before_wait = [&](int it) {
    if (ringed) (void)ring.pass_before_wait(it);
    else if (xs.finish_before_wait(it)) xs.finished(it);
  };
  auto wait = [&](int it) { return converged(it) ? 0.f : 1.f; };  // (against tol 0.5)
  auto go_on = [&](int it) {
    if (ringed ? ring.restore_r(it) : xs.restore_r(it)) {
      CHECK(r_ver == it - 1 && ap_holds == it, "%s: redoing the r update of %d from r of %d, A p of %d", tag, it, r_ver, ap_holds);
      part0 = part1 = RES + it;
      r_ver = it;
    }
  };
  auto ops = cg_loop_model(enqueue_iter, idle_before_wait, wait, go_on);
  const int iters = cg_host_loop(max_iters, stop_guess, 0.5, ops);  // the library's loop
  for (int it = 1; it <= max_iters + 1; ++it) {
    CHECK(n_ap[(size_t)it] == (it <= iters ? 1 : 0), "%s: iteration %d has %d A p (solve stopped in %d)", tag, it, n_ap[(size_t)it], iters);
    const int m = src_mask[(size_t)it];
    CHECK((m & (m - 1)) == 0, "%s: iteration %d has A p from sources %d", tag, it, m);
  }
  if (iters >= 2) CHECK(src_mask[2] == 1 << (int)(second ? ApSource::p_update : ApSource::matvec), "%s: source of A p2 %d", tag, src_mask[2]);
  if (first) CHECK(src_mask[1] == 1 << (int)ApSource::init_pass, "%s: source of A p1 %d", tag, src_mask[1]);
}

int main() {
  check_route();
  for (int K = 1; K <= kXRingMax; ++K)
    for (int max_iters = 1; max_iters <= 12; ++max_iters)
      for (int guess = 0; guess <= max_iters + 2; ++guess)  // 0: no prediction (every iteration speculates ahead)
        for (int conv = 0; conv <= max_iters + 1; ++conv)   // 0 / beyond max_iters: never converges
          for (int depth = 0; depth <= 2; ++depth) check_loop(K, max_iters, guess, conv > max_iters ? 0 : conv, depth);
  if (g_fail) {
    std::fprintf(stderr, "%d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("anchor ap2 sweep ok (%ld cases)\n", g_cases);
  return 0;
}

// Sweep of small_plan.hpp (the launch plan of the one-launch LDS solve, k_settle_small<C>): every N in [1, 10000] against
// every row pitch in {4, 8, ..., 4200}.  The limits the kernel and the chip set (LDS per workgroup, co-resident workgroups),
// "the widest C that fits" against a restatement of the rule written here, the seams by value, and where the plans differ
// from the rule that allowed two workgroups per CU (nowhere but in the C = 4 launches that could not co-reside).  Also run
// under -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../../oscillink_amd/csrc/small_plan.hpp"

using namespace osc::host;

static int fail(const char* what, long long a, long long b) {
  std::printf("ERROR %s (%lld, %lld)\n", what, a, b);
  return 1;
}

// the rule restated from the numbers alone (no constant of the header): bytes of x, r, p, Ap + [8 waves][C] doubles + 64
static long long model_lds(long long N, int C) { return N * C * 16 + 8LL * C * 8 + 64; }
static bool model_fits(long long N, long long ld, int C) {
  if (C == 1 && N > 6000) return false;
  return model_lds(N, C) <= 150 * 1024 && (ld + C - 1) / C <= 256;  // one workgroup per CU, each within the LDS limit
}
// The rule before the GPU tests of the 257- and 512-workgroup launches: two workgroups per CU under 79 KiB and 2200 rows
static bool old_fits(long long N, long long ld, int C) {
  if (C == 1 && N > 6000) return false;
  const long long lds = model_lds(N, C);
  return lds <= 150 * 1024 && (ld + C - 1) / C <= ((lds <= 79 * 1024 && N <= 2200) ? 512 : 256);
}
static int old_pick(long long N, long long ld) {
  for (int c : {4, 2, 1})
    if (old_fits(N, ld, c)) return c;
  return 0;
}

struct Pin {
  int N, D, cols, workgroups;
  long long lds;  // -1: not pinned
};

int main() {
  long long cases = 0, two_per_cu = 0, by_cols[5] = {0, 0, 0, 0, 0};
  if (kSmallThreads != 512 || kSmallWaves != 8 || kSmallMaxIters != 4096) return fail("constants", kSmallThreads, kSmallWaves);
  for (int N = 1; N <= 10000; ++N) {
    for (int ld = 4; ld <= 4200; ld += 4) {
      ++cases;
      const int C = small_pick_cols(N, ld);
      if (C != 0 && C != 1 && C != 2 && C != 4) return fail("cols not in {0, 1, 2, 4}", N, ld);
      by_cols[C] += 1;
      // the widest that fits, by the restated rule
      for (int c : {4, 2, 1}) {
        if (c > C && model_fits(N, ld, c)) return fail("a wider C fits", N, ld);
        if (c == C && !model_fits(N, ld, c)) return fail("the chosen C does not fit", N, ld);
      }
      // Against the old rule: the plans differ exactly where it asked for two workgroups per CU, and there it only ever
      // chose C = 4 (lds(N, 2) <= 79 KiB with N <= 2200 allows at most 512 workgroups = 1024 columns, and up to 1024 columns
      // C = 4 needs only 256 workgroups, which fit whenever its LDS does: C = 4 always took those shapes first).  C = 4 is the
      // one width whose registers do not admit a second workgroup on a CU, so every such launch fell back.
      const int Cold = old_pick(N, ld);
      if (Cold != C) {
        ++two_per_cu;
        if (C != 0 || Cold != 4 || (ld + 3) / 4 <= 256 || N > 1259) return fail("differs from the old rule elsewhere", N, ld);
      } else if (C > 0 && (ld + C - 1) / C > 256) {
        return fail("more than one workgroup per CU", N, ld);
      }
      if (C == 0) continue;
      const size_t lds = small_lds_bytes(N, C);
      const int wgs = small_workgroups(ld, C);
      if ((long long)lds != model_lds(N, C)) return fail("lds bytes", N, C);
      if (lds > 150 * 1024) return fail("lds beyond 150 KiB", N, ld);
      // the kernel's carve-up (x, r, p, Ap, red[waves][C] doubles, s_res, s_fail) ends inside the allocation, and the doubles
      // start on an 8-byte boundary
      const size_t red_at = (size_t)N * C * 16, used = red_at + (size_t)kSmallWaves * C * 8 + 8;
      if (red_at % 8 != 0 || used > lds) return fail("carve-up", N, C);
      // every workgroup on a CU of its own: 512 threads, within the LDS limit, at most 256 of them
      if (wgs != (ld + C - 1) / C || wgs < 1 || wgs > 256) return fail("workgroups", N, ld);
      if (C == 1 && N > 6000) return fail("one column beyond 6000 rows", N, ld);
      // osc_create pads the row pitch from N * D >= 2^22 on, which switches this path off: never inside the planned region
      if ((long long)N * ld >= (1LL << 22)) return fail("planned beyond the dense-pitch region", N, ld);
      // the plan of the N x D lattices with this pitch
      for (int D = ld - 3; D <= ld; ++D) {
        const SmallPlan p = small_plan(N, D);
        if (p.cols != C || p.workgroups != wgs || p.lds_bytes != (int64_t)lds) return fail("small_plan", N, D);
      }
    }
  }
  if (by_cols[0] == 0 || by_cols[1] == 0 || by_cols[2] == 0 || by_cols[4] == 0 || by_cols[3] != 0 || two_per_cu == 0)
    return fail("a plan never seen", by_cols[1], by_cols[2]);
  // ---- the seams by value ----
  const Pin pins[] = {
      {2395, 64, 4, 16, 153600}, {2396, 64, 2, 32, -1},   {2396, 61, 2, 32, -1},     {4794, 96, 2, 48, 153600},
      {4795, 96, 1, 96, -1},     {6000, 64, 1, 64, -1},   {6000, 256, 1, 256, -1},   {6001, 64, 0, 0, 0},
      {1259, 1028, 0, 0, 0},     {1259, 2048, 0, 0, 0},   {1260, 1028, 0, 0, 0},     {2395, 1024, 4, 256, 153600},
      {4794, 516, 0, 0, 0},      {5000, 3, 1, 4, -1},     {300, 16, 4, 4, -1},       {1259, 1024, 4, 256, 80896},
      {2200, 1025, 0, 0, 0},     {6000, 257, 0, 0, 0},    {4794, 512, 2, 256, 153600}, {1, 1028, 0, 0, 0},
  };
  for (const Pin& q : pins) {
    ++cases;
    const SmallPlan p = small_plan(q.N, q.D);
    if (p.cols != q.cols || p.workgroups != q.workgroups) return fail("pinned plan", q.N, q.D);
    if (q.lds >= 0 && p.lds_bytes != q.lds) return fail("pinned lds bytes", q.N, q.D);
  }
  // ---- sizes no lattice has plan to the general path, without overflow ----
  for (long long N : {-1LL, 0LL, (long long)INT32_MAX + 1})
    if (small_plan(N, 64).cols != 0) return fail("bad N", N, 64);
  for (long long D : {-1LL, 0LL, (long long)INT32_MAX - 7, (long long)INT32_MAX, (long long)INT32_MAX + 1})
    if (small_plan(100, D).cols != 0) return fail("bad D", 100, D);
  if (small_plan(INT32_MAX, INT32_MAX - 8).cols != 0 || small_plan(1, INT32_MAX - 8).cols != 0) return fail("huge", 0, 0);
  if (small_plan(1, 1).cols != 4 || small_plan(1, 1).workgroups != 1) return fail("1 x 1", 1, 1);
  cases += 12;
  std::printf("small plan sweep ok (%lld cases; cols 0/1/2/4: %lld/%lld/%lld/%lld; off the two-per-CU rule: %lld)\n", cases, by_cols[0],
              by_cols[1], by_cols[2], by_cols[4], two_per_cu);
  return 0;
}

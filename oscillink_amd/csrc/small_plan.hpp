// The launch plan of the one-launch LDS-resident CG (small_kernels.hip: k_settle_small<C>).  HIP-free:
// osc_solve.hip / small_kernels.hip run it, osc_small_plan (include/oscillink_hip.h) reports it without a device,
// tests/host_logic/sweep_small_plan.cpp sweeps it.
//
// A workgroup of kSmallThreads threads owns C columns of the N x ld state and keeps x, r, p, Ap of those columns in LDS for
// the whole solve; the ceil(ld / C) workgroups meet at one counter barrier per iteration, so all of them must be resident
// at once.  The plan is C: 4, 2 or 1 columns per workgroup, or 0 when the lattice takes the general path.
#pragma once
#include <cstddef>
#include <cstdint>
#include <initializer_list>

namespace osc {
namespace host {

constexpr int kSmallThreads = 512;               // threads per workgroup: one row per thread per sweep keeps the gather latency chain short
constexpr int kSmallWaves = kSmallThreads / 64;  // waves per workgroup: rows of the block reduction's scratch
constexpr size_t kSmallLdsMax = 150 * 1024;      // dynamic LDS one workgroup may ask for (160 KiB per CU)
constexpr int32_t kSmallOneColMaxRows = 6000;    // one column per workgroup: slower than the general path beyond this
constexpr int kSmallResident = 256;              // workgroups of one launch: one per compute unit (see small_fits)
constexpr int32_t kSmallMaxIters = 4096;         // iteration cap of the one-launch solve (its control words are sized for it)

// x, r, p, Ap of C columns, the block reduction's [waves][C] doubles, the stop test's two words (in a 64-byte tail)
inline size_t small_lds_bytes(int32_t N, int C) {
  return (size_t)N * C * 4 * sizeof(float) + kSmallWaves * C * sizeof(double) + 64;
}

inline int32_t small_workgroups(int32_t ld, int C) { return C > 0 ? (ld + C - 1) / C : 0; }

// does a launch with C columns per workgroup fit?
inline bool small_fits(int32_t N, int32_t ld, int C) {
  // one column per workgroup leaves most of the chip idle behind long serial row loops: past N = 6000 the general
  // multi-launch path is faster (measured: N = 5000 0.18 vs 0.23 ms, 7000 0.24 vs 0.23, 9000 0.30 vs 0.23)
  if (C == 1 && N > kSmallOneColMaxRows) return false;
  // co-residency: one workgroup per CU always fits (256 CUs).  Never two: a 512-thread workgroup is two waves per SIMD,
  // two of them need four, and k_settle_small<4> -- the only width the old "two per CU under 79 KiB of LDS and 2200
  // rows" rule could ever select -- holds 161 VGPRs, which admits three.  Every launch that rule planned (N <= 1259,
  // 1024 < ld <= 2048) ran into the barrier's 5 ms timeout and fell back (tests/test_gpu_small_solve.py).
  return small_workgroups(ld, C) <= kSmallResident && small_lds_bytes(N, C) <= kSmallLdsMax;
}

// columns per workgroup (0 = the lattice does not fit the one-launch path): the widest that fits.  ld = the row pitch the
// solve works on, a multiple of 4.
// every workgroup must be resident at once (counter barrier with a timeout that falls back to the general path)
inline int small_pick_cols(int32_t N, int32_t ld) {
  for (int C : {4, 2, 1})
    if (small_fits(N, ld, C)) return C;
  return 0;
}

struct SmallPlan {
  int32_t cols = 0;        // columns per workgroup (0: general path)
  int32_t workgroups = 0;  // ceil(dcols / cols)
  int64_t lds_bytes = 0;   // dynamic LDS of one workgroup
};

// The plan for an N x D lattice with the dense row pitch (D rounded up to 4: osc_create's choice wherever this path can
// run, since N * D < 2^22 there).  Sizes no lattice has (N < 1, D < 1, a pitch beyond int32) plan to the general path.
inline SmallPlan small_plan(int64_t N, int64_t D) {
  SmallPlan p;
  if (N < 1 || D < 1 || N > INT32_MAX || D > INT32_MAX - 8) return p;
  const int32_t ld = (int32_t)((D + 3) / 4 * 4);
  p.cols = small_pick_cols((int32_t)N, ld);
  if (p.cols > 0) {
    p.workgroups = small_workgroups(ld, p.cols);
    p.lds_bytes = (int64_t)small_lds_bytes((int32_t)N, p.cols);
  }
  return p;
}

}  // namespace host
}  // namespace osc

// Device helpers of the per-(row, query) kernels under per-query chain priors (DESIGN.md sections 11.1 and 12.3), shared by
// bundle_prior_kernels.hip and receipt_prior_kernels.hip: who a lane is, the group's butterfly sum and a lane's gamma, kappa
// and (H gamma)_b.  Include inside an anonymous namespace of namespace osc, after query.hpp.
#pragma once

// element (row, col) of a slab-major panel (gates_many_plan.hpp)
__device__ __forceinline__ size_t panel_at(int32_t N, int row, int col) {
  return ((size_t)(col >> 5) * (size_t)N + (size_t)row) * 32 + (size_t)(col & 31);
}

// A wave serves 64 / gs consecutive queries of one row: gs (a power of two, at least the largest m of the pass) lanes a query,
// lane b of a group owning node b.  Sums over the nodes run as a butterfly inside the group; lanes past m hold zeros, and
// adding them is exact, so a query's sums are the same bits under any gs.
struct BpWho {
  int row, q, b, m, koff, base;  // base: the group's first lane
  bool live;
  const int32_t* cols;
  const double* H;
};

__device__ __forceinline__ bool bp_who(const BpArgs& a, BpWho& w) {
  const int lane = threadIdx.x & 63;
  const int per = 64 / a.gs, groups = (a.nq + per - 1) / per;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wave >= (int64_t)a.N * groups) return false;
  w.row = (int)(wave / groups);
  w.b = lane & (a.gs - 1);
  w.base = lane - w.b;
  const int q = (int)(wave - (int64_t)w.row * groups) * per + w.base / a.gs;
  w.live = q < a.nq;
  w.q = w.live ? q : a.nq - 1;
  const int sy = a.q_sys[w.q];
  w.m = w.live ? a.sys_m[sy] : 0;
  w.cols = a.sys_cols + a.sys_col_at[sy];
  w.koff = (int)(a.tv_at[w.q] / a.ld);
  w.H = a.H + (size_t)w.q * kBpNodes * kBpNodes;
  return true;
}

__device__ __forceinline__ double group_sum_d(double v, int gs) {
  for (int o = gs >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// lane b's gamma, kappa and (H gamma)_b of its (row, query)
struct BpLane {
  float gamma, kappa;
  double t;
};

__device__ __forceinline__ BpLane bp_lane(const BpArgs& a, const BpWho& w, float inv) {
  BpLane v;
  v.gamma = w.b < w.m ? a.G[panel_at(a.N, w.row, w.cols[w.b])] * inv : 0.f;
  v.kappa = w.b < w.m ? a.kappa[(size_t)w.row * a.ks + w.koff + w.b] : 0.f;
  double t = 0.0;
  const double* Hb = w.H + (size_t)w.b * kBpNodes;
  for (int c = 0; c < a.gs; ++c) t += Hb[c] * (double)__shfl(v.gamma, w.base + c, 64);  // (H is zero past m)
  v.t = t;
  return v;
}

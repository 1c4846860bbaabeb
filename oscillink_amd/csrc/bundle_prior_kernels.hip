// bundle() under per-query chain priors (osc_bundle_prior_many): the per-(row, query) terms of
//   U*_q,i = X'_i + x'_i psi_q + sum_b G_ib C_b,   C = T_q V_q (m <= 64 rows),
// expanded so that U* is never formed.  Per query n2 = |psi|^2, e_b = C_b . psi, H = C C^T; per (row, query) p (the query
// dot of section 11 on the shifted basis) and kappa_ib = X'_i . C_b / di (k_query_gemm<2>).
//
// The two row kernels give a group of gs lanes to a (row, query) pair and one lane to each node of the query's chain, so
// nothing is indexed by a run-time node number in registers; gs is the pass's largest m rounded up to a power of two, and a
// wave serves 64 / gs queries of one row.  Every sum is fp64 in a fixed order -- over the nodes by the group's butterfly,
// over a row's edges in slot order -- and reads its own row, query and chain alone; lanes past a query's m add exact zeros,
// so a query's bytes do not depend on gs, the pass's width, the query's position or the chunking.
//
// The quadratic term dgamma^T H dgamma is taken in the split form nu_i + nu_j - 2 gamma_j . (H gamma_i): gamma is fp32 and H,
// H gamma_i and nu are fp64, so the three terms are exact to 2^-53 of their own size and their difference loses nothing
// that fp32 inputs could have carried.
#include "query.hpp"

namespace osc {
namespace {

#include "bundle_prior_dev.hpp"

__global__ __launch_bounds__(256) void k_bp_pack(const float* __restrict__ TV, int64_t rows, int64_t rows_pad, int32_t D,
                                                 int32_t ld, int32_t kpad, float* __restrict__ Bt) {
  const int64_t n = rows_pad * kpad;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / kpad;
    const int c = (int)(i - r * kpad);
    Bt[i] = (r < rows && c < D) ? TV[r * ld + c] : 0.f;
  }
}

// one workgroup per query; output (b, b') of H and b of e by one thread, columns in order
__global__ __launch_bounds__(256) void k_bp_scalars(const BpArgs a) {
  const int q = blockIdx.x, t = threadIdx.x;
  const int m = a.sys_m[a.q_sys[q]];
  const float* C = a.TV + a.tv_at[q];
  const float* psi = a.psi + (size_t)q * a.ld;
  double* H = a.H + (size_t)q * kBpNodes * kBpNodes;
  for (int o = t; o < kBpNodes * kBpNodes; o += 256) {
    const int b = o >> 6, c = o & 63;
    double acc = 0.0;
    if (b < m && c < m) {
      const float* Cb = C + (size_t)b * a.ld;
      const float* Cc = C + (size_t)c * a.ld;
      for (int d = 0; d < a.D; ++d) acc += (double)Cb[d] * (double)Cc[d];
    }
    H[o] = acc;
  }
  if (t < kBpNodes) {
    double acc = 0.0;
    if (t < m) {
      const float* Cb = C + (size_t)t * a.ld;
      for (int d = 0; d < a.D; ++d) acc += (double)Cb[d] * (double)psi[d];
    }
    a.e[(size_t)q * kBpNodes + t] = acc;
  }
}

__global__ __launch_bounds__(256) void k_bp_rows_self(const BpArgs a) {
  BpWho w;
  if (!bp_who(a, w)) return;
  const float di_f = a.sqrt_deg[w.row] + 1e-12f;
  const float inv = 1.0f / di_f;
  const BpLane v = bp_lane(a, w, inv);
  const double e_b = a.e[(size_t)w.q * kBpNodes + w.b];
  const double s = (double)a.s[w.row], n2 = a.pn2[w.q], g = (double)v.gamma;
  const double nu = group_sum_d(g * v.t, a.gs);
  const double lin = group_sum_d(g * ((double)v.kappa + s * e_b), a.gs);
  const double ge = group_sum_d(g * e_b, a.gs);
  if (!w.live || w.b != 0) return;
  const size_t o = (size_t)w.row * a.qs + w.q;
  const double p = (double)a.p[o], di = (double)di_f;
  const double dot = di * (p + s * n2 + ge);
  const double un2 = a.xn2[w.row] + di * di * (2.0 * s * p + s * s * n2 + 2.0 * lin + nu);
  a.nu[o] = nu;
  a.align[o] = (float)(dot / (sqrt(fmax(un2, 0.0)) + 1e-12) * a.pinv[w.q]);
}

__global__ __launch_bounds__(256) void k_bp_rows_coh(const BpArgs a) {
  BpWho w;
  if (!bp_who(a, w)) return;
  const int row = w.row;
  const float inv_i = 1.0f / (a.sqrt_deg[row] + 1e-12f);
  const BpLane vi = bp_lane(a, w, inv_i);
  const double e_b = a.e[(size_t)w.q * kBpNodes + w.b];
  const size_t o = (size_t)row * a.qs + w.q;
  const double s_i = (double)a.s[row], p_i = (double)a.p[o], nu_i = a.nu[o];
  const bool mine = w.b < w.m;
  const int my_col = mine ? w.cols[w.b] : 0;
  double acc_lane = 0.0, acc_all = 0.0;
  const int deg = a.deg[row];
  const int32_t* crow = a.col + (size_t)row * a.width;
  const float* arow = a.adj + (size_t)row * a.width;
  for (int e = 0; e < deg; ++e) {  // in slot order: every lane walks the same edges
    const float wt = arow[e];
    if (!(wt > 0.f)) continue;
    const int j = crow[e];
    const float inv_j = 1.0f / (a.sqrt_deg[j] + 1e-12f);
    const float gj = mine ? a.G[panel_at(a.N, j, my_col)] * inv_j : 0.f;
    const float kj = mine ? a.kappa[(size_t)j * a.ks + w.koff + w.b] : 0.f;
    const size_t oj = (size_t)j * a.qs + w.q;
    const double ds = s_i - (double)a.s[j], dp = p_i - (double)a.p[oj];
    const double hw = 0.5 * (double)a.lamC * (double)wt;
    const double dg = (double)vi.gamma - (double)gj, dk = (double)vi.kappa - (double)kj;
    acc_lane += hw * (2.0 * dg * (dk + ds * e_b) - 2.0 * (double)gj * vi.t);
    acc_all += 2.0 * hw * ds * dp + hw * (nu_i + a.nu[oj]);
  }
  const double extra = group_sum_d(acc_lane, a.gs);
  if (w.live && w.b == 0) a.coh[o] = (float)(a.c0[row] - a.pn2[w.q] * a.c2[row] - acc_all - extra);
}

}  // namespace

void launch_bp_pack(const float* TV, int64_t rows, int64_t rows_pad, int32_t D, int32_t ld, int32_t kpad, float* Bt,
                    hipStream_t s) {
  const int64_t n = rows_pad * kpad;
  if (n <= 0) return;
  hipLaunchKernelGGL(k_bp_pack, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), 0, s, TV, rows, rows_pad,
                     D, ld, kpad, Bt);
  HIP_CHECK(hipGetLastError());
}

void launch_bp_scalars(const BpArgs& a, hipStream_t s) {
  if (a.nq <= 0) return;
  hipLaunchKernelGGL(k_bp_scalars, dim3((unsigned)a.nq), dim3(256), 0, s, a);
  HIP_CHECK(hipGetLastError());
}

// waves of a row pass: 64 / gs queries a wave
static int64_t bp_row_waves(const BpArgs& a) {
  const int per = 64 / a.gs;
  return (int64_t)a.N * ((a.nq + per - 1) / per);
}

void launch_bp_rows_self(const BpArgs& a, hipStream_t s) {
  const int64_t waves = bp_row_waves(a);
  if (waves <= 0) return;
  hipLaunchKernelGGL(k_bp_rows_self, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, a);
  HIP_CHECK(hipGetLastError());
}

void launch_bp_rows_coh(const BpArgs& a, hipStream_t s) {
  const int64_t waves = bp_row_waves(a);
  if (waves <= 0) return;
  hipLaunchKernelGGL(k_bp_rows_coh, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, a);
  HIP_CHECK(hipGetLastError());
}

}  // namespace osc

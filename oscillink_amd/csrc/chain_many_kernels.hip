// chain_receipt() of Q (query, chain) pairs on a built lattice from its query basis (osc_chain_receipt_many, DESIGN.md
// section 12.1): U*(psi_q) = X + x psi_q^T is never formed -- a chain edge (i, j) needs row i, row j and the rows of i's
// graph and path neighbours, and each is put together from the gathered rows of X and x where it is used.
//
// k_cm_edges: one wave per (query, chain edge) unit, a grid-stride loop over the chunk's units, lanes across D with 16-byte
// loads (rows are 16-byte aligned at a pitch of a multiple of 4 floats).  Device row order throughout; ELL columns are device
// rows.  No LDS, no atomics, no unit waits on another; a unit's arithmetic depends on its own query, chain and row alone, so a
// query's bytes do not depend on its batch.
// k_cm_finish: one thread per query over its edges in order (chain_receipt_dev.hpp's rule, k_cq_chain_receipt's).
#include "chain_edges_dev.hpp"

namespace osc {
namespace {

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

__device__ __forceinline__ float4 axpy4(float x, float4 p, float4 X) {
  return make_float4(fmaf(x, p.x, X.x), fmaf(x, p.y, X.y), fmaf(x, p.z, X.z), fmaf(x, p.w, X.w));
}

__device__ __forceinline__ float4 fma4(float g, float4 w, float4 u) {
  return make_float4(fmaf(g, w.x, u.x), fmaf(g, w.y, u.y), fmaf(g, w.z, u.z), fmaf(g, w.w, u.w));
}
// element (row, col) of a slab-major panel (gates_many_plan.hpp)
__device__ __forceinline__ size_t panel_at(int32_t N, int row, int col) {
  return ((size_t)(col >> 5) * (size_t)N + (size_t)row) * 32 + (size_t)(col & 31);
}

// The row loader of the query basis: A = X + x psi (one fma per element).  PRIOR: every gathered row carries the low-rank
// correction of the query's chain prior (query.hpp: CmEdgesArgs).  The unit's arithmetic is chain_edges_dev.hpp's.
template <bool PRIOR>
__global__ __launch_bounds__(256) void k_cm_edges(const CmEdgesArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), waves = (int64_t)gridDim.x * 4;
  for (int64_t u = wave; u < a.n_units; u += waves) {
    const host::ChainManyUnit un = a.units[u];
    const int i = un.i;
    const float* psi = a.psi + (size_t)un.q * a.ld;
    const float* Xi = a.X + (size_t)i * a.ld;
    const float x_i = a.x4[(size_t)i * 4];
    const float inv_i = 1.0f / (a.sqrt_deg[i] + 1e-12f);
    int pm = 0;
    const int32_t* pcols = nullptr;
    const float* tv = nullptr;
    if constexpr (PRIOR) {
      const int sy = a.q_sys[un.q];
      pm = a.sys_m[sy];
      pcols = a.sys_cols + a.sys_col_at[sy];
      tv = a.TV + a.tv_at[un.q];
    }
    // |Un_i - Un_c|^2 of U*(psi_q), wave-uniform
    auto du_to = [&](int c) {
      const float* Xc = a.X + (size_t)c * a.ld;
      const float x_c = a.x4[(size_t)c * 4];
      const float inv_c = 1.0f / (a.sqrt_deg[c] + 1e-12f);
      float du = 0.f;
      for (int k = lane * 4; k < a.D; k += 256) {
        const float4 p = ld4(psi + k);  // (psi's pad columns are zero)
        if constexpr (PRIOR) {
          float4 ui = axpy4(x_i, p, cme_masked4(Xi, k, a.D)), uc = axpy4(x_c, p, cme_masked4(Xc, k, a.D));
          for (int b = 0; b < pm; ++b) {  // in node order, one fma per element and node
            const int col = pcols[b];
            const float4 w = ld4(tv + (size_t)b * a.ld + k);
            ui = fma4(a.G[panel_at(a.N, i, col)], w, ui);
            uc = fma4(a.G[panel_at(a.N, c, col)], w, uc);
          }
          du = cme_sq4(ui, inv_i, uc, inv_c, du);
        } else {
          du = cme_sq4(axpy4(x_i, p, cme_masked4(Xi, k, a.D)), inv_i, axpy4(x_c, p, cme_masked4(Xc, k, a.D)), inv_c, du);
        }
      }
      return wave_sum_f(du);
    };
    cm_edge_unit(a, un, u, lane, inv_i, du_to);
  }
}

__global__ __launch_bounds__(64) void k_cm_finish(const CmFinishArgs a) {
  const int q = blockIdx.x * 64 + threadIdx.x;
  if (q >= a.nq) return;
  const int e0 = a.eoff[q];
  const ChainVerdict v = chain_finish(a.term + e0, a.zmax + e0, a.eoff[q + 1] - e0, a.z_th);
  a.gain[q] = v.gain;
  a.verdict[q] = v.ok;
  a.weak_k[q] = v.weak_k;
  a.weak_z[q] = (float)v.worst;
}

// ---- per-query chain priors ------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_cp_systems(const CpSystemsArgs a) {
  __shared__ double sA[64 * 64], sT[64 * 64];
  const int c = blockIdx.x, t = threadIdx.x;
  const int m = a.m[c];
  const int32_t* cols = a.cols + a.col_at[c];
  const int32_t* rows = a.rows + a.col_at[c];
  const int e0 = a.k_at[c], e1 = a.k_at[c + 1];
  // sT <- Ghat (thread t: column t), sA <- I
  if (t < m) {
    const int col = cols[t];
    for (int r = 0; r < m; ++r) {
      sT[r * 64 + t] = (double)a.G[panel_at(a.N, rows[r], col)];
      sA[r * 64 + t] = r == t ? 1.0 : 0.0;
    }
  }
  __syncthreads();
  // sA <- I - K Ghat, entry by entry in their order (a thread owns its column: no two threads write one element)
  if (t < m)
    for (int e = e0; e < e1; ++e) sA[a.kr[e] * 64 + t] -= (double)a.lamP * (double)a.kw[e] * sT[a.kc[e] * 64 + t];
  __syncthreads();
  // sT <- K
  if (t < m)
    for (int r = 0; r < m; ++r) sT[r * 64 + t] = 0.0;
  __syncthreads();
  for (int e = e0 + t; e < e1; e += 64) sT[a.kr[e] * 64 + a.kc[e]] = (double)a.lamP * (double)a.kw[e];
  __syncthreads();
  // Gauss-Jordan on [A | T] with partial pivoting.  Column k of A is left as it is once it has been the pivot column (it is
  // read at step k alone), so a step's factors A[r][k] are not written while they are read.
  for (int k = 0; k < m; ++k) {
    double best = (t >= k && t < m) ? fabs(sA[t * 64 + k]) : -1.0;
    int at = t;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double ob = __shfl_xor(best, o, 64);
      const int oa = __shfl_xor(at, o, 64);
      if (ob > best || (ob == best && oa < at)) {
        best = ob;
        at = oa;
      }
    }
    if (at != k && t < m) {
      const double x = sA[k * 64 + t], y = sT[k * 64 + t];
      sA[k * 64 + t] = sA[at * 64 + t];
      sT[k * 64 + t] = sT[at * 64 + t];
      sA[at * 64 + t] = x;
      sT[at * 64 + t] = y;
    }
    __syncthreads();
    const double piv = sA[k * 64 + k];
    if (t < m) {
      const double ak = sA[k * 64 + t], tk = sT[k * 64 + t];
      for (int r = 0; r < m; ++r) {
        if (r == k) continue;
        const double f = sA[r * 64 + k] / piv;
        if (t > k) sA[r * 64 + t] -= f * ak;
        sT[r * 64 + t] -= f * tk;
      }
    }
    __syncthreads();
  }
  if (t < m) {
    double* T = a.T + a.t_at[c];
    for (int r = 0; r < m; ++r) T[(size_t)r * m + t] = sT[r * 64 + t] / sA[r * 64 + r];
  }
}

__global__ __launch_bounds__(256) void k_cp_tv(const CpTvArgs a) {
  __shared__ double sh[256];
  __shared__ double sres[64];
  __shared__ float sx[64];
  const int q = blockIdx.x, t = threadIdx.x;
  const int sy = a.q_sys[q];
  const int m = a.m[sy];
  const int32_t* cols = a.cols + a.col_at[sy];
  const int32_t* rows = a.rows + a.col_at[sy];
  const double* T = a.T + a.t_at[sy];
  const float* psi = a.psi + (size_t)q * a.ld;
  float* TV = a.TV + a.tv_at[q];
  if (t < m) {
    sres[t] = (double)a.col_res[cols[t]];
    sx[t] = a.x4[(size_t)rows[t] * 4];
  }
  __syncthreads();
  double worst = 0.0;
  for (int k = t; k < a.ld; k += 256) {
    double bound = 0.0;
    const float pk = k < a.D ? psi[k] : 0.f;
    for (int b = 0; b < m; ++b) {
      double acc = 0.0;
      if (k < a.D)
        for (int e = 0; e < m; ++e) acc += T[b * m + e] * (double)fmaf(sx[e], pk, a.X[(size_t)rows[e] * a.ld + k]);
      TV[(size_t)b * a.ld + k] = (float)acc;
      bound += sres[b] * fabs(acc);
    }
    worst = (bound > worst || bound != bound) ? bound : worst;  // (a NaN stays)
  }
  sh[t] = worst;
  __syncthreads();
  if (t == 0) {
    double w = 0.0;
    for (int k = 0; k < 256; ++k) w = (sh[k] > w || sh[k] != sh[k]) ? sh[k] : w;
    int it = 0;
    for (int b = 0; b < m; ++b) it = max(it, a.col_iters[cols[b]]);
    a.prior_res[q] = (float)((double)a.base[q] + w);
    a.prior_iters[q] = it;
  }
}

__global__ __launch_bounds__(256) void k_cp_scale_max(float* __restrict__ X, int32_t N, int32_t D, int32_t ld, float f,
                                                      float* __restrict__ part) {
  __shared__ float sh[256];
  float mx = 0.f;
  const int64_t n = (int64_t)N * ld;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    const float v = X[e] * f;
    X[e] = v;
    if ((int32_t)(e % ld) < D) mx = (fabsf(v) > mx || v != v) ? fabsf(v) : mx;
  }
  sh[threadIdx.x] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 256; ++k) mx = (sh[k] > mx || sh[k] != sh[k]) ? sh[k] : mx;
    part[blockIdx.x] = mx;
  }
}

}  // namespace

int cm_edge_blocks(int64_t n_units) { return (int)std::min<int64_t>((n_units + 3) / 4, kCmMaxBlocks); }

void launch_cm_edges(const CmEdgesArgs& a, hipStream_t s) {
  if (a.n_units <= 0) return;
  hipLaunchKernelGGL(k_cm_edges<false>, dim3((unsigned)cm_edge_blocks(a.n_units)), dim3(256), 0, s, a);
  HIP_CHECK(hipGetLastError());
}

void launch_cm_edges_prior(const CmEdgesArgs& a, hipStream_t s) {
  if (a.n_units <= 0) return;
  hipLaunchKernelGGL(k_cm_edges<true>, dim3((unsigned)cm_edge_blocks(a.n_units)), dim3(256), 0, s, a);
  HIP_CHECK(hipGetLastError());
}

void launch_cp_systems(const CpSystemsArgs& a, hipStream_t s) {
  if (a.n_sys <= 0) return;
  hipLaunchKernelGGL(k_cp_systems, dim3((unsigned)a.n_sys), dim3(64), 0, s, a);
  HIP_CHECK(hipGetLastError());
}

void launch_cp_tv(const CpTvArgs& a, hipStream_t s) {
  if (a.nq <= 0) return;
  hipLaunchKernelGGL(k_cp_tv, dim3((unsigned)a.nq), dim3(256), 0, s, a);
  HIP_CHECK(hipGetLastError());
}

int cp_scale_blocks(int64_t N) { return (int)std::min<int64_t>(std::max<int64_t>(N / 8, 1), 1024); }

void launch_cp_scale_max(float* X, int32_t N, int32_t D, int32_t ld, float f, float* part, hipStream_t s) {
  hipLaunchKernelGGL(k_cp_scale_max, dim3((unsigned)cp_scale_blocks(N)), dim3(256), 0, s, X, N, D, ld, f, part);
  HIP_CHECK(hipGetLastError());
}

void launch_cm_finish(const CmFinishArgs& a, hipStream_t s) {
  if (a.nq <= 0) return;
  hipLaunchKernelGGL(k_cm_finish, dim3((unsigned)((a.nq + 63) / 64)), dim3(64), 0, s, a);
  HIP_CHECK(hipGetLastError());
}

}  // namespace osc

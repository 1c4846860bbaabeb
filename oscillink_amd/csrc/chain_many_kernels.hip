// chain_receipt() of Q (query, chain) pairs on a built lattice from its query basis (osc_chain_receipt_many, DESIGN.md
// section 12.1): U*(psi_q) = X + x psi_q^T is never formed -- a chain edge (i, j) needs row i, row j and the rows of i's
// graph and path neighbours, and each is put together from the gathered rows of X and x where it is used.
//
// k_cm_edges: one wave per (query, chain edge) unit, a grid-stride loop over the chunk's units, lanes across D with 16-byte
// loads (rows are 16-byte aligned at a pitch of a multiple of 4 floats).  Device row order throughout; ELL columns are device
// rows.  No LDS, no atomics, no unit waits on another; a unit's arithmetic depends on its own query, chain and row alone, so a
// query's bytes do not depend on its batch.
// k_cm_finish: one thread per query over its edges in order (chain_receipt_dev.hpp's rule, k_cq_chain_receipt's).
#include "chain_receipt_dev.hpp"
#include "corpus_pcg.hpp"
#include "query.hpp"

namespace osc {
namespace {

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

__device__ __forceinline__ float4 masked4(const float* row, int c, int D) {
  float4 v = ld4(row + c);
  if (c + 3 >= D) {
    if (c + 1 >= D) v.y = 0.f;
    if (c + 2 >= D) v.z = 0.f;
    if (c + 3 >= D) v.w = 0.f;
  }
  return v;
}

// |A_i inv_i - A_c inv_c|^2 over this lane's columns; with psi: A = X + x psi (one fma per element)
__device__ __forceinline__ float sq4(float4 a, float sa, float4 b, float sb, float acc) {
  const float e0 = cq_sdiff(a.x, sa, b.x, sb), e1 = cq_sdiff(a.y, sa, b.y, sb);
  const float e2 = cq_sdiff(a.z, sa, b.z, sb), e3 = cq_sdiff(a.w, sa, b.w, sb);
  return fmaf(e0, e0, fmaf(e1, e1, fmaf(e2, e2, fmaf(e3, e3, acc))));
}
__device__ __forceinline__ float4 axpy4(float x, float4 p, float4 X) {
  return make_float4(fmaf(x, p.x, X.x), fmaf(x, p.y, X.y), fmaf(x, p.z, X.z), fmaf(x, p.w, X.w));
}

__global__ __launch_bounds__(256) void k_cm_edges(const CmEdgesArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), waves = (int64_t)gridDim.x * 4;
  const float lam_p = fmaxf(a.lamC, 1e-6f);
  for (int64_t u = wave; u < a.n_units; u += waves) {
    const host::ChainManyUnit un = a.units[u];
    const int i = un.i, j = un.j;
    const float* psi = a.psi + (size_t)un.q * a.ld;
    const float* Xi = a.X + (size_t)i * a.ld;
    const float x_i = a.x4[(size_t)i * 4];
    const float inv_i = 1.0f / (a.sqrt_deg[i] + 1e-12f);
    // |Un_i - Un_c|^2 of U*(psi_q), wave-uniform
    auto du_to = [&](int c) {
      const float* Xc = a.X + (size_t)c * a.ld;
      const float x_c = a.x4[(size_t)c * 4];
      const float inv_c = 1.0f / (a.sqrt_deg[c] + 1e-12f);
      float du = 0.f;
      for (int k = lane * 4; k < a.D; k += 256) {
        const float4 p = ld4(psi + k);  // (psi's pad columns are zero)
        du = sq4(axpy4(x_i, p, masked4(Xi, k, a.D)), inv_i, axpy4(x_c, p, masked4(Xc, k, a.D)), inv_c, du);
      }
      return wave_sum_f(du);
    };
    // structural row i: the ELL slots with a capped adjacency > 0, in slot order
    float rs = 0.f, rp = 0.f;
    double s1 = 0.0, s2 = 0.0, term = 0.0;
    bool found = false;
    const int deg = a.deg[i];
    const int32_t* crow = a.col + (size_t)i * a.width;
    const float* arow = a.adj + (size_t)i * a.width;
    for (int e = 0; e < deg; ++e) {
      const float w = arow[e];
      if (!(w > 0.f)) continue;
      const int c = crow[e];
      const float du = du_to(c);
      const float R = a.lamC * w * du;
      s1 += (double)R;
      s2 += (double)R * (double)R;
      if (c != j || found) continue;
      found = true;
      rs = R;
      const float* Yi = a.Y + (size_t)i * a.ld;
      const float* Yj = a.Y + (size_t)j * a.ld;
      const float inv_j = 1.0f / (a.sqrt_deg[j] + 1e-12f);
      float dy = 0.f;
      for (int k = lane * 4; k < a.D; k += 256) dy = sq4(masked4(Yi, k, a.D), inv_i, masked4(Yj, k, a.D), inv_j, dy);
      dy = wave_sum_f(dy);
      term = 0.5 * (double)a.lamC * (double)w * ((double)dy - (double)du);
    }
    const double z_s = chain_row_z(s1, s2, rs, (double)a.N);
    // path row i, in column order
    s1 = s2 = 0.0;
    found = false;
    for (int e = un.pb; e < un.pe; ++e) {
      const int c = a.pcol[e];
      const float R = lam_p * a.pa[e] * du_to(c);
      s1 += (double)R;
      s2 += (double)R * (double)R;
      if (c == j && !found) {
        found = true;
        rp = R;
      }
    }
    const double z_p = chain_row_z(s1, s2, rp, (double)a.N);
    if (lane == 0) {
      a.z_struct[u] = (float)z_s;
      a.z_path[u] = (float)z_p;
      a.r_struct[u] = rs;
      a.r_path[u] = rp;
      a.term[u] = term;
      a.zmax[u] = chain_zmax(z_s, z_p);
    }
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

}  // namespace

int cm_edge_blocks(int64_t n_units) { return (int)std::min<int64_t>((n_units + 3) / 4, kCmMaxBlocks); }

void launch_cm_edges(const CmEdgesArgs& a, hipStream_t s) {
  if (a.n_units <= 0) return;
  hipLaunchKernelGGL(k_cm_edges, dim3((unsigned)cm_edge_blocks(a.n_units)), dim3(256), 0, s, a);
  HIP_CHECK(hipGetLastError());
}

void launch_cm_finish(const CmFinishArgs& a, hipStream_t s) {
  if (a.nq <= 0) return;
  hipLaunchKernelGGL(k_cm_finish, dim3((unsigned)((a.nq + 63) / 64)), dim3(64), 0, s, a);
  HIP_CHECK(hipGetLastError());
}

}  // namespace osc

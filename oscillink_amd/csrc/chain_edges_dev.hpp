// One (query, chain edge) unit of a batched chain receipt (query.hpp: CmEdgesArgs), shared by the kernels that differ in where
// a row of U*_q comes from: the query basis, with or without the chain prior's correction (chain_many_kernels.hip), or the
// solved panel of a gated call (chain_gated_kernels.hip).  The caller passes the row loader as du_to(c) = |Un_i - Un_c|^2,
// wave-uniform; the row statistics, the z scores and the gain term are written here once.  Device code: include from .hip
// translation units only.
#pragma once
#include "chain_receipt_dev.hpp"
#include "corpus_pcg.hpp"
#include "query.hpp"

namespace osc {
namespace {

__device__ __forceinline__ float4 cme_masked4(const float* row, int c, int D) {
  float4 v = *reinterpret_cast<const float4*>(row + c);
  if (c + 3 >= D) {
    if (c + 1 >= D) v.y = 0.f;
    if (c + 2 >= D) v.z = 0.f;
    if (c + 3 >= D) v.w = 0.f;
  }
  return v;
}

// |A_i inv_i - A_c inv_c|^2 over this lane's columns
__device__ __forceinline__ float cme_sq4(float4 a, float sa, float4 b, float sb, float acc) {
  const float e0 = cq_sdiff(a.x, sa, b.x, sb), e1 = cq_sdiff(a.y, sa, b.y, sb);
  const float e2 = cq_sdiff(a.z, sa, b.z, sb), e3 = cq_sdiff(a.w, sa, b.w, sb);
  return fmaf(e0, e0, fmaf(e1, e1, fmaf(e2, e2, fmaf(e3, e3, acc))));
}

// unit u = (un.q, un.i, un.j) by one wave: structural row i over the ELL slots with a capped adjacency > 0 in slot order,
// path row i over its entries in column order, the six values out by lane 0
template <class DuTo>
__device__ __forceinline__ void cm_edge_unit(const CmEdgesArgs& a, const host::ChainManyUnit& un, int64_t u, int lane,
                                             float inv_i, DuTo du_to) {
  const int i = un.i, j = un.j;
  const float lam_p = fmaxf(a.lamC, 1e-6f);
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
    for (int k = lane * 4; k < a.D; k += 256) dy = cme_sq4(cme_masked4(Yi, k, a.D), inv_i, cme_masked4(Yj, k, a.D), inv_j, dy);
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

}  // namespace
}  // namespace osc

// Per-query chain priors under per-query gates: what osc_chain_gated_many adds to the panel PCG of
// bundle_gated_kernels.hip and the receipts of receipt_gated_kernels.hip -- W_path,q on the chain's rows, in the operator
// (k_cg_path_apply) and in the start residual (k_cg_path_init), and the chain receipt's edges read from the solved panel
// (k_cg_edges).
//
// The path kernels run one workgroup per (fix unit of the query's path rows, slab of the query): 32 rows x 8 lanes x float4 a
// step, like k_bg_apply, over the unit's kChainFixRows rows at most.  A row's entries are added in column order, a unit's
// rows by gm_fold's fixed order, and the units of a query where the sums are read (cg_unit_sum): the cut knows the path
// alone, so a query's bytes do not depend on its batch or chunk.  A row is written by its own thread group only and P is only
// read, so no unit waits on another.
#include "chain_edges_dev.hpp"
#include "chain_gated_dev.hpp"

namespace osc {
namespace {

// the rows of this workgroup's fix unit as indices into the packed rows; empty past the query's units
struct CgUnitRows {
  int r0, r1;
};
__device__ __forceinline__ CgUnitRows cg_unit_rows(const CgChain& ch, int q) {
  const int rows = ch.q_rows[q], b = (int)blockIdx.x * host::kChainFixRows;
  const int e = min(rows, b + host::kChainFixRows);
  return CgUnitRows{ch.q_row0[q] + b, ch.q_row0[q] + max(e, b)};
}
__device__ __forceinline__ double* cg_part_at(const CgChain& ch, int slab) {
  return ch.part + ((size_t)slab * ch.max_units + blockIdx.x) * 32;
}

__global__ __launch_bounds__(256) void k_cg_path_init(const BgPanel p, const CgChain ch, const float* __restrict__ src,
                                                      int32_t ld, float cP) {
  __shared__ double sh[1024];
  const int slab = blockIdx.y, q = slab / p.spq;
  const CgUnitRows ur = cg_unit_rows(ch, q);
  if (ur.r0 >= ur.r1) return;
  const int t = threadIdx.x, lr = t & 7;
  const int c = (slab % p.spq) * 32 + lr * 4;
  const size_t so = (size_t)slab * p.N * 32;
  const float* __restrict__ gate = p.gate + (size_t)q * p.N;
  float4 drz = f4(0.f);
  for (int rb = ur.r0; rb < ur.r1; rb += 32) {
    const int pr = rb + (t >> 3);
    if (pr >= ur.r1) continue;
    const int row = ch.prow[pr];
    float4 sum = f4(0.f);
    for (int e = ch.pbeg[pr]; e < ch.pend[pr]; ++e) sum = mulacc4(f4(ch.pw[e]), ld_anchor(src, ch.pcol[e], ld, c, p.D), sum);
    const size_t o = so + (size_t)row * 32 + lr * 4;
    const float inv_md = bg_inv_md(p, gate[row]);
    const float4 r0 = ld4(p.R + o);
    const float4 r = mulacc4(f4(cP), sum, r0), z = scale4(r, inv_md), z0 = scale4(r0, inv_md);
    st4(p.R + o, r);
    st4(p.P + o, z);
    drz.x += fmaf(r.x, z.x, -(r0.x * z0.x));
    drz.y += fmaf(r.y, z.y, -(r0.y * z0.y));
    drz.z += fmaf(r.z, z.z, -(r0.z * z0.z));
    drz.w += fmaf(r.w, z.w, -(r0.w * z0.w));
  }
  gm_fold(drz, sh, cg_part_at(ch, slab));
}

__global__ __launch_bounds__(256) void k_cg_path_apply(const BgPanel p, const CgChain ch, float cP) {
  __shared__ double sh[1024];
  const int slab = blockIdx.y, q = slab / p.spq;
  if (p.live[q] == 0) return;  // a frozen query's AP and sums stay as they are
  const CgUnitRows ur = cg_unit_rows(ch, q);
  if (ur.r0 >= ur.r1) return;
  const int t = threadIdx.x, lr = t & 7;
  const size_t so = (size_t)slab * p.N * 32;
  const float* __restrict__ P = p.P + so;
  float* __restrict__ AP = p.AP + so;
  float4 pap = f4(0.f);
  for (int rb = ur.r0; rb < ur.r1; rb += 32) {
    const int pr = rb + (t >> 3);
    if (pr >= ur.r1) continue;
    const int row = ch.prow[pr];
    float4 sum = f4(0.f);
    for (int e = ch.pbeg[pr]; e < ch.pend[pr]; ++e) sum = mulacc4(f4(ch.pw[e]), ld4(P + (size_t)ch.pcol[e] * 32 + lr * 4), sum);
    const size_t o = (size_t)row * 32 + lr * 4;
    const float4 d = scale4(sum, -cP), x = ld4(P + o), a = ld4(AP + o);
    st4(AP + o, make_float4(a.x + d.x, a.y + d.y, a.z + d.z, a.w + d.w));
    pap = mulacc4(x, d, pap);
  }
  gm_fold(pap, sh, cg_part_at(ch, slab));
}

// The row loader of a gated call's solved panel: query un.q owns the slabs [q spq, (q + 1) spq), whose pad columns are zero.
// The unit's arithmetic is chain_edges_dev.hpp's, launch_cm_edges' own.
__global__ __launch_bounds__(256) void k_cg_edges(const CmEdgesArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), waves = (int64_t)gridDim.x * 4;
  const int spq = (a.D + 31) / 32, cols = spq * 32;
  for (int64_t u = wave; u < a.n_units; u += waves) {
    const host::ChainManyUnit un = a.units[u];
    const int i = un.i;
    const float* Xq = a.X + (size_t)un.q * spq * a.N * 32;
    const float inv_i = 1.0f / (a.sqrt_deg[i] + 1e-12f);
    auto du_to = [&](int c) {
      const float inv_c = 1.0f / (a.sqrt_deg[c] + 1e-12f);
      float du = 0.f;
      for (int k = lane * 4; k < cols; k += 256) {
        const float* X = Xq + (size_t)(k >> 5) * a.N * 32 + (k & 31);
        du = cme_sq4(ld4(X + (size_t)i * 32), inv_i, ld4(X + (size_t)c * 32), inv_c, du);
      }
      return wave_sum_f(du);
    };
    cm_edge_unit(a, un, u, lane, inv_i, du_to);
  }
}

dim3 cg_grid(const BgPanel& p, const CgChain& ch) { return dim3((unsigned)ch.grid_units, (unsigned)p.slabs); }

}  // namespace

void launch_cg_path_init(const BgPanel& p, const CgChain& ch, const float* src, int32_t ld, float cP, hipStream_t s) {
  if (ch.grid_units <= 0) return;
  hipLaunchKernelGGL(k_cg_path_init, cg_grid(p, ch), dim3(256), 0, s, p, ch, src, ld, cP);
  HIP_CHECK(hipGetLastError());
}

void launch_cg_path_apply(const BgPanel& p, const CgChain& ch, float cP, hipStream_t s) {
  if (ch.grid_units <= 0) return;
  hipLaunchKernelGGL(k_cg_path_apply, cg_grid(p, ch), dim3(256), 0, s, p, ch, cP);
  HIP_CHECK(hipGetLastError());
}

void launch_cg_edges(const CmEdgesArgs& a, hipStream_t s) {
  if (a.n_units <= 0) return;
  hipLaunchKernelGGL(k_cg_edges, dim3((unsigned)cm_edge_blocks(a.n_units)), dim3(256), 0, s, a);
  HIP_CHECK(hipGetLastError());
}

}  // namespace osc

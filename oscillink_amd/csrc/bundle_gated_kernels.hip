// Bundles under per-query gates: nq solves of the reference's solve_Ustar (lattice.py:245-263,
// solver.py:6-37) with M_q = lamG I + lamC L_sym + lamQ diag(g_q) as ONE Jacobi-PCG over the lattice graph, then the
// bundle's alignment and coherence-drop columns from the solved panel.
//
// Layout, partition and launch geometry are gates_many_kernels.hip's: one workgroup per (row part, slab), 4 waves of 8 rows
// x 8 lanes x float4, sums in fp64 in a fixed order.  Query t owns the slabs [t spq, (t + 1) spq); what differs from the
// gates' solve is the diagonal, indexed by (row, query of the slab), the start at x0 = Y with the initial residual formed
// on the fly from the anchors, and the stop: the largest column residual of a QUERY decides for all its columns.  Nothing
// depends on which other queries fill the panel, so a query's answers are the same to the bit in any batch or chunk.
#include "chain_gated_dev.hpp"

namespace osc {
namespace {

__global__ __launch_bounds__(256) void k_bg_gates(const float* __restrict__ gate_api, const int32_t* __restrict__ api_id,
                                                  int32_t N, float* __restrict__ gate) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= N) return;
  const int64_t a = api_id ? (int64_t)api_id[r] : r;
  gate[(size_t)blockIdx.y * N + r] = gate_api[(size_t)blockIdx.y * N + a];
}

// The gather of k_gm_apply over the anchors (row-major, pitch ld) instead of a slab: r0 = RHS - M_q Y without a stored RHS.
// lamG Y cancels, so r0 = lamQ g (psi - y) + lamC (W y - y).  With a prior (chain_gated.hpp) the panel's lamG carries lamP and
// every row adds -lamP y; the chain rows' share is launch_cg_path_init's.
template <class Prior>
__global__ __launch_bounds__(256) void k_bg_init(const BgPanel p, const GmGraph g, const float* __restrict__ Y, int32_t ld,
                                                 const Prior pr) {
  __shared__ double sh[1024];
  const int slab = blockIdx.y, q = slab / p.spq, cq = (slab % p.spq) * 32;
  const int t = threadIdx.x, lane = t & 63, lr = lane & 7, g0 = lane & ~7;
  const int c = cq + lr * 4;
  const size_t so = (size_t)slab * p.N * 32;
  const float4 ps = ld4(p.psi + (size_t)q * p.spq * 32 + c);
  const float* __restrict__ gate = p.gate + (size_t)q * p.N;
  const GmRows rr = gm_rows(p);
  float4 rz = f4(0.f);
  for (int64_t rb = rr.r0; rb < rr.r1; rb += 32) {
    const int64_t row = rb + (t >> 3);
    const bool ok = row < rr.r1;
    const int deg = ok ? min(g.deg[row], g.width) : 0;
    int dmax = deg;
    dmax = max(dmax, __shfl_xor(dmax, 8, 64));
    dmax = max(dmax, __shfl_xor(dmax, 16, 64));
    dmax = max(dmax, __shfl_xor(dmax, 32, 64));
    float4 sum = f4(0.f);
    for (int e0 = 0; e0 < dmax; e0 += 8) {
      const int e = e0 + lr;
      int j = 0;
      float wv = 0.f;
      if (e < deg) {
        j = g.col[(size_t)row * g.width + e];
        wv = g.w[(size_t)row * g.width + e];
      }
      float4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int ju = __shfl(j, g0 + u, 64);
        v[u] = e0 + u < deg ? ld_anchor(Y, ju, ld, c, p.D) : f4(0.f);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const float wu = __shfl(wv, g0 + u, 64);
        sum = mulacc4(f4(wu), v[u], sum);
      }
    }
    if (ok) {
      const float4 y = ld_anchor(Y, row, ld, c, p.D);
      const float gi = gate[row], qg = p.lamQ * gi, inv_md = bg_inv_md(p, gi), lc = p.lamC;
      float4 r;
      r.x = fmaf(qg, ps.x - y.x, lc * (sum.x - y.x));
      r.y = fmaf(qg, ps.y - y.y, lc * (sum.y - y.y));
      r.z = fmaf(qg, ps.z - y.z, lc * (sum.z - y.z));
      r.w = fmaf(qg, ps.w - y.w, lc * (sum.w - y.w));
      if constexpr (Prior::active) r = mulacc4(f4(-pr.cP), y, r);
      const float4 z = scale4(r, inv_md);
      const size_t o = so + (size_t)row * 32 + lr * 4;
      st4(p.X + o, y);
      st4(p.R + o, r);
      st4(p.P + o, z);
      rz = mulacc4(r, z, rz);
    }
  }
  gm_fold(rz, sh, p.part_a + gm_part_at(p));
}

template <class Chain>
__global__ __launch_bounds__(kGmSumThreads) void k_bg_start(const BgPanel p, const Chain ch) {
  __shared__ double sh[kGmSumThreads];
  const int slab = blockIdx.x, t = threadIdx.x;
  double rz = gm_part_sum(p.part_a + (size_t)slab * p.parts * 32, p.parts, sh);
  if constexpr (Chain::active) rz += cg_unit_sum(ch, slab, slab / p.spq);
  if (t < 32) {
    const int c = slab * 32 + t;
    p.rz[c] = rz;
    p.alpha[c] = 0.f;
    p.beta[c] = 0.f;
  }
  if (t == 0 && slab % p.spq == 0) {
    const int q = slab / p.spq;
    p.live[q] = 1;
    p.iters[q] = 0;
    p.res[q] = 0.f;
    if (slab == 0) {
      p.n_live[0] = 0;
      p.n_live[1] = 0;
    }
  }
}

// k_gm_apply with the diagonal of (row, query): AP = (lamG + lamC + lamQ g) p - lamC W p
__global__ __launch_bounds__(256) void k_bg_apply(const BgPanel p, const GmGraph g) {
  __shared__ double sh[1024];
  const int slab = blockIdx.y, q = slab / p.spq;
  if (p.live[q] == 0) return;
  const int t = threadIdx.x, lane = t & 63, lr = lane & 7, g0 = lane & ~7;
  const size_t so = (size_t)slab * p.N * 32;
  const float* __restrict__ P = p.P + so;
  float* __restrict__ AP = p.AP + so;
  const float* __restrict__ gate = p.gate + (size_t)q * p.N;
  const float base = p.lamG + p.lamC, nc = -p.lamC;
  const GmRows rr = gm_rows(p);
  float4 pap = f4(0.f);
  for (int64_t rb = rr.r0; rb < rr.r1; rb += 32) {
    const int64_t row = rb + (t >> 3);
    const bool ok = row < rr.r1;
    const int deg = ok ? min(g.deg[row], g.width) : 0;
    int dmax = deg;
    dmax = max(dmax, __shfl_xor(dmax, 8, 64));
    dmax = max(dmax, __shfl_xor(dmax, 16, 64));
    dmax = max(dmax, __shfl_xor(dmax, 32, 64));
    float4 sum = f4(0.f);
    for (int e0 = 0; e0 < dmax; e0 += 8) {
      const int e = e0 + lr;
      int j = 0;
      float wv = 0.f;
      if (e < deg) {
        j = g.col[(size_t)row * g.width + e];
        wv = g.w[(size_t)row * g.width + e];
      }
      float4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int ju = __shfl(j, g0 + u, 64);
        v[u] = e0 + u < deg ? ld4(P + (size_t)ju * 32 + lr * 4) : f4(0.f);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const float wu = __shfl(wv, g0 + u, 64);  // 0 past the row's end, where v[u] is 0 as well
        sum = mulacc4(f4(wu), v[u], sum);
      }
    }
    if (ok) {
      const size_t o = (size_t)row * 32 + lr * 4;
      const float4 x = ld4(P + o);
      const float d = fmaf(p.lamQ, gate[row], base);
      const float4 a = make_float4(fmaf(d, x.x, nc * sum.x), fmaf(d, x.y, nc * sum.y), fmaf(d, x.z, nc * sum.z), fmaf(d, x.w, nc * sum.w));
      st4(AP + o, a);
      pap = mulacc4(x, a, pap);
    }
  }
  gm_fold(pap, sh, p.part_a + gm_part_at(p));
}

template <class Chain>
__global__ __launch_bounds__(kGmSumThreads) void k_bg_alpha(const BgPanel p, const Chain ch) {
  __shared__ double sh[kGmSumThreads];
  const int slab = blockIdx.x, t = threadIdx.x;
  if (p.live[slab / p.spq] == 0) return;
  double pap = gm_part_sum(p.part_a + (size_t)slab * p.parts * 32, p.parts, sh);
  if constexpr (Chain::active) pap += cg_unit_sum(ch, slab, slab / p.spq);
  if (t < 32) {
    const int c = slab * 32 + t;
    p.alpha[c] = (float)(p.rz[c] / (pap + 1e-18));  // solver.py:25-26 (a pad column: 0 / 1e-18)
  }
}

__global__ __launch_bounds__(256) void k_bg_update(const BgPanel p) {
  __shared__ double sh[1024];
  const int slab = blockIdx.y, q = slab / p.spq;
  if (p.live[q] == 0) return;  // a frozen query keeps its x and r bit for bit
  const int t = threadIdx.x, lr = t & 7;
  const size_t so = (size_t)slab * p.N * 32;
  const float4 al = ld4(p.alpha + slab * 32 + lr * 4);
  const float* __restrict__ gate = p.gate + (size_t)q * p.N;
  const GmRows rr = gm_rows(p);
  float4 rr2 = f4(0.f), rz = f4(0.f);
  for (int64_t rb = rr.r0; rb < rr.r1; rb += 32) {
    const int64_t row = rb + (t >> 3);
    if (row >= rr.r1) continue;
    const size_t o = so + (size_t)row * 32 + lr * 4;
    const float inv_md = bg_inv_md(p, gate[row]);
    float4 x = ld4(p.X + o), r = ld4(p.R + o);
    const float4 d = ld4(p.P + o), a = ld4(p.AP + o);
    x = mulacc4(d, al, x);
    r = make_float4(fmaf(-a.x, al.x, r.x), fmaf(-a.y, al.y, r.y), fmaf(-a.z, al.z, r.z), fmaf(-a.w, al.w, r.w));
    st4(p.X + o, x);
    st4(p.R + o, r);
    rr2 = mulacc4(r, r, rr2);
    rz = mulacc4(r, scale4(r, inv_md), rz);
  }
  gm_fold(rr2, sh, p.part_a + gm_part_at(p));
  gm_fold(rz, sh, p.part_b + gm_part_at(p));
}

// one workgroup per query: the stop rule of solver.py:29-31 on the query's D columns, then beta per column
__global__ __launch_bounds__(kGmSumThreads) void k_bg_beta(const BgPanel p, int it) {
  __shared__ double sh[kGmSumThreads];
  __shared__ float colmax[32];
  __shared__ int go_on;
  const int q = blockIdx.x, t = threadIdx.x;
  if (q == 0 && t == 0) p.n_live[(it + 1) & 1] = 0;
  if (p.live[q] == 0) return;
  const int s0 = q * p.spq;
  float m = 0.f;  // norms are >= 0
  for (int s = 0; s < p.spq; ++s) {
    const double rr = gm_part_sum(p.part_a + (size_t)(s0 + s) * p.parts * 32, p.parts, sh);
    if (t < 32) m = nan_max(m, (float)sqrt(rr));  // |r_c| (solver.py:29); np.max keeps a NaN
  }
  if (t < 32) colmax[t] = m;
  __syncthreads();
  if (t == 0) {
    float res = colmax[0];
    for (int c = 1; c < 32; ++c) res = nan_max(res, colmax[c]);
    p.iters[q] = it;
    p.res[q] = res;
    const int live = res <= p.tol ? 0 : 1;  // (a NaN never freezes: it runs to max_iters like cg_solve)
    if (!live) p.live[q] = 0;
    else atomicAdd(p.n_live + (it & 1), 1);
    go_on = live;
  }
  __syncthreads();
  if (!go_on) return;
  for (int s = 0; s < p.spq; ++s) {
    const double rz = gm_part_sum(p.part_b + (size_t)(s0 + s) * p.parts * 32, p.parts, sh);
    if (t < 32) {
      const int c = (s0 + s) * 32 + t;
      p.beta[c] = (float)(rz / (p.rz[c] + 1e-18));  // solver.py:33-34
      p.rz[c] = rz;
    }
  }
}

__global__ __launch_bounds__(256) void k_bg_direction(const BgPanel p) {
  const int slab = blockIdx.y, q = slab / p.spq;
  if (p.live[q] == 0) return;
  const int t = threadIdx.x, lr = t & 7;
  const size_t so = (size_t)slab * p.N * 32;
  const float4 be = ld4(p.beta + slab * 32 + lr * 4);
  const float* __restrict__ gate = p.gate + (size_t)q * p.N;
  const GmRows rr = gm_rows(p);
  for (int64_t rb = rr.r0; rb < rr.r1; rb += 32) {
    const int64_t row = rb + (t >> 3);
    if (row >= rr.r1) continue;
    const size_t o = so + (size_t)row * 32 + lr * 4;
    const float inv_md = bg_inv_md(p, gate[row]);
    const float4 r = ld4(p.R + o);
    float4 d = ld4(p.P + o);
    d.x = fmaf(d.x, be.x, r.x * inv_md);
    d.y = fmaf(d.y, be.y, r.y * inv_md);
    d.z = fmaf(d.z, be.z, r.z * inv_md);
    d.w = fmaf(d.w, be.w, r.w * inv_md);
    st4(p.P + o, d);
  }
}

// ---- the bundle's columns ---------------------------------------------------------------------------------------------
// one wave per row: ysum_i = sum_j A_ij |Yn_i - Yn_j|^2 over the slots with A_ij > 0 (receipts.py:40, 45-56).  A lane owns
// the columns 4 lane + 256 u and adds its share in (u, slot) order; the lanes are added by a fixed butterfly.
__global__ __launch_bounds__(256) void k_bg_ysum(const BgPanel p, const BgBundleArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= p.N) return;
  const int deg = min(a.deg[row], a.width);
  const double si = 1.0 / ((double)a.sqrt_deg[row] + 1e-12);
  double acc = 0.0;
  for (int c = lane * 4; c < p.D; c += 256) {
    const float4 yi = ld_anchor(a.Y, row, a.ld, c, p.D);
    for (int e = 0; e < deg; ++e) {
      const float w = a.adj[(size_t)row * a.width + e];
      if (!(w > 0.f)) continue;
      const int j = a.col[(size_t)row * a.width + e];
      const double sj = 1.0 / ((double)a.sqrt_deg[j] + 1e-12);
      acc += (double)w * sqdiff4(yi, si, ld_anchor(a.Y, j, a.ld, c, p.D), sj);
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) a.ysum[row] = acc;
}

// one wave per (row, query) over the query's solved slabs: |U_i|^2, U_i . psi and sum_j A_ij |Un_i - Un_j|^2 in fp64
__global__ __launch_bounds__(256) void k_bg_bundle(const BgPanel p, const BgBundleArgs a) {
  const int lane = threadIdx.x & 63, q = blockIdx.y;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= p.N) return;
  const int deg = min(a.deg[row], a.width);
  const double si = 1.0 / ((double)a.sqrt_deg[row] + 1e-12);
  const float* __restrict__ psi = p.psi + (size_t)q * p.spq * 32;
  const int cols = p.spq * 32;
  double usum = 0.0, un2 = 0.0, up = 0.0, pn2 = 0.0;
  for (int c = lane * 4; c < cols; c += 256) {
    const float* __restrict__ X = p.X + ((size_t)(q * p.spq + c / 32) * p.N) * 32 + (c & 31);  // (row r of this slab: + 32 r)
    const float4 ui = ld4(X + (size_t)row * 32), ps = ld4(psi + c);
    un2 += (double)ui.x * ui.x + (double)ui.y * ui.y + (double)ui.z * ui.z + (double)ui.w * ui.w;
    up += (double)ui.x * ps.x + (double)ui.y * ps.y + (double)ui.z * ps.z + (double)ui.w * ps.w;
    pn2 += (double)ps.x * ps.x + (double)ps.y * ps.y + (double)ps.z * ps.z + (double)ps.w * ps.w;
    for (int e = 0; e < deg; ++e) {
      const float w = a.adj[(size_t)row * a.width + e];
      if (!(w > 0.f)) continue;
      const int j = a.col[(size_t)row * a.width + e];
      const double sj = 1.0 / ((double)a.sqrt_deg[j] + 1e-12);
      usum += (double)w * sqdiff4(ui, si, ld4(X + (size_t)j * 32), sj);
    }
  }
  usum = wave_sum(usum);
  un2 = wave_sum(un2);
  up = wave_sum(up);
  pn2 = wave_sum(pn2);
  if (lane == 0) {
    const size_t o = (size_t)row * a.qs + q;
    a.align[o] = (float)(up / ((sqrt(un2) + 1e-12) * (sqrt(pn2) + 1e-12)));  // lattice.py:559-561
    a.coh[o] = (float)(0.5 * (double)p.lamC * (a.ysum[row] - usum));
  }
}

dim3 bg_grid(const BgPanel& p) { return dim3((unsigned)p.parts, (unsigned)p.slabs); }

}  // namespace

void launch_bg_gates(const float* gate_api, const int32_t* api_id, int32_t N, int32_t nq, float* gate, hipStream_t s) {
  hipLaunchKernelGGL(k_bg_gates, dim3((unsigned)((N + 255) / 256), (unsigned)nq), dim3(256), 0, s, gate_api, api_id, N, gate);
  HIP_CHECK(hipGetLastError());
}

void launch_bg_init(const BgPanel& p, const GmGraph& g, const float* Y, int32_t ld, hipStream_t s, const CgPrior* prior) {
  if (prior) hipLaunchKernelGGL(k_bg_init<CgPrior>, bg_grid(p), dim3(256), 0, s, p, g, Y, ld, *prior);
  else hipLaunchKernelGGL(k_bg_init<CgNoPrior>, bg_grid(p), dim3(256), 0, s, p, g, Y, ld, CgNoPrior{});
  HIP_CHECK(hipGetLastError());
}

void launch_bg_start(const BgPanel& p, hipStream_t s, const CgChain* chain) {
  if (chain) hipLaunchKernelGGL(k_bg_start<CgChain>, dim3((unsigned)p.slabs), dim3(kGmSumThreads), 0, s, p, *chain);
  else hipLaunchKernelGGL(k_bg_start<CgNoChain>, dim3((unsigned)p.slabs), dim3(kGmSumThreads), 0, s, p, CgNoChain{});
  HIP_CHECK(hipGetLastError());
}

void launch_bg_apply(const BgPanel& p, const GmGraph& g, hipStream_t s) {
  hipLaunchKernelGGL(k_bg_apply, bg_grid(p), dim3(256), 0, s, p, g);
  HIP_CHECK(hipGetLastError());
}

void launch_bg_alpha(const BgPanel& p, hipStream_t s, const CgChain* chain) {
  if (chain) hipLaunchKernelGGL(k_bg_alpha<CgChain>, dim3((unsigned)p.slabs), dim3(kGmSumThreads), 0, s, p, *chain);
  else hipLaunchKernelGGL(k_bg_alpha<CgNoChain>, dim3((unsigned)p.slabs), dim3(kGmSumThreads), 0, s, p, CgNoChain{});
  HIP_CHECK(hipGetLastError());
}

void launch_bg_update(const BgPanel& p, hipStream_t s) {
  hipLaunchKernelGGL(k_bg_update, bg_grid(p), dim3(256), 0, s, p);
  HIP_CHECK(hipGetLastError());
}

void launch_bg_beta(const BgPanel& p, int it, hipStream_t s) {
  hipLaunchKernelGGL(k_bg_beta, dim3((unsigned)p.nq), dim3(kGmSumThreads), 0, s, p, it);
  HIP_CHECK(hipGetLastError());
}

void launch_bg_direction(const BgPanel& p, hipStream_t s) {
  hipLaunchKernelGGL(k_bg_direction, bg_grid(p), dim3(256), 0, s, p);
  HIP_CHECK(hipGetLastError());
}

void launch_bg_ysum(const BgPanel& p, const BgBundleArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_bg_ysum, dim3((unsigned)((p.N + 3) / 4)), dim3(256), 0, s, p, a);
  HIP_CHECK(hipGetLastError());
}

void launch_bg_bundle(const BgPanel& p, const BgBundleArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_bg_bundle, dim3((unsigned)((p.N + 3) / 4), (unsigned)p.nq), dim3(256), 0, s, p, a);
  HIP_CHECK(hipGetLastError());
}

}  // namespace osc

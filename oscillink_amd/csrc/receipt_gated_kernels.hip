// Receipts under per-query gates: what osc_receipt_gated_many adds to the panel PCG of
// bundle_gated_kernels.hip -- the settle's start from the handle's state, deltaH as the operator's quadratic form of
// U_q - U*_q, and the per-(row, query) components and null-point candidates of the solved panel.
//
// Layout, partition and launch geometry are gates_many_kernels.hip's (one workgroup per (row part, slab), 4 waves of 8 rows
// x 8 lanes x float4); the row kernel is k_bg_bundle's (one wave per (row, query)).  Sums are fp64 in a fixed order that
// knows N and the query's own slabs alone, so a query's answers are the same to the bit in any batch or chunk.
#include "receipt_gated.hpp"
#include "chain_gated_dev.hpp"

namespace osc {
namespace {

// k_bg_init's gather over the state U (row-major, pitch ld): x0 = U and r0 = b - (I + dt M_q) U without a stored b,
// b = U + dt (lamG Y + lamQ g psi^T): the U terms cancel, r0 = dt [lamG (y - u) + lamQ g (psi - u) + lamC (W u - u)].  With a
// prior (chain_gated.hpp) every row adds -dt lamP u; the chain rows' share is launch_cg_path_init's.
template <class Prior>
__global__ __launch_bounds__(256) void k_rg_settle_init(const BgPanel p, const GmGraph g, const float* __restrict__ U,
                                                        const float* __restrict__ Y, int32_t ld, float dt, float lamG,
                                                        float lamC, float lamQ, const Prior pr) {
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
        v[u] = e0 + u < deg ? ld_anchor(U, ju, ld, c, p.D) : f4(0.f);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const float wu = __shfl(wv, g0 + u, 64);
        sum = mulacc4(f4(wu), v[u], sum);
      }
    }
    if (ok) {
      const float4 y = ld_anchor(Y, row, ld, c, p.D), x = ld_anchor(U, row, ld, c, p.D);
      const float gi = gate[row], qg = lamQ * gi, inv_md = bg_inv_md(p, gi);
      float4 r;
      r.x = dt * fmaf(lamG, y.x - x.x, fmaf(qg, ps.x - x.x, lamC * (sum.x - x.x)));
      r.y = dt * fmaf(lamG, y.y - x.y, fmaf(qg, ps.y - x.y, lamC * (sum.y - x.y)));
      r.z = dt * fmaf(lamG, y.z - x.z, fmaf(qg, ps.z - x.z, lamC * (sum.z - x.z)));
      r.w = dt * fmaf(lamG, y.w - x.w, fmaf(qg, ps.w - x.w, lamC * (sum.w - x.w)));
      if constexpr (Prior::active) r = mulacc4(f4(-pr.cP), x, r);
      const float4 z = scale4(r, inv_md);
      const size_t o = so + (size_t)row * 32 + lr * 4;
      st4(p.X + o, x);
      st4(p.R + o, r);
      st4(p.P + o, z);
      rz = mulacc4(r, z, rz);
    }
  }
  gm_fold(rz, sh, p.part_a + gm_part_at(p));
}

__global__ __launch_bounds__(256) void k_rg_diff(const BgPanel p, const float* __restrict__ Us, const float* __restrict__ U,
                                                 int32_t ld) {
  const int slab = blockIdx.y, q = slab / p.spq;
  const int t = threadIdx.x, lr = t & 7;
  const int c = (slab % p.spq) * 32 + lr * 4;
  const size_t so = (size_t)slab * p.N * 32;
  if (blockIdx.x == 0 && slab % p.spq == 0 && t == 0) p.live[q] = 1;  // launch_bg_apply runs over every query
  const GmRows rr = gm_rows(p);
  for (int64_t rb = rr.r0; rb < rr.r1; rb += 32) {
    const int64_t row = rb + (t >> 3);
    if (row >= rr.r1) continue;
    const size_t o = so + (size_t)row * 32 + lr * 4;
    const float4 x = ld4(p.X + o);
    const float4 u = Us ? ld4(Us + o) : ld_anchor(U, row, ld, c, p.D);
    st4(p.P + o, make_float4(u.x - x.x, u.y - x.y, u.z - x.z, u.w - x.w));
  }
}

// one workgroup per query: the columns' p . M_q p, parts in gm_part_sum's order, then columns and slabs in order
template <class Chain>
__global__ __launch_bounds__(kGmSumThreads) void k_rg_deltah(const BgPanel p, double* __restrict__ dh, const Chain ch) {
  __shared__ double sh[kGmSumThreads];
  __shared__ double col[32];
  const int q = blockIdx.x, t = threadIdx.x;
  double acc = 0.0;
  for (int s = 0; s < p.spq; ++s) {
    double v = gm_part_sum(p.part_a + (size_t)(q * p.spq + s) * p.parts * 32, p.parts, sh);
    if constexpr (Chain::active) v += cg_unit_sum(ch, q * p.spq + s, q);
    if (t < 32) col[t] = v;
    __syncthreads();
    if (t == 0)
      for (int c = 0; c < 32; ++c) acc += col[c];
    __syncthreads();
  }
  if (t == 0) dh[q] = acc;
}

__device__ __forceinline__ double sq4(const float4 a, const float4 b) {
  const double dx = (double)a.x - (double)b.x, dy = (double)a.y - (double)b.y;
  const double dz = (double)a.z - (double)b.z, dw = (double)a.w - (double)b.w;
  return dx * dx + dy * dy + dz * dz + dw * dw;
}

// one wave per (row, query) over the query's solved slabs.  A lane owns the columns 4 lane + 256 u; every sum over the
// columns is the lanes' shares added by the fixed butterfly, so all lanes hold the same value and walk the edges together.
__global__ __launch_bounds__(256) void k_rg_components(const BgPanel p, const RgRowsArgs a) {
  const int lane = threadIdx.x & 63, q = blockIdx.y;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= p.N) return;
  const int deg = min(a.deg[row], a.width);
  const double si = 1.0 / ((double)a.sqrt_deg[row] + 1e-12);
  const float* __restrict__ psi = p.psi + (size_t)q * p.spq * 32;
  const float* __restrict__ Xq = p.X + (size_t)q * p.spq * p.N * 32;
  const int cols = p.spq * 32;
  double an = 0.0, qr = 0.0;
  for (int c = lane * 4; c < cols; c += 256) {
    const float4 ui = ld4(Xq + ((size_t)(c / 32) * p.N + row) * 32 + (c & 31));
    an += sq4(ui, ld_anchor(a.Y, row, a.ld, c, p.D));  // (a pad column: 0 - 0)
    qr += sq4(ui, ld4(psi + c));
  }
  an = wave_sum(an);
  qr = wave_sum(qr);
  const double lamC = (double)p.lamC;
  double usum = 0.0, s1 = 0.0, s2 = 0.0, rmax = 0.0;
  int jmax = -1;
  for (int e = 0; e < deg; ++e) {
    const float w = a.adj[(size_t)row * a.width + e];
    if (!(w > 0.f)) continue;  // (the same for every lane of the wave)
    const int j = a.col[(size_t)row * a.width + e];
    const double sj = 1.0 / ((double)a.sqrt_deg[j] + 1e-12);
    double d2 = 0.0;
    for (int c = lane * 4; c < cols; c += 256) {
      const float* __restrict__ X = Xq + (size_t)(c / 32) * p.N * 32 + (c & 31);
      d2 += sqdiff4(ld4(X + (size_t)row * 32), si, ld4(X + (size_t)j * 32), sj);
    }
    d2 = wave_sum(d2);
    usum += (double)w * d2;
    const double R = lamC * (double)w * d2;
    s1 += R;
    s2 += R * R;
    // np.argmax over the dense row: strict >, ties to the smaller API column id (k_rm_rows' rule)
    bool take = R > rmax;
    if (!take && R == rmax && R > 0.0 && jmax >= 0) take = a.api_id ? a.api_id[j] < a.api_id[jmax] : j < jmax;
    if (take) {
      rmax = R;
      jmax = j;
    }
  }
  if (lane != 0) return;
  const size_t o = (size_t)row * a.qs + q, cell = (size_t)p.N * a.qs;
  a.comp[o] = 0.5 * lamC * (a.ysum[row] - usum);
  a.comp[cell + o] = (double)p.lamG * an;
  a.comp[2 * cell + o] = (double)p.lamQ * (double)p.gate[(size_t)q * p.N + row] * qr;
  const double inv_n = 1.0 / (double)p.N;
  const double mu = s1 * inv_n;
  const double var = fmax(s2 * inv_n - mu * mu, 0.0);
  const double z = (rmax - mu) / (sqrt(var) + 1e-12);
  const bool is_null = jmax >= 0 && rmax > 0.0 && z > (double)a.z_th;
  a.z[o] = is_null ? (float)z : -INFINITY;
  a.j[o] = is_null ? (a.api_id ? a.api_id[jmax] : jmax) : -1;
  a.r[o] = is_null ? (float)rmax : 0.f;
}

dim3 rg_grid(const BgPanel& p) { return dim3((unsigned)p.parts, (unsigned)p.slabs); }

}  // namespace

void launch_rg_settle_init(const BgPanel& ps, const GmGraph& g, const float* U, const float* Y, int32_t ld, float dt, float lamG,
                           float lamC, float lamQ, hipStream_t s, const CgPrior* prior) {
  if (prior)
    hipLaunchKernelGGL(k_rg_settle_init<CgPrior>, rg_grid(ps), dim3(256), 0, s, ps, g, U, Y, ld, dt, lamG, lamC, lamQ, *prior);
  else
    hipLaunchKernelGGL(k_rg_settle_init<CgNoPrior>, rg_grid(ps), dim3(256), 0, s, ps, g, U, Y, ld, dt, lamG, lamC, lamQ,
                       CgNoPrior{});
  HIP_CHECK(hipGetLastError());
}

void launch_rg_diff(const BgPanel& p, const float* Us, const float* U, int32_t ld, hipStream_t s) {
  hipLaunchKernelGGL(k_rg_diff, rg_grid(p), dim3(256), 0, s, p, Us, U, ld);
  HIP_CHECK(hipGetLastError());
}

void launch_rg_deltah(const BgPanel& p, double* dh, hipStream_t s, const CgChain* chain) {
  if (chain) hipLaunchKernelGGL(k_rg_deltah<CgChain>, dim3((unsigned)p.nq), dim3(kGmSumThreads), 0, s, p, dh, *chain);
  else hipLaunchKernelGGL(k_rg_deltah<CgNoChain>, dim3((unsigned)p.nq), dim3(kGmSumThreads), 0, s, p, dh, CgNoChain{});
  HIP_CHECK(hipGetLastError());
}

void launch_rg_components(const BgPanel& p, const RgRowsArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_rg_components, dim3((unsigned)((p.N + 3) / 4), (unsigned)p.nq), dim3(256), 0, s, p, a);
  HIP_CHECK(hipGetLastError());
}

}  // namespace osc

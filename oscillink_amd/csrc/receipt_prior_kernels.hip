// receipt() under per-query chain priors (osc_receipt_prior_many).  Query q's stationary state is
//   U*_q = X' + x' psi_q^T + G C,   C = T_q V_q (m <= 64 rows),
// on the basis (X', x') of M' = M + lamP I and the Green's columns G of the chain's m distinct nodes; it is never formed.
//
//   k_rp_moments   G^T [X' - Y | B X' | x' | B (x' - 1)] per (row part, 32-column slab) on v_mfma_f32_32x32x2_f32: a tall-skinny
//                  GEMM with K = N, the parts finished in fp64 in part order (k_rp_moments_finish)
//   k_rp_gram      G^T G and G^T diag(B) G on the m columns of every distinct chain, fp64
//   k_rp_scalars   per query deltaH by the identity of section 12.3 and the anchor / query sums
//   k_rp_rows      the fused row pass: coherence drop and the null-point candidate per (row, query)
//
// Every sum runs in an order fixed by N, the query's own chain and the row's own edge list, so a query's bytes do not depend
// on the pass's width, the query's position, the chunking or gs.  No atomics.
#include "query.hpp"

#include "gates_many_plan.hpp"

namespace osc {
namespace {

#include "bundle_prior_dev.hpp"

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kMomRows = host::kGatesStepRows;  // rows of a step: 32
constexpr int kMomCols = 128;                   // X' columns of a workgroup: 4 waves x 32, each with its X' - Y and B X' tile
constexpr int kMomPitch = 2 * kMomCols + 32;    // floats of an LDS row of V: an odd multiple of 32 banks

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// grid (parts, nslab, chunks + 1): chunk z < chunks serves the X' columns [128 z, 128 z + 128), the last one x' and B (x' - 1)
__global__ __launch_bounds__(256) void k_rp_moments(const RpMomArgs a) {
  __shared__ float sG[kMomRows][32];
  __shared__ float sV[kMomRows][kMomPitch];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int p = blockIdx.x, sl = blockIdx.y, cz = blockIdx.z;
  const bool scal = cz == (int)gridDim.z - 1;
  const int r0 = p * a.part_rows, r1 = min(a.N, r0 + a.part_rows);
  const float* Gs = a.G + (size_t)(a.slab0 + sl) * (size_t)a.N * 32;
  f32x16 acc0, acc1;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc0[i] = acc1[i] = 0.f;
  for (int rb = r0; rb < r1; rb += kMomRows) {
    {  // the panel's 32 x 32 tile: one 16-byte access a lane
      const int r = t >> 3, c4 = (t & 7) * 4;
      float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
      if (rb + r < r1) g = ld4(Gs + (size_t)(rb + r) * 32 + c4);
      *reinterpret_cast<float4*>(&sG[r][c4]) = g;
    }
    if (!scal) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int idx = t + 256 * i;
        const int r = idx >> 5, c4 = (idx & 31) * 4;
        const int col = cz * kMomCols + c4, row = rb + r;
        float4 d = make_float4(0.f, 0.f, 0.f, 0.f), bx = d;
        if (row < r1 && col < a.ld) {
          const float4 x = ld4(a.X + (size_t)row * a.ld + col), y = ld4(a.Y + (size_t)row * a.ld + col);
          const float Bi = a.B[row];
          if (col < a.D) { d.x = x.x - y.x; bx.x = Bi * x.x; }
          if (col + 1 < a.D) { d.y = x.y - y.y; bx.y = Bi * x.y; }
          if (col + 2 < a.D) { d.z = x.z - y.z; bx.z = Bi * x.z; }
          if (col + 3 < a.D) { d.w = x.w - y.w; bx.w = Bi * x.w; }
        }
        *reinterpret_cast<float4*>(&sV[r][c4]) = d;
        *reinterpret_cast<float4*>(&sV[r][kMomCols + c4]) = bx;
      }
    } else if (t < kMomRows * 8) {  // columns 0 .. 31 of the step's rows: x', B (x' - 1), zeros
      const int r = t >> 3, c4 = (t & 7) * 4, row = rb + r;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c4 == 0 && row < r1) {
        const float xi = a.x4[(size_t)row * 4];
        v.x = xi;
        v.y = a.B[row] * (xi - 1.0f);
      }
      *reinterpret_cast<float4*>(&sV[r][c4]) = v;
    }
    __syncthreads();
    if (!scal || wv == 0) {
      const int c = lane & 31, h = lane >> 5;
#pragma unroll
      for (int kk = 0; kk < kMomRows / 2; ++kk) {
        const float av = sG[2 * kk + h][c];
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, sV[2 * kk + h][32 * wv + c], acc0, 0, 0, 0);
        if (!scal) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av, sV[2 * kk + h][kMomCols + 32 * wv + c], acc1, 0, 0, 0);
      }
    }
    __syncthreads();
  }
  // the accumulator's column is the lane's w, its rows (panel columns) sit in the 16 registers
  float* out = a.part + ((size_t)sl * a.parts + p) * 32 * (size_t)a.wout;
  const int c = lane & 31, h = lane >> 5;
  if (scal) {
    if (wv == 0 && c < 2) {
#pragma unroll
      for (int i = 0; i < 16; ++i) out[(size_t)((i & 3) + 8 * (i >> 2) + 4 * h) * a.wout + 2 * a.ld + c] = acc0[i];
    }
    return;
  }
  const int col = cz * kMomCols + 32 * wv + c;
  if (col >= a.ld) return;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    float* o = out + (size_t)((i & 3) + 8 * (i >> 2) + 4 * h) * a.wout;
    o[col] = acc0[i];
    o[a.ld + col] = acc1[i];
  }
}

// mom[(32 (slab0 + sl) + c) * wout + w] = sum over the parts, in part order, fp64
__global__ __launch_bounds__(256) void k_rp_moments_finish(const float* __restrict__ part, int32_t parts, int32_t slab0,
                                                           int32_t wout, double* __restrict__ mom) {
  const int w = blockIdx.x * 256 + threadIdx.x;
  const int c = blockIdx.y, sl = blockIdx.z;
  if (w >= wout) return;
  double s = 0.0;
  for (int p = 0; p < parts; ++p) s += (double)part[(((size_t)sl * parts + p) * 32 + c) * (size_t)wout + w];
  mom[((size_t)(slab0 + sl) * 32 + c) * (size_t)wout + w] = s;
}

// grid (n_sys, groups): entry (b, c) of a chain's Gram blocks by one thread, over the group's parts in order
__global__ __launch_bounds__(256) void k_rp_gram(const RpGramArgs a) {
  const int sy = blockIdx.x, grp = blockIdx.y;
  const int m = a.sys_m[sy];
  const int32_t* cols = a.sys_cols + a.sys_col_at[sy];
  const int p0 = grp * a.per, p1 = min(a.parts, p0 + a.per);
  for (int o = threadIdx.x; o < m * m; o += 256) {
    const int cb = cols[o / m], cc = cols[o % m];
    double ga = 0.0, gb = 0.0;
    for (int p = p0; p < p1; ++p) {
      const int r0 = p * a.part_rows, r1 = min(a.N, r0 + a.part_rows);
      double sa = 0.0, sb = 0.0;
      for (int r = r0; r < r1; ++r) {
        const double pr = (double)a.G[panel_at(a.N, r, cb)] * (double)a.G[panel_at(a.N, r, cc)];
        sa += pr;
        sb += (double)a.B[r] * pr;
      }
      ga += sa;
      gb += sb;
    }
    a.part[((size_t)grp * 2) * (size_t)a.msq + (size_t)a.g_at[sy] + o] = ga;
    a.part[((size_t)grp * 2 + 1) * (size_t)a.msq + (size_t)a.g_at[sy] + o] = gb;
  }
}

// the workgroup's sum of v in a fixed tree order (every thread gets it)
__device__ __forceinline__ double block_sum(double v, double* sh) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) sh[t] += sh[t + s];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(256) void k_rp_scalars(const RpScalArgs a) {
  __shared__ float sG[kBpNodes * kBpNodes];    // Ghat[b][c] = G[row_b, col_c]
  __shared__ double sGH[kBpNodes * kBpNodes];  // Ghat H
  __shared__ double sh[256];
  const int q = blockIdx.x, t = threadIdx.x;
  const int sy = a.b.q_sys[q];
  const int m = a.b.sys_m[sy];
  const int D = a.b.D, ld = a.b.ld;
  const int32_t* cols = a.b.sys_cols + a.b.sys_col_at[sy];
  const int32_t* rows = a.sys_rows + a.b.sys_col_at[sy];
  const float* C = a.b.TV + a.b.tv_at[q];
  const float* psi = a.b.psi + (size_t)q * ld;
  const double* H = a.b.H + (size_t)q * kBpNodes * kBpNodes;
  const double* e = a.b.e + (size_t)q * kBpNodes;
  double* J = a.J + (size_t)q * kBpNodes * kBpNodes;
  double* Z = a.Z + (size_t)q * kBpNodes * kBpNodes;
  // J = F0 C^T and Z = F0 F0^T over F0 = (U - X' - x' psi^T)[nodes]: an entry by one thread, columns in order
  for (int o = t; o < m * m; o += 256) {
    const int b = o / m, c = o - b * m;
    const size_t rb = (size_t)rows[b] * ld, rc = (size_t)rows[c] * ld;
    const double xb = (double)a.x4[(size_t)rows[b] * 4], xc = (double)a.x4[(size_t)rows[c] * 4];
    const float* Cc = C + (size_t)c * ld;
    double j = 0.0, z = 0.0;
    for (int d = 0; d < D; ++d) {
      const double ps = (double)psi[d];
      const double fb = (double)a.U[rb + d] - (double)a.X[rb + d] - xb * ps;
      const double fc = (double)a.U[rc + d] - (double)a.X[rc + d] - xc * ps;
      j += fb * (double)Cc[d];
      z += fb * fc;
    }
    J[b * kBpNodes + c] = j;
    Z[b * kBpNodes + c] = z;
    sG[b * kBpNodes + c] = a.b.G[panel_at(a.b.N, rows[b], cols[c])];
  }
  __syncthreads();
  for (int o = t; o < m * m; o += 256) {
    const int b = o / m, c = o - b * m;
    double s = 0.0;
    for (int k = 0; k < m; ++k) s += (double)sG[b * kBpNodes + k] * H[k * kBpNodes + c];
    sGH[b * kBpNodes + c] = s;
  }
  __syncthreads();
  const double* base = a.base;
  const double* h1 = base + 8;
  const double* a1 = h1 + D;
  const double* b1 = a1 + D;
  double v_dh1 = 0.0, v_nd = 0.0, v_n2 = 0.0, v_a1 = 0.0, v_b1 = 0.0;
  for (int d = t; d < D; d += 256) {
    const double ps = (double)psi[d], dl = ps - (double)a.psi0[d];
    v_dh1 += dl * h1[d];
    v_nd += dl * dl;
    v_n2 += ps * ps;
    if (a.full) {
      v_a1 += ps * a1[d];
      v_b1 += ps * b1[d];
    }
  }
  const double dh1 = block_sum(v_dh1, sh), nd = block_sum(v_nd, sh), n2 = block_sum(v_n2, sh);
  double v_tr = 0.0, v_gh = 0.0, v_k = 0.0;
  for (int o = t; o < m * m; o += 256) {
    const int b = o / m, c = o - b * m;
    if (b == c) v_tr += J[b * kBpNodes + b];
    v_gh += (double)sG[b * kBpNodes + c] * H[b * kBpNodes + c];
  }
  for (int k = a.k_at[sy] + t; k < a.k_at[sy + 1]; k += 256) {  // tr(F^T K F) entry by entry, F = F0 - Ghat C
    const int r = a.kr[k], c = a.kc[k];
    double ff = Z[r * kBpNodes + c];
    for (int n = 0; n < m; ++n) {
      const double gr = (double)sG[r * kBpNodes + n], gc = (double)sG[c * kBpNodes + n];
      ff += sGH[r * kBpNodes + n] * gc - J[r * kBpNodes + n] * gc - gr * J[c * kBpNodes + n];
    }
    v_k += (double)a.lamP * (double)a.kw[k] * ff;
  }
  const double trJ = block_sum(v_tr, sh), gh = block_sum(v_gh, sh), kf = block_sum(v_k, sh);
  double anchor = 0.0, query = 0.0;
  if (a.full) {
    const double pa1 = block_sum(v_a1, sh), pb1 = block_sum(v_b1, sh);
    double v_cpa = 0.0, v_cpb = 0.0, v_ega = 0.0, v_egb = 0.0, v_hga = 0.0, v_hgb = 0.0;
    for (int b = 0; b < m; ++b) {
      const double* mrow = a.mom + (size_t)cols[b] * a.wout;
      const float* Cb = C + (size_t)b * ld;
      for (int d = t; d < D; d += 256) {
        v_cpa += (double)Cb[d] * mrow[d];
        v_cpb += (double)Cb[d] * mrow[ld + d];
      }
      if (t == 0) {
        v_ega += e[b] * mrow[2 * ld];
        v_egb += e[b] * mrow[2 * ld + 1];
      }
    }
    for (int o = t; o < m * m; o += 256) {
      const int b = o / m, c = o - b * m;
      double ga = 0.0, gb = 0.0;
      for (int g = 0; g < a.groups; ++g) {
        ga += a.gram_part[((size_t)g * 2) * (size_t)a.msq + (size_t)a.g_at[sy] + o];
        gb += a.gram_part[((size_t)g * 2 + 1) * (size_t)a.msq + (size_t)a.g_at[sy] + o];
      }
      v_hga += H[b * kBpNodes + c] * ga;
      v_hgb += H[b * kBpNodes + c] * gb;
    }
    const double cpa = block_sum(v_cpa, sh), cpb = block_sum(v_cpb, sh), ega = block_sum(v_ega, sh);
    const double egb = block_sum(v_egb, sh), hga = block_sum(v_hga, sh), hgb = block_sum(v_hgb, sh);
    anchor = base[6] * (base[2] + 2.0 * pa1 + n2 * base[3] + 2.0 * cpa + 2.0 * ega + hga);
    query = base[7] * (base[4] + 2.0 * pb1 + n2 * base[5] + 2.0 * cpb + 2.0 * egb + hgb);
  }
  if (t == 0) {
    double* o = a.scal + (size_t)q * 4;
    o[0] = base[0] - 2.0 * dh1 + nd * base[1] - 2.0 * trJ + gh - kf;
    o[1] = anchor;
    o[2] = query;
    o[3] = 0.0;
    a.res_out[q] = a.res_in[q];
    a.iters_out[q] = a.iters_in[q];
  }
}

__global__ __launch_bounds__(256) void k_rp_rows(const RpRowsArgs ra) {
  const BpArgs& a = ra.b;
  BpWho w;
  if (!bp_who(a, w)) return;
  const int row = w.row;
  const float inv_i = 1.0f / (a.sqrt_deg[row] + 1e-12f);
  const BpLane vi = bp_lane(a, w, inv_i);
  const double e_b = a.e[(size_t)w.q * kBpNodes + w.b];
  const size_t o = (size_t)row * a.qs + w.q;
  const double s_i = (double)a.s[row], p_i = (double)a.p[o], nu_i = a.nu[o], n2 = a.pn2[w.q];
  const bool mine = w.b < w.m;
  const int my_col = mine ? w.cols[w.b] : 0;
  double acc = 0.0, s1 = 0.0, s2 = 0.0, rmax = 0.0;
  int jmax = -1;
  const int deg = a.deg[row];
  const size_t eo = (size_t)row * a.width;
  const int32_t* crow = a.col + eo;
  const float* arow = a.adj + eo;
  for (int e = 0; e < deg; ++e) {  // in slot order: every lane of the group walks the same edges
    const float wt = arow[e];
    if (!(wt > 0.f)) continue;
    const int j = crow[e];
    const float inv_j = 1.0f / (a.sqrt_deg[j] + 1e-12f);
    const float gj = mine ? a.G[panel_at(a.N, j, my_col)] * inv_j : 0.f;
    const float kj = mine ? a.kappa[(size_t)j * a.ks + w.koff + w.b] : 0.f;
    const size_t oj = (size_t)j * a.qs + w.q;
    const double ds = s_i - (double)a.s[j], dp = p_i - (double)a.p[oj];
    const double dg = (double)vi.gamma - (double)gj, dk = (double)vi.kappa - (double)kj;
    const double lane_t = 2.0 * dg * (dk + ds * e_b) - 2.0 * (double)gj * vi.t;
    const double x = group_sum_d(lane_t, a.gs) + nu_i + a.nu[oj];  // 2 dgamma . (dkappa + ds e) + dgamma^T H dgamma
    const double fw = (double)a.lamC * (double)wt;
    const double cross = 2.0 * ds * dp;
    acc += 0.5 * fw * (cross + x);
    const double R = fw * ((double)ra.dslot[eo + e] + cross + ds * ds * n2 + x);
    s1 += R;
    s2 += R * R;
    // first argmax in the reference's column order: strict >, ties to the smaller API column id
    bool take = R > rmax;
    if (!take && R == rmax && R > 0.0 && jmax >= 0) take = ra.api_id ? ra.api_id[j] < ra.api_id[jmax] : j < jmax;
    if (take) {
      rmax = R;
      jmax = j;
    }
  }
  if (!w.live || w.b != 0) return;
  ra.cohd[o] = a.c0[row] - n2 * a.c2[row] - acc;
  const double inv_n = 1.0 / (double)a.N;
  const double mu = s1 * inv_n;
  const double var = fmax(s2 * inv_n - mu * mu, 0.0);
  const double z = (rmax - mu) / (sqrt(var) + 1e-12);
  const bool is_null = jmax >= 0 && rmax > 0.0 && z > (double)ra.z_th;
  ra.z[o] = is_null ? (float)z : -INFINITY;
  ra.j[o] = is_null ? (ra.api_id ? ra.api_id[jmax] : jmax) : -1;
  ra.r[o] = is_null ? (float)rmax : 0.f;
}

__global__ __launch_bounds__(256) void k_rp_colsum(const double* __restrict__ coh, int32_t N, int32_t qs, int32_t nq, int32_t nb,
                                                   double* __restrict__ part) {
  const int q = blockIdx.y * 256 + threadIdx.x, b = blockIdx.x;
  if (q >= nq) return;
  double s = 0.0;
  for (int64_t r = b; r < N; r += nb) s += coh[(size_t)r * qs + q];
  part[(size_t)b * nq + q] = s;
}

}  // namespace

void launch_rp_moments(const RpMomArgs& a, hipStream_t s) {
  if (a.nslab <= 0 || a.N <= 0) return;
  const dim3 grid((unsigned)a.parts, (unsigned)a.nslab, (unsigned)((a.ld + kMomCols - 1) / kMomCols + 1));
  hipLaunchKernelGGL(k_rp_moments, grid, dim3(256), 0, s, a);
  HIP_CHECK(hipGetLastError());
}

void launch_rp_moments_finish(const float* part, int32_t parts, int32_t slab0, int32_t nslab, int32_t wout, double* mom,
                              hipStream_t s) {
  if (nslab <= 0) return;
  hipLaunchKernelGGL(k_rp_moments_finish, dim3((unsigned)((wout + 255) / 256), 32, (unsigned)nslab), dim3(256), 0, s, part, parts,
                     slab0, wout, mom);
  HIP_CHECK(hipGetLastError());
}

void launch_rp_gram(const RpGramArgs& a, hipStream_t s) {
  if (a.n_sys <= 0) return;
  hipLaunchKernelGGL(k_rp_gram, dim3((unsigned)a.n_sys, (unsigned)a.groups), dim3(256), 0, s, a);
  HIP_CHECK(hipGetLastError());
}

void launch_rp_scalars(const RpScalArgs& a, hipStream_t s) {
  if (a.b.nq <= 0) return;
  hipLaunchKernelGGL(k_rp_scalars, dim3((unsigned)a.b.nq), dim3(256), 0, s, a);
  HIP_CHECK(hipGetLastError());
}

void launch_rp_rows(const RpRowsArgs& a, hipStream_t s) {
  const int per = 64 / a.b.gs;
  const int64_t waves = (int64_t)a.b.N * ((a.b.nq + per - 1) / per);
  if (waves <= 0) return;
  hipLaunchKernelGGL(k_rp_rows, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, a);
  HIP_CHECK(hipGetLastError());
}

void launch_rp_colsum(const double* coh, int32_t N, int32_t qs, int32_t nq, int32_t nb, double* part, hipStream_t s) {
  if (nq <= 0) return;
  hipLaunchKernelGGL(k_rp_colsum, dim3((unsigned)nb, (unsigned)((nq + 255) / 256)), dim3(256), 0, s, coh, N, qs, nq, nb, part);
  HIP_CHECK(hipGetLastError());
}

}  // namespace osc

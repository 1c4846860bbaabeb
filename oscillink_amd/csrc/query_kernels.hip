// Multi-query bundles: per-basis row constants, the fp32 MFMA GEMM behind the query dots and the
// batched MMR's similarity updates, the coherence pass, the per-query z-score and the batched MMR argmax.
// Every per-query quantity is computed the same way whatever the batch holds: a query's GEMM outputs run the same
// K order in every tile column, and its reductions run over rows only, so a query's answer does not depend on the
// other queries of its batch, on its position or on the chunking.
#include "query.hpp"

namespace osc {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

__device__ __forceinline__ float wave_sum_f(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// a * sa - b * sb with both products rounded on their own (receipt_kernels.hip: sdiff)
__device__ __forceinline__ float sdiff(float a, float sa, float b, float sb) {
#pragma clang fp contract(off)
  const float p = a * sa;
  const float q = b * sb;
  return p - q;
}

__device__ __forceinline__ float4 masked4(const float* row, int c, int D) {
  float4 v = ld4(row + c);
  if (c + 3 >= D) {
    if (c + 1 >= D) v.y = 0.f;
    if (c + 2 >= D) v.z = 0.f;
    if (c + 3 >= D) v.w = 0.f;
  }
  return v;
}

// ---- per-basis row constants (one wave per row) --------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_query_basis_stats(const QueryBasisArgs a) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.N) return;
  const float inv_i = 1.0f / (a.sqrt_deg[row] + 1e-12f);
  // s in fp64: (s_i - s_j)^2 |psi|^2 carries one rounding of s through every column of the row
  const double s_i = (double)a.x4[(size_t)row * 4] / ((double)a.sqrt_deg[row] + 1e-12);
  const float* yi = a.Y + (size_t)row * a.ld;
  const float* Xi = a.X + (size_t)row * a.ld;
  double n2 = 0.0;
  for (int c = lane * 4; c < a.D; c += 256) {
    const float4 v = masked4(Xi, c, a.D);
    n2 += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
  }
  n2 = wave_sum_d(n2);
  const int deg = a.deg[row];
  const int32_t* crow = a.col + (size_t)row * a.width;
  const float* arow = a.adj + (size_t)row * a.width;
  double c0 = 0.0, c2 = 0.0;
  for (int e = 0; e < deg; ++e) {  // in edge order: every lane forms the same sums
    const float w = arow[e];
    if (!(w > 0.f)) continue;
    const int j = crow[e];
    const float inv_j = 1.0f / (a.sqrt_deg[j] + 1e-12f);
    const float* yj = a.Y + (size_t)j * a.ld;
    const float* Xj = a.X + (size_t)j * a.ld;
    float dy = 0.f, dp = 0.f;
    for (int c = lane * 4; c < a.D; c += 256) {
      const float4 y0 = masked4(yi, c, a.D), y1 = masked4(yj, c, a.D);
      const float4 p0 = masked4(Xi, c, a.D), p1 = masked4(Xj, c, a.D);
      const float e0 = sdiff(y0.x, inv_i, y1.x, inv_j), e1 = sdiff(y0.y, inv_i, y1.y, inv_j);
      const float e2 = sdiff(y0.z, inv_i, y1.z, inv_j), e3 = sdiff(y0.w, inv_i, y1.w, inv_j);
      const float f0 = sdiff(p0.x, inv_i, p1.x, inv_j), f1 = sdiff(p0.y, inv_i, p1.y, inv_j);
      const float f2 = sdiff(p0.z, inv_i, p1.z, inv_j), f3 = sdiff(p0.w, inv_i, p1.w, inv_j);
      dy = fmaf(e0, e0, fmaf(e1, e1, fmaf(e2, e2, fmaf(e3, e3, dy))));
      dp = fmaf(f0, f0, fmaf(f1, f1, fmaf(f2, f2, fmaf(f3, f3, dp))));
    }
    dy = wave_sum_f(dy);
    dp = wave_sum_f(dp);
    const double hw = 0.5 * (double)a.lamC * (double)w;
    const double ds = s_i - (double)a.x4[(size_t)j * 4] / ((double)a.sqrt_deg[j] + 1e-12);
    c0 += hw * ((double)dy - (double)dp);
    c2 += hw * ds * ds;
  }
  if (lane == 0) {
    a.s[row] = s_i;
    a.xn2[row] = n2;
    a.c0[row] = c0;
    a.c2[row] = c2;
  }
}

// ---- C = A . Bt^T on v_mfma_f32_32x32x2_f32 -------------------------------------------------------------------------
// 128 x 128 outputs per workgroup, 4 waves of 2 x 2 tiles of 32 x 32; K in steps of 32 through LDS.  Operand lanes
// (cdna_hip_programming.md section 3): A[i = l & 31][k = l >> 5], B[k = l >> 5][j = l & 31]; C: col = l & 31,
// row = (r & 3) + 8 (r >> 2) + 4 (l >> 5).  Every output accumulates k = 0, 1, ..., kpad - 1 in that order, one fma
// per product, whichever tile it falls in.
constexpr int kTM = 128, kTS = kQueryTileK + 4;  // LDS row stride 36 floats: 16-byte rows, 2-way read conflicts at most

template <int MODE>
__global__ __launch_bounds__(256) void k_query_gemm(const QueryGemmArgs a) {
  __shared__ __attribute__((aligned(16))) float As[kTM * kTS];
  __shared__ __attribute__((aligned(16))) float Bs[kQueryTileQ * kTS];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int wr = w & 1, wc = w >> 1;
  const int64_t row0 = (int64_t)blockIdx.x * kTM;
  const int q0 = blockIdx.y * kQueryTileQ;
  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  const int kq = (t & 7) * 4;
  for (int k0 = 0; k0 < a.kpad; k0 += kQueryTileK) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int r = (t >> 3) + 32 * it;
      const int64_t gr = row0 + r;
      const int k = k0 + kq;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (gr < a.N && k < a.D) v = masked4(a.A + gr * a.ld, k, a.D);
      *reinterpret_cast<float4*>(&As[r * kTS + kq]) = v;
      *reinterpret_cast<float4*>(&Bs[r * kTS + kq]) = ld4(a.Bt + (size_t)(q0 + r) * a.kpad + k);
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < kQueryTileK; kk += 2) {
      const int kl = kk + (lane >> 5);
      float av[2], bv[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) av[i] = As[(wr * 64 + i * 32 + (lane & 31)) * kTS + kl];
#pragma unroll
      for (int j = 0; j < 2; ++j) bv[j] = Bs[(wc * 64 + j * 32 + (lane & 31)) * kTS + kl];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t row = row0 + wr * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      if (row >= a.N) continue;
      float inv = 0.f, x = 0.f;
      double xn2 = 0.0;
      if (MODE == 0) {
        inv = 1.0f / (a.sqrt_deg[row] + 1e-12f);
        x = a.x4[row * 4];
        xn2 = a.xn2[row];
      }
      if (MODE == 2) inv = 1.0f / (a.sqrt_deg[row] + 1e-12f);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int q = q0 + wc * 64 + j * 32 + (lane & 31);
        if (q >= a.qs) continue;
        const size_t o = (size_t)row * a.qs + q;
        const float g = acc[i][j][r];
        if (MODE == 0) {
          if (q < a.nq) {
            const double pn2 = a.pn2[q], xd = (double)x, gd = (double)g;
            const double dot = gd + xd * pn2;
            const double un2 = xn2 + 2.0 * xd * gd + xd * xd * pn2;
            a.align[o] = (float)(dot / (sqrt(fmax(un2, 0.0)) + 1e-12) * a.pinv[q]);
            a.p[o] = g * inv;
          } else {
            a.align[o] = 0.f;
            a.p[o] = 0.f;
          }
        } else if (MODE == 2) {
          a.p[o] = q < a.nq ? g * inv : 0.f;
        } else if (q < a.nq) {
          const float m = a.maxsim[o];
          if (m != INFINITY) a.maxsim[o] = a.first ? g : fmaxf(m, g);
        }
      }
    }
  }
}

// ---- coherence drop per (row, query): one wave per row, lanes over the queries (Q-wide, coalesced neighbour rows) -----
__global__ __launch_bounds__(256) void k_query_coh(const int32_t* __restrict__ col, const float* __restrict__ adj,
                                                   const int32_t* __restrict__ degs, int32_t width, int32_t N, float lamC,
                                                   const double* __restrict__ s, const double* __restrict__ c0,
                                                   const double* __restrict__ c2, const double* __restrict__ pn2,
                                                   const float* __restrict__ p, int32_t qs, int32_t nq,
                                                   float* __restrict__ coh) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  constexpr int U = kQueryChunk / 64;
  double acc[U], pi[U];
  const float* prow = p + (size_t)row * qs;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int q = lane + 64 * u;
    acc[u] = 0.0;
    pi[u] = q < nq ? (double)prow[q] : 0.0;
  }
  const double si = s[row];
  const int deg = degs[row];
  const int32_t* crow = col + (size_t)row * width;
  const float* arow = adj + (size_t)row * width;
  for (int e0 = 0; e0 < deg; e0 += 64) {
    const int e = e0 + lane;
    const int jl = e < deg ? crow[e] : 0;
    const float wl = e < deg ? arow[e] : 0.f;
    const double sl = e < deg ? s[jl] : 0.0;
    const int n = min(64, deg - e0);
    for (int tt = 0; tt < n; ++tt) {
      const float wt = __shfl(wl, tt, 64);
      const int jt = __shfl(jl, tt, 64);
      const double st = __shfl(sl, tt, 64);
      if (!(wt > 0.f)) continue;
      const double f = (double)lamC * (double)wt * (si - st);
      const float* pj = p + (size_t)jt * qs;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int q = lane + 64 * u;
        if (q < nq) acc[u] += f * (pi[u] - (double)pj[q]);
      }
    }
  }
  const double a0 = c0[row], a2 = c2[row];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int q = lane + 64 * u;
    if (q < qs) coh[(size_t)row * qs + q] = q < nq ? (float)(a0 - pn2[q] * a2 - acc[u]) : 0.f;
  }
}

// ---- per-query mean / std of coh (two stages, fp64, fixed order) and the score ---------------------------------------
__global__ __launch_bounds__(256) void k_query_colsum(const float* coh, int32_t N, int32_t qs, int32_t nq, double2* part) {
  const int q = blockIdx.y * 256 + threadIdx.x;
  if (q >= nq) return;
  double s1 = 0.0, s2 = 0.0;
  for (int64_t r = blockIdx.x; r < N; r += gridDim.x) {
    const double v = (double)coh[(size_t)r * qs + q];
    s1 += v;
    s2 += v * v;
  }
  part[(size_t)blockIdx.x * nq + q] = make_double2(s1, s2);
}

__global__ __launch_bounds__(256) void k_query_colstats(const double2* part, int nb, int32_t N, int32_t nq, double2* stats) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= nq) return;
  double s1 = 0.0, s2 = 0.0;
  for (int b = 0; b < nb; ++b) {
    const double2 v = part[(size_t)b * nq + q];
    s1 += v.x;
    s2 += v.y;
  }
  const double mu = s1 / (double)N;
  const double var = fmax(s2 / (double)N - mu * mu, 0.0);
  stats[q] = make_double2(mu, sqrt(var) + 1e-12);  // np.mean / np.std(coh) + 1e-12 (lattice.py:530-568)
}

__global__ __launch_bounds__(256) void k_query_score(float* cs, const float* align, int64_t n, int32_t qs, int32_t nq,
                                                     double alpha, const double2* stats) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int q = (int)(i % qs);
  if (q >= nq) {
    cs[i] = 0.f;
    return;
  }
  const double2 st = stats[q];
  const double z = st.y > 0.0 ? ((double)cs[i] - st.x) / st.y : 0.0;
  cs[i] = (float)(alpha * z + (1.0 - alpha) * (double)align[i]);
}

// ---- row-normalised anchors -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rows_normalise(const float* Y, float* Yn, int32_t N, int32_t D, int32_t ld) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  const float* y = Y + (size_t)row * ld;
  float n2 = 0.f;
  for (int c = lane * 4; c < D; c += 256) {
    const float4 v = masked4(y, c, D);
    n2 = fmaf(v.x, v.x, fmaf(v.y, v.y, fmaf(v.z, v.z, fmaf(v.w, v.w, n2))));
  }
  n2 = wave_sum_f(n2);
  const float inv = 1.0f / (sqrtf(n2) + 1e-12f);
  float* o = Yn + (size_t)row * ld;
  for (int c = lane * 4; c < ld; c += 256) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < D) v = masked4(y, c, D);
    *reinterpret_cast<float4*>(o + c) = make_float4(v.x * inv, v.y * inv, v.z * inv, v.w * inv);
  }
}

// ---- batched MMR ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool mmr_better(double v, int id, double bv, int bid) { return v > bv || (v == bv && id < bid); }

// stage 1: per (row block, query) best (value, API id, device row); rows strided by the grid
__global__ __launch_bounds__(256) void k_mmr_many_argmax1(const MmrManyArgs a, int first) {
  const int q = blockIdx.y * 256 + threadIdx.x;
  if (q >= a.nq) return;
  double bv = -1.0e300;
  int bid = 0x7fffffff, brow = -1;
  for (int64_t r = blockIdx.x; r < a.N; r += gridDim.x) {
    const size_t o = (size_t)r * a.qs + q;
    const float m = a.maxsim[o];
    if (m == INFINITY) continue;
    const double v = (1.0 - a.lambda) * (double)a.score[o] - (first ? 0.0 : a.lambda * (double)m);
    const int id = a.api_id ? a.api_id[r] : (int)r;
    if (brow < 0 || mmr_better(v, id, bv, bid)) {
      bv = v;
      bid = id;
      brow = (int)r;
    }
  }
  const size_t o = (size_t)blockIdx.x * a.nq + q;
  a.pval[o] = bv;
  a.pid[o] = bid;
  a.prow[o] = brow;
}

// stage 2: one workgroup per query -- the winner; record it, mark it taken, write its normalised anchor row into Bt
__global__ __launch_bounds__(256) void k_mmr_many_argmax2(const MmrManyArgs a, int nb, int step) {
  __shared__ double sv[256];
  __shared__ int sid[256], srow[256];
  const int q = blockIdx.x;
  double bv = -1.0e300;
  int bid = 0x7fffffff, brow = -1;
  for (int b = threadIdx.x; b < nb; b += 256) {
    const size_t o = (size_t)b * a.nq + q;
    if (a.prow[o] >= 0 && (brow < 0 || mmr_better(a.pval[o], a.pid[o], bv, bid))) {
      bv = a.pval[o];
      bid = a.pid[o];
      brow = a.prow[o];
    }
  }
  sv[threadIdx.x] = bv;
  sid[threadIdx.x] = bid;
  srow[threadIdx.x] = brow;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) {
      const int t = threadIdx.x + o;
      if (srow[t] >= 0 && (srow[threadIdx.x] < 0 || mmr_better(sv[t], sid[t], sv[threadIdx.x], sid[threadIdx.x]))) {
        sv[threadIdx.x] = sv[t];
        sid[threadIdx.x] = sid[t];
        srow[threadIdx.x] = srow[t];
      }
    }
    __syncthreads();
  }
  const int row = srow[0];
  if (threadIdx.x == 0) {
    a.chosen_api[(size_t)q * a.k + step] = row >= 0 ? sid[0] : -1;
    a.chosen_row[(size_t)q * a.k + step] = row;
    if (row >= 0) a.maxsim[(size_t)row * a.qs + q] = INFINITY;
  }
  float* bt = a.Bt + (size_t)q * a.kpad;
  for (int c = threadIdx.x; c < a.kpad; c += 256) bt[c] = (row >= 0 && c < a.D) ? a.Yn[(size_t)row * a.ld + c] : 0.f;
}

__global__ __launch_bounds__(256) void k_query_pack(const float* score, const float* align, const int32_t* chosen_row,
                                                    int32_t qs, int32_t nq, int32_t k, float* os, float* oa) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nq * k) return;
  const int q = i / k;
  const int row = chosen_row[i];
  os[i] = row >= 0 ? score[(size_t)row * qs + q] : 0.f;
  oa[i] = row >= 0 ? align[(size_t)row * qs + q] : 0.f;
}

}  // namespace

void launch_query_basis_stats(const QueryBasisArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_query_basis_stats, dim3((unsigned)((a.N + 3) / 4)), dim3(256), 0, s, a);
  HIP_CHECK(hipGetLastError());
}

void launch_query_gemm(const QueryGemmArgs& a, hipStream_t s) {
  const dim3 grid((unsigned)((a.N + kTM - 1) / kTM), (unsigned)(query_qpad(a.nq) / kQueryTileQ));
  if (a.mode == 0) hipLaunchKernelGGL(k_query_gemm<0>, grid, dim3(256), 0, s, a);
  else if (a.mode == 2) hipLaunchKernelGGL(k_query_gemm<2>, grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL(k_query_gemm<1>, grid, dim3(256), 0, s, a);
  HIP_CHECK(hipGetLastError());
}

void launch_query_coh(const int32_t* col, const float* adj, const int32_t* deg, int32_t width, int32_t N, float lamC,
                      const double* s, const double* c0, const double* c2, const double* pn2, const float* p, int32_t qs,
                      int32_t nq, float* coh, hipStream_t st) {
  hipLaunchKernelGGL(k_query_coh, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, col, adj, deg, width, N, lamC, s, c0, c2,
                     pn2, p, qs, nq, coh);
  HIP_CHECK(hipGetLastError());
}

int query_stat_parts(int32_t N) { return (int)std::max<int64_t>(1, std::min<int64_t>(((int64_t)N + 63) / 64, 512)); }

void launch_query_score(float* cs, const float* align, int32_t N, int32_t qs, int32_t nq, double alpha, double2* part,
                        double2* stats, hipStream_t st) {
  const int nb = query_stat_parts(N);
  const unsigned qb = (unsigned)((nq + 255) / 256);
  hipLaunchKernelGGL(k_query_colsum, dim3((unsigned)nb, qb), dim3(256), 0, st, cs, N, qs, nq, part);
  hipLaunchKernelGGL(k_query_colstats, dim3(qb), dim3(256), 0, st, part, nb, N, nq, stats);
  const int64_t n = (int64_t)N * qs;
  hipLaunchKernelGGL(k_query_score, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, cs, align, n, qs, nq, alpha, stats);
  HIP_CHECK(hipGetLastError());
}

void launch_rows_normalise(const float* Y, float* Yn, int32_t N, int32_t D, int32_t ld, hipStream_t st) {
  hipLaunchKernelGGL(k_rows_normalise, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, Y, Yn, N, D, ld);
  HIP_CHECK(hipGetLastError());
}

int mmr_many_parts(int32_t N) { return (int)std::max<int64_t>(1, std::min<int64_t>(((int64_t)N + 63) / 64, 512)); }

void launch_mmr_many_argmax(const MmrManyArgs& a, int step, hipStream_t st) {
  const int nb = mmr_many_parts(a.N);
  hipLaunchKernelGGL(k_mmr_many_argmax1, dim3((unsigned)nb, (unsigned)((a.nq + 255) / 256)), dim3(256), 0, st, a,
                     step == 0 ? 1 : 0);
  hipLaunchKernelGGL(k_mmr_many_argmax2, dim3((unsigned)a.nq), dim3(256), 0, st, a, nb, step);
  HIP_CHECK(hipGetLastError());
}

void launch_query_pack(const float* score, const float* align, const int32_t* chosen_row, int32_t qs, int32_t nq, int32_t k,
                       float* out_score, float* out_align, hipStream_t st) {
  const int n = nq * k;
  if (n <= 0) return;
  hipLaunchKernelGGL(k_query_pack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, score, align, chosen_row, qs, nq, k,
                     out_score, out_align);
  HIP_CHECK(hipGetLastError());
}

}  // namespace osc

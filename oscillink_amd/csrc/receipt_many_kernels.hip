// Multi-query receipts: the per-basis and per-call terms of receipt_many, the fused per-(row,
// query) coherence / null-point pass and the per-query null-point selection.  Every per-query quantity is formed the
// same way whatever the batch holds: reductions run over rows in a fixed order per query column, so a query's receipt
// does not depend on the other queries of its batch, its position or the chunking.
#include "query.hpp"

namespace osc {
namespace {

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

// a * sa - b * sb with both products rounded on their own (query_kernels.hip / receipt_kernels.hip: sdiff)
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

// ---- per basis: M x and the per-slot |P_i - P_j|^2 (one wave per row) ---------------------------------------------------
__global__ __launch_bounds__(256) void k_rm_basis_rows(const RmBasisArgs a) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.N) return;
  const int deg = a.g.deg[row];
  const size_t eo = (size_t)row * a.g.width;
  const int32_t* crow = a.g.col + eo;
  const float* wrow = a.g.w + eo;
  double acc = 0.0;
  for (int e = lane; e < deg; e += 64) acc += (double)wrow[e] * (double)a.x4[(size_t)crow[e] * 4];
  acc = wave_sum_d(acc);
  double accp = 0.0;
  if (a.g.path_slot != nullptr) {
    const int ps = a.g.path_slot[row];
    if (ps >= 0) {
      const int pd = a.g.pdeg[ps];
      for (int e = lane; e < pd; e += 64) {
        const size_t o = (size_t)ps * a.g.pwidth + e;
        accp += (double)a.g.pw[o] * (double)a.x4[(size_t)a.g.pcol[o] * 4];
      }
    }
  }
  accp = wave_sum_d(accp);
  const double xi = (double)a.x4[(size_t)row * 4];
  const double cs = (double)a.op.cs_const + (double)a.op.cs_B * (double)a.B[row];
  if (lane == 0) a.Mx[row] = cs * xi - (double)a.op.cW * acc - (double)a.op.cP * accp;
  if (a.dslot == nullptr) return;
  const float inv_i = 1.0f / (a.sqrt_deg[row] + 1e-12f);
  const float* Xi = a.X + (size_t)row * a.ld;
  const float* arow = a.adj + eo;
  for (int e = 0; e < deg; ++e) {  // k_query_basis_stats' dp, edge by edge
    const float w = arow[e];
    if (!(w > 0.f)) {
      if (lane == 0) a.dslot[eo + e] = 0.f;
      continue;
    }
    const int j = crow[e];
    const float inv_j = 1.0f / (a.sqrt_deg[j] + 1e-12f);
    const float* Xj = a.X + (size_t)j * a.ld;
    float dp = 0.f;
    for (int c = lane * 4; c < a.D; c += 256) {
      const float4 p0 = masked4(Xi, c, a.D), p1 = masked4(Xj, c, a.D);
      const float f0 = sdiff(p0.x, inv_i, p1.x, inv_j), f1 = sdiff(p0.y, inv_i, p1.y, inv_j);
      const float f2 = sdiff(p0.z, inv_i, p1.z, inv_j), f3 = sdiff(p0.w, inv_i, p1.w, inv_j);
      dp = fmaf(f0, f0, fmaf(f1, f1, fmaf(f2, f2, fmaf(f3, f3, dp))));
    }
    dp = wave_sum_f(dp);
    if (lane == 0) a.dslot[eo + e] = dp;
  }
}

// ---- fp64 column sums, rows dealt to nb partials (row r -> r % nb, in row order) ---------------------------------------
template <int MODE>
__global__ __launch_bounds__(256) void k_rm_cols(const RmColArgs a) {
  const int c = blockIdx.y * 256 + threadIdx.x;
  const int b = blockIdx.x;
  const bool scal = MODE == 0 && blockIdx.y == 0 && threadIdx.x == 0;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, t0 = 0.0, t1 = 0.0, t2 = 0.0;
  const double pc = (MODE == 1 && c < a.ld) ? (double)a.psi0[c] : 0.0;
  for (int64_t r = b; r < a.N; r += a.nb) {
    const double xd = (double)a.x4[(size_t)r * 4];
    const size_t o = (size_t)r * a.ld + c;
    if (MODE == 0) {
      const double Bd = (double)a.B[r];
      if (scal) {
        t0 += xd * xd;
        t1 += Bd * (xd - 1.0) * (xd - 1.0);
        t2 += xd * a.Mx[r];
      }
      if (c < a.D) {
        const double X = (double)a.X[o], dxy = X - (double)a.Y[o];
        s0 += xd * dxy;
        s1 += Bd * (xd - 1.0) * X;
        s2 += dxy * dxy;
        s3 += Bd * X * X;
      }
    } else if (c < a.ld) {
      const double X = (double)a.X[o], u0 = X + xd * pc;
      a.U0[o] = (float)u0;
      if (c < a.D) s0 += ((double)a.U[o] - u0) * a.Mx[r];
    }
  }
  if (c < a.ld) {
    if (MODE == 0) {
      double* p = a.part + (size_t)b * 4 * a.ld + c;
      p[0] = s0;
      p[(size_t)a.ld] = s1;
      p[(size_t)2 * a.ld] = s2;
      p[(size_t)3 * a.ld] = s3;
    } else {
      a.part[(size_t)b * a.ld + c] = s0;
    }
  }
  if (scal) {
    a.spart[(size_t)b * 3] = t0;
    a.spart[(size_t)b * 3 + 1] = t1;
    a.spart[(size_t)b * 3 + 2] = t2;
  }
}

// out[y * W + w] = sum over the rows b of group y (per rows each, y = blockIdx.y) of part[b * W + w], in row order
__global__ __launch_bounds__(256) void k_rm_colfinish(const double* part, int nb, int per, int64_t W, double* out) {
  const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (w >= W) return;
  const int b0 = blockIdx.y * per, b1 = min(nb, b0 + per);
  double s = 0.0;
  for (int b = b0; b < b1; ++b) s += part[(size_t)b * W + w];
  out[(size_t)blockIdx.y * W + w] = s;
}

// ---- fused per-(row, query) pass: one wave per row at a time, lanes over the queries --------------------------------------
__global__ __launch_bounds__(256) void k_rm_rows(const RmRowsArgs a) {
  const int lane = threadIdx.x & 63;
  const int wv = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wv >= a.nw) return;
  constexpr int U = kQueryChunk / 64;
  double csum[U], pn2[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int q = lane + 64 * u;
    csum[u] = 0.0;
    pn2[u] = q < a.nq ? a.pn2[q] : 0.0;
  }
  const double lamC = (double)a.lamC, inv_n = 1.0 / (double)a.N;
  for (int row = wv; row < a.N; row += a.nw) {
    double acc[U], pi[U], s1[U], s2[U], rmax[U];
    int jmax[U];
    const float* prow = a.p + (size_t)row * a.qs;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int q = lane + 64 * u;
      acc[u] = s1[u] = s2[u] = rmax[u] = 0.0;
      jmax[u] = -1;
      pi[u] = q < a.nq ? (double)prow[q] : 0.0;
    }
    const double si = a.s[row];
    const int deg = a.deg[row];
    const size_t eo = (size_t)row * a.width;
    for (int e0 = 0; e0 < deg; e0 += 64) {
      const int e = e0 + lane;
      const int jl = e < deg ? a.col[eo + e] : 0;
      const float wl = e < deg ? a.adj[eo + e] : 0.f;
      const double sl = e < deg ? a.s[jl] : 0.0;
      const float dl = e < deg ? a.dslot[eo + e] : 0.f;
      const int n = min(64, deg - e0);
      for (int tt = 0; tt < n; ++tt) {
        const float wt = __shfl(wl, tt, 64);
        const int jt = __shfl(jl, tt, 64);
        const double st = __shfl(sl, tt, 64);
        const float dt = __shfl(dl, tt, 64);
        if (!(wt > 0.f)) continue;
        const double ds = si - st;
        const double fw = lamC * (double)wt;
        const double f = fw * ds;  // k_query_coh's factor
        const double ds2p = ds * ds;
        const float* pj = a.p + (size_t)jt * a.qs;
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int q = lane + 64 * u;
          if (q < a.nq) {
            const double dpq = pi[u] - (double)pj[q];
            acc[u] += f * dpq;
            const double R = fw * ((double)dt + 2.0 * ds * dpq + ds2p * pn2[u]);
            s1[u] += R;
            s2[u] += R * R;
            // first argmax in the reference's column order: strict >, ties to the smaller API column id
            bool take = R > rmax[u];
            if (!take && R == rmax[u] && R > 0.0 && jmax[u] >= 0)
              take = a.api_id ? a.api_id[jt] < a.api_id[jmax[u]] : jt < jmax[u];
            if (take) {
              rmax[u] = R;
              jmax[u] = jt;
            }
          }
        }
      }
    }
    const double c0 = a.c0[row], c2 = a.c2[row];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int q = lane + 64 * u;
      if (q >= a.qs) continue;
      const size_t o = (size_t)row * a.qs + q;
      if (q >= a.nq) {
        a.z[o] = -INFINITY;
        a.j[o] = -1;
        a.r[o] = 0.f;
        continue;
      }
      csum[u] += c0 - pn2[u] * c2 - acc[u];
      const double mu = s1[u] * inv_n;
      const double var = fmax(s2[u] * inv_n - mu * mu, 0.0);
      const double z = (rmax[u] - mu) / (sqrt(var) + 1e-12);
      const bool is_null = jmax[u] >= 0 && rmax[u] > 0.0 && z > (double)a.z_th;
      a.z[o] = is_null ? (float)z : -INFINITY;
      a.j[o] = is_null ? (a.api_id ? a.api_id[jmax[u]] : jmax[u]) : -1;
      a.r[o] = is_null ? (float)rmax[u] : 0.f;
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int q = lane + 64 * u;
    if (q < a.nq) a.cohpart[(size_t)wv * a.nq + q] = csum[u];
  }
}

// ---- z per query in API row order (64 x 64 tiles through LDS) -----------------------------------------------------------
__global__ __launch_bounds__(256) void k_rm_transpose(const float* z, const int32_t* inv, int32_t N, int32_t qs, int32_t nq,
                                                      float* zt) {
  __shared__ float t[64][65];
  const int a0 = blockIdx.x * 64, q0 = blockIdx.y * 64;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  for (int k = ty; k < 64; k += 4) {
    const int a = a0 + k, q = q0 + tx;
    float v = -INFINITY;
    if (a < N && q < nq) {
      const int d = inv ? inv[a] : a;
      v = z[(size_t)d * qs + q];
    }
    t[k][tx] = v;
  }
  __syncthreads();
  for (int k = ty; k < 64; k += 4) {
    const int q = q0 + k, a = a0 + tx;
    if (q < nq && a < N) zt[(size_t)q * N + a] = t[tx][k];
  }
}

__global__ __launch_bounds__(256) void k_rm_null_count(const float* zt, int32_t N, int32_t* total) {
  __shared__ int part[4];
  const float* zq = zt + (size_t)blockIdx.x * N;
  int n = 0;
  for (int a = threadIdx.x; a < N; a += 256) n += zq[a] > -INFINITY ? 1 : 0;
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) total[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// ---- per-query selection: 1024 threads, API rows in chunks of 1024 ----------------------------------------------------------
constexpr int kSelT = 1024;
static_assert(kRmSelectMax == kSelT, "the selection sorts one key per thread");

// order-preserving key of a float (0 = no null point: never the key of a finite value)
__device__ __forceinline__ uint32_t zkey(float v) {
  if (!(v > -INFINITY)) return 0u;
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// exclusive prefix count of flag over the block (thread order = API row order); *total = the block's count
__device__ __forceinline__ int block_scan(bool flag, int* wsum, int* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long m = __ballot(flag);
  const int pre = __popcll(m & ((1ull << lane) - 1ull));
  if (lane == 0) wsum[w] = __popcll(m);
  __syncthreads();
  int wpre = 0, tot = 0;
#pragma unroll
  for (int t = 0; t < kSelT / 64; ++t) {
    const int v = wsum[t];
    wpre += t < w ? v : 0;
    tot += v;
  }
  __syncthreads();
  *total = tot;
  return wpre + pre;
}

__global__ __launch_bounds__(kSelT) void k_rm_null_select(const RmSelectArgs a) {
  __shared__ uint32_t hist[256];
  __shared__ uint32_t skey[kSelT];
  __shared__ int32_t sapi[kSelT];
  __shared__ int wsum[kSelT / 64];
  __shared__ uint32_t st_prefix, st_mask, st_k;
  __shared__ int st_n;
  const int q = blockIdx.x, tid = threadIdx.x;
  const float* zq = a.zt + (size_t)q * a.N;
  const int64_t base = a.off[q];
  auto emit = [&](int64_t o, int ar) {
    const size_t d = (size_t)(a.inv ? a.inv[ar] : ar) * a.qs + q;
    a.oi[o] = ar;
    a.oj[o] = a.j[d];
    a.oz[o] = zq[ar];
    a.orr[o] = a.r[d];
  };
  if (!a.sel[q]) {  // every null point, API row order
    int run = 0;
    for (int a0 = 0; a0 < a.N; a0 += kSelT) {
      const int ar = a0 + tid;
      const bool flag = ar < a.N && zq[ar] > -INFINITY;
      int tot = 0;
      const int pos = block_scan(flag, wsum, &tot);
      if (flag) emit(base + run + pos, ar);
      run += tot;
    }
    return;
  }
  // the cap-th largest key by an 8-bit radix select, then how many keys equal to it are kept (the first in API order)
  uint32_t prefix = 0u, mask = 0u, k = (uint32_t)a.cap;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    if (tid < 256) hist[tid] = 0u;
    __syncthreads();
    for (int ar = tid; ar < a.N; ar += kSelT) {
      const uint32_t kk = zkey(zq[ar]);
      if (kk != 0u && (kk & mask) == prefix) atomicAdd(&hist[(kk >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      uint32_t cum = 0u;
      for (int b = 255; b >= 0; --b) {
        const uint32_t h = hist[b];
        if (cum + h >= k) {
          prefix |= (uint32_t)b << shift;
          k -= cum;
          break;
        }
        cum += h;
      }
      mask |= 255u << shift;
      st_prefix = prefix;
      st_mask = mask;
      st_k = k;
    }
    __syncthreads();
    prefix = st_prefix;
    mask = st_mask;
    k = st_k;
  }
  const uint32_t T = prefix;
  if (tid == 0) st_n = 0;
  sapi[tid] = 0x7fffffff;
  skey[tid] = 0u;
  __syncthreads();
  int eqrun = 0;
  for (int a0 = 0; a0 < a.N; a0 += kSelT) {
    const int ar = a0 + tid;
    const uint32_t kk = ar < a.N ? zkey(zq[ar]) : 0u;
    int tot = 0;
    const int eqpos = eqrun + block_scan(kk == T, wsum, &tot);
    if (kk > T || (kk == T && eqpos < (int)k)) {
      const int slot = atomicAdd(&st_n, 1);
      if (slot < kSelT) {
        skey[slot] = kk;
        sapi[slot] = ar;
      }
    }
    eqrun += tot;
  }
  __syncthreads();
  // bitonic sort: z descending, then API row ascending (the reference's stable sort of the API-ordered list)
  for (int size = 2; size <= kSelT; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      const int l = tid ^ stride;
      if (l > tid) {
        const uint32_t ki = skey[tid], kl = skey[l];
        const int ai = sapi[tid], al = sapi[l];
        const bool l_first = kl > ki || (kl == ki && al < ai);
        const bool i_first = ki > kl || (ki == kl && ai < al);
        if ((tid & size) == 0 ? l_first : i_first) {
          skey[tid] = kl;
          skey[l] = ki;
          sapi[tid] = al;
          sapi[l] = ai;
        }
      }
      __syncthreads();
    }
  }
  if (tid < a.cap && skey[tid] != 0u) emit(base + tid, sapi[tid]);
}

}  // namespace

void launch_rm_basis_rows(const RmBasisArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_rm_basis_rows, dim3((unsigned)((a.N + 3) / 4)), dim3(256), 0, s, a);
  HIP_CHECK(hipGetLastError());
}

int rm_col_parts(int64_t N) { return (int)std::max<int64_t>(1, std::min<int64_t>((N + 63) / 64, 512)); }

void launch_rm_cols(const RmColArgs& a, int mode, hipStream_t s) {
  const dim3 grid((unsigned)a.nb, (unsigned)((a.ld + 255) / 256));
  if (mode == 0) hipLaunchKernelGGL(k_rm_cols<0>, grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL(k_rm_cols<1>, grid, dim3(256), 0, s, a);
  HIP_CHECK(hipGetLastError());
}

void launch_rm_colfinish(const double* part, int nb, int64_t W, double* out, double* scratch, hipStream_t s) {
  if (W <= 0) return;
  const dim3 wb((unsigned)((W + 255) / 256));
  if (nb <= kRmFinishRows) {
    hipLaunchKernelGGL(k_rm_colfinish, wb, dim3(256), 0, s, part, nb, nb, W, out);
  } else {  // groups of rows into scratch, then all groups in order
    const int ng = rm_finish_groups(nb);
    hipLaunchKernelGGL(k_rm_colfinish, dim3(wb.x, (unsigned)ng), dim3(256), 0, s, part, nb, kRmFinishRows, W, scratch);
    hipLaunchKernelGGL(k_rm_colfinish, wb, dim3(256), 0, s, scratch, ng, ng, W, out);
  }
  HIP_CHECK(hipGetLastError());
}

int rm_row_waves(int64_t N) { return (int)std::max<int64_t>(1, std::min<int64_t>(N, 8192)); }

void launch_rm_rows(const RmRowsArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_rm_rows, dim3((unsigned)((a.nw + 3) / 4)), dim3(256), 0, s, a);
  HIP_CHECK(hipGetLastError());
}

void launch_rm_transpose(const float* z, const int32_t* inv, int32_t N, int32_t qs, int32_t nq, float* zt, hipStream_t s) {
  hipLaunchKernelGGL(k_rm_transpose, dim3((unsigned)((N + 63) / 64), (unsigned)((nq + 63) / 64)), dim3(256), 0, s, z, inv, N,
                     qs, nq, zt);
  HIP_CHECK(hipGetLastError());
}

void launch_rm_null_count(const float* zt, int32_t N, int32_t nq, int32_t* total, hipStream_t s) {
  hipLaunchKernelGGL(k_rm_null_count, dim3((unsigned)nq), dim3(256), 0, s, zt, N, total);
  HIP_CHECK(hipGetLastError());
}

void launch_rm_null_select(const RmSelectArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_rm_null_select, dim3((unsigned)a.nq), dim3(kSelT), 0, s, a);
  HIP_CHECK(hipGetLastError());
}

}  // namespace osc

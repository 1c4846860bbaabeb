// Settle and receipt of every candidate lattice of a corpus refine chunk, behind the U* solve and
// the bundle of osc_corpus.hip: k_cq_settle (one implicit-Euler step from U = Y) and k_cq_receipt (deltaH, the component
// sums, the null points), one workgroup per lattice each.  No workgroup waits on another.
#include "common.hpp"
#include "corpus_receipts.hpp"

namespace osc {
namespace {

__device__ __forceinline__ float wave_sum_f(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum_d2(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// settle() of a fresh lattice (U = Y), one workgroup per lattice: Jacobi-PCG of the implicit-Euler step
// (I + dt M) U+ = Y + dt (lamG Y + lamQ B psi^T) from x0 = Y (lattice.py:159-230; settle_op of osc_solve.hip): operator
// constant 1 + dt (lamG + lamC) + dt lamQ B_i, off-diagonal -dt lamC W, Jacobi diagonal 1 + dt lamG + dt lamQ B_i (without
// lamC: lattice.py:185-192), solver.py's epsilons and stop rule.  k_cq_solve's structure: thread t owns the columns
// t + 256 m and walks the lattice's rows in row order with fp64 column sums; only the stop test crosses threads.  The
// rows' constants are formed once in LDS, with B_i = 1.0f where there are no gates, so gates of exactly 1 give the ungated
// bytes.  A kernel of its own: k_cq_solve's instantiations are not touched by it.
template <int NC>
__global__ __launch_bounds__(256) void k_cq_settle(const CqSettleArgs a) {
  __shared__ float red[4];
  __shared__ float s_cs[host::kCorpusMaxTopK], s_inv[host::kCorpusMaxTopK], s_qb[host::kCorpusMaxTopK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lat = blockIdx.x;
  const int64_t r0 = (int64_t)lat * a.K, r1 = r0 + a.K;
  const float* psi = a.psi + (size_t)lat * a.ldn;
  const float cW = a.dt * a.lamC, rbY = a.dt * a.lamG, cQ = a.dt * a.lamQ;
  for (int r = tid; r < a.K; r += 256) {
    const float Bi = a.B ? a.B[r0 + r] : 1.0f;
    s_cs[r] = fmaf(cQ, Bi, 1.0f + a.dt * (a.lamG + a.lamC));
    s_inv[r] = 1.f / (fmaf(cQ, Bi, 1.0f + a.dt * a.lamG) + 1e-12f);
    s_qb[r] = cQ * Bi;
  }
  __syncthreads();
  int cidx[NC];
  bool on[NC];
#pragma unroll
  for (int m = 0; m < NC; ++m) {
    cidx[m] = tid + 256 * m;
    on[m] = cidx[m] < a.ldn;
    if (!on[m]) cidx[m] = 0;
  }
  auto apply = [&](const float* v, int64_t i, float (&out)[NC]) {
    float acc[NC];
#pragma unroll
    for (int m = 0; m < NC; ++m) acc[m] = 0.f;
    const int d = a.deg[i];
    for (int e = 0; e < d; ++e) {
      const int64_t j = a.col[i * a.k + e];
      const float wij = a.w[i * a.k + e];
#pragma unroll
      for (int m = 0; m < NC; ++m) acc[m] = fmaf(wij, v[j * a.ldn + cidx[m]], acc[m]);
    }
    const float csi = s_cs[i - r0];
#pragma unroll
    for (int m = 0; m < NC; ++m) out[m] = csi * v[i * a.ldn + cidx[m]] - cW * acc[m];
  };
  double rz[NC], t1[NC], t2[NC];
#pragma unroll
  for (int m = 0; m < NC; ++m) rz[m] = 0.0;
  for (int64_t i = r0; i < r1; ++i) {  // x0 = Y, r = b - A x0, p = z = r / diag
    float o[NC];
    apply(a.Y, i, o);
    const float qbi = s_qb[i - r0], invMdi = s_inv[i - r0];
#pragma unroll
    for (int m = 0; m < NC; ++m) {
      if (!on[m]) continue;
      const size_t off = (size_t)i * a.ldn + cidx[m];
      const float y = a.Y[off];
      const float rr = (y + rbY * y + qbi * psi[cidx[m]]) - o[m];
      const float z = rr * invMdi;
      a.X[off] = y;
      a.R[off] = rr;
      a.P[off] = z;
      rz[m] += (double)rr * (double)z;
    }
  }
  int it = 1;
  float resv = 0.f;
  for (; it <= a.max_iters; ++it) {
#pragma unroll
    for (int m = 0; m < NC; ++m) t1[m] = 0.0;
    for (int64_t i = r0; i < r1; ++i) {
      float o[NC];
      apply(a.P, i, o);
#pragma unroll
      for (int m = 0; m < NC; ++m) {
        if (!on[m]) continue;
        const size_t off = (size_t)i * a.ldn + cidx[m];
        a.AP[off] = o[m];
        t1[m] += (double)a.P[off] * (double)o[m];
      }
    }
    float alpha[NC];
#pragma unroll
    for (int m = 0; m < NC; ++m) {
      alpha[m] = (float)(rz[m] / (t1[m] + 1e-18));  // solver.py:25-26
      t1[m] = t2[m] = 0.0;
    }
    for (int64_t i = r0; i < r1; ++i) {
      const float invMdi = s_inv[i - r0];
#pragma unroll
      for (int m = 0; m < NC; ++m) {
        if (!on[m]) continue;
        const size_t off = (size_t)i * a.ldn + cidx[m];
        a.X[off] = fmaf(a.P[off], alpha[m], a.X[off]);
        const float rr = fmaf(-a.AP[off], alpha[m], a.R[off]);
        a.R[off] = rr;
        t1[m] += (double)rr * (double)rr;
        t2[m] += (double)rr * (double)(rr * invMdi);
      }
    }
    float mx = 0.f;
#pragma unroll
    for (int m = 0; m < NC; ++m) {  // NaN propagates (solver.py:29 reports NaN for a diverged column)
      const float v = on[m] ? (float)sqrt(t1[m]) : 0.f;
      mx = (v != v || mx != mx) ? __uint_as_float(0x7FC00000u) : fmaxf(mx, v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float v = __shfl_xor(mx, o, 64);
      mx = (v != v || mx != mx) ? __uint_as_float(0x7FC00000u) : fmaxf(mx, v);
    }
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    resv = red[0];
#pragma unroll
    for (int u = 1; u < 4; ++u) resv = (red[u] != red[u] || resv != resv) ? __uint_as_float(0x7FC00000u) : fmaxf(resv, red[u]);
    __syncthreads();
    if (resv <= a.tol) break;  // solver.py:30-31, before the beta / p update
    if (it == a.max_iters) break;
    for (int64_t i = r0; i < r1; ++i) {
      const float invMdi = s_inv[i - r0];
#pragma unroll
      for (int m = 0; m < NC; ++m) {
        if (!on[m]) continue;
        const size_t off = (size_t)i * a.ldn + cidx[m];
        const float beta = (float)(t2[m] / (rz[m] + 1e-18));  // solver.py:33-34
        a.P[off] = fmaf(a.P[off], beta, a.R[off] * invMdi);
      }
    }
#pragma unroll
    for (int m = 0; m < NC; ++m) rz[m] = t2[m];
  }
  if (tid == 0) {
    a.iters[lat] = it > a.max_iters ? a.max_iters : it;
    a.res[lat] = resv;
  }
}


// receipt_kernels.hip's sdiff: a sa - b sb with both products rounded on their own, so that edge (i, j) and edge (j, i) get
// bit-identical energies
__device__ __forceinline__ float cq_sdiff(float a, float sa, float b, float sb) {
#pragma clang fp contract(off)
  const float p = a * sa;
  const float q = b * sb;
  return p - q;
}

// receipt() of one lattice per workgroup (lattice.py receipt(), receipts.py:10-83), a wave per row:
//   deltaH   = sum_i E_i . (M E)_i, E = U+ - U*, M the U* operator (lamG + lamC + lamQ B_i on the diagonal, -lamC W off it)
//   full detail, from U* as k_receipt_rows: coh_drop_i, anchor_i = lamG |U*_i - Y_i|^2, query_i = lamQ B_i |U*_i - psi|^2, and
//   the null point of the dense row (K entries, zeros included): R_ij = lamC a_ij |Un_i - Un_j|^2, mu = sum R / K,
//   sigma = sqrt(sum R^2 / K - mu^2) + 1e-12, first argmax (ties to the smaller column), R > 0 and z > z_th.
// The per-row values meet in LDS; each of the four sums is then added up in fp64 in row order by one thread, and the null
// points are written in local row order -- or, when there are more than the cap, the cap highest z in receipt()'s order (z
// descending, then row ascending: a rank count over the at most 1024 rows in LDS).  Nothing but the lattice enters.
__global__ __launch_bounds__(256) void k_cq_receipt(const CqReceiptArgs a) {
  __shared__ float s_psi[kCqMaxCols];
  __shared__ double s_dh[kCqMaxRows];
  __shared__ float s_coh[kCqMaxRows], s_anc[kCqMaxRows], s_qry[kCqMaxRows], s_nz[kCqMaxRows], s_nr[kCqMaxRows];
  __shared__ int32_t s_nj[kCqMaxRows];
  __shared__ int s_cnt[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lat = blockIdx.x, K = a.K;
  const int64_t r0 = (int64_t)lat * K;
  const float* psi = a.psi + (size_t)lat * a.ldn;
  for (int c = tid; c < a.ldn; c += 256) s_psi[c] = psi[c];
  __syncthreads();
  for (int r = wave; r < K; r += 4) {
    const int64_t i = r0 + r;
    const size_t io = (size_t)i * a.ldn;
    const float Bi = a.B ? a.B[i] : 1.0f;
    const float cs = fmaf(a.lamQ, Bi, a.lamG + a.lamC);
    const int d = a.deg[i];
    const int32_t* crow = a.col + i * a.k;
    double dh = 0.0;
    for (int c = lane; c < a.ldn; c += 64) {
      const float ei = a.Up[io + c] - a.Us[io + c];
      float acc = 0.f;
      for (int e = 0; e < d; ++e) {
        const size_t jo = (size_t)crow[e] * a.ldn + c;
        acc = fmaf(a.w[i * a.k + e], a.Up[jo] - a.Us[jo], acc);
      }
      const float me = cs * ei - a.lamC * acc;
      dh += (double)ei * (double)me;
    }
    dh = wave_sum_d2(dh);
    if (lane == 0) s_dh[r] = dh;
    if (!a.full) continue;
    float an = 0.f, qu = 0.f;
    for (int c = lane; c < a.ldn; c += 64) {
      const float us = a.Us[io + c];
      const float dy = us - a.Y[io + c], dq = us - s_psi[c];
      an = fmaf(dy, dy, an);
      qu = fmaf(dq, dq, qu);
    }
    an = wave_sum_f(an);
    qu = wave_sum_f(qu);
    const float inv_i = 1.0f / (a.sd[i] + 1e-12f);
    float coh = 0.f, rmax = 0.f;
    double s1 = 0.0, s2 = 0.0;
    int jmax = -1;
    for (int e = 0; e < d; ++e) {
      const int j = crow[e];
      const float wij = a.adj[i * a.k + e];
      const float inv_j = 1.0f / (a.sd[j] + 1e-12f);
      const size_t jo = (size_t)j * a.ldn;
      float dy = 0.f, du = 0.f;
      for (int c = lane; c < a.ldn; c += 64) {
        const float y = cq_sdiff(a.Y[io + c], inv_i, a.Y[jo + c], inv_j);
        const float u = cq_sdiff(a.Us[io + c], inv_i, a.Us[jo + c], inv_j);
        dy = fmaf(y, y, dy);
        du = fmaf(u, u, du);
      }
      dy = wave_sum_f(dy);
      du = wave_sum_f(du);
      if (wij > 0.f) {
        coh += 0.5f * a.lamC * wij * (dy - du);
        const float R = a.lamC * wij * du;
        s1 += (double)R;
        s2 += (double)R * (double)R;
        if (R > rmax || (R == rmax && R > 0.f && jmax >= 0 && j < jmax)) {
          rmax = R;
          jmax = j;
        }
      }
    }
    if (lane == 0) {
      const double mu = s1 / (double)K;
      double var = s2 / (double)K - mu * mu;
      if (var < 0.0) var = 0.0;
      const double z = ((double)rmax - mu) / (sqrt(var) + 1e-12);
      const bool is_null = (jmax >= 0) && (rmax > 0.f) && (z > (double)a.z_th);
      s_coh[r] = coh;
      s_anc[r] = a.lamG * an;
      s_qry[r] = a.lamQ * Bi * qu;
      s_nj[r] = is_null ? (int32_t)(jmax - r0) : -1;
      s_nz[r] = (float)z;
      s_nr[r] = rmax;
    }
  }
  __syncthreads();
  if (lane == 0) {  // one thread per sum, rows in order
    double t = 0.0;
    if (wave == 0) {
      for (int r = 0; r < K; ++r) t += s_dh[r];
    } else if (a.full) {
      const float* v = wave == 1 ? s_coh : (wave == 2 ? s_anc : s_qry);
      for (int r = 0; r < K; ++r) t += (double)v[r];
    }
    a.sums[(size_t)lat * 4 + wave] = t;
  }
  if (!a.full) {
    if (tid == 0) a.n_total[lat] = a.n_kept[lat] = 0;
    return;
  }
  int mine = 0;
  for (int r = tid; r < K; r += 256) mine += s_nj[r] >= 0 ? 1 : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
  if (lane == 0) s_cnt[wave] = mine;
  __syncthreads();
  const int total = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
  __syncthreads();
  const bool capped = a.cap > 0 && total > a.cap;
  const size_t base = (size_t)lat * a.slots;
  auto emit = [&](int slot, int r) {
    if (slot >= a.slots) return;  // (cannot happen: slots = K, or min(cap, K) under a cap)
    a.n_i[base + slot] = r;
    a.n_j[base + slot] = s_nj[r];
    a.n_z[base + slot] = s_nz[r];
    a.n_r[base + slot] = s_nr[r];
  };
  if (!capped) {
    int run = 0;
    for (int c0 = 0; c0 < K; c0 += 256) {  // (uniform trip count: barriers inside)
      const int r = c0 + tid;
      const bool flag = r < K && s_nj[r] >= 0;
      const unsigned long long m = __ballot(flag);
      if (lane == 0) s_cnt[wave] = __popcll(m);
      __syncthreads();
      int pre = __popcll(m & ((1ull << lane) - 1ull));
      for (int u = 0; u < wave; ++u) pre += s_cnt[u];
      const int tot = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
      __syncthreads();
      if (flag) emit(run + pre, r);
      run += tot;
    }
  } else {
    for (int r = tid; r < K; r += 256) {
      if (s_nj[r] < 0) continue;
      const float z = s_nz[r];
      int rank = 0;
      for (int m = 0; m < K; ++m) {
        const float zm = s_nz[m];
        rank += (s_nj[m] >= 0 && (zm > z || (zm == z && m < r))) ? 1 : 0;
      }
      if (rank < a.cap) emit(rank, r);
    }
  }
  if (tid == 0) {
    a.n_total[lat] = total;
    a.n_kept[lat] = capped ? a.cap : total;
  }
}

}  // namespace

void launch_cq_settle(const CqSettleArgs& a, int32_t nq, hipStream_t s) {
  const int nc = (a.ldn + 255) / 256;
  const dim3 g((unsigned)nq), b(256);
  if (nc <= 1) hipLaunchKernelGGL((k_cq_settle<1>), g, b, 0, s, a);
  else if (nc == 2) hipLaunchKernelGGL((k_cq_settle<2>), g, b, 0, s, a);
  else if (nc == 3) hipLaunchKernelGGL((k_cq_settle<3>), g, b, 0, s, a);
  else if (nc == 4) hipLaunchKernelGGL((k_cq_settle<4>), g, b, 0, s, a);
  else hipLaunchKernelGGL((k_cq_settle<6>), g, b, 0, s, a);
  HIP_CHECK(hipGetLastError());
}

void launch_cq_receipt(const CqReceiptArgs& a, int32_t nq, hipStream_t s) {
  hipLaunchKernelGGL(k_cq_receipt, dim3((unsigned)nq), dim3(256), 0, s, a);
  HIP_CHECK(hipGetLastError());
}

}  // namespace osc

// Settle and receipt of every candidate lattice of a corpus refine chunk, behind the U* solve and
// the bundle of osc_corpus.hip: k_cq_settle (one implicit-Euler step from U = Y) and k_cq_receipt (deltaH, the component
// sums, the null points), one workgroup per lattice each.  No workgroup waits on another.
// k_cq_settle_chain and k_cq_receipt<true> are the same two for a call with chains: lamP L_path in
// the operator.  A call without chains launches k_cq_settle and k_cq_receipt<false> only.
#include "common.hpp"
#include "corpus_receipts.hpp"

namespace osc {
namespace {

// the implicit-Euler step as cq_pcg's operator: the rows' constants in LDS, the start read from Y
struct CqSettleOp {
  const float* s_cs;
  const float* s_inv;
  const float* s_qb;
  int64_t r0;
  float cW, rbY;
  static constexpr bool kFromY = true, kPath = false;
  __device__ __forceinline__ float cs(int64_t i) const { return s_cs[i - r0]; }
  __device__ __forceinline__ float inv_diag(int64_t i) const { return s_inv[i - r0]; }
  __device__ __forceinline__ float qb(int64_t i) const { return s_qb[i - r0]; }
  __device__ __forceinline__ float rhs(float y, float qbi, float p) const { return y + rbY * y + qbi * p; }
};

// a b rounded on its own, whatever it is added to later.  The settle's dt lamG enters both the right-hand side and the
// Jacobi diagonal 1 + dt lamG + ...; left to the compiler, that sum is fused with the product or not depending on where the
// product ends up, and fused the diagonal differs in the last bit for steps other than 1.
__device__ __forceinline__ float cq_rounded_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

// settle() of a fresh lattice (U = Y), one workgroup per lattice: Jacobi-PCG of the implicit-Euler step
// (I + dt M) U+ = Y + dt (lamG Y + lamQ B psi^T) from x0 = Y (lattice.py:159-230; settle_op of osc_solve.hip): operator
// constant 1 + dt (lamG + lamC) + dt lamQ B_i, off-diagonal -dt lamC W, Jacobi diagonal 1 + dt lamG + dt lamQ B_i (without
// lamC: lattice.py:185-192), solver.py's epsilons and stop rule.  The iteration is cq_pcg, k_cq_solve's.  The rows'
// constants are formed once in LDS, with B_i = 1.0f where there are no gates, so gates of exactly 1 give the ungated
// bytes.
template <int NC>
__global__ __launch_bounds__(256) void k_cq_settle(const CqPcgArgs a) {
  __shared__ float red[4];
  __shared__ float s_cs[host::kCorpusMaxTopK], s_inv[host::kCorpusMaxTopK], s_qb[host::kCorpusMaxTopK];
  const CqLattice& g = a.lat;
  const int tid = threadIdx.x, lat = blockIdx.x;
  const int64_t r0 = (int64_t)lat * g.K;
  const int n = g.rows(lat);
  const float lamG = g.lamG(lat), lamC = g.lamC(lat), lamQ = g.lamQ(lat), dt = g.settle_dt(lat, a.dt);  // (uniform)
  const float cW = dt * lamC, rbY = cq_rounded_mul(dt, lamG), cQ = dt * lamQ;
  for (int r = tid; r < n; r += 256) {
    const float Bi = g.B ? g.B[r0 + r] : 1.0f;
    s_cs[r] = fmaf(cQ, Bi, 1.0f + dt * (lamG + lamC));
    s_inv[r] = 1.f / (fmaf(cQ, Bi, 1.0f + rbY) + 1e-12f);
    s_qb[r] = cQ * Bi;
  }
  __syncthreads();
  cq_pcg<NC>(a, CqSettleOp{s_cs, s_inv, s_qb, r0, cW, rbY}, red, g.settle_max_iters(lat, a.max_iters),
             g.settle_tol(lat, a.tol));
}

// the same step of a lattice with a chain prior (lattice.py:180-181, 187-191): the operator gains dt lamP L_path while
// lamP > 0 -- its diagonal part in the rows' constants, the rest through cq_pcg's path hook -- and the Jacobi diagonal gains
// dt lamP whenever a chain is present.  Each is added to the chainless expression, so a lattice without a chain, or with one
// at lamP = 0, gets k_cq_settle's bytes.
struct CqChainSettleOp : CqSettleOp {
  static constexpr bool kPath = true;
  CqPathRows path;
};

template <int NC>
__global__ __launch_bounds__(256) void k_cq_settle_chain(const CqChainPcgArgs ca) {
  __shared__ float red[4];
  __shared__ float s_cs[host::kCorpusMaxTopK], s_inv[host::kCorpusMaxTopK], s_qb[host::kCorpusMaxTopK];
  __shared__ int32_t s_slot[host::kCorpusMaxTopK];
  const CqPcgArgs& a = ca.pcg;
  const CqLattice& g = a.lat;
  const int tid = threadIdx.x, lat = blockIdx.x;
  const int64_t r0 = (int64_t)lat * g.K;
  const int n = g.rows(lat);
  const float lamG = g.lamG(lat), lamC = g.lamC(lat), lamQ = g.lamQ(lat), dt = g.settle_dt(lat, a.dt);  // (uniform)
  const float lamP = g.lamP(lat, ca.chain.lamP);
  const bool present = ca.chain.rec(lat)[0] > 0, active = present && lamP > 0.f;
  const float cW = dt * lamC, rbY = cq_rounded_mul(dt, lamG), cQ = dt * lamQ;
  const float cP = active ? cq_rounded_mul(dt, lamP) : 0.f;
  const float dP = present ? cq_rounded_mul(dt, lamP) : 0.f;
  cq_path_slots(ca.chain, lat, n, active, s_slot);
  for (int r = tid; r < n; r += 256) {
    const float Bi = g.B ? g.B[r0 + r] : 1.0f;
    const float cs = fmaf(cQ, Bi, 1.0f + dt * (lamG + lamC));
    s_cs[r] = active ? cs + cP : cs;
    s_inv[r] = 1.f / (fmaf(cQ, Bi, present ? (1.0f + rbY) + dP : 1.0f + rbY) + 1e-12f);
    s_qb[r] = cQ * Bi;
  }
  __syncthreads();
  cq_pcg<NC>(a, CqChainSettleOp{{s_cs, s_inv, s_qb, r0, cW, rbY}, cq_path_rows(ca.chain, lat, s_slot, cP)}, red,
             g.settle_max_iters(lat, a.max_iters), g.settle_tol(lat, a.tol));
}

__device__ __forceinline__ const CqReceiptArgs& cq_receipt_args(const CqReceiptArgs& a) { return a; }
__device__ __forceinline__ const CqReceiptArgs& cq_receipt_args(const CqChainReceiptArgs& a) { return a.rec; }

// receipt() of one lattice per workgroup (lattice.py receipt(), receipts.py:10-83), a wave per row:
//   deltaH   = sum_i E_i . (M E)_i, E = U+ - U*, M the U* operator (lamG + lamC + lamQ B_i on the diagonal, -lamC W off it)
//   full detail, from U* as k_receipt_rows: coh_drop_i, anchor_i = lamG |U*_i - Y_i|^2, query_i = lamQ B_i |U*_i - psi|^2, and
//   the null point of the dense row (K entries, zeros included): R_ij = lamC a_ij |Un_i - Un_j|^2, mu = sum R / K,
//   sigma = sqrt(sum R^2 / K - mu^2) + 1e-12, first argmax (ties to the smaller column), R > 0 and z > z_th.
// The per-row values meet in LDS; each of the four sums is then added up in fp64 in row order by one thread, and the null
// points are written in local row order -- or, when there are more than the cap, the cap highest z in receipt()'s order (z
// descending, then row ascending: a rank count over the at most 1024 rows in LDS).  Nothing but the lattice enters.
// CHAIN (a call with chains): M gains lamP L_path for a lattice whose chain is active (lamP > 0) -- lamP on the diagonal and
// the row's path entries in the deltaH pass; everything else reads U* alone and stays as it is.
template <bool CHAIN>
__global__ __launch_bounds__(256) void k_cq_receipt(const std::conditional_t<CHAIN, CqChainReceiptArgs, CqReceiptArgs> args) {
  const CqReceiptArgs& a = cq_receipt_args(args);
  __shared__ float s_psi[kCqMaxCols];
  __shared__ double s_dh[kCqMaxRows];
  __shared__ float s_coh[kCqMaxRows], s_anc[kCqMaxRows], s_qry[kCqMaxRows], s_nz[kCqMaxRows], s_nr[kCqMaxRows];
  __shared__ int32_t s_nj[kCqMaxRows];
  __shared__ int s_cnt[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const CqLattice& g = a.lat;
  const int lat = blockIdx.x, K = g.rows(lat);  // (the lattice's own row count; its slot is g.K rows)
  const int64_t r0 = (int64_t)lat * g.K;
  const float* psi = g.psi + (size_t)lat * g.ldn;
  const float lamG = g.lamG(lat), lamC = g.lamC(lat), lamQ = g.lamQ(lat);  // (uniform: the lattice's own, or the launch's)
  for (int c = tid; c < g.ldn; c += 256) s_psi[c] = psi[c];
  [[maybe_unused]] CqPathRows path{};
  [[maybe_unused]] bool active = false;
  if constexpr (CHAIN) {
    __shared__ int32_t s_slot[kCqMaxRows];
    const CqChain& ch = args.chain;
    const float lamP = g.lamP(lat, ch.lamP);
    active = ch.rec(lat)[0] > 0 && lamP > 0.f;
    cq_path_slots(ch, lat, K, active, s_slot);
    path = cq_path_rows(ch, lat, s_slot, active ? lamP : 0.f);
  }
  __syncthreads();
  for (int r = wave; r < K; r += 4) {
    const int64_t i = r0 + r;
    const size_t io = (size_t)i * g.ldn;
    const float Bi = g.B ? g.B[i] : 1.0f;
    float cs = fmaf(lamQ, Bi, lamG + lamC);
    [[maybe_unused]] int ps = -1;
    if constexpr (CHAIN) {
      if (active) cs = cs + path.cP;
      ps = path.s_slot[r];
    }
    const int d = g.deg[i];
    const int32_t* crow = g.col + i * g.k;
    double dh = 0.0;
    for (int c = lane; c < g.ldn; c += 64) {
      const float ei = a.Up[io + c] - a.Us[io + c];
      float acc = 0.f;
      for (int e = 0; e < d; ++e) {
        const size_t jo = (size_t)crow[e] * g.ldn + c;
        acc = fmaf(g.w[i * g.k + e], a.Up[jo] - a.Us[jo], acc);
      }
      float me = cs * ei - lamC * acc;
      if constexpr (CHAIN) {
        if (ps >= 0) {
          float accp = 0.f;
          for (int e = path.ptr[ps]; e < path.ptr[ps + 1]; ++e) {
            const size_t jo = (size_t)(r0 + path.col[e]) * g.ldn + c;
            accp = fmaf(path.w[e], a.Up[jo] - a.Us[jo], accp);
          }
          me = fmaf(-path.cP, accp, me);
        }
      }
      dh += (double)ei * (double)me;
    }
    dh = wave_sum_d(dh);
    if (lane == 0) s_dh[r] = dh;
    if (!a.full) continue;
    float an = 0.f, qu = 0.f;
    for (int c = lane; c < g.ldn; c += 64) {
      const float us = a.Us[io + c];
      const float dy = us - g.Y[io + c], dq = us - s_psi[c];
      an = fmaf(dy, dy, an);
      qu = fmaf(dq, dq, qu);
    }
    an = wave_sum_f(an);
    qu = wave_sum_f(qu);
    const float inv_i = 1.0f / (g.sd[i] + 1e-12f);
    float coh = 0.f, rmax = 0.f;
    double s1 = 0.0, s2 = 0.0;
    int jmax = -1;
    for (int e = 0; e < d; ++e) {
      const int j = crow[e];
      const float wij = g.adj[i * g.k + e];
      const float inv_j = 1.0f / (g.sd[j] + 1e-12f);
      const size_t jo = (size_t)j * g.ldn;
      float dy = 0.f, du = 0.f;
      for (int c = lane; c < g.ldn; c += 64) {
        const float y = cq_sdiff(g.Y[io + c], inv_i, g.Y[jo + c], inv_j);
        const float u = cq_sdiff(a.Us[io + c], inv_i, a.Us[jo + c], inv_j);
        dy = fmaf(y, y, dy);
        du = fmaf(u, u, du);
      }
      dy = wave_sum_f(dy);
      du = wave_sum_f(du);
      if (wij > 0.f) {
        coh += 0.5f * lamC * wij * (dy - du);
        const float R = lamC * wij * du;
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
      s_anc[r] = lamG * an;
      s_qry[r] = lamQ * Bi * qu;
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

void launch_cq_settle(const CqPcgArgs& a, int32_t nq, hipStream_t s) {
  cq_with_nc(a.lat.ldn, [&](auto nc) {
    hipLaunchKernelGGL((k_cq_settle<decltype(nc)::value>), dim3((unsigned)nq), dim3(256), 0, s, a);
  });
  HIP_CHECK(hipGetLastError());
}

void launch_cq_receipt(const CqReceiptArgs& a, int32_t nq, hipStream_t s) {
  hipLaunchKernelGGL(k_cq_receipt<false>, dim3((unsigned)nq), dim3(256), 0, s, a);
  HIP_CHECK(hipGetLastError());
}

void launch_cq_settle_chain(const CqChainPcgArgs& a, int32_t nq, hipStream_t s) {
  cq_with_nc(a.pcg.lat.ldn, [&](auto nc) {
    hipLaunchKernelGGL((k_cq_settle_chain<decltype(nc)::value>), dim3((unsigned)nq), dim3(256), 0, s, a);
  });
  HIP_CHECK(hipGetLastError());
}

void launch_cq_receipt_chain(const CqChainReceiptArgs& a, int32_t nq, hipStream_t s) {
  hipLaunchKernelGGL(k_cq_receipt<true>, dim3((unsigned)nq), dim3(256), 0, s, a);
  HIP_CHECK(hipGetLastError());
}

}  // namespace osc

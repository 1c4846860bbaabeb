// What the per-lattice kernels of a corpus refine chunk share: the lattice block every argument
// struct embeds, the wave reductions, the NaN-keeping max, and cq_pcg -- the one column-owned Jacobi-PCG that k_cq_solve
// (U*, osc_corpus.hip) and k_cq_settle (the implicit-Euler step, corpus_receipt_kernels.hip) both run.  The stop rule and
// the reduction order live here and nowhere else, which is what keeps "gates of exactly 1 give the ungated bytes" and
// "settle reduces like the solve" true by construction.  Device code: include from .hip translation units only.
#pragma once
#include <cstdint>
#include <type_traits>

#include <hip/hip_runtime.h>

#include "corpus_plan.hpp"
#include "corpus_settings.hpp"

namespace osc {

constexpr int kCqMaxRows = host::kCorpusMaxTopK;  // rows of a candidate lattice
constexpr int kCqMaxCols = 1536;                  // columns (Corpus: D <= 1536)

// the lattices of one chunk, back to back: lattice q is union rows [q K, q K + K) and query row q.  In a ragged chunk
//  lattice q has nrows[q] <= K rows at the front of its K-row slot: row bases, strides and LDS
// sizes stay functions of K, every row loop and every row count runs to rows(q).  In a chunk armed by osc_corpus_settings
//  lattice q has its own record st[q], and every reader of a setting takes it through the accessors
// below: a workgroup serves one lattice, so each is one uniform load, and the value enters the expression the launch's
// scalar enters otherwise
struct CqLattice {
  const float* Y;       // union rows x ldn
  const float* psi;     // nq x ldn
  const float* qnorm;   // nq: |psi_q| + 1e-12
  const int32_t* col;   // union ELL (width k, union row ids)
  const float* w;       // normalised weights (the operators')
  const float* adj;     // capped adjacency (the bundle's and the receipt's)
  const int32_t* deg;
  const float* sd;      // sqrt of the capped degree
  const float* B;       // union rows: the gates, or nullptr (B = 1)
  int32_t K, k, ldn;
  float lamG_, lamC_, lamQ_;  // the launch's values: a call that is not armed
  const int32_t* nrows; // nq: rows of each lattice, or nullptr (every lattice has K)
  const host::CorpusSetting* st = nullptr;  // nq: the lattices' own settings, or nullptr (the call is not armed)
  __device__ __forceinline__ int32_t rows(int lat) const { return nrows ? nrows[lat] : K; }
  __device__ __forceinline__ float lamG(int lat) const { return st ? st[lat].lamG : lamG_; }
  __device__ __forceinline__ float lamC(int lat) const { return st ? st[lat].lamC : lamC_; }
  __device__ __forceinline__ float lamQ(int lat) const { return st ? st[lat].lamQ : lamQ_; }
  // the settings that live in other argument blocks: `given` is that block's scalar
  __device__ __forceinline__ float lamP(int lat, float given) const { return st ? st[lat].lamP : given; }
  __device__ __forceinline__ float alpha(int lat, float given) const { return st ? st[lat].alpha : given; }
  __device__ __forceinline__ int32_t picks(int lat, int32_t given) const { return st ? st[lat].k : given; }
  __device__ __forceinline__ float settle_dt(int lat, float given) const { return st ? st[lat].settle_dt : given; }
  __device__ __forceinline__ float settle_tol(int lat, float given) const { return st ? st[lat].settle_tol : given; }
  __device__ __forceinline__ int32_t settle_max_iters(int lat, int32_t given) const {
    return st ? st[lat].settle_max_iters : given;
  }
};

// k_cq_solve and k_cq_settle
struct CqPcgArgs {
  CqLattice lat;
  float* X;           // the solve: x0 = Y on entry, U* on return; the settle: out, the settled state U+
  float* R;
  float* P;
  float* AP;
  int32_t* iters;     // nq
  float* res;         // nq
  int32_t max_iters;  // the three below: the launch's values; an armed settle takes the lattice's own (CqLattice)
  float tol;
  float dt;           // the settle's step (the solve ignores it)
};

// the chain priors of one chunk: per lattice the int and float records host::pack_chain fills
// (corpus_chain.hpp).  n_edges = 0: the lattice has no chain
struct CqChain {
  const int32_t* ints;  // nq x int_words: [n_edges, n_rows, nodes[cap + 1], rows[R], ptr[R + 1], col[2 cap]], local ids
  const float* flts;    // nq x 4 cap: [a[2 cap], w[2 cap]]
  int32_t int_words, cap, rows_at, ptr_at, col_at;
  float lamP;
  __device__ __forceinline__ const int32_t* rec(int lat) const { return ints + (size_t)lat * int_words; }
  __device__ __forceinline__ const float* a(int lat) const { return flts + (size_t)lat * 4 * cap; }
  __device__ __forceinline__ const float* w(int lat) const { return flts + (size_t)lat * 4 * cap + 2 * cap; }
};

// what cq_pcg's path hook reads: (L_path v)_i = v_i - sum_p w_p v_col(p) over row i's path entries; the v_i part is in the
// policy's cs(i), this is the sum.  s_slot (LDS): local row -> its path row, or -1 (every row when the hook is inactive)
struct CqPathRows {
  const int32_t* s_slot;
  const int32_t* ptr;
  const int32_t* col;  // local ids
  const float* w;
  float cP;            // lamP for the solve, dt lamP for the settle
};

// fills s_slot for one lattice of n rows (the caller's barrier publishes it); active = the lattice has a chain and lamP > 0
__device__ __forceinline__ void cq_path_slots(const CqChain& c, int lat, int n, bool active, int32_t* s_slot) {
  const int32_t* rec = c.rec(lat);
  for (int r = threadIdx.x; r < n; r += 256) s_slot[r] = -1;
  __syncthreads();
  if (active)
    for (int t = threadIdx.x; t < rec[1]; t += 256) s_slot[rec[c.rows_at + t]] = t;
}
__device__ __forceinline__ CqPathRows cq_path_rows(const CqChain& c, int lat, const int32_t* s_slot, float cP) {
  const int32_t* rec = c.rec(lat);
  return CqPathRows{s_slot, rec + c.ptr_at, rec + c.col_at, c.w(lat), cP};
}

// a sa - b sb with both products rounded on their own (receipt_kernels.hip's sdiff), so that edge (i, j) and edge (j, i)
// get bit-identical energies
__device__ __forceinline__ float cq_sdiff(float a, float sa, float b, float sb) {
#pragma clang fp contract(off)
  const float p = a * sa;
  const float q = b * sb;
  return p - q;
}

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

// np.max / np.min: a NaN on either side stays
__device__ __forceinline__ float nan_max(float a, float b) {
  return (b != b || a != a) ? __uint_as_float(0x7FC00000u) : fmaxf(a, b);
}
__device__ __forceinline__ float nan_min(float a, float b) {
  return (b != b || a != a) ? __uint_as_float(0x7FC00000u) : fminf(a, b);
}

// calls f(std::integral_constant<int, NC>) for the columns-per-thread count that covers ldn columns with 256 threads
template <class F>
void cq_with_nc(int32_t ldn, F&& f) {
  const int nc = (ldn + 255) / 256;
  if (nc <= 1) f(std::integral_constant<int, 1>{});
  else if (nc == 2) f(std::integral_constant<int, 2>{});
  else if (nc == 3) f(std::integral_constant<int, 3>{});
  else if (nc == 4) f(std::integral_constant<int, 4>{});
  else f(std::integral_constant<int, 6>{});
}

// Jacobi-PCG of one lattice per workgroup of 256 threads, every column a right-hand side of its own: thread t owns the
// columns t + 256 m and runs their recurrences over the lattice's rows in row order (fp64 column sums), so only the stop
// test max_c |r_c| <= tol crosses threads (a NaN-keeping max: solver.py:29 reports NaN for a diverged column).  Same
// iteration structure as k_settle_small: stop test after the x / r update, before beta.  The operator is
// (A v)_i = cs(i) v_i - cW sum_e w_ie v_col(ie) with the Jacobi diagonal 1 / inv_diag(i); Op supplies, for union row i,
//   cs(i), inv_diag(i), qb(i)   the row's operator constant, inverse Jacobi diagonal and query coefficient
//   cW                          the off-diagonal coefficient
//   kFromY                      false: x0 is in a.X already; true: x0 = Y, read from there and stored to a.X by INIT
//   rhs(y, qb_i, psi_c)         the right-hand side from the anchor entry, written out by the policy so that its operands
//                               and association are its own
//   kPath                       true: the policy has a CqPathRows `path`, and rows with path entries get
//                               - path.cP sum_p w_p v_col(p) on top (a chain prior; its diagonal part is in cs(i)).  A
//                               compile-time switch: the kPath = false instantiations hold no trace of it
// red: four floats of LDS.  max_iters, tol: the lattice's stop rule (a.max_iters / a.tol, or its own under per-query
// settings).  Writes a.X, a.R, a.P, a.AP and, from thread 0, a.iters / a.res of the lattice.
template <int NC, class Op>
__device__ __forceinline__ void cq_pcg(const CqPcgArgs& a, const Op& op, float* red, const int max_iters, const float tol) {
  const CqLattice& g = a.lat;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lat = blockIdx.x;
  const int64_t r0 = (int64_t)lat * g.K, r1 = r0 + g.rows(lat);
  const float* psi = g.psi + (size_t)lat * g.ldn;
  int cidx[NC];
  bool on[NC];
#pragma unroll
  for (int m = 0; m < NC; ++m) {
    cidx[m] = tid + 256 * m;
    on[m] = cidx[m] < g.ldn;
    if (!on[m]) cidx[m] = 0;
  }
  auto apply = [&](const float* v, int64_t i, float (&out)[NC]) {
    float acc[NC];
#pragma unroll
    for (int m = 0; m < NC; ++m) acc[m] = 0.f;
    const int d = g.deg[i];
    for (int e = 0; e < d; ++e) {
      const int64_t j = g.col[i * g.k + e];
      const float wij = g.w[i * g.k + e];
#pragma unroll
      for (int m = 0; m < NC; ++m) acc[m] = fmaf(wij, v[j * g.ldn + cidx[m]], acc[m]);
    }
    const float csi = op.cs(i);
#pragma unroll
    for (int m = 0; m < NC; ++m) out[m] = csi * v[i * g.ldn + cidx[m]] - op.cW * acc[m];
    if constexpr (Op::kPath) {
      const int ps = op.path.s_slot[i - r0];
      if (ps >= 0) {
        float accp[NC];
#pragma unroll
        for (int m = 0; m < NC; ++m) accp[m] = 0.f;
        for (int e = op.path.ptr[ps]; e < op.path.ptr[ps + 1]; ++e) {
          const int64_t j = r0 + op.path.col[e];
          const float wp = op.path.w[e];
#pragma unroll
          for (int m = 0; m < NC; ++m) accp[m] = fmaf(wp, v[j * g.ldn + cidx[m]], accp[m]);
        }
#pragma unroll
        for (int m = 0; m < NC; ++m) out[m] = fmaf(-op.path.cP, accp[m], out[m]);
      }
    }
  };
  double rz[NC], t1[NC], t2[NC];
#pragma unroll
  for (int m = 0; m < NC; ++m) rz[m] = 0.0;
  for (int64_t i = r0; i < r1; ++i) {  // r = b - A x0, p = z = r / diag
    float o[NC];
    apply(Op::kFromY ? g.Y : a.X, i, o);
    const float qbi = op.qb(i), invMdi = op.inv_diag(i);
#pragma unroll
    for (int m = 0; m < NC; ++m) {
      if (!on[m]) continue;
      const size_t off = (size_t)i * g.ldn + cidx[m];
      const float y = g.Y[off];
      const float rr = op.rhs(y, qbi, psi[cidx[m]]) - o[m];
      const float z = rr * invMdi;
      if constexpr (Op::kFromY) a.X[off] = y;
      a.R[off] = rr;
      a.P[off] = z;
      rz[m] += (double)rr * (double)z;
    }
  }
  int it = 1;
  float resv = 0.f;
  for (; it <= max_iters; ++it) {
#pragma unroll
    for (int m = 0; m < NC; ++m) t1[m] = 0.0;
    for (int64_t i = r0; i < r1; ++i) {
      float o[NC];
      apply(a.P, i, o);
#pragma unroll
      for (int m = 0; m < NC; ++m) {
        if (!on[m]) continue;
        const size_t off = (size_t)i * g.ldn + cidx[m];
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
      const float invMdi = op.inv_diag(i);
#pragma unroll
      for (int m = 0; m < NC; ++m) {
        if (!on[m]) continue;
        const size_t off = (size_t)i * g.ldn + cidx[m];
        a.X[off] = fmaf(a.P[off], alpha[m], a.X[off]);
        const float rr = fmaf(-a.AP[off], alpha[m], a.R[off]);
        a.R[off] = rr;
        t1[m] += (double)rr * (double)rr;
        t2[m] += (double)rr * (double)(rr * invMdi);
      }
    }
    float mx = 0.f;
#pragma unroll
    for (int m = 0; m < NC; ++m) mx = nan_max(mx, on[m] ? (float)sqrt(t1[m]) : 0.f);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = nan_max(mx, __shfl_xor(mx, o, 64));
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    resv = red[0];
#pragma unroll
    for (int u = 1; u < 4; ++u) resv = nan_max(resv, red[u]);
    __syncthreads();
    if (resv <= tol) break;  // solver.py:30-31, before the beta / p update
    if (it == max_iters) break;
    for (int64_t i = r0; i < r1; ++i) {
      const float invMdi = op.inv_diag(i);
#pragma unroll
      for (int m = 0; m < NC; ++m) {
        if (!on[m]) continue;
        const size_t off = (size_t)i * g.ldn + cidx[m];
        const float beta = (float)(t2[m] / (rz[m] + 1e-18));  // solver.py:33-34
        a.P[off] = fmaf(a.P[off], beta, a.R[off] * invMdi);
      }
    }
#pragma unroll
    for (int m = 0; m < NC; ++m) rz[m] = t2[m];
  }
  if (tid == 0) {
    a.iters[lat] = it > max_iters ? max_iters : it;
    a.res[lat] = resv;
  }
}

}  // namespace osc

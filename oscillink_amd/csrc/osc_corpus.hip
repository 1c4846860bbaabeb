// Corpus refine: for each query the top-K cosine candidates of a resident corpus, a K-row lattice
// over them, its U* and its bundle -- the reference's retrieval loop (scripts/bench_beir.py:84-94) for a whole batch at
// once.  A chunk of queries runs as:
//
//   k_cq_prep    : |psi_q| + 1e-12                                             one wave per query
//   k_cq_gemm    : dots = Yn psi^T / (|psi| + 1e-12), fp32 MFMA, one fixed K order (k_query_gemm's tile)
//   k_cq_select  : per query the K largest (ties to the smaller corpus id), sorted: radix select + bitonic sort
//   k_cq_gather  : the candidates' rows of Y and Yn, back to back (lattice q = union rows [q K, q K + K))
//   k_knn_dense / k_knn_select (batched over the lattices), k_mutual_ell, cap and normalise over the block-diagonal union
//   k_cq_gates   : (gated form only) screened-diffusion gates B of every lattice: s = beta max(0, Yn psi / |psi|), one
//                  single-right-hand-side Jacobi-PCG of (L_sym + gamma I) h = s per workgroup, min-max to [0, 1]
//   k_cq_solve   : Jacobi-PCG for U*, one workgroup per lattice, a thread per column (the columns are independent
//                  recurrences; only the stop test max_c |r_c| <= tol couples them, inside the workgroup); its GATED
//                  instance reads B per row, the other one has B = 1 folded in.  The iteration is cq_pcg (corpus_pcg.hpp)
//   k_cq_bundle  : coherence drop, alignment, fp64 z-score and MMR over S, one workgroup per lattice
//   (corpus_receipt_kernels.hip)
//   k_cq_settle  : (receipts only) settle() of the fresh lattice: one implicit-Euler step from U = Y by the same cq_pcg, one
//                  workgroup per lattice; its state takes the gathered Yn block, which nothing reads after the bundle
//   k_cq_receipt : (receipts only) deltaH of the settled state against U*, and in full detail the three component sums and
//                  the null points (cap applied in the workgroup), one workgroup per lattice
//   (calls with chains only, DESIGN.md section 13.4: corpus_chain_kernels.hip)
//   k_cq_solve_chain / k_cq_settle_chain / k_cq_receipt_chain : the three above with lamP L_path in the operator
//   k_cq_chain_receipt : chain_receipt() of every lattice's own chain from U*, behind the bundle
//
//   (a call armed by osc_corpus_ragged) lattice q has nrows[q] <= K rows at the front of its K-row
//   slot: the ragged instances of the masked select, the gather and the dense kNN write -1 / 0 behind them, and every
//   per-lattice kernel runs its row loops to CqLattice::rows(q).  When every lattice has K rows the chunk is the one above.
//
//   (a call armed by osc_corpus_settings) lattice q has its own lambdas, list length, picks, alpha and
//   settle settings: the chunk's records are uploaded once, CqLattice points at them, and every per-lattice kernel reads its
//   lattice's values through CqLattice's accessors; the lists and the outputs are as wide as the chunk's maxima.
//
// No workgroup waits on another: every kernel's workgroups are independent.  Every per-lattice kernel's arguments begin with
// the same CqLattice block (corpus_pcg.hpp), which run_chunk fills once.
#include "osc_internal.hpp"
#include "knn.hpp"
#include "corpus_plan.hpp"
#include "corpus_ragged.hpp"
#include "corpus_select.hpp"
#include "corpus_settings.hpp"
#include "corpus_store.hpp"
#include "corpus_receipts.hpp"
#include "corpus_chain.hpp"

#include <cmath>
#include <cstddef>
#include <vector>

// a filter armed by osc_corpus_filter for the next query call: rows = 0 none, 1 shared, else one row of words per query
struct CorpusFilter {
  std::vector<uint32_t> words;
  int32_t rows = 0;
  int64_t words_per_row = 0;
};

// armed by osc_corpus_ragged for the next query call: that call's lattices may have fewer than K
// rows.  rows empty = the counts come from the filter, or from the -1 padding of cand_in
struct CorpusRagged {
  bool armed = false;
  std::vector<int32_t> rows;
};

static_assert(sizeof(osc_corpus_setting) == sizeof(osc::host::CorpusSetting) &&
                  offsetof(osc_corpus_setting, kneighbors) == offsetof(osc::host::CorpusSetting, kneighbors) &&
                  offsetof(osc_corpus_setting, settle_max_iters) == offsetof(osc::host::CorpusSetting, settle_max_iters),
              "the public record is corpus_settings.hpp's");

struct osc_corpus {
  int device = 0;
  hipStream_t stream = nullptr;
  int64_t N = 0;        // rows, tombstones included: ids are [0, N)
  int64_t cap = 0;      // rows allocated in Y / Yn
  int64_t n_live = 0;
  int32_t D = 0, ldn = 0;
  int32_t chunk_req = osc::host::kCorpusDefaultChunk;  // OSC_CORPUS_CHUNK, read at creation
  osc::DevBuf<float> Y, Yn;
  std::vector<uint32_t> live;      // corpus_store.hpp's bitmap, store_words(N) words
  osc::DevBuf<uint32_t> d_live;    // its device copy, brought up to date by the first masked select after a change
  bool d_live_current = false;
  CorpusFilter filter;
  osc::DevBuf<uint32_t> d_filter;  // one chunk's rows of the call's filter
  CorpusRagged ragged;
  std::vector<int32_t> last_rows;  // the row counts of the last call that was armed ragged (osc_corpus_ragged_rows)
  osc::DevBuf<int32_t> d_rows;     // one chunk's row counts of a ragged call
  std::vector<osc::host::CorpusSetting> settings;  // armed by osc_corpus_settings for the next query call (section 13.8)
  osc::DevBuf<osc::host::CorpusSetting> d_settings;  // one chunk's records of such a call
  osc::DevBuf<int32_t> d_klist;    // and its lattices' list lengths
  osc::DevBuf<unsigned char> scratch;
  std::string err;
  ~osc_corpus() {
    Y.release();
    Yn.release();
    d_live.release();
    d_filter.release();
    d_rows.release();
    d_settings.release();
    d_klist.release();
    scratch.release();
    if (stream) release_stream(device, stream);
  }
};

namespace osc {
namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;
constexpr int kTM = 128, kTQ = 128, kTK = 32, kTS = kTK + 4;
constexpr int kGemmFold = 128;  // columns the MFMA accumulator runs over before it is folded into the total
static_assert(kGemmFold % kTK == 0, "a fold ends on a tile boundary");

// qnorm[q] = |psi_q| + 1e-12 (psi: nq rows of ldn, pad columns zero)
__global__ __launch_bounds__(256) void k_cq_prep(const float* psi, int32_t ldn, int32_t nq, float* qnorm) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= nq) return;
  const float* p = psi + (size_t)q * ldn;
  float ss = 0.f;
  for (int c = lane; c < ldn; c += 64) ss = fmaf(p[c], p[c], ss);
  ss = wave_sum_f(ss);
  if (lane == 0) qnorm[q] = sqrtf(ss) + 1e-12f;
}

// dots[q][i] = <Yn_i, psi_q> / qnorm[q]: 128 x 128 outputs per workgroup.  Every output sums k = 0 .. ldn - 1 in one fixed
// order: runs of kGemmFold columns in the MFMA accumulator, the runs added up in order.  One accumulator over all of ldn
// rounds at the size of the partial sum at every step; for rows close to the query (every product positive) that error
// grows like sqrt(ldn) and passed 1e-6 at ldn >= 1312 (1.5e-6 measured at D = 1290).  Folded, the partial sums that meet
// are ldn / kGemmFold totals and the short runs behind them.
__global__ __launch_bounds__(256) void k_cq_gemm(const float* __restrict__ Yn, int64_t N, int32_t ldn,
                                                 const float* __restrict__ psi, int32_t nq, const float* qnorm,
                                                 float* __restrict__ dots) {
  __shared__ __attribute__((aligned(16))) float As[kTM * kTS];
  __shared__ __attribute__((aligned(16))) float Bs[kTQ * kTS];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int wr = w & 1, wc = w >> 1;
  const int64_t row0 = (int64_t)blockIdx.x * kTM;
  const int q0 = blockIdx.y * kTQ;
  f32x16 acc[2][2], tot[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = tot[i][j][r] = 0.f;
  const int kq = (t & 7) * 4;
  for (int k0 = 0; k0 < ldn; k0 += kTK) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int r = (t >> 3) + 32 * it;
      const int64_t gr = row0 + r;
      const int k = k0 + kq;
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
      if (gr < N) a = *reinterpret_cast<const float4*>(Yn + gr * ldn + k);
      if (q0 + r < nq) b = *reinterpret_cast<const float4*>(psi + (size_t)(q0 + r) * ldn + k);
      *reinterpret_cast<float4*>(&As[r * kTS + kq]) = a;
      *reinterpret_cast<float4*>(&Bs[r * kTS + kq]) = b;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < kTK; kk += 2) {
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
    if ((k0 + kTK) % kGemmFold == 0 || k0 + kTK >= ldn) {  // (uniform: the end of a run, or of the row)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            tot[i][j][r] += acc[i][j][r];
            acc[i][j][r] = 0.f;
          }
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int64_t row = row0 + wr * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      if (row >= N) continue;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int q = q0 + wc * 64 + j * 32 + (lane & 31);
        if (q < nq) dots[(size_t)q * N + row] = tot[i][j][r] / qnorm[q];
      }
    }
}

// ---- per-query top K: 1024 threads, radix select of the K-th key, then a bitonic sort (k_rm_null_select's pattern) -----
__global__ __launch_bounds__(kSelT) void k_cq_select(const float* dots, int64_t N, int32_t K, int32_t* cand, float* ccos) {
  __shared__ uint32_t hist[256];
  __shared__ uint32_t skey[kSelT];
  __shared__ int32_t sid[kSelT];
  __shared__ int wsum[kSelT / 64];
  __shared__ uint32_t st_prefix, st_mask, st_k;
  __shared__ int st_n;
  const int q = blockIdx.x, tid = threadIdx.x;
  const float* d = dots + (size_t)q * N;
  uint32_t prefix = 0u, mask = 0u, k = (uint32_t)K;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    if (tid < 256) hist[tid] = 0u;
    __syncthreads();
    for (int64_t i = tid; i < N; i += kSelT) {
      const uint32_t kk = fkey(d[i]);
      if ((kk & mask) == prefix) atomicAdd(&hist[(kk >> shift) & 255u], 1u);
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
  const uint32_t T = prefix;  // the K-th largest key; k = how many keys equal to T are kept (the smallest ids)
  if (tid == 0) st_n = 0;
  sid[tid] = 0x7fffffff;
  skey[tid] = 0u;
  __syncthreads();
  int eqrun = 0;
  for (int64_t i0 = 0; i0 < N; i0 += kSelT) {
    const int64_t i = i0 + tid;
    const uint32_t kk = i < N ? fkey(d[i]) : 0u;
    int tot = 0;
    const int eqpos = eqrun + block_scan(i < N && kk == T, wsum, &tot);
    if (i < N && (kk > T || (kk == T && eqpos < (int)k))) {
      const int slot = atomicAdd(&st_n, 1);
      if (slot < kSelT) {
        skey[slot] = kk;
        sid[slot] = (int32_t)i;
      }
    }
    eqrun += tot;
  }
  __syncthreads();
  for (int size = 2; size <= kSelT; size <<= 1) {  // key descending, then id ascending
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      const int l = tid ^ stride;
      if (l > tid) {
        const uint32_t ki = skey[tid], kl = skey[l];
        const int ai = sid[tid], al = sid[l];
        const bool l_first = kl > ki || (kl == ki && al < ai);
        const bool i_first = ki > kl || (ki == kl && ai < al);
        if ((tid & size) == 0 ? l_first : i_first) {
          skey[tid] = kl;
          skey[l] = ki;
          sid[tid] = al;
          sid[l] = ai;
        }
      }
      __syncthreads();
    }
  }
  if (tid < K) {
    const int32_t i = sid[tid];
    cand[(size_t)q * K + tid] = i;
    ccos[(size_t)q * K + tid] = d[i];
  }
}

// union row g = q K + r <- corpus row cand[q][r]: Y, Yn and the solve's x0 = Y (lattice.py:245-263)
// RAGGED: lattice q has nrows[q] <= K rows; the rows behind them in its slot are written as zeros
// (cand is -1 there), so that nothing downstream can meet scratch left by an earlier chunk
template <bool RAGGED>
__global__ __launch_bounds__(256) void k_cq_gather(const float* Y, const float* Yn, int32_t ldn, const int32_t* cand,
                                                   int64_t rows, float* Yc, float* Ync, float* X, int32_t K,
                                                   const int32_t* nrows) {
  const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= rows) return;
  const int lane = threadIdx.x & 63;
  const size_t dst = (size_t)g * ldn;
  if constexpr (RAGGED) {
    const int64_t q = g / K;
    if (g - q * K >= nrows[q]) {  // (wave-uniform: a wave per row)
      const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int c = lane * 4; c < ldn; c += 256) {
        *reinterpret_cast<float4*>(Yc + dst + c) = z;
        *reinterpret_cast<float4*>(X + dst + c) = z;
        *reinterpret_cast<float4*>(Ync + dst + c) = z;
      }
      return;
    }
  }
  const size_t src = (size_t)cand[g] * ldn;
  for (int c = lane * 4; c < ldn; c += 256) {
    const float4 y = *reinterpret_cast<const float4*>(Y + src + c);
    *reinterpret_cast<float4*>(Yc + dst + c) = y;
    *reinterpret_cast<float4*>(X + dst + c) = y;
    *reinterpret_cast<float4*>(Ync + dst + c) = *reinterpret_cast<const float4*>(Yn + src + c);
  }
}

// the U* operator as cq_pcg's operator, B = 1 folded in: one constant, one inverse diagonal and lamQ for every row
struct CqSolveOp {
  float cs_, inv_, cW, lamG, lamQ;
  static constexpr bool kFromY = false, kPath = false;
  __device__ __forceinline__ float cs(int64_t) const { return cs_; }
  __device__ __forceinline__ float inv_diag(int64_t) const { return inv_; }
  __device__ __forceinline__ float qb(int64_t) const { return lamQ; }
  __device__ __forceinline__ float rhs(float y, float qbi, float p) const { return lamG * y + qbi * p; }
};

// the same with gates: the rows' operator constants and inverse Jacobi diagonals formed once in LDS (every thread walks all
// rows in every pass; a reciprocal per row and pass is on its critical path), lamQ B_i from global memory
struct CqGatedSolveOp {
  const float* s_cs;
  const float* s_inv;
  const float* B;
  int64_t r0;
  float cW, lamG, lamQ;
  static constexpr bool kFromY = false, kPath = false;
  __device__ __forceinline__ float cs(int64_t i) const { return s_cs[i - r0]; }
  __device__ __forceinline__ float inv_diag(int64_t i) const { return s_inv[i - r0]; }
  __device__ __forceinline__ float qb(int64_t i) const { return lamQ * B[i]; }
  __device__ __forceinline__ float rhs(float y, float qbi, float p) const { return lamG * y + qbi * p; }
};

// Jacobi-PCG for M U* = lamG Y + lamQ 1 psi^T from x0 = Y (the U* operator of osc_solve_ustar with B = 1, no chain):
// M v = (lamG + lamC + lamQ) v - lamC W v, Jacobi diagonal lamG + lamQ.  One workgroup per lattice; the iteration is
// cq_pcg (corpus_pcg.hpp), which k_cq_settle runs too.
// GATED: B_i comes from the lattice block (set_query(psi, gates=B), lattice.py:245-263): row i has the operator constant
// lamG + lamC + lamQ B_i, the Jacobi diagonal lamG + lamQ B_i and the right-hand side lamG Y_i + (lamQ B_i) psi, each formed
// so that B_i = 1.0f gives the ungated instance's arithmetic operation for operation.
template <int NC, bool GATED>
__global__ __launch_bounds__(256) void k_cq_solve(const CqPcgArgs a) {
  __shared__ float red[4];
  const CqLattice& g = a.lat;
  const int lat = blockIdx.x;
  const float lamG = g.lamG(lat), lamC = g.lamC(lat), lamQ = g.lamQ(lat);  // (uniform: the lattice's own, or the launch's)
  if constexpr (GATED) {
    __shared__ float s_cs[host::kCorpusMaxTopK], s_inv[host::kCorpusMaxTopK];
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)lat * g.K;
    const int n = g.rows(lat);
    for (int r = tid; r < n; r += 256) {
      const float Bi = g.B[r0 + r];
      s_cs[r] = fmaf(lamQ, Bi, lamG + lamC);
      s_inv[r] = 1.f / (fmaf(lamQ, Bi, lamG) + 1e-12f);
    }
    __syncthreads();
    cq_pcg<NC>(a, CqGatedSolveOp{s_cs, s_inv, g.B, r0, lamC, lamG, lamQ}, red, a.max_iters, a.tol);
  } else {
    const float cs = fmaf(lamQ, 1.0f, lamG + lamC);
    const float invMd = 1.f / (fmaf(lamQ, 1.0f, lamG) + 1e-12f);
    cq_pcg<NC>(a, CqSolveOp{cs, invMd, lamC, lamG, lamQ}, red, a.max_iters, a.tol);
  }
}

struct BundleArgs {
  CqLattice lat;
  const float* U;       // U* (union rows x ldn)
  const float* Sm;      // per lattice K x lds similarity matrix
  int32_t lds, kk;
  double alpha, lambda;
  int32_t* o_local;
  float* o_score;
  float* o_align;
};

constexpr int kBundleRows = host::kCorpusMaxTopK;
constexpr int kBundleCols = 1536;
static_assert(kBundleCols == kCqMaxCols && kBundleRows == kCqMaxRows, "the receipt kernel keeps the same rows and columns in LDS");

// bundle(kk, alpha) of one lattice per workgroup (lattice.py:530-568): align_i = cos(U*_i, psi), coh_i (receipts.py:28-38,
// the receipt kernel's per-edge arithmetic), z-scored with fp64 mean / std, score = alpha z + (1 - alpha) align, then
// greedy MMR (graph.py:114-133, lambda 0.5) over the lattice's similarity matrix under osc_mmr's order (value, then the
// smaller local id)
__global__ __launch_bounds__(256) void k_cq_bundle(const BundleArgs a) {
  __shared__ float qn[kBundleCols];
  __shared__ float s_coh[kBundleRows], s_align[kBundleRows];
  __shared__ double s_base[kBundleRows], s_max[kBundleRows];
  __shared__ double s_red[4];
  __shared__ double s_bv[4];
  __shared__ int s_bi[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const CqLattice& g = a.lat;
  const int lat = blockIdx.x, K = g.rows(lat);  // (the lattice's own row count; its slot is g.K rows)
  const int64_t r0 = (int64_t)lat * g.K;
  const int steps = min(min(g.picks(lat, a.kk), a.kk), K);  // the lattice's own picks (at most the kk-wide output); a
                                                            // lattice of fewer rows is picked empty: the rest is padding
  const float lamC = g.lamC(lat);
  const double alpha = g.st ? (double)g.alpha(lat, 0.f) : a.alpha;
  const float* psi = g.psi + (size_t)lat * g.ldn;
  const float qinv = 1.0f / g.qnorm[lat];
  for (int c = tid; c < g.ldn; c += 256) qn[c] = psi[c] * qinv;
  __syncthreads();
  for (int r = wave; r < K; r += 4) {
    const int64_t i = r0 + r;
    const float* ui = a.U + (size_t)i * g.ldn;
    const float* yi = g.Y + (size_t)i * g.ldn;
    float s = 0.f, n2 = 0.f;
    for (int c = lane; c < g.ldn; c += 64) {
      s = fmaf(ui[c], qn[c], s);
      n2 = fmaf(ui[c], ui[c], n2);
    }
    s = wave_sum_f(s);
    n2 = wave_sum_f(n2);
    const float inv_i = 1.0f / (g.sd[i] + 1e-12f);
    float coh = 0.f;
    const int d = g.deg[i];
    for (int e = 0; e < d; ++e) {
      const int64_t j = g.col[i * g.k + e];
      const float wij = g.adj[i * g.k + e];
      const float inv_j = 1.0f / (g.sd[j] + 1e-12f);
      const float* uj = a.U + (size_t)j * g.ldn;
      const float* yj = g.Y + (size_t)j * g.ldn;
      float dy = 0.f, du = 0.f;
      for (int c = lane; c < g.ldn; c += 64) {
        const float y = yi[c] * inv_i - yj[c] * inv_j;
        const float u = ui[c] * inv_i - uj[c] * inv_j;
        dy = fmaf(y, y, dy);
        du = fmaf(u, u, du);
      }
      dy = wave_sum_f(dy);
      du = wave_sum_f(du);
      if (wij > 0.f) coh += 0.5f * lamC * wij * (dy - du);
    }
    if (lane == 0) {
      s_coh[r] = coh;
      s_align[r] = s / (sqrtf(n2) + 1e-12f);
    }
  }
  __syncthreads();
  // fp64 mean and (population) std of coh, fixed reduction order
  auto block_sum = [&](double v) {
    v = wave_sum_d(v);
    if (lane == 0) s_red[wave] = v;
    __syncthreads();
    const double t = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
    __syncthreads();
    return t;
  };
  double part = 0.0;
  for (int r = tid; r < K; r += 256) part += (double)s_coh[r];
  const double mu = block_sum(part) / (double)K;
  part = 0.0;
  for (int r = tid; r < K; r += 256) {
    const double dv = (double)s_coh[r] - mu;
    part += dv * dv;
  }
  const double sigma = sqrt(block_sum(part) / (double)K) + 1e-12;
  for (int r = tid; r < K; r += 256) {
    const double z = sigma > 0.0 ? ((double)s_coh[r] - mu) / sigma : 0.0;
    const float score = (float)(alpha * z + (1.0 - alpha) * (double)s_align[r]);
    s_coh[r] = score;  // (coh is not needed any more)
    s_base[r] = (1.0 - a.lambda) * (double)score;
    s_max[r] = 0.0;
  }
  __syncthreads();
  const float* S = a.Sm + (size_t)lat * g.K * a.lds;
  for (int t = tid + steps; t < a.kk; t += 256) {  // (ragged or armed chunks only: steps = kk otherwise)
    a.o_local[(size_t)lat * a.kk + t] = -1;
    a.o_score[(size_t)lat * a.kk + t] = 0.f;
    a.o_align[(size_t)lat * a.kk + t] = 0.f;
  }
  for (int t = 0; t < steps; ++t) {
    double bv = -1.0e300;
    int bi = 0x7fffffff;
    for (int r = tid; r < K; r += 256) {
      if (s_base[r] == -INFINITY) continue;  // taken
      const double v = s_base[r] - (t == 0 ? 0.0 : a.lambda * s_max[r]);
      if (bi == 0x7fffffff || v > bv || (v == bv && r < bi)) {
        bv = v;
        bi = r;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (oi != 0x7fffffff && (bi == 0x7fffffff || ov > bv || (ov == bv && oi < bi))) {
        bv = ov;
        bi = oi;
      }
    }
    if (lane == 0) {
      s_bv[wave] = bv;
      s_bi[wave] = bi;
    }
    __syncthreads();
    bv = s_bv[0];
    bi = s_bi[0];
#pragma unroll
    for (int u = 1; u < 4; ++u)
      if (s_bi[u] != 0x7fffffff && (bi == 0x7fffffff || s_bv[u] > bv || (s_bv[u] == bv && s_bi[u] < bi))) {
        bv = s_bv[u];
        bi = s_bi[u];
      }
    __syncthreads();
    if (bi == 0x7fffffff) break;  // (cannot happen for kk <= K)
    if (tid == 0) {
      a.o_local[(size_t)lat * a.kk + t] = bi;
      a.o_score[(size_t)lat * a.kk + t] = s_coh[bi];
      a.o_align[(size_t)lat * a.kk + t] = s_align[bi];
      s_base[bi] = -INFINITY;
    }
    if (t + 1 < steps) {
      const float* srow = S + (size_t)bi * a.lds;
      for (int r = tid; r < K; r += 256) {
        const double sv = (double)srow[r];
        s_max[r] = t == 0 ? sv : fmax(s_max[r], sv);
      }
    }
    __syncthreads();
  }
}

struct GateArgs {
  CqLattice lat;
  const float* Yn;      // union rows x ldn, row-normalised
  float* gates;         // union rows
  int32_t* iters;       // nq
  float* res;           // nq
  int32_t max_iters, direct, clamp;
  float beta, gamma, tol;
};

constexpr int kGateOwn = host::kCorpusMaxTopK / 256;  // rows per thread: row = tid + 256 m

// compute_diffusion_gates (preprocess/diffusion.py:35-124) of one lattice per workgroup, the whole solve in one launch:
// s_i = beta max(0, <Yn_i, psi / (|psi| + 1e-12)>), Jacobi-PCG of (L_sym + gamma I) h = s from x0 = 0 under solver.py's
// stop rule (operator (1 + gamma) v_i - sum_e w_ie v_col(ie), diagonal 1 + gamma), then min-max to [0, 1].  direct != 0
// stands for the reference's dense solve: tol = 1e-7 max(1, |s|) formed here, max_iters from the host (2048).
// Thread t owns rows t + 256 m: their h, r and A p live in its registers, p in LDS (the only vector other threads read).
// Every dot product is fp64: per-thread partials in row order, the wave's butterfly, then the four waves in order -- a
// lattice's gates depend on nothing but the lattice.  Every thread reads the reduced sums from LDS after a barrier, so the
// stop decision is uniform and nobody is left behind a __syncthreads().
__global__ __launch_bounds__(256) void k_cq_gates(const GateArgs a) {
  __shared__ float qn[kBundleCols];
  __shared__ float sp[host::kCorpusMaxTopK];
  __shared__ double s_red[2][4];
  __shared__ float s_mm[2][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const CqLattice& g = a.lat;
  const int lat = blockIdx.x, K = g.rows(lat);  // (the lattice's own row count; its slot is g.K rows)
  const int64_t r0 = (int64_t)lat * g.K;
  const float* psi = g.psi + (size_t)lat * g.ldn;
  const float qinv = 1.0f / g.qnorm[lat];
  for (int c = tid; c < g.ldn; c += 256) qn[c] = psi[c] * qinv;
  __syncthreads();
  for (int r = wave; r < K; r += 4) {  // a wave per row
    const float* yi = a.Yn + (size_t)(r0 + r) * g.ldn;
    float s = 0.f;
    for (int c = lane; c < g.ldn; c += 64) s = fmaf(yi[c], qn[c], s);
    s = wave_sum_f(s);
    if (lane == 0) sp[r] = a.beta * fmaxf(0.f, s);
  }
  __syncthreads();
  auto block_sum2 = [&](double u, double v, double& U, double& V) {
    u = wave_sum_d(u);
    v = wave_sum_d(v);
    if (lane == 0) {
      s_red[0][wave] = u;
      s_red[1][wave] = v;
    }
    __syncthreads();
    U = ((s_red[0][0] + s_red[0][1]) + s_red[0][2]) + s_red[0][3];
    V = ((s_red[1][0] + s_red[1][1]) + s_red[1][2]) + s_red[1][3];
    __syncthreads();
  };
  auto block_sum = [&](double u) {
    u = wave_sum_d(u);
    if (lane == 0) s_red[0][wave] = u;
    __syncthreads();
    const double U = ((s_red[0][0] + s_red[0][1]) + s_red[0][2]) + s_red[0][3];
    __syncthreads();
    return U;
  };
  const float cs = 1.0f + a.gamma;
  const float invMd = 1.f / ((1.0f + a.gamma) + 1e-12f);
  float h[kGateOwn], r[kGateOwn], ap[kGateOwn];
  double t1 = 0.0, t2 = 0.0, ss, rz;
#pragma unroll
  for (int m = 0; m < kGateOwn; ++m) {  // x0 = 0: r = s, p = z = r / diag
    const int row = tid + 256 * m;
    h[m] = r[m] = ap[m] = 0.f;
    if (row < K) {
      const float sv = sp[row];
      const float z = sv * invMd;
      r[m] = sv;
      sp[row] = z;
      t1 += (double)sv * (double)sv;
      t2 += (double)sv * (double)z;
    }
  }
  block_sum2(t1, t2, ss, rz);  // (its barriers also publish p)
  const float tol = a.direct ? 1e-7f * fmaxf(1.0f, (float)sqrt(ss)) : a.tol;
  int it = 1;
  float resv = 0.f;
  for (; it <= a.max_iters; ++it) {
    double pap = 0.0, T1, T2;
#pragma unroll
    for (int m = 0; m < kGateOwn; ++m) {
      const int row = tid + 256 * m;
      if (row < K) {
        const int64_t i = r0 + row;
        const int d = g.deg[i];
        float acc = 0.f;
        for (int e = 0; e < d; ++e) acc = fmaf(g.w[i * g.k + e], sp[g.col[i * g.k + e] - r0], acc);
        const float pv = sp[row];
        ap[m] = cs * pv - acc;
        pap += (double)pv * (double)ap[m];
      }
    }
    const float alpha = (float)(rz / (block_sum(pap) + 1e-18));  // solver.py:25-26
    t1 = t2 = 0.0;
#pragma unroll
    for (int m = 0; m < kGateOwn; ++m) {
      const int row = tid + 256 * m;
      if (row < K) {
        h[m] = fmaf(sp[row], alpha, h[m]);
        const float rr = fmaf(-ap[m], alpha, r[m]);
        r[m] = rr;
        t1 += (double)rr * (double)rr;
        t2 += (double)rr * (double)(rr * invMd);
      }
    }
    block_sum2(t1, t2, T1, T2);
    resv = (float)sqrt(T1);
    if (resv <= tol) break;  // solver.py:30-31, before the beta / p update (uniform: T1 comes from LDS)
    if (it == a.max_iters) break;
    const float beta = (float)(T2 / (rz + 1e-18));  // solver.py:33-34
#pragma unroll
    for (int m = 0; m < kGateOwn; ++m) {
      const int row = tid + 256 * m;
      if (row < K) sp[row] = fmaf(sp[row], beta, r[m] * invMd);
    }
    rz = T2;
    __syncthreads();
  }
  float lo = INFINITY, hi = -INFINITY;
#pragma unroll
  for (int m = 0; m < kGateOwn; ++m)
    if (tid + 256 * m < K) {
      lo = nan_min(lo, h[m]);
      hi = nan_max(hi, h[m]);
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = nan_min(lo, __shfl_xor(lo, o, 64));
    hi = nan_max(hi, __shfl_xor(hi, o, 64));
  }
  if (lane == 0) {
    s_mm[0][wave] = lo;
    s_mm[1][wave] = hi;
  }
  __syncthreads();
  lo = nan_min(nan_min(s_mm[0][0], s_mm[0][1]), nan_min(s_mm[0][2], s_mm[0][3]));
  hi = nan_max(nan_max(s_mm[1][0], s_mm[1][1]), nan_max(s_mm[1][2], s_mm[1][3]));
  const bool flat = (double)hi - (double)lo < 1e-12;  // diffusion.py:119-122; false for a NaN, which then spreads
  const float span = hi - lo;
#pragma unroll
  for (int m = 0; m < kGateOwn; ++m) {
    const int row = tid + 256 * m;
    if (row < K) {
      float g = h[m];
      if (a.clamp) {
        g = flat ? 1.0f : __fdiv_rn(g - lo, span);
        g = g < 0.f ? 0.f : (g > 1.f ? 1.f : g);  // np.clip: a NaN stays
      }
      a.gates[r0 + row] = g;
    }
  }
  for (int row = K + tid; row < a.lat.K; row += 256) a.gates[r0 + row] = 0.f;  // a ragged slot's padding
  if (tid == 0) {
    a.iters[lat] = it > a.max_iters ? a.max_iters : it;
    a.res[lat] = resv;
  }
}

}  // namespace
}  // namespace osc

using namespace osc;

namespace {

thread_local std::string g_corpus_error;

template <class F>
int corpus_guarded(osc_corpus* h, F&& f) {
  if (!h) return OSC_E_INVALID;
  try {
    HIP_CHECK(hipSetDevice(h->device));
    alloc_ctx() = AllocCtx{h->device, h->stream};
    f(*h);
    return OSC_OK;
  } catch (const Invalid& e) {
    h->err = e.what();
    return OSC_E_INVALID;
  } catch (const Unsupported& e) {
    h->err = e.what();
    return OSC_E_UNSUPPORTED;
  } catch (const std::exception& e) {
    h->err = e.what();
    return OSC_E_HIP;
  }
}

// a call that searches or takes candidates: whatever it returns, the filter, the ragged arming and the per-query settings
// made for it are spent
template <class F>
int corpus_query(osc_corpus* h, F&& f) {
  const int rc = corpus_guarded(h, f);
  if (h) h->filter = CorpusFilter{};
  if (h) h->ragged = CorpusRagged{};
  if (h) h->settings.clear();
  return rc;
}

template <class T>
T* at(osc_corpus& c, int64_t off) {
  return reinterpret_cast<T*>(c.scratch.p + off);
}

struct RefineReq {
  const float* psis;
  int32_t Q;
  int32_t top_k, kneighbors;  // as given; set_shape turns them into K and knn
  const int32_t* cand_in;  // Q x K or nullptr (search)
  int32_t K;
  int32_t knn;             // effective list length (0: K == 1, no edges)
  float row_cap, lamG, lamC, lamQ, tol;
  int32_t max_iters, kk;
  float alpha;
  int32_t stage;           // 0 = search only, 1 = up to the graph (and the gates, if asked for), 2 = everything
  int32_t gate = 0;        // 0 = none (B = 1), 1 = diffusion gates computed per lattice, 2 = gates_in
  const float* gates_in = nullptr;  // Q x K
  float g_beta = 1.f, g_gamma = 0.1f, g_tol = 1e-4f;
  int32_t g_direct = 1, g_max_iters = 2048, g_clamp = 1;
  int32_t receipts = 0;    // 0 = none, 1 = light, 2 = full: settle + receipt behind the bundle (stage 2 only)
  float s_dt = 1.f, s_tol = 1e-3f, z_th = 3.f;
  int32_t s_max_iters = 12, null_cap = 0, null_slots = 0;
  // chains (osc_corpus_refine_chains): chain_cap = the largest edge count of the call's chains, 0 = a call without chains
  int32_t chain_cap = 0;
  const int64_t* c_off = nullptr;    // Q + 1 offsets into c_nodes; an empty range = no chain
  const int32_t* c_nodes = nullptr;  // local row ids
  const float* c_w = nullptr;        // per chain edge, at c_eoff, or nullptr (ones)
  const int64_t* c_eoff = nullptr;   // Q + 1 offsets over chain edges
  float lamP = 0.f, c_zth = 2.5f;
  // the call's filter (osc_corpus_filter), set by set_k_and_filter: rows of store_words(N) words, nullptr = none
  const uint32_t* allow = nullptr;
  int64_t allow_stride = 0;  // words from one query's row to the next; 0 = one row for every query
  // a call armed by osc_corpus_ragged (set_k_and_filter / set_ragged): rows_store = the Q row counts, empty when the call was
  // not armed; ragged = some lattice has fewer than K rows, so the chunk runs the ragged kernels
  std::vector<int32_t> rows_store;
  std::vector<float> gates_store;  // gates_in of a ragged call with zeros behind each lattice's rows
  bool ragged = false;
  // a call armed by osc_corpus_settings (set_settings): the Q lattices' effective records (host::setting_effective) and their
  // list lengths, empty when the call was not armed; knn and kk are then the records' maxima
  std::vector<host::CorpusSetting> settings;
  std::vector<int32_t> klist;
  bool armed() const { return !settings.empty(); }
  int32_t rows_of(int32_t q) const { return rows_store.empty() ? K : rows_store[(size_t)q]; }
};

// the device copy of the live bitmap, as of now
const uint32_t* live_on_device(osc_corpus& c) {
  const size_t nw = (size_t)host::store_words(c.N);
  if (c.d_live.n < nw) c.d_live.alloc((size_t)host::store_words(std::max(c.cap, c.N)));
  if (!c.d_live_current) {
    HIP_CHECK(hipMemcpyAsync(c.d_live.p, c.live.data(), nw * 4, hipMemcpyHostToDevice, c.stream));
    c.d_live_current = true;
  }
  return c.d_live.p;
}

// one chunk [q0, q0 + nq): psi upload, candidates, and the requested stages in the order of the list at the top of this
// file; returns the layout used
host::CorpusLayout run_chunk(osc_corpus& c, const RefineReq& rq, int32_t q0, int32_t nq, int32_t cap_nq) {
  const int32_t K = rq.K, ldn = c.ldn, k = std::max(1, rq.knn), kk = std::max(1, rq.kk);
  const host::CorpusLayout L = host::corpus_layout(c.N, ldn, K, k, kk, cap_nq, rq.receipts != 0, rq.null_slots, rq.chain_cap);
  if ((int64_t)c.scratch.n < L.total) c.scratch.alloc((size_t)L.total);
  hipStream_t s = c.stream;
  const dim3 per_lattice((unsigned)nq), wg(256);
  std::vector<float> hp((size_t)nq * ldn, 0.f);
  for (int32_t q = 0; q < nq; ++q)
    std::copy(rq.psis + (size_t)(q0 + q) * c.D, rq.psis + (size_t)(q0 + q + 1) * c.D, hp.begin() + (size_t)q * ldn);
  float* psi = at<float>(c, L.psi);
  float* qnorm = at<float>(c, L.qnorm);
  int32_t* cand = at<int32_t>(c, L.cand);
  const int32_t* nrows = nullptr;  // the chunk's row counts on the device: a ragged chunk only
  if (rq.ragged) {
    if (c.d_rows.n < (size_t)cap_nq) c.d_rows.alloc((size_t)cap_nq);
    HIP_CHECK(hipMemcpyAsync(c.d_rows.p, rq.rows_store.data() + q0, (size_t)nq * 4, hipMemcpyHostToDevice, s));
    nrows = c.d_rows.p;
  }
  // an armed chunk: its lattices' records and list lengths, and -- for the ragged dense build, which gives every lattice its
  // own list length -- the row counts even when every lattice has K rows
  const host::CorpusSetting* st = nullptr;
  const int32_t* klist = nullptr;
  const int32_t* knn_rows = nrows;
  if (rq.armed()) {
    const host::CorpusSetting* hs = host::settings_slice(rq.settings.data(), rq.Q, q0, nq);
    if (!hs) throw Invalid("settings: chunk outside the armed records");
    if (c.d_settings.n < (size_t)cap_nq) c.d_settings.alloc((size_t)cap_nq);
    if (c.d_klist.n < (size_t)cap_nq) c.d_klist.alloc((size_t)cap_nq);
    HIP_CHECK(hipMemcpyAsync(c.d_settings.p, hs, (size_t)nq * sizeof(host::CorpusSetting), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(c.d_klist.p, rq.klist.data() + q0, (size_t)nq * 4, hipMemcpyHostToDevice, s));
    st = c.d_settings.p;
    klist = c.d_klist.p;
    if (!rq.ragged) {
      if (c.d_rows.n < (size_t)cap_nq) c.d_rows.alloc((size_t)cap_nq);
      const std::vector<int32_t> full((size_t)nq, K);
      HIP_CHECK(hipMemcpyAsync(c.d_rows.p, full.data(), (size_t)nq * 4, hipMemcpyHostToDevice, s));
      knn_rows = c.d_rows.p;
    }
  }
  // prep, and the candidates: given, or gemm + select
  HIP_CHECK(hipMemcpyAsync(psi, hp.data(), hp.size() * 4, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_cq_prep, dim3((unsigned)((nq + 3) / 4)), wg, 0, s, psi, ldn, nq, qnorm);
  if (rq.cand_in) {
    HIP_CHECK(hipMemcpyAsync(cand, rq.cand_in + (size_t)q0 * K, (size_t)nq * K * 4, hipMemcpyHostToDevice, s));
  } else {
    float* dots = at<float>(c, L.dots);
    const dim3 grid((unsigned)((c.N + kTM - 1) / kTM), (unsigned)((nq + kTQ - 1) / kTQ));
    hipLaunchKernelGGL(k_cq_gemm, grid, wg, 0, s, c.Yn.p, c.N, ldn, psi, nq, qnorm, dots);
    if (c.n_live == c.N && !rq.allow) {
      hipLaunchKernelGGL(k_cq_select, per_lattice, dim3(kSelT), 0, s, dots, c.N, K, cand, at<float>(c, L.ccos));
    } else {  // tombstones or a filter: the chunk's rows of the filter go into a buffer of their own
      const uint32_t* d_allow = nullptr;
      if (rq.allow) {
        const bool shared = rq.allow_stride == 0;
        const size_t wpr = (size_t)host::store_words(c.N), words = (shared ? 1 : (size_t)nq) * wpr;
        if (c.d_filter.n < words) c.d_filter.alloc((shared ? 1 : (size_t)cap_nq) * wpr);
        HIP_CHECK(hipMemcpyAsync(c.d_filter.p, rq.allow + (size_t)q0 * rq.allow_stride, words * 4, hipMemcpyHostToDevice, s));
        d_allow = c.d_filter.p;
      }
      if (rq.ragged)  // (writes the counts it finds over the uploaded ones: the same numbers, from the device's own popcount)
        launch_cq_select_ragged(dots, c.N, K, live_on_device(c), d_allow, rq.allow_stride, cand, at<float>(c, L.ccos),
                                c.d_rows.p, nq, s);
      else
        launch_cq_select_masked(dots, c.N, K, live_on_device(c), d_allow, rq.allow_stride, cand, at<float>(c, L.ccos), nq, s);
    }
  }
  HIP_CHECK(hipGetLastError());
  if (rq.stage == 0) return L;
  // gather
  const int64_t rows = (int64_t)nq * K;
  float* Yc = at<float>(c, L.Y);
  float* Ync = at<float>(c, L.Yn);
  float* X = at<float>(c, L.X);
  if (rq.ragged)
    hipLaunchKernelGGL(k_cq_gather<true>, dim3((unsigned)((rows + 3) / 4)), wg, 0, s, c.Y.p, c.Yn.p, ldn, cand, rows, Yc, Ync, X,
                       K, nrows);
  else
    hipLaunchKernelGGL(k_cq_gather<false>, dim3((unsigned)((rows + 3) / 4)), wg, 0, s, c.Y.p, c.Yn.p, ldn, cand, rows, Yc, Ync,
                       X, K, nrows);
  HIP_CHECK(hipGetLastError());
  // the graph of every lattice
  const int32_t lds = host::corpus_lds(K);
  int32_t* col = at<int32_t>(c, L.col);
  float* adj = at<float>(c, L.adj);
  float* w = at<float>(c, L.w);
  int32_t* deg = at<int32_t>(c, L.deg);
  float* sd = at<float>(c, L.sd);
  float* Sm = at<float>(c, L.Sm);
  if (rq.knn > 0) {  // the dense route of the lattice build (osc_graph.hip, KnnRoute::dense), every lattice at once
    if (knn_rows)
      launch_knn_dense_ragged(Ync, ldn, K, knn_rows, nq, k, Sm, lds, at<float>(c, L.kval), at<int32_t>(c, L.kidx), s, klist);
    else launch_knn_dense_many(Ync, ldn, K, nq, k, Sm, lds, at<float>(c, L.kval), at<int32_t>(c, L.kidx), s);
    launch_mutual_ell(at<float>(c, L.kval), at<int32_t>(c, L.kidx), (int32_t)rows, k, k, col, adj, deg, s);
  } else {  // one-row lattices have no edges (graph.py:30-32)
    HIP_CHECK(hipMemsetAsync(deg, 0, (size_t)rows * 4, s));
  }
  launch_cap_and_normalize(adj, w, col, deg, k, (int32_t)rows, rq.row_cap, 1, at<float>(c, L.scale), sd, s);
  float* gates = at<float>(c, L.gates);
  const CqLattice lat{Yc, psi, qnorm, col, w, adj, deg, sd, rq.gate ? gates : nullptr, K, k, ldn, rq.lamG, rq.lamC, rq.lamQ,
                      nrows, st};
  // gates: solved per lattice, or given
  if (rq.gate == 1) {
    const GateArgs ga{lat, Ync, gates, at<int32_t>(c, L.g_iters), at<float>(c, L.g_res), rq.g_max_iters, rq.g_direct,
                      rq.g_clamp, rq.g_beta, rq.g_gamma, rq.g_tol};
    hipLaunchKernelGGL(k_cq_gates, per_lattice, wg, 0, s, ga);
    HIP_CHECK(hipGetLastError());
  } else if (rq.gate == 2) {
    HIP_CHECK(hipMemcpyAsync(gates, rq.gates_in + (size_t)q0 * K, (size_t)rows * 4, hipMemcpyHostToDevice, s));
  }
  if (rq.stage == 1) return L;
  // the chunk's chain records (a call with chains only)
  const bool chains = rq.chain_cap > 0;
  CqChain chain{};
  if (chains) {
    const int32_t cap = rq.chain_cap;
    const int64_t iw = host::chain_int_words(K, cap), fw = host::chain_flt_words(cap);
    std::vector<int32_t> hi((size_t)(nq * iw), 0);
    std::vector<float> hf((size_t)(nq * fw), 0.f);
    for (int32_t q = 0; q < nq; ++q) {
      const int64_t b = rq.c_off[q0 + q], len = rq.c_off[q0 + q + 1] - b;
      host::pack_chain(rq.c_nodes + b, rq.c_w ? rq.c_w + rq.c_eoff[q0 + q] : nullptr, (int32_t)len, K, cap,
                       hi.data() + (size_t)(q * iw), hf.data() + (size_t)(q * fw));
    }
    HIP_CHECK(hipMemcpyAsync(at<int32_t>(c, L.c_int), hi.data(), hi.size() * 4, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipMemcpyAsync(at<float>(c, L.c_flt), hf.data(), hf.size() * 4, hipMemcpyHostToDevice, s));
    chain = CqChain{at<int32_t>(c, L.c_int), at<float>(c, L.c_flt), (int32_t)iw, cap, (int32_t)host::chain_rows_at(cap),
                    (int32_t)host::chain_ptr_at(K, cap), (int32_t)host::chain_col_at(K, cap), rq.lamP};
  }
  // solve: U* into X
  const CqPcgArgs sa{lat, X, at<float>(c, L.R), at<float>(c, L.P), at<float>(c, L.AP), at<int32_t>(c, L.iters),
                     at<float>(c, L.res), rq.max_iters, rq.tol, 0.f};
  if (chains) {
    launch_cq_solve_chain(CqChainPcgArgs{sa, chain}, nq, s);
  } else {
    cq_with_nc(ldn, [&](auto nc) {
      constexpr int NC = decltype(nc)::value;
      if (rq.gate) hipLaunchKernelGGL((k_cq_solve<NC, true>), per_lattice, wg, 0, s, sa);
      else hipLaunchKernelGGL((k_cq_solve<NC, false>), per_lattice, wg, 0, s, sa);
    });
    HIP_CHECK(hipGetLastError());
  }
  // bundle
  if (rq.kk > 0) {
    const BundleArgs ba{lat, X, Sm, lds, rq.kk, (double)rq.alpha, 0.5, at<int32_t>(c, L.o_local), at<float>(c, L.o_score),
                        at<float>(c, L.o_align)};
    hipLaunchKernelGGL(k_cq_bundle, per_lattice, wg, 0, s, ba);
    HIP_CHECK(hipGetLastError());
  }
  if (chains)  // chain_receipt(): U* alone, no settle needed
    launch_cq_chain_receipt(CqChainEdgesArgs{lat, chain, X, rq.c_zth, at<float>(c, L.c_edge), at<double>(c, L.c_gain),
                                             at<int32_t>(c, L.c_verdict), at<int32_t>(c, L.c_weak_k),
                                             at<float>(c, L.c_weak_z)}, nq, s);
  if (!rq.receipts) return L;
  // settle: the solve's R, P and AP again; the settled state takes Ync, dead since the graph, the gates and the bundle, and
  // U* stays in X
  CqPcgArgs ta = sa;
  ta.X = Ync;
  ta.iters = at<int32_t>(c, L.s_iters);
  ta.res = at<float>(c, L.s_res);
  ta.max_iters = rq.s_max_iters;
  ta.tol = rq.s_tol;
  ta.dt = rq.s_dt;
  if (chains) launch_cq_settle_chain(CqChainPcgArgs{ta, chain}, nq, s);
  else launch_cq_settle(ta, nq, s);
  // receipt
  const CqReceiptArgs ra{lat, X, Ync, rq.receipts == 2, rq.null_cap, rq.null_slots, rq.z_th, at<double>(c, L.r_sums),
                         at<int32_t>(c, L.n_total), at<int32_t>(c, L.n_kept), at<int32_t>(c, L.n_i), at<int32_t>(c, L.n_j),
                         at<float>(c, L.n_z), at<float>(c, L.n_r)};
  if (chains) launch_cq_receipt_chain(CqChainReceiptArgs{ra, chain}, nq, s);
  else launch_cq_receipt(ra, nq, s);
  return L;
}

void check_queries(const osc_corpus& c, const float* psis, int32_t Q, int32_t top_k) {
  if (Q < 0 || (Q > 0 && !psis)) throw Invalid("psis must be a (Q, D) array");
  if (top_k < 1 || top_k > host::kCorpusMaxTopK) throw Invalid("top_k must be between 1 and 1024");
  for (int64_t i = 0; i < (int64_t)Q * c.D; ++i)
    if (!std::isfinite(psis[i])) throw Invalid("psis must be finite");
}

void check_candidates(const osc_corpus& c, const int32_t* cand, int32_t Q, int32_t K) {
  for (int64_t i = 0; i < (int64_t)Q * K; ++i) {
    if (cand[i] < 0 || cand[i] >= c.N) throw Invalid("candidates: corpus id out of range");
    if (!host::store_get(c.live.data(), cand[i]))
      throw Invalid("candidates: query " + std::to_string(i / K) + " names removed id " + std::to_string(cand[i]));
  }
}

// the same for a ragged call: row q's first rows[q] entries are checked, the entries behind them must be the pad id
void check_candidates_ragged(const osc_corpus& c, const int32_t* cand, int32_t Q, int32_t K, const int32_t* rows) {
  for (int32_t q = 0; q < Q; ++q) {
    const int32_t* row = cand + (size_t)q * K;
    if (host::ragged_lead(row, K) != rows[q])
      throw Invalid("candidates: query " + std::to_string(q) + " must hold its " + std::to_string(rows[q]) +
                    " ids in front and -1 behind them");
    for (int32_t t = 0; t < rows[q]; ++t) {
      if (row[t] >= c.N) throw Invalid("candidates: corpus id out of range");
      if (!host::store_get(c.live.data(), row[t]))
        throw Invalid("candidates: query " + std::to_string(q) + " names removed id " + std::to_string(row[t]));
    }
  }
}

// K of a call, and its filter attached to the request: min(top_k, live rows), of which every query must have K eligible
// ones (live and allowed).  Before any device work.
int32_t set_k_and_filter(const osc_corpus& c, RefineReq& rq, int32_t top_k) {
  if (c.n_live == 0) throw Invalid("the corpus has no live rows");
  const int32_t K = (int32_t)std::min<int64_t>(top_k, c.n_live);
  const CorpusFilter& fl = c.filter;
  const bool rg = c.ragged.armed;  // a ragged call keeps whichever rows pass (proof_hallucination.py:203-221): 1 .. K of them
  if (rg) rq.rows_store.assign((size_t)rq.Q, K);
  if (fl.rows == 0) return K;
  if (rq.cand_in) throw Invalid("a filter cannot be combined with candidates");
  if (fl.rows != 1 && fl.rows != rq.Q) throw Invalid("the filter must have 1 row or one row per query");
  if (fl.words_per_row != host::store_words(c.N)) throw Invalid("the filter was armed for another row count");
  for (int32_t q = 0; q < (fl.rows == 1 ? std::min(rq.Q, 1) : rq.Q); ++q) {
    const int64_t n = host::store_count(c.live.data(), fl.words.data() + (size_t)q * fl.words_per_row, c.N);
    if (rg && n > 0) {
      if (fl.rows == 1) rq.rows_store.assign((size_t)rq.Q, host::ragged_rows(n, K));
      else rq.rows_store[(size_t)q] = host::ragged_rows(n, K);
      continue;
    }
    if (n < K)
      throw Invalid("filter: query " + std::to_string(q) + " has " + std::to_string(n) + " eligible rows, fewer than K = " +
                    std::to_string(K));
  }
  rq.allow = fl.words.data();
  rq.allow_stride = fl.rows == 1 ? 0 : fl.words_per_row;
  return K;
}

// the row counts of a call armed by osc_corpus_ragged, behind set_k_and_filter (which took them from the filter): given with
// the arming, or read off cand_in's padding; checked, kept for osc_corpus_ragged_rows, and the call marked ragged unless
// every lattice fills its slot.  Before any device work.
void set_ragged(osc_corpus& c, RefineReq& rq) {
  if (!c.ragged.armed) return;
  const int32_t Q = rq.Q, K = rq.K;
  if (!c.ragged.rows.empty()) {
    if ((int64_t)c.ragged.rows.size() != Q) throw Invalid("ragged: the row counts were armed for another Q");
    if (!rq.cand_in && c.ragged.rows != rq.rows_store)  // (searched candidates: the counts are the eligible rows', or K)
      throw Invalid("ragged: the row counts given are not min(K, eligible rows)");
    rq.rows_store = c.ragged.rows;
  } else if (rq.cand_in) {
    for (int32_t q = 0; q < Q; ++q) {
      const int32_t n = host::ragged_lead(rq.cand_in + (size_t)q * K, K);
      if (n < 0) throw Invalid("candidates: query " + std::to_string(q) + " has an id behind a -1");
      rq.rows_store[(size_t)q] = n;
    }
  }
  const int32_t bad = host::ragged_first_bad(rq.rows_store.data(), Q, K);
  if (bad >= 0)
    throw Invalid("ragged: query " + std::to_string(bad) + " has " + std::to_string(rq.rows_store[(size_t)bad]) +
                  " rows, need 1 .. K = " + std::to_string(K));
  c.last_rows = rq.rows_store;
  rq.ragged = !host::ragged_is_uniform(rq.rows_store.data(), Q, K);
}

int32_t chunk_for(const osc_corpus& c, int32_t K, int32_t knn, int32_t kk, bool receipts = false, int32_t null_slots = 0,
                  int32_t chain_cap = 0) {
  return host::corpus_chunk(c.N, c.ldn, K, std::max(1, knn), std::max(1, kk), c.chunk_req, host::kCorpusBudgetBytes, receipts,
                            null_slots, chain_cap);
}

struct RefineOut {
  int32_t* cand;
  int32_t* local;
  float* score;
  float* align;
  int32_t* iters;
  float* res;
  float* gates = nullptr;     // the three below: gated calls only
  int32_t* g_iters = nullptr;
  float* g_res = nullptr;
};

// what a receipts call returns on top of RefineOut (osc_corpus_refine_receipts)
struct ReceiptOut {
  int32_t* s_iters;
  float* s_res;
  double* sums[4];          // deltaH, coh_drop, anchor_pen, query_term
  int32_t* null_total;
  int64_t* null_offsets;    // Q + 1
  int32_t* null_i;
  int32_t* null_j;
  float* null_z;
  float* null_r;
  int64_t capacity;
  int64_t* nnz;             // the three below: optional (state signature / degree fields of the dict form)
  int64_t* edge_prefix;     // Q x prefix_cap x 2
  int32_t* edge_prefix_n;
  int32_t prefix_cap;
};

// what a call with chains returns on top of that (osc_corpus_refine_chains); the four edge arrays are flat over the chain
// edges of all queries, in query order
struct ChainOut {
  float* z_struct;
  float* z_path;
  float* r_struct;
  float* r_path;
  double* gain;
  int32_t* verdict;
  int32_t* weak_k;
  float* weak_z;
};

void check_gate_settings(float beta, float gamma, int32_t method, int32_t max_iters) {
  if (!(gamma > 0.f) || !std::isfinite(gamma)) throw Invalid("gamma must be > 0 for SPD");
  if (!std::isfinite(beta)) throw Invalid("beta must be finite");
  if (method != 0 && method != 1) throw Invalid("method must be 0 (direct) or 1 (cg)");
  if (max_iters < 1) throw Invalid("max_iters must be >= 1");
}

// the gates of a request: mode 0 = none, 1 = diffusion gates under these (checked) settings, 2 = gates_in
void set_gate_request(RefineReq& rq, int32_t mode, const float* gates_in, float beta, float gamma, int32_t method, float tol,
                      int32_t max_iters) {
  rq.gate = mode;
  if (mode == 2) rq.gates_in = gates_in;
  if (mode != 1) return;
  check_gate_settings(beta, gamma, method, max_iters);
  rq.g_beta = beta;
  rq.g_gamma = gamma;
  rq.g_direct = method == 0;
  rq.g_tol = tol;
  rq.g_max_iters = method == 0 ? 2048 : max_iters;  // direct: the reference's dense solve, served by a long CG
}

// the gate_mode argument of the entry points that take one
void check_gate_mode(int32_t gate_mode, const float* gates_in, int32_t Q) {
  if (gate_mode < 0 || gate_mode > 2) throw Invalid("gate_mode must be 0 (none), 1 (diffusion) or 2 (given)");
  if (gate_mode == 2 && !gates_in && Q > 0) throw Invalid("gate_mode 2 needs gates_in");
}

// the settle and the receipt of a request, under these (checked) settings; detail 0 = light, 1 = full
void set_receipt_request(RefineReq& rq, int32_t detail, float dt, int32_t settle_max_iters, float settle_tol, float z_th,
                         int32_t null_cap) {
  if (!(dt > 0.f) || !std::isfinite(dt)) throw Invalid("dt must be finite and > 0");
  if (settle_max_iters < 1) throw Invalid("settle_max_iters must be >= 1");
  if (!std::isfinite(settle_tol)) throw Invalid("settle_tol must be finite");
  if (!std::isfinite(z_th)) throw Invalid("z_th must be finite");
  rq.receipts = detail ? 2 : 1;
  rq.s_dt = dt;
  rq.s_max_iters = settle_max_iters;
  rq.s_tol = settle_tol;
  rq.z_th = z_th;
  rq.null_cap = std::max(0, null_cap);
}

ReceiptOut receipt_out(int32_t* settle_iters, float* settle_res, double* dH, double* coh_sum, double* anchor_sum,
                       double* query_sum, int32_t* null_total, int64_t* null_offsets, int32_t* null_i, int32_t* null_j,
                       float* null_z, float* null_r, int64_t null_capacity, int64_t* nnz_out, int64_t* edge_prefix,
                       int32_t* edge_prefix_n, int32_t edge_prefix_cap) {
  return ReceiptOut{settle_iters, settle_res, {dH, coh_sum, anchor_sum, query_sum}, null_total, null_offsets, null_i,
                    null_j, null_z, null_r, null_capacity, nnz_out, edge_prefix, edge_prefix_n, edge_prefix_cap};
}

// the queries, top_k, kneighbors and candidates of a request (checked by check_request and set_shape)
RefineReq lattice_request(const float* psis, int32_t Q, int32_t top_k, int32_t kneighbors, const int32_t* cand_in) {
  RefineReq rq{};
  rq.psis = psis;
  rq.Q = Q;
  rq.top_k = top_k;
  rq.kneighbors = kneighbors;
  rq.cand_in = cand_in;
  return rq;
}

// a full refine: the lattices, the U* solve's settings and the bundle's
RefineReq refine_request(const float* psis, int32_t Q, int32_t top_k, const int32_t* cand_in, int32_t kneighbors,
                         float row_cap, float lamG, float lamC, float lamQ, float tol, int32_t max_iters, int32_t k,
                         float alpha) {
  RefineReq rq = lattice_request(psis, Q, top_k, kneighbors, cand_in);
  rq.row_cap = row_cap;
  rq.lamG = lamG;
  rq.lamC = lamC;
  rq.lamQ = lamQ;
  rq.tol = tol;
  rq.max_iters = std::max(1, max_iters);
  rq.kk = k;  // as given; refine_body clamps it to [0, K]
  rq.alpha = alpha;
  rq.stage = 2;
  return rq;
}

// what every per-lattice entry point checks first, in this order
void check_request(const osc_corpus& c, const RefineReq& rq) {
  check_queries(c, rq.psis, rq.Q, rq.top_k);
  if (rq.kneighbors < 1) throw Invalid("kneighbors must be >= 1");
}

// the records of a call armed by osc_corpus_settings, behind set_ragged (which knows the lattices' rows): each lattice's
// effective record and list length, and the request's list width and output width as their maxima.  Before any device work.
void set_settings(const osc_corpus& c, RefineReq& rq) {
  if (c.settings.empty()) return;
  const int32_t Q = rq.Q, K = rq.K;
  if ((int64_t)c.settings.size() != Q) throw Invalid("settings: the records were armed for another Q");
  const int32_t lng = host::settings_first_long_list(c.settings.data(), Q, K);
  if (lng >= 0) throw Invalid("settings: query " + std::to_string(lng) + ": min(kneighbors, K - 1) must be at most 128");
  rq.settings.resize((size_t)Q);
  rq.klist.resize((size_t)Q);
  for (int32_t q = 0; q < Q; ++q) {
    rq.settings[(size_t)q] = host::setting_effective(c.settings[(size_t)q], rq.rows_of(q), K);
    rq.klist[(size_t)q] = rq.settings[(size_t)q].kneighbors;
  }
  rq.knn = host::settings_max_knn(rq.settings.data(), Q);
  rq.kk = host::settings_max_kk(rq.settings.data(), Q);
}

// what an armed call's own scalar arguments of the records' names become: query 0's (checked) values, so that the scalar
// checks pass and say nothing about arguments the call ignores; nothing reads them afterwards.  Any pointer may be null.
struct SettingScalars {
  int32_t* kneighbors = nullptr;
  float *lamG = nullptr, *lamC = nullptr, *lamQ = nullptr;
  int32_t* k = nullptr;
  float* alpha = nullptr;
  float* dt = nullptr;
  int32_t* settle_max_iters = nullptr;
  float *settle_tol = nullptr, *lamP = nullptr;
};
void take_armed(const osc_corpus& c, int32_t Q, const SettingScalars& a) {
  if (c.settings.empty()) return;
  if ((int64_t)c.settings.size() != Q) throw Invalid("settings: the records were armed for another Q");
  const host::CorpusSetting& s0 = c.settings[0];
  if (a.kneighbors) *a.kneighbors = s0.kneighbors;
  if (a.lamG) *a.lamG = s0.lamG;
  if (a.lamC) *a.lamC = s0.lamC;
  if (a.lamQ) *a.lamQ = s0.lamQ;
  if (a.k) *a.k = s0.k;
  if (a.alpha) *a.alpha = s0.alpha;
  if (a.dt) *a.dt = s0.settle_dt;
  if (a.settle_max_iters) *a.settle_max_iters = s0.settle_max_iters;
  if (a.settle_tol) *a.settle_tol = s0.settle_tol;
  if (a.lamP) *a.lamP = s0.lamP;
}

// K and the list length of the request's lattices, its filter attached, and its candidates checked if given
void set_shape(osc_corpus& c, RefineReq& rq) {
  rq.K = set_k_and_filter(c, rq, rq.top_k);
  rq.knn = rq.K > 1 ? host::corpus_knn(rq.kneighbors, rq.K) : 0;
  if (c.settings.empty() && rq.knn > host::kCorpusMaxKnn) throw Invalid("min(kneighbors, K - 1) must be at most 128");
  set_ragged(c, rq);
  set_settings(c, rq);
  if (rq.cand_in && !rq.rows_store.empty()) check_candidates_ragged(c, rq.cand_in, rq.Q, rq.K, rq.rows_store.data());
  else if (rq.cand_in) check_candidates(c, rq.cand_in, rq.Q, rq.K);
}

// runs the request chunk by chunk; fetch(L, q0, n, down) queues the chunk's downloads, then the stream is drained
template <class F>
void for_each_chunk(osc_corpus& c, const RefineReq& rq, F&& fetch) {
  const int32_t nq = chunk_for(c, rq.K, rq.knn, rq.kk, rq.receipts != 0, rq.null_slots, rq.chain_cap);
  auto down = [&](void* dst, int64_t off, size_t bytes) {
    HIP_CHECK(hipMemcpyAsync(dst, c.scratch.p + off, bytes, hipMemcpyDeviceToHost, c.stream));
  };
  for (int32_t ch = 0; ch < host::chunk_count(rq.Q, nq); ++ch) {
    const int32_t q0 = host::chunk_begin(ch, nq), n = host::chunk_size(rq.Q, ch, nq);
    const host::CorpusLayout L = run_chunk(c, rq, q0, n, nq);
    fetch(L, q0, n, down);
    HIP_CHECK(hipStreamSynchronize(c.stream));
  }
}

// a chunk's receipts: per-query scalars and the slabs of kept null points (null_slots per query), packed back to back on the
// host once the chunk's copies have landed (the stream is drained here: the staging vectors live in this call)
template <class Down>
void fetch_receipts(osc_corpus& c, const RefineReq& rq, const ReceiptOut& ro, const host::CorpusLayout& L, int32_t q0,
                    int32_t n, Down& down) {
  const bool full = rq.receipts == 2;
  const int32_t slots = rq.null_slots, kw = std::max(1, rq.knn);
  std::vector<double> hs((size_t)n * 4);
  std::vector<int32_t> hk((size_t)n), hi((size_t)n * slots), hj((size_t)n * slots), hd, hc;
  std::vector<float> hz((size_t)n * slots), hr((size_t)n * slots);
  down(ro.s_iters + q0, L.s_iters, (size_t)n * 4);
  down(ro.s_res + q0, L.s_res, (size_t)n * 4);
  down(hs.data(), L.r_sums, hs.size() * 8);
  down(ro.null_total + q0, L.n_total, (size_t)n * 4);
  down(hk.data(), L.n_kept, (size_t)n * 4);
  if (full && slots > 0) {
    down(hi.data(), L.n_i, hi.size() * 4);
    down(hj.data(), L.n_j, hj.size() * 4);
    down(hz.data(), L.n_z, hz.size() * 4);
    down(hr.data(), L.n_r, hr.size() * 4);
  }
  const bool want_graph = ro.nnz || ro.edge_prefix;
  if (want_graph) {
    hd.resize((size_t)n * rq.K);
    hc.resize((size_t)n * rq.K * kw);
    down(hd.data(), L.deg, hd.size() * 4);
    down(hc.data(), L.col, hc.size() * 4);
  }
  HIP_CHECK(hipStreamSynchronize(c.stream));
  for (int32_t q = 0; q < n; ++q) {
    for (int t = 0; t < 4; ++t) ro.sums[t][q0 + q] = hs[(size_t)q * 4 + t];
    int64_t at0 = ro.null_offsets[q0 + q];
    const int32_t kept = full ? std::min(std::max(hk[(size_t)q], 0), slots) : 0;
    for (int32_t t = 0; t < kept; ++t) {
      const size_t sidx = (size_t)q * slots + t;
      ro.null_i[at0 + t] = hi[sidx];
      ro.null_j[at0 + t] = hj[sidx];
      ro.null_z[at0 + t] = hz[sidx];
      ro.null_r[at0 + t] = hr[sidx];
    }
    ro.null_offsets[q0 + q + 1] = at0 + kept;
    if (!want_graph) continue;
    int64_t nnz = 0, np = 0;
    const int64_t r0 = (int64_t)q * rq.K;
    int64_t* pairs = ro.edge_prefix ? ro.edge_prefix + (size_t)(q0 + q) * ro.prefix_cap * 2 : nullptr;
    for (int32_t i = 0; i < rq.K; ++i) {
      const int32_t d = rq.knn > 0 ? hd[(size_t)(r0 + i)] : 0;
      for (int32_t e = 0; e < d && pairs && np < ro.prefix_cap; ++e, ++np) {
        pairs[np * 2] = i;
        pairs[np * 2 + 1] = (int64_t)hc[(size_t)(r0 + i) * kw + e] - r0;
      }
      nnz += d;
    }
    if (ro.nnz) ro.nnz[q0 + q] = nnz;
    if (ro.edge_prefix_n) ro.edge_prefix_n[q0 + q] = (int32_t)np;
  }
}

// a chunk's chain receipts: the edge slabs (chain_cap per query) packed to the queries' edge ranges, and the per-query scalars
template <class Down>
void fetch_chains(osc_corpus& c, const RefineReq& rq, const ChainOut& co, const host::CorpusLayout& L, int32_t q0, int32_t n,
                  Down& down) {
  const int32_t cap = rq.chain_cap;
  std::vector<float> he((size_t)n * 4 * cap);
  down(he.data(), L.c_edge, he.size() * 4);
  down(co.gain + q0, L.c_gain, (size_t)n * 8);
  down(co.verdict + q0, L.c_verdict, (size_t)n * 4);
  down(co.weak_k + q0, L.c_weak_k, (size_t)n * 4);
  down(co.weak_z + q0, L.c_weak_z, (size_t)n * 4);
  HIP_CHECK(hipStreamSynchronize(c.stream));
  float* dst[4] = {co.z_struct, co.z_path, co.r_struct, co.r_path};
  for (int32_t q = 0; q < n; ++q) {
    const int64_t e0 = rq.c_eoff[q0 + q], ne = rq.c_eoff[q0 + q + 1] - e0;
    for (int t = 0; t < 4; ++t)
      std::copy(he.begin() + ((size_t)q * 4 + t) * cap, he.begin() + ((size_t)q * 4 + t) * cap + ne, dst[t] + e0);
  }
}

// validates a refine_request (with its gates, receipts and chains set) and its buffers, in the order the messages are
// documented in, and runs it
void refine_body(osc_corpus& c, RefineReq rq, const RefineOut& o, const char* null_msg, const ReceiptOut* ro = nullptr,
                 const ChainOut* co = nullptr) {
  const int32_t Q = rq.Q;
  check_request(c, rq);
  if (!(rq.lamG > 0.f) || rq.lamC < 0.f || rq.lamQ < 0.f) throw Invalid("need lamG > 0, lamC >= 0, lamQ >= 0");
  set_shape(c, rq);
  rq.kk = std::min(std::max(rq.kk, 0), rq.K);
  if (rq.gate == 2)
    for (int32_t q = 0; q < Q; ++q)
      for (int32_t r = 0; r < rq.rows_of(q); ++r) {
        const float gv = rq.gates_in[(size_t)q * rq.K + r];
        if (!std::isfinite(gv) || gv < 0.f) throw Invalid("gates must be finite and >= 0");
      }
  if (rq.gate == 2 && rq.ragged) {  // only a lattice's own rows are read: zeros behind them
    rq.gates_store.resize((size_t)Q * rq.K);
    for (int32_t q = 0; q < Q; ++q)
      host::ragged_copy_padded(rq.gates_in + (size_t)q * rq.K, rq.rows_of(q), rq.K, 0.f, rq.gates_store.data() + (size_t)q * rq.K);
    rq.gates_in = rq.gates_store.data();
  }
  if (ro) {
    if (!ro->null_offsets) throw Invalid(null_msg);
    ro->null_offsets[0] = 0;
  }
  std::vector<int64_t> eoff;  // the chains: checked as add_chain checks them (lattice.py:129-142), edge offsets formed
  if (co) {
    if (!(rq.lamP >= 0.f) || !std::isfinite(rq.lamP)) throw Invalid("lamP must be >= 0");
    if (!std::isfinite(rq.c_zth)) throw Invalid("chain_z_th must be finite");
    if (!rq.c_off || rq.c_off[0] != 0) throw Invalid("chain_offsets must start at 0");
    eoff.assign((size_t)Q + 1, 0);
    for (int32_t q = 0; q < Q; ++q) {
      const int64_t len = rq.c_off[q + 1] - rq.c_off[q];
      if (len < 0) throw Invalid("chain_offsets must not decrease");
      if (len == 1) throw Invalid("chain must contain at least two indices");
      if (len > host::kCorpusMaxChain) throw Invalid("a chain has at most 1024 indices");
      if (len > 0 && !rq.c_nodes) throw Invalid(null_msg);
      for (int64_t t = rq.c_off[q]; t < rq.c_off[q + 1]; ++t)
        if (rq.c_nodes[t] < 0 || rq.c_nodes[t] >= rq.rows_of(q)) throw Invalid("chain indices out of bounds");
      eoff[(size_t)q + 1] = eoff[(size_t)q] + std::max<int64_t>(0, len - 1);
      rq.chain_cap = std::max(rq.chain_cap, (int32_t)std::max<int64_t>(0, len - 1));
    }
    if (rq.c_w)
      for (int64_t t = 0; t < eoff[(size_t)Q]; ++t)
        if (!std::isfinite(rq.c_w[t])) throw Invalid("chain weights must be finite");
    rq.c_eoff = eoff.data();
    if (rq.chain_cap == 0) co = nullptr;  // no query has a chain: the call without chains
  }
  if (Q == 0) return;
  if (co && (!co->z_struct || !co->z_path || !co->r_struct || !co->r_path || !co->gain || !co->verdict || !co->weak_k ||
             !co->weak_z))
    throw Invalid(null_msg);
  if (!o.cand || !o.iters || !o.res || (rq.kk > 0 && (!o.local || !o.score || !o.align)) ||
      (rq.gate && (!o.gates || !o.g_iters || !o.g_res)))
    throw Invalid(null_msg);
  if (ro) {
    const bool full = rq.receipts == 2;
    if (!ro->s_iters || !ro->s_res || !ro->sums[0] || !ro->sums[1] || !ro->sums[2] || !ro->sums[3] || !ro->null_total ||
        (full && (!ro->null_i || !ro->null_j || !ro->null_z || !ro->null_r)) ||
        (ro->edge_prefix && (!ro->edge_prefix_n || ro->prefix_cap < 0)))
      throw Invalid(null_msg);
    rq.null_slots = host::corpus_null_slots(rq.K, full, rq.null_cap);
    if (full && ro->capacity < (int64_t)Q * rq.null_slots) throw Invalid("null point capacity too small");
  }
  for_each_chunk(c, rq, [&](const host::CorpusLayout& L, int32_t q0, int32_t n, auto& down) {
    down(o.cand + (size_t)q0 * rq.K, L.cand, (size_t)n * rq.K * 4);
    down(o.iters + q0, L.iters, (size_t)n * 4);
    down(o.res + q0, L.res, (size_t)n * 4);
    if (rq.kk > 0) {
      down(o.local + (size_t)q0 * rq.kk, L.o_local, (size_t)n * rq.kk * 4);
      down(o.score + (size_t)q0 * rq.kk, L.o_score, (size_t)n * rq.kk * 4);
      down(o.align + (size_t)q0 * rq.kk, L.o_align, (size_t)n * rq.kk * 4);
    }
    if (rq.gate) down(o.gates + (size_t)q0 * rq.K, L.gates, (size_t)n * rq.K * 4);
    if (rq.gate == 1) {
      down(o.g_iters + q0, L.g_iters, (size_t)n * 4);
      down(o.g_res + q0, L.g_res, (size_t)n * 4);
    }
    if (ro) fetch_receipts(c, rq, *ro, L, q0, n, down);
    if (co) fetch_chains(c, rq, *co, L, q0, n, down);
  });
  if (rq.gate == 2) {  // nothing was solved for given gates
    std::fill(o.g_iters, o.g_iters + Q, 0);
    std::fill(o.g_res, o.g_res + Q, 0.f);
  }
}

}  // namespace

extern "C" {

int osc_corpus_create(const float* Y, int64_t N, int32_t D, int32_t device, osc_corpus_handle* out) {
  if (!out) return OSC_E_INVALID;
  *out = nullptr;
  if (!Y || N < 1 || D < 1 || N >= (int64_t)1 << 31 || D > osc::kBundleCols) {
    g_corpus_error = "osc_corpus_create: need Y != NULL, 1 <= N < 2^31, 1 <= D <= 1536";
    return OSC_E_INVALID;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1 || device < 0 || device >= ndev) {
    g_corpus_error = "osc_corpus_create: no usable HIP device (this library has no CPU fallback)";
    return OSC_E_NODEVICE;
  }
  std::unique_ptr<osc_corpus> h(new osc_corpus());
  try {
    h->device = device;
    HIP_CHECK(hipSetDevice(device));
    h->stream = acquire_stream(device);
    alloc_ctx() = AllocCtx{device, h->stream};
    h->N = h->cap = h->n_live = N;
    h->live.assign((size_t)host::store_words(N), 0xffffffffu);
    h->live.back() = host::store_tail_mask(N);
    h->D = D;
    h->ldn = host::corpus_ldn(D);
    if (const char* e = getenv("OSC_CORPUS_CHUNK")) {  // queries per chunk (read once, like read_env's switches)
      const int v = atoi(e);
      if (v >= 1) h->chunk_req = v;
    }
    h->Y.alloc((size_t)N * h->ldn);
    h->Yn.alloc((size_t)N * h->ldn);
    HIP_CHECK(hipMemsetAsync(h->Y.p, 0, (size_t)N * h->ldn * 4, h->stream));
    HIP_CHECK(hipMemcpy2DAsync(h->Y.p, (size_t)h->ldn * 4, Y, (size_t)D * 4, (size_t)D * 4, (size_t)N,
                               hipMemcpyHostToDevice, h->stream));
    launch_normalize_rows(h->Y.p, h->ldn, h->Yn.p, h->ldn, N, D, h->stream);  // osc_create's row normalisation
    HIP_CHECK(hipStreamSynchronize(h->stream));
  } catch (const std::exception& e) {
    g_corpus_error = e.what();
    return OSC_E_HIP;
  }
  *out = h.release();
  return OSC_OK;
}

int osc_corpus_destroy(osc_corpus_handle h) {
  if (!h) return OSC_OK;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  alloc_ctx() = AllocCtx{h->device, nullptr};
  delete h;
  return OSC_OK;
}

const char* osc_corpus_last_error(osc_corpus_handle h) { return h ? h->err.c_str() : g_corpus_error.c_str(); }

int osc_corpus_info(osc_corpus_handle h, int32_t top_k, int32_t kneighbors, int32_t k, int32_t* chunk, int64_t* bytes) {
  return corpus_guarded(h, [&](osc_corpus& c) {
    if (c.n_live == 0) throw Invalid("the corpus has no live rows");
    const int32_t K = (int32_t)std::min<int64_t>(std::max(1, top_k), c.n_live);
    const int32_t knn = K > 1 ? host::corpus_knn(kneighbors, K) : 0;
    const int32_t kk = std::min(std::max(k, 0), K);
    const int32_t nq = chunk_for(c, K, knn, kk);
    if (chunk) *chunk = nq;
    if (bytes) *bytes = host::corpus_layout(c.N, c.ldn, K, std::max(1, knn), std::max(1, kk), nq).total;
  });
}

int osc_corpus_search(osc_corpus_handle h, const float* psis, int32_t Q, int32_t top_k, int32_t* ids, float* cos) {
  return corpus_query(h, [&](osc_corpus& c) {
    check_queries(c, psis, Q, top_k);
    if (Q == 0) return;
    if (!ids || !cos) throw Invalid("osc_corpus_search: NULL buffer");
    RefineReq rq{};
    rq.psis = psis;
    rq.Q = Q;
    rq.K = set_k_and_filter(c, rq, top_k);
    set_ragged(c, rq);
    rq.stage = 0;
    for_each_chunk(c, rq, [&](const host::CorpusLayout& L, int32_t q0, int32_t n, auto& down) {
      down(ids + (size_t)q0 * rq.K, L.cand, (size_t)n * rq.K * 4);
      down(cos + (size_t)q0 * rq.K, L.ccos, (size_t)n * rq.K * 4);
    });
  });
}

int osc_corpus_refine(osc_corpus_handle h, const float* psis, int32_t Q, int32_t top_k, const int32_t* cand_in,
                      int32_t kneighbors, float row_cap, float lamG, float lamC, float lamQ, float tol, int32_t max_iters,
                      int32_t k, float alpha, int32_t* cand_out, int32_t* local, float* score, float* align, int32_t* iters,
                      float* res) {
  return corpus_query(h, [&](osc_corpus& c) {
    take_armed(c, Q, SettingScalars{&kneighbors, &lamG, &lamC, &lamQ, &k, &alpha});
    refine_body(c, refine_request(psis, Q, top_k, cand_in, kneighbors, row_cap, lamG, lamC, lamQ, tol, max_iters, k, alpha),
                RefineOut{cand_out, local, score, align, iters, res}, "osc_corpus_refine: NULL buffer");
  });
}

int osc_corpus_refine_gated(osc_corpus_handle h, const float* psis, int32_t Q, int32_t top_k, const int32_t* cand_in,
                            const float* gates_in, float beta, float gamma, int32_t method, float gate_tol,
                            int32_t gate_max_iters, int32_t kneighbors, float row_cap, float lamG, float lamC, float lamQ,
                            float tol, int32_t max_iters, int32_t k, float alpha, int32_t* cand_out, float* gates_out,
                            int32_t* local, float* score, float* align, int32_t* iters, float* res, int32_t* gate_iters,
                            float* gate_res) {
  return corpus_query(h, [&](osc_corpus& c) {
    take_armed(c, Q, SettingScalars{&kneighbors, &lamG, &lamC, &lamQ, &k, &alpha});
    RefineReq rq = refine_request(psis, Q, top_k, cand_in, kneighbors, row_cap, lamG, lamC, lamQ, tol, max_iters, k, alpha);
    set_gate_request(rq, gates_in ? 2 : 1, gates_in, beta, gamma, method, gate_tol, gate_max_iters);
    refine_body(c, rq, RefineOut{cand_out, local, score, align, iters, res, gates_out, gate_iters, gate_res},
                "osc_corpus_refine_gated: NULL buffer");
  });
}

int osc_corpus_refine_receipts(osc_corpus_handle h, const float* psis, int32_t Q, int32_t top_k, const int32_t* cand_in,
                               int32_t gate_mode, const float* gates_in, float beta, float gamma, int32_t method,
                               float gate_tol, int32_t gate_max_iters, int32_t kneighbors, float row_cap, float lamG,
                               float lamC, float lamQ, float tol, int32_t max_iters, int32_t k, float alpha, float dt,
                               int32_t settle_max_iters, float settle_tol, int32_t detail, float z_th, int32_t null_cap,
                               int32_t* cand_out, float* gates_out, int32_t* local, float* score, float* align,
                               int32_t* iters, float* res, int32_t* gate_iters, float* gate_res, int32_t* settle_iters,
                               float* settle_res, double* dH, double* coh_sum, double* anchor_sum, double* query_sum,
                               int32_t* null_total, int64_t* null_offsets, int32_t* null_i, int32_t* null_j, float* null_z,
                               float* null_r, int64_t null_capacity, int64_t* nnz_out, int64_t* edge_prefix,
                               int32_t* edge_prefix_n, int32_t edge_prefix_cap) {
  return corpus_query(h, [&](osc_corpus& c) {
    take_armed(c, Q, SettingScalars{&kneighbors, &lamG, &lamC, &lamQ, &k, &alpha, &dt, &settle_max_iters, &settle_tol});
    check_gate_mode(gate_mode, gates_in, Q);
    if (detail != 0 && detail != 1) throw Invalid("detail must be 0 (light) or 1 (full)");
    RefineReq rq = refine_request(psis, Q, top_k, cand_in, kneighbors, row_cap, lamG, lamC, lamQ, tol, max_iters, k, alpha);
    set_receipt_request(rq, detail, dt, settle_max_iters, settle_tol, z_th, null_cap);  // checked ahead of the gates' settings
    set_gate_request(rq, gate_mode, gates_in, beta, gamma, method, gate_tol, gate_max_iters);
    const ReceiptOut ro = receipt_out(settle_iters, settle_res, dH, coh_sum, anchor_sum, query_sum, null_total, null_offsets,
                                      null_i, null_j, null_z, null_r, null_capacity, nnz_out, edge_prefix, edge_prefix_n,
                                      edge_prefix_cap);
    refine_body(c, rq, RefineOut{cand_out, local, score, align, iters, res, gates_out, gate_iters, gate_res},
                "osc_corpus_refine_receipts: NULL buffer", &ro);
  });
}

int osc_corpus_refine_chains(osc_corpus_handle h, const float* psis, int32_t Q, int32_t top_k, const int32_t* cand_in,
                             int32_t gate_mode, const float* gates_in, float beta, float gamma, int32_t method,
                             float gate_tol, int32_t gate_max_iters, int32_t kneighbors, float row_cap, float lamG, float lamC,
                             float lamQ, float tol, int32_t max_iters, int32_t k, float alpha, float dt,
                             int32_t settle_max_iters, float settle_tol, int32_t detail, float z_th, int32_t null_cap,
                             const int64_t* chain_offsets, const int32_t* chain_nodes, const float* chain_weights, float lamP,
                             float chain_z_th, int32_t* cand_out, float* gates_out, int32_t* local, float* score,
                             float* align, int32_t* iters, float* res, int32_t* gate_iters, float* gate_res,
                             int32_t* settle_iters, float* settle_res, double* dH, double* coh_sum, double* anchor_sum,
                             double* query_sum, int32_t* null_total, int64_t* null_offsets, int32_t* null_i, int32_t* null_j,
                             float* null_z, float* null_r, int64_t null_capacity, int64_t* nnz_out, int64_t* edge_prefix,
                             int32_t* edge_prefix_n, int32_t edge_prefix_cap, float* chain_z_struct, float* chain_z_path,
                             float* chain_r_struct, float* chain_r_path, double* chain_gain, int32_t* chain_verdict,
                             int32_t* chain_weakest_k, float* chain_weakest_z) {
  return corpus_query(h, [&](osc_corpus& c) {
    take_armed(c, Q, SettingScalars{&kneighbors, &lamG, &lamC, &lamQ, &k, &alpha, &dt, &settle_max_iters, &settle_tol, &lamP});
    check_gate_mode(gate_mode, gates_in, Q);
    if (detail < -1 || detail > 1) throw Invalid("detail must be -1 (no receipts), 0 (light) or 1 (full)");
    RefineReq rq = refine_request(psis, Q, top_k, cand_in, kneighbors, row_cap, lamG, lamC, lamQ, tol, max_iters, k, alpha);
    set_gate_request(rq, gate_mode, gates_in, beta, gamma, method, gate_tol, gate_max_iters);
    if (detail >= 0) set_receipt_request(rq, detail, dt, settle_max_iters, settle_tol, z_th, null_cap);
    rq.c_off = chain_offsets;
    rq.c_nodes = chain_nodes;
    rq.c_w = chain_weights;
    rq.lamP = lamP;
    rq.c_zth = chain_z_th;
    const ReceiptOut ro = receipt_out(settle_iters, settle_res, dH, coh_sum, anchor_sum, query_sum, null_total, null_offsets,
                                      null_i, null_j, null_z, null_r, null_capacity, nnz_out, edge_prefix, edge_prefix_n,
                                      edge_prefix_cap);
    const ChainOut co{chain_z_struct, chain_z_path, chain_r_struct, chain_r_path, chain_gain, chain_verdict, chain_weakest_k,
                      chain_weakest_z};
    if (!chain_offsets) throw Invalid("osc_corpus_refine_chains: NULL buffer");
    refine_body(c, rq, RefineOut{cand_out, local, score, align, iters, res, gates_out, gate_iters, gate_res},
                "osc_corpus_refine_chains: NULL buffer", detail >= 0 ? &ro : nullptr, &co);
  });
}

int osc_corpus_gates(osc_corpus_handle h, const float* psis, int32_t Q, int32_t top_k, const int32_t* cand_in,
                     int32_t kneighbors, float row_cap, float beta, float gamma, int32_t method, float tol,
                     int32_t max_iters, int32_t clamp, int32_t* cand_out, float* gates_out, int32_t* iters, float* res) {
  return corpus_query(h, [&](osc_corpus& c) {
    take_armed(c, Q, SettingScalars{&kneighbors});
    RefineReq rq = lattice_request(psis, Q, top_k, kneighbors, cand_in);
    check_request(c, rq);
    set_gate_request(rq, 1, nullptr, beta, gamma, method, tol, max_iters);
    set_shape(c, rq);
    if (Q == 0) return;
    if (!cand_out || !gates_out || !iters || !res) throw Invalid("osc_corpus_gates: NULL buffer");
    rq.row_cap = row_cap;
    rq.stage = 1;
    rq.g_clamp = clamp != 0;
    for_each_chunk(c, rq, [&](const host::CorpusLayout& L, int32_t q0, int32_t n, auto& down) {
      down(cand_out + (size_t)q0 * rq.K, L.cand, (size_t)n * rq.K * 4);
      down(gates_out + (size_t)q0 * rq.K, L.gates, (size_t)n * rq.K * 4);
      down(iters + q0, L.g_iters, (size_t)n * 4);
      down(res + q0, L.g_res, (size_t)n * 4);
    });
  });
}

int osc_corpus_graph(osc_corpus_handle h, const float* psi, const int32_t* cand_in, int32_t top_k, int32_t kneighbors,
                     float row_cap, int32_t* cand_out, int64_t* rowptr, int32_t* col, float* a, float* w, float* sqrt_deg,
                     int64_t capacity, int64_t* nnz) {
  return corpus_query(h, [&](osc_corpus& c) {
    take_armed(c, 1, SettingScalars{&kneighbors});
    RefineReq rq = lattice_request(psi, 1, top_k, kneighbors, cand_in);
    check_request(c, rq);
    set_shape(c, rq);
    if (!cand_out || !rowptr || !col || !a || !w || !sqrt_deg || !nnz) throw Invalid("osc_corpus_graph: NULL buffer");
    rq.row_cap = row_cap;
    rq.stage = 1;
    const int32_t K = rq.K, k = std::max(1, rq.knn);
    const host::CorpusLayout L = run_chunk(c, rq, 0, 1, 1);
    std::vector<int32_t> hc((size_t)K * k), hd((size_t)K);
    std::vector<float> ha((size_t)K * k), hw((size_t)K * k);
    HIP_CHECK(hipMemcpyAsync(cand_out, c.scratch.p + L.cand, (size_t)K * 4, hipMemcpyDeviceToHost, c.stream));
    HIP_CHECK(hipMemcpyAsync(hd.data(), c.scratch.p + L.deg, (size_t)K * 4, hipMemcpyDeviceToHost, c.stream));
    HIP_CHECK(hipMemcpyAsync(hc.data(), c.scratch.p + L.col, hc.size() * 4, hipMemcpyDeviceToHost, c.stream));
    HIP_CHECK(hipMemcpyAsync(ha.data(), c.scratch.p + L.adj, ha.size() * 4, hipMemcpyDeviceToHost, c.stream));
    HIP_CHECK(hipMemcpyAsync(hw.data(), c.scratch.p + L.w, hw.size() * 4, hipMemcpyDeviceToHost, c.stream));
    HIP_CHECK(hipMemcpyAsync(sqrt_deg, c.scratch.p + L.sd, (size_t)K * 4, hipMemcpyDeviceToHost, c.stream));
    HIP_CHECK(hipStreamSynchronize(c.stream));
    int64_t n = 0;
    rowptr[0] = 0;
    for (int32_t i = 0; i < K; ++i) {
      for (int32_t e = 0; e < hd[(size_t)i]; ++e) {
        if (n >= capacity) throw Invalid("osc_corpus_graph: capacity too small");
        col[n] = hc[(size_t)i * k + e];
        a[n] = ha[(size_t)i * k + e];
        w[n] = hw[(size_t)i * k + e];
        ++n;
      }
      rowptr[i + 1] = n;
    }
    *nnz = n;
  });
}

int osc_corpus_rows(osc_corpus_handle h, int64_t* N, int64_t* live, int64_t* capacity) {
  return corpus_guarded(h, [&](osc_corpus& c) {
    if (N) *N = c.N;
    if (live) *live = c.n_live;
    if (capacity) *capacity = c.cap;
  });
}

int osc_corpus_get_live(osc_corpus_handle h, uint32_t* words) {
  return corpus_guarded(h, [&](osc_corpus& c) {
    if (!words) throw Invalid("osc_corpus_get_live: NULL buffer");
    std::copy(c.live.begin(), c.live.end(), words);
  });
}

int osc_corpus_append(osc_corpus_handle h, const float* Y, int64_t M, int64_t* first_id) {
  return corpus_guarded(h, [&](osc_corpus& c) {
    if (M < 0 || (M > 0 && !Y)) throw Invalid("osc_corpus_append: need M >= 0 and Y != NULL");
    if (M > host::kCorpusMaxRows - c.N) throw Invalid("osc_corpus_append: N + M must stay below 2^31");
    if (first_id) *first_id = c.N;
    if (M == 0) return;
    const int64_t N1 = c.N + M;
    const size_t ldn = (size_t)c.ldn;
    std::vector<uint32_t> live = c.live;  // everything that can fail comes before the handle changes
    live.resize((size_t)host::store_words(N1), 0u);
    for (int64_t i = c.N; i < N1; ++i) host::store_set(live.data(), i);
    if (N1 > c.cap) {  // grow: new buffers first, then copy, swap, and the old ones go once the stream has drained
      const int64_t cap1 = host::store_capacity(c.cap, N1);
      DevBuf<float> Y1, Yn1;
      Y1.alloc((size_t)cap1 * ldn);
      Yn1.alloc((size_t)cap1 * ldn);
      HIP_CHECK(hipMemcpyAsync(Y1.p, c.Y.p, (size_t)c.N * ldn * 4, hipMemcpyDeviceToDevice, c.stream));
      HIP_CHECK(hipMemcpyAsync(Yn1.p, c.Yn.p, (size_t)c.N * ldn * 4, hipMemcpyDeviceToDevice, c.stream));
      c.Y.swap(Y1);
      c.Yn.swap(Yn1);
      c.cap = cap1;
    }  // (Y1 / Yn1 release here: pool_free waits for the stream)
    float* y = c.Y.p + (size_t)c.N * ldn;
    HIP_CHECK(hipMemsetAsync(y, 0, (size_t)M * ldn * 4, c.stream));  // the pitch padding: the GEMM reads it
    HIP_CHECK(hipMemcpy2DAsync(y, ldn * 4, Y, (size_t)c.D * 4, (size_t)c.D * 4, (size_t)M, hipMemcpyHostToDevice, c.stream));
    launch_normalize_rows(y, c.ldn, c.Yn.p + (size_t)c.N * ldn, c.ldn, M, c.D, c.stream);
    HIP_CHECK(hipStreamSynchronize(c.stream));
    c.live.swap(live);
    c.d_live_current = false;
    c.n_live += M;
    c.N = N1;
  });
}

int osc_corpus_remove(osc_corpus_handle h, const int32_t* ids, int64_t n, int64_t* newly_removed) {
  return corpus_guarded(h, [&](osc_corpus& c) {
    if (n < 0 || (n > 0 && !ids)) throw Invalid("osc_corpus_remove: need n >= 0 and ids != NULL");
    for (int64_t t = 0; t < n; ++t)
      if (ids[t] < 0 || ids[t] >= c.N)
        throw Invalid("osc_corpus_remove: id " + std::to_string(ids[t]) + " is outside [0, " + std::to_string(c.N) + ")");
    int64_t gone = 0;
    for (int64_t t = 0; t < n; ++t)
      if (host::store_get(c.live.data(), ids[t])) {
        host::store_clear(c.live.data(), ids[t]);
        ++gone;
      }
    c.n_live -= gone;
    if (gone) c.d_live_current = false;
    if (newly_removed) *newly_removed = gone;
  });
}

int osc_corpus_update(osc_corpus_handle h, const int32_t* ids, const float* Y, int64_t M) {
  return corpus_guarded(h, [&](osc_corpus& c) {
    if (M < 0 || (M > 0 && (!ids || !Y))) throw Invalid("osc_corpus_update: need M >= 0, ids != NULL and Y != NULL");
    if (M == 0) return;
    {  // everything that can fail comes before the handle changes
      std::vector<int32_t> keep((size_t)c.N);
      const int32_t bad = host::update_ids(ids, M, c.N, keep.data());
      if (bad == host::kUpdateIdOutOfRange) {
        for (int64_t t = 0; t < M; ++t)
          if (ids[t] < 0 || ids[t] >= c.N)
            throw Invalid("osc_corpus_update: id " + std::to_string(ids[t]) + " is outside [0, " + std::to_string(c.N) + ")");
      }
      if (bad == host::kUpdateIdDuplicate) throw Invalid("osc_corpus_update: an id is named twice");
      if (bad != host::kUpdateIdsOk) throw Invalid("osc_corpus_update: bad sizes");
    }
    for (int64_t t = 0; t < M; ++t)
      if (!host::store_get(c.live.data(), ids[t]))
        throw Invalid("osc_corpus_update: id " + std::to_string(ids[t]) + " names a removed row");
    for (int64_t t = 0; t < M * c.D; ++t)
      if (!std::isfinite(Y[t])) throw Invalid("osc_corpus_update: row " + std::to_string(t / c.D) + " of Y is not finite");
    DevBuf<float> rows;
    DevBuf<int32_t> at;
    rows.alloc((size_t)M * c.D);
    at.alloc((size_t)M);
    HIP_CHECK(hipMemcpyAsync(rows.p, Y, (size_t)M * c.D * 4, hipMemcpyHostToDevice, c.stream));
    HIP_CHECK(hipMemcpyAsync(at.p, ids, (size_t)M * 4, hipMemcpyHostToDevice, c.stream));
    launch_corpus_update_rows(rows.p, c.D, at.p, M, c.Y.p, c.Yn.p, c.ldn, c.stream);
    HIP_CHECK(hipStreamSynchronize(c.stream));
  });
}

int osc_corpus_compact(osc_corpus_handle h, int32_t* new_id_of_old_or_null, int64_t* N_new) {
  return corpus_guarded(h, [&](osc_corpus& c) {
    if (c.n_live == 0) throw Invalid("the corpus has no live rows");
    std::vector<int32_t> kept;
    const int64_t n = host::store_compact_map(c.live.data(), c.N, new_id_of_old_or_null, kept);
    if (N_new) *N_new = n;
    if (n == c.N) return;  // no tombstone: the rows stay where they are
    const size_t ldn = (size_t)c.ldn;
    const int64_t cap1 = host::store_capacity(0, n);
    std::vector<uint32_t> live((size_t)host::store_words(n), 0xffffffffu);
    live.back() = host::store_tail_mask(n);
    {
      DevBuf<float> Y1, Yn1;
      DevBuf<int32_t> d_kept;
      Y1.alloc((size_t)cap1 * ldn);
      Yn1.alloc((size_t)cap1 * ldn);
      d_kept.alloc((size_t)n);
      HIP_CHECK(hipMemcpyAsync(d_kept.p, kept.data(), (size_t)n * 4, hipMemcpyHostToDevice, c.stream));
      launch_cq_compact(c.Y.p, c.Yn.p, c.ldn, d_kept.p, n, Y1.p, Yn1.p, c.stream);
      HIP_CHECK(hipStreamSynchronize(c.stream));
      c.Y.swap(Y1);
      c.Yn.swap(Yn1);
    }
    c.cap = cap1;
    c.live.swap(live);
    c.d_live_current = false;
    c.N = c.n_live = n;
    c.filter = CorpusFilter{};  // (armed for ids that no longer exist)
    c.ragged = CorpusRagged{};
    c.settings.clear();
  });
}

int osc_corpus_filter(osc_corpus_handle h, const uint32_t* words, int32_t rows, int64_t words_per_row) {
  return corpus_guarded(h, [&](osc_corpus& c) {
    c.filter = CorpusFilter{};
    if (rows == 0) return;
    if (rows < 0 || !words) throw Invalid("osc_corpus_filter: need rows >= 0 and words != NULL");
    if (words_per_row != host::store_words(c.N))
      throw Invalid("osc_corpus_filter: words_per_row must be ceil(N / 32) = " + std::to_string(host::store_words(c.N)));
    c.filter.words.assign(words, words + (size_t)rows * words_per_row);
    c.filter.rows = rows;
    c.filter.words_per_row = words_per_row;
  });
}

int osc_corpus_ragged(osc_corpus_handle h, const int32_t* rows_or_null, int32_t Q) {
  return corpus_guarded(h, [&](osc_corpus& c) {
    c.ragged = CorpusRagged{};
    if (Q < 0) return;
    c.ragged.armed = true;
    if (rows_or_null) c.ragged.rows.assign(rows_or_null, rows_or_null + Q);
  });
}

int osc_corpus_settings(osc_corpus_handle h, const osc_corpus_setting* per_query, int32_t Q) {
  return corpus_guarded(h, [&](osc_corpus& c) {
    c.settings.clear();
    if (Q == 0 || !per_query) return;
    if (Q < 0) throw Invalid("osc_corpus_settings: need Q >= 0");
    const host::CorpusSetting* s = reinterpret_cast<const host::CorpusSetting*>(per_query);
    const char* what = nullptr;
    const int32_t bad = host::settings_first_bad(s, Q, &what);
    if (bad >= 0) throw Invalid("osc_corpus_settings: query " + std::to_string(bad) + ": " + what);
    c.settings.assign(s, s + Q);
  });
}

int osc_corpus_ragged_rows(osc_corpus_handle h, int32_t* rows, int32_t Q) {
  return corpus_guarded(h, [&](osc_corpus& c) {
    if (Q < 0 || (Q > 0 && !rows)) throw Invalid("osc_corpus_ragged_rows: need Q >= 0 and rows != NULL");
    if ((int64_t)c.last_rows.size() != Q) throw Invalid("osc_corpus_ragged_rows: the last ragged call had another Q");
    std::copy(c.last_rows.begin(), c.last_rows.end(), rows);
  });
}

}  // extern "C"

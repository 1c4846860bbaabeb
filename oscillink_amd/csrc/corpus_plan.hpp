// Chunk and offset arithmetic of the corpus refine path (osc_corpus_*).  HIP-free: osc_corpus.hip
// runs it, tests/host_logic/sweep_corpus_plan.cpp sweeps it under the sanitizers.
//
// A chunk of nq queries holds nq candidate lattices of K rows each, back to back (lattice q's rows start at q * K of the
// union).  Every per-chunk array is carved out of ONE scratch block at the offsets below, each 256-byte aligned.
#pragma once
#include <algorithm>
#include <cstdint>

namespace osc {
namespace host {

constexpr int64_t kCorpusBudgetBytes = (int64_t)1 << 30;  // scratch of one chunk
constexpr int32_t kCorpusMaxTopK = 1024;                  // K: one key per thread of the per-query select
constexpr int32_t kCorpusMaxKnn = 128;                    // k_knn_select's list length (the dense route)
constexpr int32_t kCorpusDefaultChunk = 256;              // queries per chunk without OSC_CORPUS_CHUNK

inline int32_t corpus_ldn(int32_t D) { return (D + 31) / 32 * 32; }      // row pitch of Y / Yn (the build's Yn pitch)
inline int32_t corpus_lds(int32_t K) { return (K + 31) / 32 * 32; }      // row pitch of a lattice's similarity matrix
inline int32_t corpus_knn(int32_t kneighbors, int32_t K) {               // lattice.py:60 for a K-row lattice
  return (int32_t)std::min<int64_t>(kneighbors, std::max<int64_t>(1, (int64_t)K - 1));
}
inline int64_t corpus_align(int64_t b) { return (b + 255) / 256 * 256; }

// byte offsets of the per-chunk arrays for nq lattices of K rows (k list entries per row, ldn-float rows, N corpus rows)
struct CorpusLayout {
  int64_t dots;              // float  [nq][N]     search: Yn psi^T, query-major
  int64_t cand;              // int32  [nq][K]     corpus ids, cosine descending
  int64_t ccos;              // float  [nq][K]
  int64_t Y, Yn;             // float  [nq K][ldn] gathered rows
  int64_t Sm;                // float  [nq K][lds] similarity matrices
  int64_t kval, kidx;        // float / int32 [nq K][k]
  int64_t col, adj, w;       // int32 / float / float [nq K][k] ELL of the union
  int64_t deg, sd, scale;    // int32 / float / float [nq K]
  int64_t X, R, P, AP;       // float  [nq K][ldn] the solve
  int64_t psi;               // float  [nq][ldn]
  int64_t qnorm;             // float  [nq]
  int64_t iters, res;        // int32 / float [nq]
  int64_t o_local, o_score, o_align;  // int32 / float / float [nq][kk]
  int64_t gates;             // float  [nq][K]     diffusion gates B (computed or given); after every older block, so
  int64_t g_iters, g_res;    // int32 / float [nq]  that those keep the offsets they had before gates existed
  int64_t total;
  // receipts (settle + receipt per lattice): behind g_res, and only when asked for -- all zero otherwise, total unchanged
  int64_t s_iters, s_res;    // int32 / float [nq]  the settle's iterations and residual
  int64_t r_sums;            // double [nq][4]      deltaH, coh_drop, anchor_pen, query_term
  int64_t n_total, n_kept;   // int32  [nq]         null points found / written (the cap)
  int64_t n_i, n_j, n_z, n_r;  // int32 / int32 / float / float [nq][null_slots] the kept null points, local ids
  // chains (a path prior and a chain receipt per lattice): behind everything above, and only when the call has chains --
  // all zero otherwise, total unchanged.  E = chain_cap, the largest edge count of the call's chains
  int64_t c_int;             // int32  [nq][chain_int_words(K, E)]  corpus_chain.hpp's int record
  int64_t c_flt;             // float  [nq][4 E]                    its float record
  int64_t c_edge;            // float  [nq][4][E]                   z_struct, z_path, r_struct, r_path per chain edge
  int64_t c_gain;            // double [nq]                         coherence gain
  int64_t c_verdict, c_weak_k;  // int32 [nq]
  int64_t c_weak_z;          // float  [nq]
};

// words of one query's chain records (corpus_chain.hpp packs them)
inline int64_t corpus_chain_int_words(int32_t K, int32_t cap) {
  return 2 + ((int64_t)cap + 1) + 2 * (int64_t)std::min(K, cap + 1) + 1 + 2 * (int64_t)cap;
}

// null-point slots per query of a receipts call: none in light detail, else K, or the cap when one is set
inline int32_t corpus_null_slots(int32_t K, bool full, int32_t null_cap) {
  if (!full) return 0;
  return null_cap > 0 ? std::min(null_cap, K) : K;
}

// receipts = false: the layout of a plain / gated refine (null_slots ignored).  receipts = true adds the receipts blocks,
// chain_cap > 0 the chain blocks.
inline CorpusLayout corpus_layout(int64_t N, int32_t ldn, int32_t K, int32_t k, int32_t kk, int32_t nq, bool receipts = false,
                                  int32_t null_slots = 0, int32_t chain_cap = 0) {
  CorpusLayout L{};
  const int64_t rows = (int64_t)nq * K, lds = corpus_lds(K);
  int64_t o = 0;
  auto take = [&](int64_t bytes) {
    const int64_t at = o;
    o += corpus_align(bytes);
    return at;
  };
  L.dots = take((int64_t)nq * N * 4);
  L.cand = take((int64_t)nq * K * 4);
  L.ccos = take((int64_t)nq * K * 4);
  L.Y = take(rows * ldn * 4);
  L.Yn = take(rows * ldn * 4);
  L.Sm = take(rows * lds * 4);
  L.kval = take(rows * k * 4);
  L.kidx = take(rows * k * 4);
  L.col = take(rows * k * 4);
  L.adj = take(rows * k * 4);
  L.w = take(rows * k * 4);
  L.deg = take(rows * 4);
  L.sd = take(rows * 4);
  L.scale = take(rows * 4);
  L.X = take(rows * ldn * 4);
  L.R = take(rows * ldn * 4);
  L.P = take(rows * ldn * 4);
  L.AP = take(rows * ldn * 4);
  L.psi = take((int64_t)nq * ldn * 4);
  L.qnorm = take((int64_t)nq * 4);
  L.iters = take((int64_t)nq * 4);
  L.res = take((int64_t)nq * 4);
  L.o_local = take((int64_t)nq * kk * 4);
  L.o_score = take((int64_t)nq * kk * 4);
  L.o_align = take((int64_t)nq * kk * 4);
  L.gates = take((int64_t)nq * K * 4);
  L.g_iters = take((int64_t)nq * 4);
  L.g_res = take((int64_t)nq * 4);
  if (receipts) {
    const int64_t slots = std::max<int64_t>(0, null_slots);
    L.s_iters = take((int64_t)nq * 4);
    L.s_res = take((int64_t)nq * 4);
    L.r_sums = take((int64_t)nq * 4 * 8);
    L.n_total = take((int64_t)nq * 4);
    L.n_kept = take((int64_t)nq * 4);
    L.n_i = take((int64_t)nq * slots * 4);
    L.n_j = take((int64_t)nq * slots * 4);
    L.n_z = take((int64_t)nq * slots * 4);
    L.n_r = take((int64_t)nq * slots * 4);
  }
  if (chain_cap > 0) {
    L.c_int = take((int64_t)nq * corpus_chain_int_words(K, chain_cap) * 4);
    L.c_flt = take((int64_t)nq * 4 * chain_cap * 4);
    L.c_edge = take((int64_t)nq * 4 * chain_cap * 4);
    L.c_gain = take((int64_t)nq * 8);
    L.c_verdict = take((int64_t)nq * 4);
    L.c_weak_k = take((int64_t)nq * 4);
    L.c_weak_z = take((int64_t)nq * 4);
  }
  L.total = o;
  return L;
}

// queries per chunk: the requested count (OSC_CORPUS_CHUNK, else kCorpusDefaultChunk), lowered until one chunk's scratch
// fits the budget; at least 1 (a single query over budget still runs: its scratch is what it is)
inline int32_t corpus_chunk(int64_t N, int32_t ldn, int32_t K, int32_t k, int32_t kk, int32_t requested, int64_t budget,
                            bool receipts = false, int32_t null_slots = 0, int32_t chain_cap = 0) {
  int32_t nq = std::max<int32_t>(1, requested);
  const int64_t one = corpus_layout(N, ldn, K, k, kk, 1, receipts, null_slots, chain_cap).total;
  const int64_t fit = std::max<int64_t>(1, budget / std::max<int64_t>(1, one));
  nq = (int32_t)std::min<int64_t>(nq, fit);
  while (nq > 1 && corpus_layout(N, ldn, K, k, kk, nq, receipts, null_slots, chain_cap).total > budget) --nq;
  return nq;
}

// the chunks of Q queries: [chunk_begin(c), chunk_begin(c) + chunk_size(c)), c < chunk_count
inline int32_t chunk_count(int32_t Q, int32_t nq) { return Q <= 0 ? 0 : (Q + nq - 1) / nq; }
inline int32_t chunk_begin(int32_t c, int32_t nq) { return c * nq; }
inline int32_t chunk_size(int32_t Q, int32_t c, int32_t nq) { return std::min(nq, Q - c * nq); }

}  // namespace host
}  // namespace osc

// Host arithmetic of a ragged corpus refine chunk (osc_corpus_ragged): candidate lattices of
// different sizes in one batch.  The reference's filtered loop (scripts/proof_hallucination.py:203-221) keeps whichever rows
// pass the filter and builds the lattice over len(idx_map) rows with kneighbors = min(k, len(idx_map) - 1); here lattice q has
// n_q rows, 1 <= n_q <= K, at the front of its K-row slot of the union.  HIP-free: osc_corpus.hip runs it,
// tests/host_logic/sweep_corpus_ragged.cpp sweeps it under the sanitizers.
#pragma once
#include <algorithm>
#include <cstdint>

namespace osc {
namespace host {

constexpr int32_t kRaggedPadId = -1;  // cand / local / list ids behind a lattice's rows; values there are 0

// rows of a lattice whose filter leaves `eligible` rows: min(K, eligible); 0 = no lattice (the call is rejected)
inline int32_t ragged_rows(int64_t eligible, int32_t K) {
  return (int32_t)std::min<int64_t>(std::max<int32_t>(K, 0), std::max<int64_t>(eligible, 0));
}

// neighbours per row of an n-row lattice (lattice.py:60 leaves 1 for n = 1, graph.py:30-32 then builds no edge: 0 here)
inline int32_t ragged_knn(int32_t kneighbors, int32_t n) {
  return n > 1 ? (int32_t)std::min<int64_t>(std::max(kneighbors, 0), (int64_t)n - 1) : 0;
}

// picks of bundle(kk) on an n-row lattice
inline int32_t ragged_picks(int32_t kk, int32_t n) { return std::max(0, std::min(kk, n)); }

// "k" of the state signature of an n-row lattice: min(kneighbors, max(1, n - 1)) (lattice.py:60)
inline int32_t ragged_sig_k(int32_t kneighbors, int32_t n) {
  return (int32_t)std::min<int64_t>(kneighbors, std::max<int64_t>(1, (int64_t)n - 1));
}

// the first query whose row count is outside [1, K], or -1
inline int32_t ragged_first_bad(const int32_t* rows, int32_t Q, int32_t K) {
  for (int32_t q = 0; q < Q; ++q)
    if (rows[q] < 1 || rows[q] > K) return q;
  return -1;
}

// true when every lattice fills its slot: the chunk is the uniform one and runs the uniform kernels
inline bool ragged_is_uniform(const int32_t* rows, int32_t Q, int32_t K) {
  for (int32_t q = 0; q < Q; ++q)
    if (rows[q] != K) return false;
  return true;
}

// a candidate row of K entries, real ids in front and kRaggedPadId behind them: the count of real ids, or -1 when a negative
// entry is followed by a real id (or a negative entry is not the pad id)
inline int32_t ragged_lead(const int32_t* row, int32_t K) {
  int32_t n = 0;
  while (n < K && row[n] >= 0) ++n;
  for (int32_t t = n; t < K; ++t)
    if (row[t] != kRaggedPadId) return -1;
  return n;
}

// union row of local row r of lattice q, and the first entry of its k-wide list: functions of K, not of the row counts
inline int64_t ragged_row(int32_t q, int32_t r, int32_t K) { return (int64_t)q * K + r; }
inline int64_t ragged_list_at(int32_t q, int32_t r, int32_t K, int32_t k) { return ragged_row(q, r, K) * k; }

// dst[0 .. n) = src[0 .. n), dst[n .. K) = fill
template <class T>
inline void ragged_copy_padded(const T* src, int32_t n, int32_t K, T fill, T* dst) {
  const int32_t m = std::max(0, std::min(n, K));
  std::copy(src, src + m, dst);
  std::fill(dst + m, dst + std::max(K, 0), fill);
}

}  // namespace host
}  // namespace osc

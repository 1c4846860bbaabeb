// Host arithmetic of a corpus refine call with per-query settings (osc_corpus_settings).  The
// reference carries the operator and solver settings per request (cloud/app/models.py:8-23, cloud/app/main.py:887-947),
// overrides them per API key and jitters them per request (cloud/app/learners.py:148-192), and sweeps them per query
// (scripts/benchmark_adaptive.py:186-232); here query q of a batch has its own record, and a chunk is sized by the
// records' maxima.  HIP-free: osc_corpus.hip runs it, tests/host_logic/sweep_corpus_settings.cpp sweeps it under the
// sanitizers.  The record is also what the per-lattice kernels read (corpus_pcg.hpp), one per lattice of a chunk.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "corpus_plan.hpp"
#include "corpus_ragged.hpp"

namespace osc {
namespace host {

// one query's settings: the layout of osc_corpus_setting (include/oscillink_hip.h)
struct CorpusSetting {
  float lamG, lamC, lamQ, lamP, alpha, settle_dt, settle_tol;
  int32_t kneighbors, k, settle_max_iters;
};
static_assert(sizeof(CorpusSetting) == 40, "seven floats and three int32, no padding");

// the scalar arguments' own checks on one record: nullptr, or what is wrong with it
inline const char* setting_error(const CorpusSetting& s) {
  if (!(s.lamG > 0.f)) return "lamG must be > 0 for SPD";
  if (!(s.lamC >= 0.f) || !std::isfinite(s.lamC)) return "lamC must be >= 0 and finite";
  if (!(s.lamQ >= 0.f) || !std::isfinite(s.lamQ)) return "lamQ must be >= 0 and finite";
  if (!(s.lamP >= 0.f) || !std::isfinite(s.lamP)) return "lamP must be >= 0 and finite";
  if (s.kneighbors < 1) return "kneighbors must be >= 1";
  if (!(s.settle_dt > 0.f) || !std::isfinite(s.settle_dt)) return "settle_dt must be finite and > 0";
  if (s.settle_max_iters < 1) return "settle_max_iters must be >= 1";
  if (!std::isfinite(s.settle_tol)) return "settle_tol must be finite";
  if (!std::isfinite(s.alpha)) return "alpha must be finite";
  return nullptr;
}

// the first query whose record fails setting_error (its text in *what), or -1
inline int32_t settings_first_bad(const CorpusSetting* s, int32_t Q, const char** what) {
  for (int32_t q = 0; q < Q; ++q)
    if (const char* e = setting_error(s[q])) {
      if (what) *what = e;
      return q;
    }
  return -1;
}

// the first query whose list would be longer than the dense route's (min(kneighbors, K - 1) > 128), or -1
inline int32_t settings_first_long_list(const CorpusSetting* s, int32_t Q, int32_t K) {
  for (int32_t q = 0; q < Q; ++q)
    if (K > 1 && corpus_knn(s[q].kneighbors, K) > kCorpusMaxKnn) return q;
  return -1;
}

// the record lattice q runs under: n = its rows (K when the call is not ragged).  kneighbors becomes the list length
// min(kneighbors, n - 1) (0 for a one-row lattice), k the picks' bound min(k, K) (the bundle takes min(k, n) of them);
// everything else is the query's own
inline CorpusSetting setting_effective(const CorpusSetting& s, int32_t n, int32_t K) {
  CorpusSetting e = s;
  e.kneighbors = ragged_knn(s.kneighbors, n);
  e.k = std::min(std::max(s.k, 0), std::max(K, 0));
  return e;
}
inline int32_t setting_picks(const CorpusSetting& effective, int32_t n) { return ragged_picks(effective.k, n); }
// "k" of the state signature of query q's n-row lattice
inline int32_t setting_sig_k(const CorpusSetting& s, int32_t n) { return ragged_sig_k(s.kneighbors, n); }

// the maxima that size corpus_layout and chunk_for: the ELL and list width, and the output width
inline int32_t settings_max_knn(const CorpusSetting* effective, int32_t Q) {
  int32_t m = 0;
  for (int32_t q = 0; q < Q; ++q) m = std::max(m, effective[q].kneighbors);
  return m;
}
inline int32_t settings_max_kk(const CorpusSetting* effective, int32_t Q) {
  int32_t m = 0;
  for (int32_t q = 0; q < Q; ++q) m = std::max(m, effective[q].k);
  return m;
}

// the records of chunk [q0, q0 + nq) of Q: their first one, or nullptr when the range does not lie inside [0, Q)
inline const CorpusSetting* settings_slice(const CorpusSetting* s, int32_t Q, int32_t q0, int32_t nq) {
  if (!s || q0 < 0 || nq < 0 || (int64_t)q0 + nq > Q) return nullptr;
  return s + q0;
}

}  // namespace host
}  // namespace osc

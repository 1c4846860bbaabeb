// Row-store arithmetic of a mutable corpus (osc_corpus_append / _remove / _compact / _filter).
// HIP-free: osc_corpus.hip runs it, tests/host_logic/sweep_corpus_store.cpp sweeps it under the sanitizers.
//
// Rows are named by position.  A bitmap of uint32 words says which rows are live: bit i & 31 of word i >> 5 for row i,
// 1 = live, zero bits beyond N.  A filter (allow) has the same form, one row of words for all queries or one per query.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace osc {
namespace host {

constexpr int64_t kCorpusMaxRows = ((int64_t)1 << 31) - 1;  // ids are int32
constexpr int64_t kCorpusCapStep = 128;                     // capacities are whole GEMM row tiles

inline int64_t store_words(int64_t n) { return (n + 31) / 32; }
// the bits of the last word that name rows below n (all of them when n is a multiple of 32; 0 for n = 0)
inline uint32_t store_tail_mask(int64_t n) {
  if (n <= 0) return 0u;
  const int r = (int)(n & 31);
  return r == 0 ? 0xffffffffu : (1u << r) - 1u;
}
inline bool store_get(const uint32_t* w, int64_t i) { return (w[i >> 5] >> (i & 31)) & 1u; }
inline void store_set(uint32_t* w, int64_t i) { w[i >> 5] |= 1u << (i & 31); }
inline void store_clear(uint32_t* w, int64_t i) { w[i >> 5] &= ~(1u << (i & 31)); }

// rows to allocate so that `need` fit when `cap` are allocated: max(need, cap + cap / 2) rounded up to 128 rows.  -1 when
// need is not a row count a corpus can have (ids are int32).  The result may pass 2^31 - 1 by the rounding: it counts
// allocated rows, not ids.
inline int64_t store_capacity(int64_t cap, int64_t need) {
  if (need < 0 || need > kCorpusMaxRows || cap < 0) return -1;
  const int64_t want = std::max(need, cap + cap / 2);  // cap <= 2^31 here: no overflow in int64
  const int64_t top = (kCorpusMaxRows + kCorpusCapStep) / kCorpusCapStep * kCorpusCapStep;
  return std::min(top, (want + kCorpusCapStep - 1) / kCorpusCapStep * kCorpusCapStep);
}

inline int32_t store_popcount(uint32_t v) {
  v = v - ((v >> 1) & 0x55555555u);
  v = (v & 0x33333333u) + ((v >> 2) & 0x33333333u);
  return (int32_t)((((v + (v >> 4)) & 0x0f0f0f0fu) * 0x01010101u) >> 24);
}

// rows below n that are live and allowed (allow == nullptr: every row is allowed)
inline int64_t store_count(const uint32_t* live, const uint32_t* allow, int64_t n) {
  const int64_t nw = store_words(n);
  int64_t c = 0;
  for (int64_t w = 0; w < nw; ++w) {
    uint32_t v = live[w] & (allow ? allow[w] : 0xffffffffu);
    if (w == nw - 1) v &= store_tail_mask(n);
    c += store_popcount(v);
  }
  return c;
}

// compaction: the live rows in order (kept), and per old row its new id or -1 (new_id_of_old may be nullptr); returns the
// number kept
inline int64_t store_compact_map(const uint32_t* live, int64_t n, int32_t* new_id_of_old, std::vector<int32_t>& kept) {
  kept.clear();
  for (int64_t i = 0; i < n; ++i) {
    const bool on = store_get(live, i);
    if (new_id_of_old) new_id_of_old[i] = on ? (int32_t)kept.size() : -1;
    if (on) kept.push_back((int32_t)i);
  }
  return (int64_t)kept.size();
}

}  // namespace host
}  // namespace osc

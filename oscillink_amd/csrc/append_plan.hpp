// The route and the sizes of osc_create_appended, and what the three builds seeded from a base's kept
// lists share (append, remove, update): the eligibility checks, the threshold, the query list and its
// chunks.  HIP-free: osc_graph.hip / osc_api.hip run it, tests/host_logic/sweep_append_plan.cpp and sweep_update_plan.cpp
// sweep it under the sanitizers.
//
// An appended lattice holds the N rows of a base lattice followed by M new ones.  Its top-k lists are either built from
// scratch (route rebuild) or grown from the base's kept lists (route incremental): the new rows -- and the old rows whose
// lists cannot be merged, the redo set -- are scored against all N + M columns in chunks of query rows, each chunk's k best
// are selected, and every other old row scans its column of the chunk's score block for new columns that beat its worst
// member.  All sizes are int64 here; a row or column id is int32.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace osc {
namespace host {

constexpr int32_t kAppendRowTile = 128;   // query rows of one MFMA score tile: chunks are whole tiles
constexpr int32_t kAppendListMax = 128;   // longest list the merge kernel and the register-resident routes hold
constexpr int32_t kAppendBflyMaxLdn = 1536;  // widest unit row the butterfly score kernels keep in registers (6 x 256 floats)
constexpr int64_t kAppendMaxRows = ((int64_t)1 << 31) - 1;  // N + M: ids are int32
constexpr int64_t kAppendScratchBytes = (int64_t)1 << 30;   // budget of one chunk's score block

// Which arithmetic a handle's list values come from: the two are not bit-identical, so a list never mixes them.
//   mfma      : fp32 MFMA tiles (k_knn_dense, knn_topk_body: the dense, exact and any-k routes)
//   butterfly : per-lane fma chains + a wave butterfly (k_knn_rescore, k_rows_scores: the tile and panel routes)
enum AppendFamily : int32_t { kFamilyNone = 0, kFamilyMfma = 1, kFamilyButterfly = 2 };

enum AppendRoute : int32_t { kRouteNone = 0, kRouteIncremental = 1, kRouteRebuild = 2 };

// Why a base cannot seed an incremental build (0: it can)
enum AppendDenied : int32_t {
  kAppendOk = 0,
  kAppendNoLists,      // no kept lists: an injected graph (osc_set_csr), N <= 1, or never built
  kAppendComm,         // a communicator is attached
  kAppendKChanges,     // min(k requested, N + M - 1) differs from the lists' length
  kAppendKTooLong,     // k > 128
  kAppendTooManyRows,  // N + M >= 2^31
  kAppendWideRows,     // butterfly family with unit rows wider than the score kernel's registers
  kAppendMixedLists,   // butterfly family whose build sent rows to the MFMA kernel (more than 32 fallback rows)
  kAppendSlower,       // eligible, but the planner expects the rebuild to be no slower (auto mode only)
  kRemoveTooFewRows,   // fewer than two rows are left (only a removal gets there; remove_plan.hpp has its text)
};

inline const char* append_denied_text(int32_t why) {
  switch (why) {
    case kAppendOk: return "";
    case kAppendNoLists: return "the base lattice keeps no kNN lists (an injected graph, a lattice never built, or fewer than two rows)";
    case kAppendComm: return "the base lattice has a communicator";
    case kAppendKChanges: return "the effective k changes with the new row count";
    case kAppendKTooLong: return "k > 128";
    case kAppendTooManyRows: return "N + M >= 2^31";
    case kAppendWideRows: return "butterfly-scored lists with rows wider than 1536 columns";
    case kAppendMixedLists: return "the base's build redid more than 32 rows with the MFMA kernel: its lists mix score families";
    case kAppendSlower: return "the rebuild is expected to be no slower";
    default: return "unknown";
  }
}

struct SeedInputs {
  int64_t N = 0, M = 0;       // rows of the base; rows appended, distinct rows removed, rows replaced
  int32_t D = 0;
  int32_t k_requested = 0;    // k as asked for at the base's creation
  int32_t knn_k = 0;          // length of the base's kept lists (0: none)
  int32_t family = kFamilyNone;
  int32_t fallback_rows = 0;  // rows the base's prefilter build handed to its fallback
  bool comm = false;
};
using AppendInputs = SeedInputs;

inline int64_t append_ldn(int32_t D) { return (((int64_t)D + 31) / 32) * 32; }  // pitch of the unit rows (int64: D near 2^31)
inline int64_t append_lds(int64_t cols) { return ((cols + 31) / 32) * 32; }               // pitch of a score block's rows
inline int32_t append_k_eff(int32_t k_requested, int64_t rows) {
  return (int32_t)std::min<int64_t>(k_requested, std::max<int64_t>(1, rows - 1));
}

// What every seeded build asks of its base, sizes aside: `rows_after` rows stand in the lattice afterwards
inline int32_t seed_eligible(const SeedInputs& in, int64_t rows_after) {
  if (in.knn_k <= 0 || in.family == kFamilyNone || in.N < 2) return kAppendNoLists;
  if (in.comm) return kAppendComm;
  if (rows_after < 2) return kRemoveTooFewRows;
  if (append_k_eff(in.k_requested, rows_after) != in.knn_k) return kAppendKChanges;
  if (in.knn_k > kAppendListMax) return kAppendKTooLong;
  if (in.family == kFamilyButterfly && append_ldn(in.D) > kAppendBflyMaxLdn) return kAppendWideRows;
  if (in.family == kFamilyButterfly && in.fallback_rows > 32) return kAppendMixedLists;
  return kAppendOk;
}

// Eligibility of the incremental route, thresholds aside (they need the redo count, which the device computes)
inline int32_t append_eligible(const AppendInputs& in) {
  if (in.N < 0 || in.M < 0 || in.N + in.M > kAppendMaxRows) return kAppendTooManyRows;  // (int64: no overflow below 2^63)
  return seed_eligible(in, in.N + in.M);
}

// The thresholds of the automatic route, from scripts/bench_append.py on an MI355X (DESIGN.md section 14 has the table).  The
// incremental build costs the new handle, the back half and the score block of its redo + M query rows; the rebuild
// costs a whole build.
//   butterfly: a query row against N columns costs ~0.06 us per 1000 pairs whatever the width (the butterfly, not the fma
//     chain, is the bound).  100 000 x 768, k 32: incremental 6.4 ms + 6.3 us per query row (12.79 ms at 1024) against a
//     17.1 ms rebuild, they cross at q ~ 1700 = N / 60; 1M x 384, k 16: 26-40 ms + 73 us per row (109 ms at 1024) against
//     435 ms, q ~ 5300 = N / 190.  N / 256 keeps a margin at both.
//   mfma (8000 x 64, k 16, dense route): the score block is cheap, the merge scan of a small lattice is latency-bound
//     (8000 threads): 0.46 against 0.65 ms at q = 256, 1.14 against 0.66 ms at q = 2048; they cross near N / 12.  N / 32.
inline int64_t append_max_query_rows(int32_t family, int64_t rows) {
  if (family == kFamilyMfma) return std::max<int64_t>(32, rows / 32);
  return std::max<int64_t>(32, rows / 256);
}
inline bool seed_pays(int32_t family, int64_t rows_after, int64_t query_rows) {
  return query_rows <= append_max_query_rows(family, rows_after);
}
inline bool append_pays(int32_t family, int64_t N, int64_t M, int64_t redo) { return seed_pays(family, N + M, redo + M); }

// Query rows of one chunk: as many as fit the scratch budget, whole 128-row tiles, at least one tile.  `cols` = N + M.
inline int64_t append_chunk_rows(int64_t cols, int64_t budget_bytes = kAppendScratchBytes) {
  const int64_t lds = append_lds(std::max<int64_t>(1, cols));
  const int64_t fit = budget_bytes / (lds * 4);
  return std::max<int64_t>(kAppendRowTile, fit / kAppendRowTile * kAppendRowTile);
}
inline int64_t append_chunk_count(int64_t query_rows, int64_t chunk) {
  return query_rows <= 0 ? 0 : (query_rows + chunk - 1) / chunk;
}
// chunk c covers query rows [begin, end)
inline void append_chunk_range(int64_t query_rows, int64_t chunk, int64_t c, int64_t& begin, int64_t& end) {
  begin = std::min(query_rows, c * chunk);
  end = std::min(query_rows, begin + chunk);
}
// floats of the score block a build allocates (one chunk's rows, or all query rows when they are fewer)
inline int64_t append_scratch_floats(int64_t query_rows, int64_t cols, int64_t budget_bytes = kAppendScratchBytes) {
  const int64_t rows = std::min(std::max<int64_t>(1, query_rows), append_chunk_rows(cols, budget_bytes));
  return rows * append_lds(std::max<int64_t>(1, cols));
}
// The query list of a seeded build: the flagged rows that are not fresh in ascending order, then the fresh rows (the
// appended rows, none, the replaced rows; ascending as given).  `flagged` is in any order (the device's).
inline std::vector<int32_t> seed_query_list(const std::vector<int32_t>& flagged, const std::vector<int32_t>& fresh) {
  std::vector<int32_t> q;
  q.reserve(flagged.size() + fresh.size());
  for (int32_t r : flagged)
    if (!std::binary_search(fresh.begin(), fresh.end(), r)) q.push_back(r);
  std::sort(q.begin(), q.end());
  q.insert(q.end(), fresh.begin(), fresh.end());
  return q;
}
// The part of a chunk [begin, end) of that list that holds FRESH rows, `redo` other rows standing before them: query rows
// [nb, ne) of the chunk-local block, which score the columns named by entries [begin + nb, begin + ne) of the list.
inline void seed_chunk_fresh_part(int64_t redo, int64_t begin, int64_t end, int64_t& nb, int64_t& ne) {
  nb = std::min(end, std::max(begin, redo)) - begin;
  ne = end - begin;
}

}  // namespace host
}  // namespace osc

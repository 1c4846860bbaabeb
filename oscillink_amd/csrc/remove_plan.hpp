// The route and the sizes of osc_create_removed.  HIP-free: osc_graph.hip / osc_api.hip run it,
// tests/host_logic/sweep_remove_plan.cpp sweeps it under the sanitizers.
//
// A removed lattice holds the N' = N - M rows of a base lattice that an id list does not name, renumbered densely in
// order.  Its top-k lists are either built from scratch (route rebuild) or shrunk from the base's kept lists (route
// incremental): a kept row whose list names no removed row keeps it with the ids renumbered -- the renumbering is
// monotone, so (score desc, index asc) and every tie decision survive it -- and the rows that lost a member, the redo set,
// are scored against all N' columns in chunks of query rows like an appended build's redo rows.  There is no merge pass:
// no column is new.  The enums, pitches, chunk arithmetic, shared eligibility checks (seed_eligible) and thresholds are
// append_plan.hpp's.
#pragma once
#include "append_plan.hpp"

namespace osc {
namespace host {

// Why a base cannot seed an incremental removal: AppendDenied's codes, the last of them (kRemoveTooFewRows) its own
inline const char* remove_denied_text(int32_t why) {
  if (why == kRemoveTooFewRows) return "fewer than two rows are left";
  if (why == kAppendKChanges) return "the effective k changes with the new row count";
  if (why == kAppendTooManyRows) return "N >= 2^31";
  return append_denied_text(why);
}

// What is wrong with an id list (0: nothing)
enum RemoveIdError : int32_t { kRemoveIdsOk = 0, kRemoveIdOutOfRange = 1, kRemoveAllRows = 2, kRemoveBadSizes = 3 };

// Rows left after M distinct rows leave N (sizes only; -1: not a removal that leaves a lattice)
inline int64_t remove_rows_left(int64_t N, int64_t M) { return (N < 1 || M < 0 || M >= N) ? -1 : N - M; }

// The map of a removal from an id list of any order, duplicates allowed: new_id_of_old[i] = the row's id among the kept
// rows (dense, in order), -1 for a removed row.  `new_id_of_old` has N entries; nothing is written past them, and on
// kRemoveIdOutOfRange / kRemoveBadSizes its content is unspecified.  *M: distinct ids named.
template <typename Id>
inline int32_t remove_map(const Id* ids, int64_t n, int64_t N, int32_t* new_id_of_old, int64_t* M) {
  if (M) *M = 0;
  if (N < 1 || N > kAppendMaxRows || n < 0 || (n > 0 && ids == nullptr) || new_id_of_old == nullptr) return kRemoveBadSizes;
  for (int64_t i = 0; i < N; ++i) new_id_of_old[i] = 0;
  int64_t m = 0;
  for (int64_t j = 0; j < n; ++j) {
    const int64_t id = (int64_t)ids[j];
    if (id < 0 || id >= N) return kRemoveIdOutOfRange;
    if (new_id_of_old[id] == 0) new_id_of_old[id] = -1, ++m;
  }
  int32_t next = 0;
  for (int64_t i = 0; i < N; ++i) new_id_of_old[i] = new_id_of_old[i] < 0 ? -1 : next++;
  if (M) *M = m;
  return m >= N ? kRemoveAllRows : kRemoveIdsOk;
}

// old_of_new[new_id_of_old[i]] = i for the kept rows (N - M entries)
inline void remove_inverse(const int32_t* new_id_of_old, int64_t N, int32_t* old_of_new) {
  for (int64_t i = 0; i < N; ++i)
    if (new_id_of_old[i] >= 0) old_of_new[new_id_of_old[i]] = (int32_t)i;
}

using RemoveInputs = SeedInputs;  // (M: distinct rows removed)

// Eligibility of the incremental route, the threshold aside (it needs the redo count, which the device computes)
inline int32_t remove_eligible(const RemoveInputs& in) {
  if (in.N < 0 || in.M < 0 || in.N > kAppendMaxRows) return kAppendTooManyRows;
  return seed_eligible(in, remove_rows_left(in.N, in.M));
}

// The threshold of the automatic route.  The incremental removal costs the new handle, the list pass, the back half and
// the score block of its redo rows (about k M of them): an appended build's cost without the merge scan, with the same
// score kernels per query row, so the cap is append_max_query_rows.  scripts/bench_remove.py on an MI355X confirmed it
// (DESIGN.md section 15 has the table; both routes in one process, medians of 20):
//   butterfly, 100 000 x 768, k 32: 6.5 ms + 6.8 us per redo row (6.73 ms at 33, 8.45 at 279, 13.61 at 1049) against a 16.9 ms rebuild,
//     they cross at redo ~ 1500 = N / 66; 1M x 384, k 16: 21-40 ms + 77 us per row (202.5 ms at 2126) against 402 ms,
//     redo ~ 5000 = N / 200.  N / 256 keeps a margin at both, as it does for append.
//   mfma (8000 x 64, k 16): 0.34-0.36 ms from 14 to 473 redo rows against 0.46 ms: no crossing up to N / 17.  N / 32.
inline int64_t remove_max_query_rows(int32_t family, int64_t rows_left) { return append_max_query_rows(family, rows_left); }
inline bool remove_pays(int32_t family, int64_t rows_left, int64_t redo) { return seed_pays(family, rows_left, redo); }

}  // namespace host
}  // namespace osc

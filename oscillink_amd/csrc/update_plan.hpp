// The route and the sizes of osc_create_updated.  HIP-free: osc_graph.hip / osc_api.hip run it,
// tests/host_logic/sweep_update_plan.cpp sweeps it under the sanitizers.
//
// An updated lattice holds the N rows of a base lattice with M of them, named by distinct ids, replaced by new vectors.
// No row moves and N does not change.  Its top-k lists are either built from scratch (route rebuild) or taken from the
// base's kept lists (route incremental): a row whose list names no replaced row keeps it; the rows that lost a member (the
// redo set) and the replaced rows themselves are scored against all N columns in chunks of query rows, like an appended
// build's redo rows and new rows; every other row scans its column of the replaced rows' score block for replaced columns
// that now precede its worst member.  Unlike an appended column a replaced column's index can be BELOW a member's, so an
// equal score can win there (update_kernels.hip: k_update_merge).  The enums, pitches, chunk arithmetic, shared
// eligibility checks (seed_eligible), query list and thresholds are append_plan.hpp's.
#pragma once
#include "append_plan.hpp"

namespace osc {
namespace host {

// What is wrong with an id list (0: nothing)
enum UpdateIdError : int32_t { kUpdateIdsOk = 0, kUpdateIdOutOfRange = 1, kUpdateIdDuplicate = 2, kUpdateBadSizes = 3 };

// The map of an update from an id list of any order: keep[i] = i for a row that stays as it is, -1 for a replaced row
// (k_update_lists sends every list member through it).  `keep` has N entries; nothing is written past them, and on an
// error its content is unspecified.  The range check is made in int64 whatever Id is; an id named twice is an error of
// its own (there is no single meaning for which of two new rows wins).
template <typename Id>
inline int32_t update_ids(const Id* ids, int64_t n, int64_t N, int32_t* keep) {
  if (N < 1 || N > kAppendMaxRows || n < 0 || (n > 0 && ids == nullptr) || keep == nullptr) return kUpdateBadSizes;
  for (int64_t i = 0; i < N; ++i) keep[i] = (int32_t)i;
  for (int64_t j = 0; j < n; ++j) {
    const int64_t id = (int64_t)ids[j];
    if (id < 0 || id >= N) return kUpdateIdOutOfRange;
    if (keep[id] < 0) return kUpdateIdDuplicate;
    keep[id] = -1;
  }
  return kUpdateIdsOk;
}

using UpdateInputs = SeedInputs;  // (M: rows replaced)

// Eligibility of the incremental route, the threshold aside (it needs the redo count, which the device computes)
inline int32_t update_eligible(const UpdateInputs& in) {
  if (in.N < 0 || in.M < 0 || in.M > in.N || in.N > kAppendMaxRows) return kAppendTooManyRows;
  return seed_eligible(in, in.N);  // (k changes: a rebuild with another k came between)
}

// The threshold of the automatic route.  The incremental update costs the new handle, the list pass, the back half, the
// score block of its query rows -- the `redo` rows that lost a member (about k M of them) and the M replaced rows -- and
// the merge scan of the replaced rows' part of that block: an appended build of M rows whose redo set is a removal's.  The
// cap therefore is append_max_query_rows over redo + M, append's meaning of the sum.  scripts/bench_update.py on an MI355X
// confirmed it: in seven of the eight rows where auto takes the incremental route its interval lay below the rebuild's at
// once, in the eighth when the row was measured a second time (DESIGN.md section 16 has the table; all routes in one
// process, medians of 20, [min, max]):
//   butterfly, 100 000 x 768, k 32: 6.5 ms + 6.7 us per query row (6.75 ms at M = 1 / 34 query rows, 8.37 at 8 / 287, 13.54
//     at 32 / 1081) against a 16.4 ms rebuild, they cross near 1500 query rows = N / 66; 1M x 384, k 16: 21-40 ms + 77 us per
//     row (200 ms [188, 210] at M = 128 / 2254 rows) against 385 ms [384, 387], crossing near 4600 = N / 220.  N / 256 keeps a
//     margin at both, as it does for append and remove; auto took route 1 in six of these rows and its interval lay below
//     the rebuild's in all six.
//   mfma (8000 x 64, k 16): 0.36 ms at M = 1 and 8 (15 and 125 query rows) against 0.47 and 0.46 ms; 0.42 against 0.46 at
//     M = 32 (505 rows, above the cap of 250: auto rebuilds), 0.61 against 0.49 at M = 128 (1939 rows).  They cross near
//     N / 8.  N / 32.  At M = 1 auto's interval [0.34, 0.37] lies below the rebuild's [0.46, 0.60]; at M = 8 the medians are
//     as far apart but the intervals touch, [0.34, 0.48] against [0.45, 0.59]: every form of that row, the fresh create
//     included, has one call about 0.12 ms above the rest.  The same two rows again, in a later session: [0.35, 0.38]
//     against [0.47, 0.50] and [0.38, 0.40] against [0.47, 0.50].
//   The merge scan is 0.05-0.5 ms of any of these; one replaced row costs what one removed row costs (6.75 against 6.73 ms).
inline int64_t update_max_query_rows(int32_t family, int64_t N) { return append_max_query_rows(family, N); }
inline bool update_pays(int32_t family, int64_t N, int64_t M, int64_t redo) { return seed_pays(family, N, redo + M); }

}  // namespace host
}  // namespace osc

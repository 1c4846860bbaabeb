// Sweep of remove_plan.hpp (the route and sizes of osc_create_removed): the id normalisation against a brute-force map
// (duplicates, any order, extremes, n = 0, ids at 0 and N - 1, int32 and int64 ids), sizes near 2^31 without arrays, the
// eligibility table row by row, and the chunks of the redo list at cols = N'.  Run under -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../oscillink_amd/csrc/remove_plan.hpp"

using namespace osc::host;

static int fail(const char* what, long long a, long long b) {
  std::printf("ERROR %s (%lld, %lld)\n", what, a, b);
  return 1;
}

static RemoveInputs base_inputs() {
  RemoveInputs in;
  in.N = 1000;
  in.M = 10;
  in.D = 64;
  in.k_requested = 16;
  in.knn_k = 16;
  in.family = kFamilyMfma;
  return in;
}

// the map by the definition: a row's new id is the number of kept rows before it
template <typename Id>
static int check_map(const std::vector<Id>& ids, long long N, int expect) {
  std::vector<int32_t> map((size_t)N + 2, 12345);  // one guard entry on each side
  int64_t M = -7;
  const int32_t rc = remove_map(ids.empty() ? (const Id*)nullptr : ids.data(), (int64_t)ids.size(), N, map.data() + 1, &M);
  if (map[0] != 12345 || map[(size_t)N + 1] != 12345) return fail("map wrote outside its N entries", N, (long long)ids.size());
  if (rc != expect) return fail("map status", rc, expect);
  if (rc == kRemoveIdOutOfRange) return 0;
  std::vector<char> gone((size_t)N, 0);
  for (Id id : ids) gone[(size_t)id] = 1;
  long long kept = 0, m = 0;
  for (long long i = 0; i < N; ++i) {
    const int32_t want = gone[(size_t)i] ? -1 : (int32_t)kept;
    if (map[(size_t)i + 1] != want) return fail("map entry", i, map[(size_t)i + 1]);
    kept += !gone[(size_t)i];
    m += gone[(size_t)i];
  }
  if (M != m) return fail("distinct count", M, m);
  if (remove_rows_left(N, M) != (m < N ? N - m : -1)) return fail("rows left", N, M);
  if (m < N) {
    std::vector<int32_t> inv((size_t)(N - m) + 1, 777);
    remove_inverse(map.data() + 1, N, inv.data());
    if (inv[(size_t)(N - m)] != 777) return fail("inverse wrote past its N - M entries", N, m);
    for (long long j = 0; j < N - m; ++j) {
      if (inv[(size_t)j] < 0 || inv[(size_t)j] >= N || map[(size_t)inv[(size_t)j] + 1] != j) return fail("inverse", j, inv[(size_t)j]);
      if (j > 0 && inv[(size_t)j] <= inv[(size_t)j - 1]) return fail("inverse not monotone", j, inv[(size_t)j]);
    }
  }
  return 0;
}

int main() {
  long long cases = 0;
  // ---- the id map ----
  for (long long N : {1LL, 2LL, 3LL, 17LL, 128LL, 129LL, 1000LL}) {
    if (check_map<int32_t>({}, N, kRemoveIdsOk)) return 1;  // n = 0: the identity
    if (check_map<int32_t>({0}, N, N == 1 ? kRemoveAllRows : kRemoveIdsOk)) return 1;
    if (check_map<int32_t>({(int32_t)(N - 1)}, N, N == 1 ? kRemoveAllRows : kRemoveIdsOk)) return 1;
    if (check_map<int64_t>({0, N - 1, 0, N - 1}, N, N <= 2 ? kRemoveAllRows : kRemoveIdsOk)) return 1;
    if (check_map<int32_t>({(int32_t)N}, N, kRemoveIdOutOfRange)) return 1;
    if (check_map<int32_t>({-1}, N, kRemoveIdOutOfRange)) return 1;
    if (check_map<int32_t>({0, INT32_MAX}, N, kRemoveIdOutOfRange)) return 1;
    if (check_map<int32_t>({0, INT32_MIN}, N, kRemoveIdOutOfRange)) return 1;
    if (check_map<int64_t>({INT64_MAX}, N, kRemoveIdOutOfRange)) return 1;
    if (check_map<int64_t>({INT64_MIN}, N, kRemoveIdOutOfRange)) return 1;
    if (check_map<int64_t>({N + ((int64_t)1 << 32)}, N, kRemoveIdOutOfRange)) return 1;  // (no truncation to int32)
    std::vector<int32_t> all;
    for (long long i = N - 1; i >= 0; --i) all.push_back((int32_t)i), all.push_back((int32_t)i);
    if (check_map(all, N, kRemoveAllRows)) return 1;
    cases += 12;
    unsigned long long x = 88172645463325252ULL + (unsigned long long)N;  // xorshift: random lists, unsorted, with duplicates
    for (int rep = 0; rep < 40; ++rep) {
      std::vector<int32_t> ids;
      const long long n = (long long)(rep * 7) % (2 * N + 1);
      for (long long j = 0; j < n; ++j) {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        ids.push_back((int32_t)(x % (unsigned long long)N));
      }
      std::vector<char> seen((size_t)N, 0);
      long long m = 0;
      for (int32_t id : ids) m += !seen[(size_t)id], seen[(size_t)id] = 1;
      if (check_map(ids, N, m == N ? kRemoveAllRows : kRemoveIdsOk)) return 1;
      ++cases;
    }
  }
  {  // bad sizes never touch the arrays
    int32_t one = 5;
    int64_t M = 3;
    const int32_t id = 0;
    if (remove_map(&id, 1, 0, &one, &M) != kRemoveBadSizes || one != 5 || M != 0) return fail("N = 0", 0, 0);
    if (remove_map(&id, -1, 1, &one, &M) != kRemoveBadSizes || one != 5) return fail("n < 0", 0, 0);
    if (remove_map((const int32_t*)nullptr, 1, 1, &one, &M) != kRemoveBadSizes || one != 5) return fail("null ids", 0, 0);
    if (remove_map(&id, 1, (int64_t)kAppendMaxRows + 1, &one, &M) != kRemoveBadSizes || one != 5) return fail("N = 2^31", 0, 0);
    if (remove_map(&id, 1, 1, (int32_t*)nullptr, &M) != kRemoveBadSizes) return fail("null map", 0, 0);
    cases += 5;
  }
  // ---- sizes only, up to 2^31 - 1 rows ----
  for (long long N : {1LL, 2LL, 1000LL, (long long)kAppendMaxRows - 1, (long long)kAppendMaxRows})
    for (long long M : {-1LL, 0LL, 1LL, 2LL, N - 2, N - 1, N, N + 1, (long long)INT64_MAX}) {
      const long long left = remove_rows_left(N, M);
      const bool ok = M >= 0 && M < N;
      if (ok ? left != N - M : left != -1) return fail("rows left", N, M);
      if (ok && (left < 1 || left > kAppendMaxRows)) return fail("rows left range", N, M);
      ++cases;
    }
  if (remove_rows_left(0, 0) != -1 || remove_rows_left(-5, 0) != -1 || remove_rows_left(INT64_MAX, INT64_MAX - 1) != 1) return fail("rows left extremes", 0, 0);
  // ---- eligibility: one condition at a time ----
  {
    RemoveInputs in = base_inputs();
    if (remove_eligible(in) != kAppendOk) return fail("plain case", 0, 0);
    in.family = kFamilyButterfly;
    if (remove_eligible(in) != kAppendOk) return fail("butterfly case", 0, 0);
    in = base_inputs(), in.knn_k = 0;
    if (remove_eligible(in) != kAppendNoLists) return fail("no lists", 0, 0);
    in = base_inputs(), in.family = kFamilyNone;
    if (remove_eligible(in) != kAppendNoLists) return fail("no family", 0, 0);
    in = base_inputs(), in.N = 1, in.M = 0;
    if (remove_eligible(in) != kAppendNoLists) return fail("one row", 0, 0);
    in = base_inputs(), in.comm = true;
    if (remove_eligible(in) != kAppendComm) return fail("communicator", 0, 0);
    in = base_inputs(), in.N = 20, in.M = 1, in.k_requested = 19, in.knn_k = 19;  // k_eff 19 -> 18
    if (remove_eligible(in) != kAppendKChanges) return fail("k changes", 0, 0);
    in.k_requested = 30;  // (still clamped by the rows)
    if (remove_eligible(in) != kAppendKChanges) return fail("k changes, larger request", 0, 0);
    in.k_requested = in.knn_k = 18;
    if (remove_eligible(in) != kAppendOk) return fail("k stays", 0, 0);
    in = base_inputs(), in.M = 998;  // two rows left, k_eff 1
    if (remove_eligible(in) != kAppendKChanges) return fail("two rows left, k 16", 0, 0);
    in.k_requested = in.knn_k = 1;
    if (remove_eligible(in) != kAppendOk) return fail("two rows left, k 1", 0, 0);
    in.M = 999;
    if (remove_eligible(in) != kRemoveTooFewRows) return fail("one row left", 0, 0);
    in.M = 1000;
    if (remove_eligible(in) != kRemoveTooFewRows) return fail("no row left", 0, 0);
    in.M = 5000;
    if (remove_eligible(in) != kRemoveTooFewRows) return fail("more removed than rows", 0, 0);
    in = base_inputs(), in.k_requested = in.knn_k = 129;
    if (remove_eligible(in) != kAppendKTooLong) return fail("k > 128", 0, 0);
    in.k_requested = in.knn_k = 128;
    if (remove_eligible(in) != kAppendOk) return fail("k = 128", 0, 0);
    in = base_inputs(), in.N = (int64_t)kAppendMaxRows + 1;
    if (remove_eligible(in) != kAppendTooManyRows) return fail("2^31 rows", 0, 0);
    in.N = kAppendMaxRows;
    if (remove_eligible(in) != kAppendOk) return fail("2^31 - 1 rows", 0, 0);
    in.M = kAppendMaxRows - 2;
    in.k_requested = in.knn_k = 1;
    if (remove_eligible(in) != kAppendOk) return fail("2^31 - 3 rows removed", 0, 0);
    in = base_inputs(), in.N = -1;
    if (remove_eligible(in) != kAppendTooManyRows) return fail("negative rows", 0, 0);
    in = base_inputs(), in.M = -1;
    if (remove_eligible(in) != kAppendTooManyRows) return fail("negative removal", 0, 0);
    in = base_inputs(), in.family = kFamilyButterfly, in.D = 1537;
    if (remove_eligible(in) != kAppendWideRows) return fail("wide rows", 0, 0);
    in.D = 1536;
    if (remove_eligible(in) != kAppendOk) return fail("1536 columns", 0, 0);
    in.family = kFamilyMfma, in.D = 4000;
    if (remove_eligible(in) != kAppendOk) return fail("wide rows, mfma", 0, 0);
    in = base_inputs(), in.family = kFamilyButterfly, in.fallback_rows = 33;
    if (remove_eligible(in) != kAppendMixedLists) return fail("mixed lists", 0, 0);
    in.fallback_rows = 32;
    if (remove_eligible(in) != kAppendOk) return fail("few fallback rows", 0, 0);
    in.family = kFamilyMfma, in.fallback_rows = 1000;
    if (remove_eligible(in) != kAppendOk) return fail("fallback rows, mfma", 0, 0);
    for (int why = kAppendOk; why <= kRemoveTooFewRows + 1; ++why)
      if (remove_denied_text(why) == nullptr) return fail("text", why, 0);
    if (remove_denied_text(kRemoveTooFewRows)[0] == 'u') return fail("text of the code of its own", 0, 0);
    cases += 29;
  }
  // ---- the redo list's chunks at cols = N': whole tiles, within budget (or one tile), covering the list in order ----
  for (long long N : {3LL, 46LL, 1001LL, 8500LL, 100000LL, 1LL << 20, (long long)kAppendMaxRows})
    for (long long M : {1LL, 37LL, 200LL, 1024LL})
      for (long long budget : {1LL << 20, 1LL << 28, (long long)kAppendScratchBytes})
        for (long long redo : {0LL, 1LL, 129LL, 5000LL}) {
          const long long cols = remove_rows_left(N, M);
          if (cols < 2 || redo > cols) continue;
          const long long chunk = append_chunk_rows(cols, budget);
          if (chunk < kAppendRowTile || chunk % kAppendRowTile != 0) return fail("chunk tiles", cols, chunk);
          if (chunk > kAppendRowTile && chunk * append_lds(cols) * 4 > budget) return fail("chunk over budget", cols, chunk);
          const long long fl = append_scratch_floats(redo, cols, budget);
          if (fl < 1 || fl / append_lds(cols) > chunk) return fail("scratch rows", cols, fl);
          if (fl / append_lds(cols) < std::min<long long>(std::max<long long>(1, redo), chunk)) return fail("scratch too small", cols, fl);
          const long long nc = append_chunk_count(redo, chunk);
          if (redo == 0 && nc != 0) return fail("chunks of nothing", cols, nc);
          long long at = 0;
          for (long long c = 0; c < nc; ++c) {
            int64_t b, e;
            append_chunk_range(redo, chunk, c, b, e);
            if (b != at || e <= b || e - b > chunk || e > redo) return fail("chunk range", c, b);
            if ((e - b) > fl / append_lds(cols)) return fail("chunk beyond scratch", c, e - b);
            at = e;
            ++cases;
          }
          if (at != redo) return fail("chunks do not cover", at, redo);
          ++cases;
        }
  // ---- the threshold: monotone in the redo rows; never more than the lattice ----
  for (int fam : {(int)kFamilyMfma, (int)kFamilyButterfly})
    for (long long rows : {2LL, 100LL, 8192LL, 100000LL, 1LL << 20, (long long)kAppendMaxRows}) {
      const long long cap = remove_max_query_rows(fam, rows);
      if (cap < 1) return fail("threshold floor", fam, rows);
      if (rows >= 128 && cap > rows) return fail("threshold above the lattice", fam, rows);
      if (!remove_pays(fam, rows, 0) || !remove_pays(fam, rows, cap)) return fail("at the cap", fam, rows);
      if (remove_pays(fam, rows, cap + 1)) return fail("past the cap", fam, rows);
      ++cases;
    }
  std::printf("remove plan sweep ok (%lld cases)\n", cases);
  return 0;
}

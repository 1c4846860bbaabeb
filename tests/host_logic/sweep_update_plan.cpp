// Sweep of update_plan.hpp (the route and sizes of osc_create_updated): the id check against a brute-force one (any order,
// extremes, n = 0, ids at 0 and N - 1, duplicates as an error of their own, int32 and int64 ids), the eligibility table row
// by row, the threshold, and the chunks of the query list with the replaced rows' part of each chunk; and what append,
// remove and update share (append_plan.hpp): the query list and the fresh part of a chunk against a brute-force
// construction, for all three kinds.  Run under -fsanitize=address,undefined.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../oscillink_amd/csrc/update_plan.hpp"

using namespace osc::host;

static int fail(const char* what, long long a, long long b) {
  std::printf("ERROR %s (%lld, %lld)\n", what, a, b);
  return 1;
}

static UpdateInputs base_inputs() {
  UpdateInputs in;
  in.N = 1000;
  in.M = 10;
  in.D = 64;
  in.k_requested = 16;
  in.knn_k = 16;
  in.family = kFamilyMfma;
  return in;
}

// the map by the definition: the first id out of range decides before a later duplicate does, and the reverse
template <typename Id>
static int check_ids(const std::vector<Id>& ids, long long N) {
  int expect = kUpdateIdsOk;
  std::vector<char> seen((size_t)N, 0);
  for (Id id : ids) {
    if ((long long)id < 0 || (long long)id >= N) {
      expect = kUpdateIdOutOfRange;
      break;
    }
    if (seen[(size_t)id]) {
      expect = kUpdateIdDuplicate;
      break;
    }
    seen[(size_t)id] = 1;
  }
  std::vector<int32_t> map((size_t)N + 2, 12345);  // one guard entry on each side
  const int32_t rc = update_ids(ids.empty() ? (const Id*)nullptr : ids.data(), (int64_t)ids.size(), N, map.data() + 1);
  if (map[0] != 12345 || map[(size_t)N + 1] != 12345) return fail("map wrote outside its N entries", N, (long long)ids.size());
  if (rc != expect) return fail("id status", rc, expect);
  if (rc != kUpdateIdsOk) return 0;
  for (long long i = 0; i < N; ++i)
    if (map[(size_t)i + 1] != (seen[(size_t)i] ? -1 : (int32_t)i)) return fail("map entry", i, map[(size_t)i + 1]);
  return 0;
}

// seed_query_list and seed_chunk_fresh_part against the definition: n rows, the rows `flagged` marks and the ascending
// `fresh` rows (among the flagged ones or not); the list is every flagged row that is not fresh, ascending, then the fresh
// rows, and position p of it is fresh iff p >= redo.  Chunks of `chunk` rows: edges before, inside and after the fresh part.
static int check_query_list(long long n, const std::vector<char>& flagged, const std::vector<int32_t>& fresh, long long n_old,
                            long long& cases) {
  std::vector<char> is_fresh((size_t)n, 0);
  for (int32_t f : fresh) is_fresh[(size_t)f] = 1;
  std::vector<int32_t> expect, given;
  for (long long i = 0; i < n; ++i)
    if (flagged[(size_t)i] && !is_fresh[(size_t)i]) expect.push_back((int32_t)i);
  const long long redo = (long long)expect.size();
  for (long long i = 0; i < n; ++i)
    if (is_fresh[(size_t)i]) expect.push_back((int32_t)i);
  for (long long i = n - 1; i >= 0; --i)  // the device's order is any order: descending, the odd rows first
    if (flagged[(size_t)i] && (i & 1)) given.push_back((int32_t)i);
  for (long long i = n - 1; i >= 0; --i)
    if (flagged[(size_t)i] && !(i & 1)) given.push_back((int32_t)i);
  const std::vector<int32_t> q = seed_query_list(given, fresh);
  if (q != expect) return fail("query list", n, redo);
  const long long nq = (long long)q.size();
  for (long long chunk : {1LL, 2LL, 3LL, 5LL, 128LL}) {
    long long fresh_at = redo;
    for (long long c = 0; c < append_chunk_count(nq, chunk); ++c) {
      int64_t b, e, nb, ne;
      append_chunk_range(nq, chunk, c, b, e);
      seed_chunk_fresh_part(redo, b, e, nb, ne);
      if (nb < 0 || nb > ne || ne != e - b) return fail("fresh part bounds", nb, ne);
      for (long long r = 0; r < e - b; ++r)  // block row r of the chunk: in the fresh part iff its row is fresh
        if ((r >= nb && r < ne) != (is_fresh[(size_t)q[(size_t)(b + r)]] != 0)) return fail("fresh part membership", c, r);
      for (long long r = nb; r < ne; ++r, ++fresh_at) {
        if (q[(size_t)(b + r)] != fresh[(size_t)(fresh_at - redo)]) return fail("fresh part order", c, r);
        if (n_old >= 0 && q[(size_t)(b + r)] != n_old + (fresh_at - redo)) return fail("appended column id", c, r);  // append: n_old + j
      }
      ++cases;
    }
    if (fresh_at != nq) return fail("fresh parts do not cover", fresh_at, nq);
  }
  return 0;
}

int main() {
  long long cases = 0;
  // ---- the shared query list: append (fresh rows behind the listed ones, never flagged), remove (none), update (fresh
  // rows among the flagged ones: interleaved with the others, below them, above them) at redo = 0, 1 and many ----
  for (long long n : {2LL, 9LL, 64LL, 301LL})
    for (int pattern = 0; pattern < 3; ++pattern) {  // flagged among the listed rows: none, one, every third
      auto flag = [&](long long i) { return pattern == 1 ? i == n / 3 : pattern == 2 ? i % 3 == 1 : false; };
      for (long long m : {1LL, 2LL, 7LL}) {  // append: rows n .. n + m - 1 are fresh
        std::vector<char> fl((size_t)(n + m), 0);
        std::vector<int32_t> fresh;
        for (long long i = 0; i < n; ++i) fl[(size_t)i] = flag(i);
        for (long long j = 0; j < m; ++j) fresh.push_back((int32_t)(n + j));
        if (check_query_list(n + m, fl, fresh, n, cases)) return 1;
      }
      {  // remove: no fresh row
        std::vector<char> fl((size_t)n, 0);
        for (long long i = 0; i < n; ++i) fl[(size_t)i] = flag(i);
        if (check_query_list(n, fl, {}, -1, cases)) return 1;
      }
      for (int where = 0; where < 3; ++where)  // update: fresh rows interleaved with, below, above the other flagged rows
        for (long long m : {1LL, 2LL, 5LL}) {
          if (m > n) continue;
          std::vector<char> fl((size_t)n, 0);
          std::vector<int32_t> fresh;
          for (long long j = 0; j < m; ++j) fresh.push_back((int32_t)(where == 0 ? j * (n / m) : where == 1 ? j : n - m + j));
          for (long long i = 0; i < n; ++i) fl[(size_t)i] = flag(i);
          for (int32_t f : fresh) fl[(size_t)f] = 1;  // (a replaced row's list is empty: always flagged)
          if (check_query_list(n, fl, fresh, -1, cases)) return 1;
        }
    }
  // ---- the id map ----
  for (long long N : {1LL, 2LL, 3LL, 17LL, 128LL, 129LL, 1000LL}) {
    if (check_ids<int32_t>({}, N)) return 1;  // n = 0: the identity
    if (check_ids<int32_t>({0}, N)) return 1;
    if (check_ids<int32_t>({(int32_t)(N - 1)}, N)) return 1;
    if (check_ids<int64_t>({N - 1, 0}, N)) return 1;  // (a duplicate at N = 1)
    if (check_ids<int64_t>({0, N - 1, 0}, N)) return 1;
    if (check_ids<int32_t>({(int32_t)N}, N)) return 1;
    if (check_ids<int32_t>({-1}, N)) return 1;
    if (check_ids<int32_t>({0, INT32_MAX}, N)) return 1;
    if (check_ids<int32_t>({0, INT32_MIN}, N)) return 1;
    if (check_ids<int32_t>({0, 0, INT32_MIN}, N)) return 1;  // (the duplicate comes first)
    if (check_ids<int64_t>({INT64_MAX}, N)) return 1;
    if (check_ids<int64_t>({INT64_MIN}, N)) return 1;
    if (check_ids<int64_t>({N + ((int64_t)1 << 32)}, N)) return 1;  // (no truncation to int32)
    if (check_ids<int64_t>({(int64_t)1 << 32}, N)) return 1;         // (would be 0 in int32)
    std::vector<int32_t> all;
    for (long long i = N - 1; i >= 0; --i) all.push_back((int32_t)i);
    if (check_ids(all, N)) return 1;  // every row replaced: fine
    all.push_back(0);
    if (check_ids(all, N)) return 1;
    cases += 16;
    unsigned long long x = 88172645463325252ULL + (unsigned long long)N;  // xorshift: random lists, unsorted
    for (int rep = 0; rep < 40; ++rep) {
      std::vector<int32_t> ids;
      const long long n = (long long)(rep * 7) % (N + 2);
      for (long long j = 0; j < n; ++j) {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        ids.push_back((int32_t)(x % (unsigned long long)N));
      }
      if (check_ids(ids, N)) return 1;
      if (rep % 2) {  // the same list without its duplicates: always accepted
        std::vector<char> seen((size_t)N, 0);
        std::vector<int32_t> distinct;
        for (int32_t id : ids)
          if (!seen[(size_t)id]) seen[(size_t)id] = 1, distinct.push_back(id);
        if (check_ids(distinct, N)) return 1;
        ++cases;
      }
      ++cases;
    }
  }
  {  // bad sizes never touch the arrays
    int32_t one = 5;
    const int32_t id = 0;
    if (update_ids(&id, 1, 0, &one) != kUpdateBadSizes || one != 5) return fail("N = 0", 0, 0);
    if (update_ids(&id, -1, 1, &one) != kUpdateBadSizes || one != 5) return fail("n < 0", 0, 0);
    if (update_ids((const int32_t*)nullptr, 1, 1, &one) != kUpdateBadSizes || one != 5) return fail("null ids", 0, 0);
    if (update_ids(&id, 1, (int64_t)kAppendMaxRows + 1, &one) != kUpdateBadSizes || one != 5) return fail("N = 2^31", 0, 0);
    if (update_ids(&id, 1, 1, (int32_t*)nullptr) != kUpdateBadSizes) return fail("null map", 0, 0);
    cases += 5;
  }
  // ---- eligibility: one condition at a time ----
  {
    UpdateInputs in = base_inputs();
    if (update_eligible(in) != kAppendOk) return fail("plain case", 0, 0);
    in.family = kFamilyButterfly;
    if (update_eligible(in) != kAppendOk) return fail("butterfly case", 0, 0);
    in = base_inputs(), in.knn_k = 0;
    if (update_eligible(in) != kAppendNoLists) return fail("no lists", 0, 0);
    in = base_inputs(), in.family = kFamilyNone;
    if (update_eligible(in) != kAppendNoLists) return fail("no family", 0, 0);
    in = base_inputs(), in.N = 1, in.M = 1;
    if (update_eligible(in) != kAppendNoLists) return fail("one row", 0, 0);
    in = base_inputs(), in.comm = true;
    if (update_eligible(in) != kAppendComm) return fail("communicator", 0, 0);
    in = base_inputs(), in.N = 20, in.M = 1, in.k_requested = 30, in.knn_k = 19;  // clamped by the rows: N does not change
    if (update_eligible(in) != kAppendOk) return fail("k clamped and kept", 0, 0);
    in.knn_k = 18;
    if (update_eligible(in) != kAppendKChanges) return fail("lists of another length", 0, 0);
    in = base_inputs(), in.N = 2, in.M = 2, in.k_requested = 16, in.knn_k = 1;
    if (update_eligible(in) != kAppendOk) return fail("two rows, both replaced", 0, 0);
    in = base_inputs(), in.M = 1000;
    if (update_eligible(in) != kAppendOk) return fail("every row replaced", 0, 0);
    in.M = 1001;
    if (update_eligible(in) != kAppendTooManyRows) return fail("more replaced than rows", 0, 0);
    in = base_inputs(), in.k_requested = in.knn_k = 129;
    if (update_eligible(in) != kAppendKTooLong) return fail("k > 128", 0, 0);
    in.k_requested = in.knn_k = 128;
    if (update_eligible(in) != kAppendOk) return fail("k = 128", 0, 0);
    in = base_inputs(), in.N = (int64_t)kAppendMaxRows + 1;
    if (update_eligible(in) != kAppendTooManyRows) return fail("2^31 rows", 0, 0);
    in.N = kAppendMaxRows;
    if (update_eligible(in) != kAppendOk) return fail("2^31 - 1 rows", 0, 0);
    in.M = kAppendMaxRows;
    if (update_eligible(in) != kAppendOk) return fail("2^31 - 1 rows replaced", 0, 0);
    in = base_inputs(), in.N = -1;
    if (update_eligible(in) != kAppendTooManyRows) return fail("negative rows", 0, 0);
    in = base_inputs(), in.M = -1;
    if (update_eligible(in) != kAppendTooManyRows) return fail("negative replacement", 0, 0);
    in = base_inputs(), in.family = kFamilyButterfly, in.D = 1537;
    if (update_eligible(in) != kAppendWideRows) return fail("wide rows", 0, 0);
    in.D = 1536;
    if (update_eligible(in) != kAppendOk) return fail("1536 columns", 0, 0);
    in.family = kFamilyMfma, in.D = 4000;
    if (update_eligible(in) != kAppendOk) return fail("wide rows, mfma", 0, 0);
    in = base_inputs(), in.family = kFamilyButterfly, in.fallback_rows = 33;
    if (update_eligible(in) != kAppendMixedLists) return fail("mixed lists", 0, 0);
    in.fallback_rows = 32;
    if (update_eligible(in) != kAppendOk) return fail("few fallback rows", 0, 0);
    in.family = kFamilyMfma, in.fallback_rows = 1000;
    if (update_eligible(in) != kAppendOk) return fail("fallback rows, mfma", 0, 0);
    cases += 24;
  }
  // ---- the query list's chunks at N columns: whole tiles, within budget (or one tile), covering the list in order; the
  // replaced rows' parts cover the list's last M entries exactly once, in order ----
  for (long long N : {2LL, 46LL, 1001LL, 8500LL, 100000LL, 1LL << 20, (long long)kAppendMaxRows})
    for (long long M : {1LL, 37LL, 200LL, 1024LL})
      for (long long budget : {1LL << 20, 1LL << 28, (long long)kAppendScratchBytes})
        for (long long redo : {0LL, 1LL, 127LL, 128LL, 129LL, 5000LL}) {
          if (M > N || redo > N - M) continue;
          const long long nq = redo + M;
          const long long chunk = append_chunk_rows(N, budget);
          if (chunk < kAppendRowTile || chunk % kAppendRowTile != 0) return fail("chunk tiles", N, chunk);
          if (chunk > kAppendRowTile && chunk * append_lds(N) * 4 > budget) return fail("chunk over budget", N, chunk);
          const long long fl = append_scratch_floats(nq, N, budget);
          if (fl < 1 || fl / append_lds(N) > chunk) return fail("scratch rows", N, fl);
          if (fl / append_lds(N) < std::min<long long>(nq, chunk)) return fail("scratch too small", N, fl);
          const long long nc = append_chunk_count(nq, chunk);
          long long at = 0, replaced_at = redo;
          for (long long c = 0; c < nc; ++c) {
            int64_t b, e, nb, ne;
            append_chunk_range(nq, chunk, c, b, e);
            if (b != at || e <= b || e - b > chunk || e > nq) return fail("chunk range", c, b);
            if ((e - b) > fl / append_lds(N)) return fail("chunk beyond scratch", c, e - b);
            seed_chunk_fresh_part(redo, b, e, nb, ne);
            if (nb < 0 || nb > ne || ne != e - b) return fail("replaced part bounds", nb, ne);
            if (nb < ne) {  // entries [b + nb, b + ne) of the query list: replaced rows only, none skipped
              if (b + nb != replaced_at) return fail("replaced part start", b + nb, replaced_at);
              replaced_at = b + ne;
            } else if (e > redo) {
              return fail("a chunk with replaced rows and no replaced part", b, e);
            }
            at = e;
            ++cases;
          }
          if (at != nq) return fail("chunks do not cover", at, nq);
          if (replaced_at != nq) return fail("replaced parts do not cover", replaced_at, nq);
          ++cases;
        }
  // ---- the threshold: redo + M against append's cap at N rows ----
  for (int fam : {(int)kFamilyMfma, (int)kFamilyButterfly})
    for (long long rows : {2LL, 100LL, 8192LL, 100000LL, 1LL << 20, (long long)kAppendMaxRows}) {
      const long long cap = update_max_query_rows(fam, rows);
      if (cap != append_max_query_rows(fam, rows)) return fail("threshold is append's", fam, rows);
      if (cap < 1) return fail("threshold floor", fam, rows);
      if (rows >= 128 && cap > rows) return fail("threshold above the lattice", fam, rows);
      if (!update_pays(fam, rows, 1, 0) || !update_pays(fam, rows, 1, cap - 1) || !update_pays(fam, rows, cap, 0))
        return fail("at the cap", fam, rows);
      if (update_pays(fam, rows, 1, cap) || update_pays(fam, rows, cap + 1, 0)) return fail("past the cap", fam, rows);
      for (long long M : {1LL, 8LL, cap / 2})
        if (update_pays(fam, rows, M, cap - M) != append_pays(fam, rows - M, M, cap - M)) return fail("append's meaning of the sum", fam, rows);
      ++cases;
    }
  std::printf("update plan sweep ok (%lld cases)\n", cases);
  return 0;
}

// Sweep of append_plan.hpp (the route and sizes of osc_create_appended): the eligibility table row by row, the chunks of
// the query list (cover, order, whole 128-row tiles, scratch within budget, the new-row part of a chunk), and sizes
// near 2^31.  Run under -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../oscillink_amd/csrc/append_plan.hpp"

using namespace osc::host;

static int fail(const char* what, long long a, long long b) {
  std::printf("ERROR %s (%lld, %lld)\n", what, a, b);
  return 1;
}

static AppendInputs base_inputs() {
  AppendInputs in;
  in.N = 1000;
  in.M = 10;
  in.D = 64;
  in.k_requested = 16;
  in.knn_k = 16;
  in.family = kFamilyMfma;
  return in;
}

int main() {
  long long cases = 0;
  // ---- eligibility: one condition at a time ----
  {
    AppendInputs in = base_inputs();
    if (append_eligible(in) != kAppendOk) return fail("plain case", 0, 0);
    in.family = kFamilyButterfly;
    if (append_eligible(in) != kAppendOk) return fail("butterfly case", 0, 0);
    in = base_inputs(), in.knn_k = 0;
    if (append_eligible(in) != kAppendNoLists) return fail("no lists", 0, 0);
    in = base_inputs(), in.family = kFamilyNone;
    if (append_eligible(in) != kAppendNoLists) return fail("no family", 0, 0);
    in = base_inputs(), in.comm = true;
    if (append_eligible(in) != kAppendComm) return fail("communicator", 0, 0);
    in = base_inputs(), in.N = 10, in.k_requested = 16, in.knn_k = 9;  // k_eff 9 -> 16
    if (append_eligible(in) != kAppendKChanges) return fail("k changes", 0, 0);
    in.M = 0;  // (no new rows: the clamp stays)
    if (append_eligible(in) != kAppendOk) return fail("k stays", 0, 0);
    in = base_inputs(), in.k_requested = in.knn_k = 129;
    if (append_eligible(in) != kAppendKTooLong) return fail("k > 128", 0, 0);
    in.k_requested = in.knn_k = 128;
    if (append_eligible(in) != kAppendOk) return fail("k = 128", 0, 0);
    in = base_inputs(), in.N = kAppendMaxRows - 5, in.M = 6;
    if (append_eligible(in) != kAppendTooManyRows) return fail("2^31 rows", 0, 0);
    in.M = 5;
    if (append_eligible(in) != kAppendOk) return fail("2^31 - 1 rows", 0, 0);
    in = base_inputs(), in.N = INT64_MAX / 2, in.M = INT64_MAX / 2;  // (the sum stays in int64)
    if (append_eligible(in) != kAppendTooManyRows) return fail("huge rows", 0, 0);
    in = base_inputs(), in.N = -1;
    if (append_eligible(in) != kAppendTooManyRows) return fail("negative rows", 0, 0);
    in = base_inputs(), in.family = kFamilyButterfly, in.D = 1537;
    if (append_eligible(in) != kAppendWideRows) return fail("wide rows", 0, 0);
    in.D = 1536;
    if (append_eligible(in) != kAppendOk) return fail("1536 columns", 0, 0);
    in.family = kFamilyMfma, in.D = 4000;
    if (append_eligible(in) != kAppendOk) return fail("wide rows, mfma", 0, 0);
    in = base_inputs(), in.family = kFamilyButterfly, in.fallback_rows = 33;
    if (append_eligible(in) != kAppendMixedLists) return fail("mixed lists", 0, 0);
    in.fallback_rows = 32;
    if (append_eligible(in) != kAppendOk) return fail("few fallback rows", 0, 0);
    in.family = kFamilyMfma, in.fallback_rows = 1000;
    if (append_eligible(in) != kAppendOk) return fail("fallback rows, mfma", 0, 0);
    for (int why = kAppendOk; why <= kAppendSlower + 1; ++why)
      if (append_denied_text(why) == nullptr) return fail("text", why, 0);
    cases += 24;
  }
  // ---- k_eff, pitches ----
  for (long long rows : {1LL, 2LL, 3LL, 17LL, 129LL, 1LL << 20, (long long)kAppendMaxRows})
    for (int k : {1, 2, 16, 128, 1 << 30}) {
      const int ke = append_k_eff(k, rows);
      if (ke < 1 || ke > k || (rows > 1 && ke > rows - 1)) return fail("k_eff", rows, k);
      ++cases;
    }
  for (int D : {1, 31, 32, 33, 768, 1536, 1537, INT32_MAX}) {
    const long long l = append_ldn(D);
    if (l < D || l % 32 != 0 || l - D > 31) return fail("ldn", D, l);
  }
  for (long long c : {1LL, 31LL, 32LL, 33LL, (long long)kAppendMaxRows}) {
    const long long l = append_lds(c);
    if (l < c || l % 32 != 0 || l - c > 31) return fail("lds", c, l);
  }
  // ---- chunks: whole tiles, within budget (or one tile), covering the query list in order; the new part of each ----
  for (long long cols : {2LL, 45LL, 1000LL, 8300LL, 100000LL, 1LL << 20, 1LL << 25, (long long)kAppendMaxRows})
    for (long long budget : {1LL << 20, 1LL << 28, (long long)kAppendScratchBytes})
      for (long long redo : {0LL, 1LL, 40LL, 5000LL})
        for (long long m : {0LL, 1LL, 37LL, 128LL, 129LL, 16384LL}) {
          if (redo >= cols || m > cols - 1) continue;
          const long long n_old = cols - m, nq = redo + m;
          const long long chunk = append_chunk_rows(cols, budget);
          if (chunk < kAppendRowTile || chunk % kAppendRowTile != 0) return fail("chunk tiles", cols, chunk);
          if (chunk > kAppendRowTile && chunk * append_lds(cols) * 4 > budget) return fail("chunk over budget", cols, chunk);
          const long long fl = append_scratch_floats(nq, cols, budget);
          if (fl < 1 || fl / append_lds(cols) > chunk) return fail("scratch rows", cols, fl);
          if (fl / append_lds(cols) < std::min<long long>(std::max<long long>(1, nq), chunk)) return fail("scratch too small", cols, fl);
          const long long nc = append_chunk_count(nq, chunk);
          if (nq == 0 && nc != 0) return fail("chunks of nothing", cols, nc);
          if (nc > 4096) continue;  // (walking them adds nothing)
          // the query list, whose fresh entries are the column ids the merge computes as n_old + (b + nb - redo) + j: `redo`
          // old rows in the device's (any) order, then the new rows (where the case has that many old rows; the arithmetic
          // below is asserted in every case)
          std::vector<int32_t> q;
          if (redo <= n_old) {
            std::vector<int32_t> flagged, fresh;
            for (long long j = redo - 1; j >= 0; --j) flagged.push_back((int32_t)j);  // (here: descending)
            for (long long j = 0; j < m; ++j) fresh.push_back((int32_t)(n_old + j));
            q = seed_query_list(flagged, fresh);
            if ((long long)q.size() != nq) return fail("query list length", (long long)q.size(), nq);
            for (long long j = 0; j < redo; ++j)
              if (q[(size_t)j] != (int32_t)j) return fail("redo rows ascending", j, q[(size_t)j]);
          }
          long long at = 0, new_seen = 0;
          for (long long c = 0; c < nc; ++c) {
            int64_t b, e, nb, ne;
            append_chunk_range(nq, chunk, c, b, e);
            if (b != at || e <= b || e - b > chunk || e > nq) return fail("chunk range", c, b);
            if ((e - b) > fl / append_lds(cols)) return fail("chunk beyond scratch", c, e - b);
            seed_chunk_fresh_part(redo, b, e, nb, ne);
            if (nb < 0 || nb > ne || ne != e - b) return fail("new part", c, nb);
            if (ne > nb) {
              // entries [b + nb, b + ne) of the query list are the columns n_old + new_seen, ...: none skipped, none twice
              if (b + nb - redo != new_seen) return fail("first new column", c, b + nb - redo);
              if (b + nb < redo) return fail("new part holds a redo row", c, nb);
              if (n_old + new_seen + (ne - nb) > cols) return fail("new column past the lattice", c, n_old + new_seen);
              for (long long j = nb; j < ne && !q.empty(); ++j)
                if (q[(size_t)(b + j)] != n_old + new_seen + (j - nb)) return fail("new column id", c, q[(size_t)(b + j)]);
            }
            new_seen += ne - nb;
            at = e;
            ++cases;
          }
          if (at != nq || new_seen != m) return fail("chunks do not cover", at, new_seen);
        }
  // ---- thresholds: monotone in the query rows; never more than the lattice ----
  for (int fam : {(int)kFamilyMfma, (int)kFamilyButterfly})
    for (long long rows : {2LL, 100LL, 8192LL, 100000LL, 1LL << 20, (long long)kAppendMaxRows}) {
      const long long cap = append_max_query_rows(fam, rows);
      if (cap < 32) return fail("threshold floor", fam, rows);
      if (rows >= 128 && cap > rows) return fail("threshold above the lattice", fam, rows);
      if (!append_pays(fam, rows - 1, 1, 0)) return fail("one row does not pay", fam, rows);
      if (append_pays(fam, rows - 1, 1, cap)) return fail("redo rows ignored", fam, rows);
      ++cases;
    }
  std::printf("append plan sweep ok (%lld cases)\n", cases);
  return 0;
}

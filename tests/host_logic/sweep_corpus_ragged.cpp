// Sweep of corpus_ragged.hpp (the host arithmetic of a ragged corpus refine chunk): row counts
// 0 .. 1025 against K 1 .. 1024 -- the clamp to the slot, the per-lattice list length and pick count, the validation of the
// counts, the candidate rows' padding and the padded copies -- and, for a chunk of lattices, that every lattice's rows and
// lists lie inside its own slot of the union corpus_plan.hpp lays out.  Run under -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../oscillink_amd/csrc/corpus_plan.hpp"
#include "../../oscillink_amd/csrc/corpus_ragged.hpp"

using namespace osc::host;

static int fail(const char* what, long long a, long long b) {
  std::printf("ERROR %s (%lld, %lld)\n", what, a, b);
  return 1;
}

int main() {
  long long cases = 0;
  std::vector<int32_t> row(1024), out(1024);
  std::vector<float> gin(1024), gout(1024);
  for (int K = 1; K <= 1024; ++K) {
    for (int e = 0; e <= 1025; ++e) {
      const int n = ragged_rows(e, K);
      if (n != (e < K ? e : K)) return fail("rows", e, K);
      const int32_t one[1] = {e};
      const bool ok = e >= 1 && e <= K;
      if ((ragged_first_bad(one, 1, K) == -1) != ok) return fail("first_bad", e, K);
      if (ragged_is_uniform(one, 1, K) != (e == K)) return fail("uniform", e, K);
      if (n < 1) continue;
      for (int kn : {1, 6, 128, 5000}) {
        const int kq = ragged_knn(kn, n), kK = K > 1 ? corpus_knn(kn, K) : 0;
        if (kq != (n > 1 ? std::min(kn, n - 1) : 0)) return fail("knn", kn, n);
        if (kq > kK) return fail("list longer than the slot's", kq, kK);  // the k-wide list holds every lattice's
        if (std::min(kK, n - 1) != kq && n > 1) return fail("knn from the stride", kq, kK);  // what the kernel computes
        if (ragged_sig_k(kn, n) != std::min(kn, std::max(1, n - 1))) return fail("sig k", kn, n);
      }
      for (int kk : {0, 1, 8, 2000}) {
        const int p = ragged_picks(std::min(kk, K), n);
        if (p != std::min(kk, n) || p > n) return fail("picks", kk, n);
      }
      ++cases;
    }
    // candidate rows: n ids in front, the pad id behind; anything else is refused
    for (int n : {0, 1, K / 2, K - 1, K}) {
      if (n < 0 || n > K) continue;
      for (int t = 0; t < K; ++t) row[t] = t < n ? 3 * t : kRaggedPadId;
      if (ragged_lead(row.data(), K) != n) return fail("lead", n, K);
      if (n + 1 < K) {
        row[K - 1] = 5;  // an id behind the padding
        if (ragged_lead(row.data(), K) != -1) return fail("lead accepts an id behind the padding", n, K);
        row[K - 1] = -7;  // a negative entry that is not the pad id
        if (ragged_lead(row.data(), K) != -1) return fail("lead accepts a stray negative", n, K);
      }
      for (int t = 0; t < K; ++t) gin[t] = 1.f + t;
      std::fill(gout.begin(), gout.end(), -1.f);
      ragged_copy_padded(gin.data(), n, K, 0.f, gout.data());
      for (int t = 0; t < K; ++t)
        if (gout[t] != (t < n ? gin[t] : 0.f)) return fail("copy_padded", t, n);
      for (int t = K; t < 1024; ++t)
        if (gout[t] != -1.f) return fail("copy_padded wrote behind K", t, K);
    }
  }
  // a chunk of nq lattices: rows and lists of lattice q lie in [q K, (q + 1) K) of the union, whatever the counts are, and the
  // union's blocks are corpus_layout's
  for (int K : {1, 2, 7, 100, 300, 1024})
    for (int nq : {1, 3, 16, 256})
      for (int kn : {1, 6, 128}) {
        const int k = std::max(1, K > 1 ? corpus_knn(kn, K) : 0);
        const CorpusLayout L = corpus_layout(1000, 64, K, k, 1, nq);
        for (int q = 0; q < nq; ++q) {
          const int n = 1 + (int)((1103515245u * (unsigned)(q + K) + 12345u) % (unsigned)K);
          for (int r : {0, n - 1}) {
            const long long u = ragged_row(q, r, K), l = ragged_list_at(q, r, K, k);
            if (u < (long long)q * K || u >= (long long)(q + 1) * K) return fail("row outside its slot", q, r);
            if (l < 0 || (l + k) * 4 > L.kidx - L.kval) return fail("list outside the block", q, r);
            if (u * 4 >= L.sd - L.deg) return fail("row outside the block", q, r);
          }
          ++cases;
        }
      }
  std::printf("corpus ragged sweep ok: %lld cases\n", cases);
  return 0;
}

// Sweep of corpus_settings.hpp (the host arithmetic of a corpus refine call with per-query settings, DESIGN.md section
// 13.8): the value checks record by record, the effective record of a lattice of n rows in a K-row slot, the maxima that
// size a chunk's lists and outputs -- every lattice's own list and picks lie inside them, and inside corpus_plan.hpp's
// blocks -- and the slice of a chunk.  Run under -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../oscillink_amd/csrc/corpus_plan.hpp"
#include "../../oscillink_amd/csrc/corpus_ragged.hpp"
#include "../../oscillink_amd/csrc/corpus_settings.hpp"

using namespace osc::host;

static int fail(const char* what, long long a, long long b) {
  std::printf("ERROR %s (%lld, %lld)\n", what, a, b);
  return 1;
}

static CorpusSetting good() { return CorpusSetting{1.f, 0.5f, 4.f, 0.2f, 0.5f, 1.f, 1e-3f, 6, 8, 12}; }

int main() {
  long long cases = 0;
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  // the value checks: one bad field at a time, and the first offending query of a batch
  {
    if (setting_error(good())) return fail("a good record is refused", 0, 0);
    CorpusSetting z = good();
    z.lamC = z.lamQ = z.lamP = 0.f;  // exact zeros are allowed
    z.settle_tol = 0.f;
    z.alpha = 0.f;
    z.k = 0;
    if (setting_error(z)) return fail("zeros are refused", 0, 0);
    std::vector<CorpusSetting> bad;
    auto with = [&](auto&& f) {
      CorpusSetting s = good();
      f(s);
      bad.push_back(s);
    };
    for (float v : {0.f, -1.f, nan}) with([&](CorpusSetting& s) { s.lamG = v; });
    for (float v : {-1e-9f, nan, inf}) {
      with([&](CorpusSetting& s) { s.lamC = v; });
      with([&](CorpusSetting& s) { s.lamQ = v; });
      with([&](CorpusSetting& s) { s.lamP = v; });
    }
    for (int v : {0, -3}) with([&](CorpusSetting& s) { s.kneighbors = v; });
    for (float v : {0.f, -1.f, nan, inf}) with([&](CorpusSetting& s) { s.settle_dt = v; });
    for (int v : {0, -1}) with([&](CorpusSetting& s) { s.settle_max_iters = v; });
    for (float v : {nan, inf, -inf}) {
      with([&](CorpusSetting& s) { s.settle_tol = v; });
      with([&](CorpusSetting& s) { s.alpha = v; });
    }
    for (size_t b = 0; b < bad.size(); ++b) {
      if (!setting_error(bad[b])) return fail("a bad record passes", (long long)b, 0);
      for (int at : {0, 3, 6}) {
        std::vector<CorpusSetting> batch(7, good());
        batch[(size_t)at] = bad[b];
        if (at < 6) batch[6] = bad[(b + 1) % bad.size()];  // a later offender does not win
        const char* what = nullptr;
        if (settings_first_bad(batch.data(), 7, &what) != at || !what) return fail("first bad", (long long)b, at);
        ++cases;
      }
    }
    std::vector<CorpusSetting> fine(5, good());
    if (settings_first_bad(fine.data(), 5, nullptr) != -1 || settings_first_bad(nullptr, 0, nullptr) != -1)
      return fail("first bad of a good batch", 0, 0);
  }
  // effective records and maxima: lattices of n rows in K-row slots
  const int kns[] = {1, 2, 6, 16, 64, 128, 129, 5000}, ks[] = {-2, 0, 1, 8, 130, 500, 2000};
  for (int K : {1, 2, 3, 7, 64, 129, 130, 300, 1024}) {
    for (int Q : {1, 5, 12}) {
      std::vector<CorpusSetting> s((size_t)Q), e((size_t)Q);
      std::vector<int32_t> rows((size_t)Q);
      for (int variant = 0; variant < 8; ++variant) {
        for (int q = 0; q < Q; ++q) {
          s[(size_t)q] = good();
          s[(size_t)q].kneighbors = kns[(q + variant) % 8];
          s[(size_t)q].k = ks[(q * 3 + variant) % 7];
          rows[(size_t)q] = (variant & 1) ? 1 + (int)((1103515245u * (unsigned)(q + K + variant) + 12345u) % (unsigned)K) : K;
        }
        const int32_t lng = settings_first_long_list(s.data(), Q, K);
        int want = -1;
        for (int q = Q - 1; q >= 0; --q)
          if (K > 1 && std::min(s[(size_t)q].kneighbors, K - 1) > kCorpusMaxKnn) want = q;
        if (lng != want) return fail("first long list", lng, want);
        if (lng >= 0) continue;  // the call is refused
        for (int q = 0; q < Q; ++q) {
          const int n = rows[(size_t)q];
          e[(size_t)q] = setting_effective(s[(size_t)q], n, K);
          const CorpusSetting& x = e[(size_t)q];
          if (x.kneighbors != ragged_knn(s[(size_t)q].kneighbors, n)) return fail("effective list length", q, n);
          if (x.kneighbors < 0 || x.kneighbors > std::max(0, n - 1) || x.kneighbors > kCorpusMaxKnn)
            return fail("list longer than the lattice allows", x.kneighbors, n);
          if (x.k != std::min(std::max(s[(size_t)q].k, 0), K)) return fail("effective k", q, K);
          if (setting_picks(x, n) != std::max(0, std::min(s[(size_t)q].k, n))) return fail("picks", q, n);
          if (setting_sig_k(s[(size_t)q], n) != std::min(s[(size_t)q].kneighbors, std::max(1, n - 1))) return fail("sig k", q, n);
          if (x.lamG != s[(size_t)q].lamG || x.settle_max_iters != s[(size_t)q].settle_max_iters) return fail("other fields", q, 0);
        }
        const int32_t mk = settings_max_knn(e.data(), Q), mkk = settings_max_kk(e.data(), Q);
        if (mk > kCorpusMaxKnn || mkk > K) return fail("maxima beyond the limits", mk, mkk);
        const int k = std::max(1, (int)mk), kk = std::max(1, (int)mkk);
        const CorpusLayout L = corpus_layout(1000, 64, K, k, kk, Q);
        bool hit_k = mk == 0, hit_kk = mkk == 0;
        for (int q = 0; q < Q; ++q) {
          const CorpusSetting& x = e[(size_t)q];
          if (x.kneighbors > k || setting_picks(x, rows[(size_t)q]) > kk) return fail("a lattice exceeds the maxima", q, K);
          hit_k = hit_k || x.kneighbors == mk;
          hit_kk = hit_kk || x.k == mkk;
          // the lattice's last list entry and last pick lie inside the chunk's blocks
          const long long l = ragged_list_at(q, std::max(0, rows[(size_t)q] - 1), K, k) + std::max(0, x.kneighbors - 1);
          if (l < 0 || (l + 1) * 4 > L.kidx - L.kval) return fail("list entry outside the block", q, K);
          const long long o = (long long)q * kk + std::max(0, setting_picks(x, rows[(size_t)q]) - 1);
          if ((o + 1) * 4 > L.o_score - L.o_local) return fail("pick outside the block", q, K);
        }
        if (!hit_k || !hit_kk) return fail("a maximum nobody attains", mk, mkk);
        // the slices of the chunks of this batch
        for (int nq : {1, 5, 256}) {
          int seen = 0;
          for (int c = 0; c < chunk_count(Q, nq); ++c) {
            const int q0 = chunk_begin(c, nq), n = chunk_size(Q, c, nq);
            const CorpusSetting* p = settings_slice(e.data(), Q, q0, n);
            if (p != e.data() + q0) return fail("slice", q0, n);
            for (int t = 0; t < n; ++t)
              if (p[t].k != e[(size_t)(q0 + t)].k) return fail("slice entry", q0, t);
            seen += n;
          }
          if (seen != Q) return fail("chunks do not cover the batch", seen, Q);
        }
        if (settings_slice(e.data(), Q, Q, 1) || settings_slice(e.data(), Q, -1, 1) || settings_slice(e.data(), Q, 0, Q + 1) ||
            settings_slice(nullptr, Q, 0, 1) || settings_slice(e.data(), Q, 0, -1))
          return fail("slice outside the batch accepted", Q, K);
        if (settings_slice(e.data(), Q, Q, 0) != e.data() + Q) return fail("empty slice at the end", Q, K);
        ++cases;
      }
    }
  }
  std::printf("corpus settings sweep ok: %lld cases\n", cases);
  return 0;
}

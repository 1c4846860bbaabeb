// Sweep of the gates block of corpus_plan.hpp (diffusion gates of the gated refine path) over sweep_corpus_plan.cpp's grid:
// the block is 256-byte aligned, holds nq K floats, lies between the end of o_align and total together with its two
// per-query arrays, and every block that existed before it sits where the layout without gates put it (recomputed here
// with that layout's formula).  Run under -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>

#include "../../oscillink_amd/csrc/corpus_plan.hpp"

using namespace osc::host;

static int fail(const char* what, long long a, long long b) {
  std::printf("ERROR %s (%lld, %lld)\n", what, a, b);
  return 1;
}

int main() {
  const long long Ns[] = {1, 2, 7, 1000, 100000, 1000000};
  const int Ds[] = {1, 50, 128, 768, 1536};
  const int Ks[] = {1, 2, 7, 100, 1024};
  const int reqs[] = {1, 3, 64, 256, 100000};
  long long cases = 0;
  for (long long N : Ns)
    for (int D : Ds)
      for (int Kr : Ks)
        for (int kn : {1, 6, 128})
          for (int kr : {0, 1, 8, 2000})
            for (int req : reqs) {
              const int K = (int)std::min<long long>(Kr, N);
              const int knn = K > 1 ? corpus_knn(kn, K) : 0, k = std::max(1, knn);
              const int kk = std::max(1, std::min(kr, K));
              const int ldn = corpus_ldn(D);
              const int nq = corpus_chunk(N, ldn, K, k, kk, req, kCorpusBudgetBytes);
              if (nq < 1 || nq > req) return fail("chunk range", nq, req);
              const CorpusLayout L = corpus_layout(N, ldn, K, k, kk, nq);
              if (nq > 1 && L.total > kCorpusBudgetBytes) return fail("budget", nq, L.total);
              // the layout as it was before the gates block: the same blocks in the same order, each rounded up to 256
              const long long rows = (long long)nq * K, lds = corpus_lds(K);
              const long long bytes[] = {nq * N * 4, rows * 4, rows * 4, rows * ldn * 4, rows * ldn * 4, rows * lds * 4,
                                         rows * k * 4, rows * k * 4, rows * k * 4, rows * k * 4, rows * k * 4, rows * 4,
                                         rows * 4, rows * 4, rows * ldn * 4, rows * ldn * 4, rows * ldn * 4, rows * ldn * 4,
                                         (long long)nq * ldn * 4, nq * 4LL, nq * 4LL, nq * 4LL, (long long)nq * kk * 4,
                                         (long long)nq * kk * 4, (long long)nq * kk * 4};
              const long long got[] = {L.dots, L.cand, L.ccos, L.Y, L.Yn, L.Sm, L.kval, L.kidx, L.col, L.adj, L.w, L.deg,
                                       L.sd, L.scale, L.X, L.R, L.P, L.AP, L.psi, L.qnorm, L.iters, L.res, L.o_local,
                                       L.o_score, L.o_align};
              long long o = 0;
              for (int i = 0; i < (int)(sizeof got / sizeof got[0]); ++i) {
                if (got[i] != o) return fail("an older block moved", i, got[i]);
                o += (bytes[i] + 255) / 256 * 256;
              }
              const long long align_end = L.o_align + (long long)nq * kk * 4;
              if (L.gates % 256 != 0 || L.g_iters % 256 != 0 || L.g_res % 256 != 0) return fail("alignment", L.gates, L.g_iters);
              if (L.gates < align_end) return fail("gates overlaps o_align", L.gates, align_end);
              if (L.gates != o) return fail("gates does not follow o_align", L.gates, o);
              if (L.gates + rows * 4 > L.g_iters) return fail("gates block too small", L.gates, L.g_iters);
              if (L.g_iters + nq * 4LL > L.g_res) return fail("g_iters block too small", L.g_iters, L.g_res);
              if (L.g_res + nq * 4LL > L.total) return fail("g_res passes total", L.g_res, L.total);
              if (L.gates + rows * 4 > L.total) return fail("gates passes total", L.gates, L.total);
              ++cases;
            }
  std::printf("corpus gates plan sweep ok (%lld cases)\n", cases);
  return 0;
}

// Sweep of corpus_plan.hpp (the chunk and offset arithmetic of the corpus refine path) over corpus sizes, widths, K, list
// lengths, picks and requested chunk sizes: every chunk's layout fits the budget (or is a single query), offsets are
// aligned, ordered and disjoint, and the chunks tile [0, Q) exactly.  Run under -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <vector>

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
              if (ldn % 32 != 0 || ldn < D) return fail("ldn", D, ldn);
              if (corpus_lds(K) < K) return fail("lds", K, corpus_lds(K));
              const int nq = corpus_chunk(N, ldn, K, k, kk, req, kCorpusBudgetBytes);
              if (nq < 1 || nq > req) return fail("chunk range", nq, req);
              const CorpusLayout L = corpus_layout(N, ldn, K, k, kk, nq);
              if (nq > 1 && L.total > kCorpusBudgetBytes) return fail("budget", nq, L.total);
              if (nq < req && nq < 2 * (kCorpusBudgetBytes / corpus_layout(N, ldn, K, k, kk, 1).total) / 3)
                return fail("chunk far below the budget", nq, req);
              const long long offs[] = {L.dots, L.cand, L.ccos, L.Y, L.Yn, L.Sm, L.kval, L.kidx, L.col, L.adj, L.w, L.deg,
                                        L.sd, L.scale, L.X, L.R, L.P, L.AP, L.psi, L.qnorm, L.iters, L.res, L.o_local,
                                        L.o_score, L.o_align, L.total};
              const long long rows = (long long)nq * K;
              const long long need[] = {nq * N * 4, rows * 4, rows * 4, rows * ldn * 4, rows * ldn * 4,
                                        rows * corpus_lds(K) * 4, rows * k * 4, rows * k * 4, rows * k * 4, rows * k * 4,
                                        rows * k * 4, rows * 4, rows * 4, rows * 4, rows * ldn * 4, rows * ldn * 4,
                                        rows * ldn * 4, rows * ldn * 4, (long long)nq * ldn * 4, nq * 4LL, nq * 4LL,
                                        nq * 4LL, (long long)nq * kk * 4, (long long)nq * kk * 4, (long long)nq * kk * 4};
              for (int i = 0; i + 1 < (int)(sizeof offs / sizeof offs[0]); ++i) {
                if (offs[i] % 256 != 0) return fail("alignment", i, offs[i]);
                if (offs[i] + need[i] > offs[i + 1]) return fail("overlap", i, offs[i]);
              }
              for (int Q : {0, 1, nq - 1, nq, nq + 1, 3 * nq + 2}) {
                if (Q < 0) continue;
                std::vector<int> seen((size_t)Q, 0);
                for (int c = 0; c < chunk_count(Q, nq); ++c) {
                  const int b = chunk_begin(c, nq), n = chunk_size(Q, c, nq);
                  if (n < 1 || n > nq || b + n > Q) return fail("chunk bounds", b, n);
                  for (int q = b; q < b + n; ++q) seen[(size_t)q] += 1;
                }
                for (int q = 0; q < Q; ++q)
                  if (seen[(size_t)q] != 1) return fail("tiling", Q, q);
              }
              ++cases;
            }
  std::printf("corpus plan sweep ok (%lld cases)\n", cases);
  return 0;
}

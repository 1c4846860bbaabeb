// Sweep of the receipts blocks of corpus_plan.hpp (settle + receipt per candidate lattice) over sweep_corpus_plan.cpp's grid.
// Receipts off: the layout and the chunk are EQUAL to what the six- and seven-argument calls give (every field).  Receipts
// on: every older offset is where it was, the new blocks are 256-byte aligned, in order, disjoint, large enough for what they
// hold and inside total, and the chunk never passes the budget unless it is one query.  Run under
// -fsanitize=address,undefined.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>

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
  const int caps[] = {0, 3, 5000};
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
              const int nq0 = corpus_chunk(N, ldn, K, k, kk, req, kCorpusBudgetBytes);
              const CorpusLayout L0 = corpus_layout(N, ldn, K, k, kk, nq0);
              // receipts off, spelled out: the same chunk and the same layout, whatever the slot count says
              for (int slots : {0, K}) {
                if (corpus_chunk(N, ldn, K, k, kk, req, kCorpusBudgetBytes, false, slots) != nq0) return fail("chunk moved", nq0, slots);
                const CorpusLayout Lf = corpus_layout(N, ldn, K, k, kk, nq0, false, slots);
                if (std::memcmp(&Lf, &L0, sizeof L0) != 0) return fail("layout moved with receipts off", nq0, slots);
              }
              if (L0.s_iters || L0.s_res || L0.r_sums || L0.n_total || L0.n_kept || L0.n_i || L0.n_j || L0.n_z || L0.n_r)
                return fail("receipt offsets set with receipts off", L0.s_iters, L0.n_i);
              for (int full = 0; full < 2; ++full)
                for (int cap : caps) {
                  const int slots = corpus_null_slots(K, full != 0, cap);
                  if (slots < 0 || slots > K || (!full && slots != 0) || (full && cap > 0 && slots > cap) ||
                      (full && cap == 0 && slots != K))
                    return fail("null slots", slots, cap);
                  const int nq = corpus_chunk(N, ldn, K, k, kk, req, kCorpusBudgetBytes, true, slots);
                  if (nq < 1 || nq > req || nq > nq0) return fail("chunk range", nq, req);
                  const CorpusLayout L = corpus_layout(N, ldn, K, k, kk, nq, true, slots);
                  if (nq > 1 && L.total > kCorpusBudgetBytes) return fail("budget", nq, L.total);
                  const CorpusLayout B = corpus_layout(N, ldn, K, k, kk, nq);  // the plain layout of the same chunk
                  if (std::memcmp(&L, &B, offsetof(CorpusLayout, total)) != 0) return fail("an older block moved", nq, slots);
                  const long long old_end = B.total;
                  const long long off[] = {L.s_iters, L.s_res, L.r_sums, L.n_total, L.n_kept, L.n_i, L.n_j, L.n_z, L.n_r, L.total};
                  const long long need[] = {nq * 4LL, nq * 4LL, nq * 32LL, nq * 4LL, nq * 4LL, (long long)nq * slots * 4,
                                            (long long)nq * slots * 4, (long long)nq * slots * 4, (long long)nq * slots * 4};
                  if (off[0] != old_end) return fail("receipt blocks do not follow g_res", off[0], old_end);
                  for (int i = 0; i < 9; ++i) {
                    if (off[i] % 256 != 0) return fail("alignment", i, off[i]);
                    if (off[i] + need[i] > off[i + 1]) return fail("block overlaps its successor", i, off[i]);
                  }
                  if (L.total % 256 != 0 || L.total < old_end) return fail("total", L.total, old_end);
                  // a few KB per query: what the new blocks add is bounded by nq (48 + 16 slots) bytes plus their padding
                  if (L.total - old_end > nq * (48LL + 16LL * slots) + 9 * 256) return fail("growth", L.total - old_end, nq);
                  ++cases;
                }
            }
  std::printf("corpus receipts plan sweep ok (%lld cases)\n", cases);
  return 0;
}

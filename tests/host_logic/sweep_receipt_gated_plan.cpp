// Sweep of receipt_gated_plan.hpp (osc_receipt_gated_many) over N from 1 to 1 000 000, D from 1 to
// 1536, with and without the settle's panel, light and full detail, requested chunks from 0 to 10 000 and budgets from 1 GiB
// down to one byte (too small for one query): the chunk is in [1, 256], at most the request, fits the budget unless it is the
// floor of one query, and is not lowered further than the budget asks; the chunks tile [0, Q) and a query's slab range lies
// inside its chunk's panel; the arrays behind bundle_gated_plan.hpp's are 256-byte aligned, pairwise disjoint, behind the
// panel's block and inside `total`, each large enough for what the kernels and the finish index; the settle's panel is as
// large as X; a narrower chunk fits the block allocated for the widest.  The driver then walks a real scratch block of small
// cases the way the kernels index it, so the sanitizers see the indexing.  Run under -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../oscillink_amd/csrc/receipt_gated_plan.hpp"

using namespace osc::host;

static int fail(const char* what, long long a, long long b) {
  std::printf("ERROR %s (%lld, %lld)\n", what, a, b);
  return 1;
}

struct Block {
  long long at, bytes;
};

static int check_layout(long long N, int D, int nq, bool settle, bool full) {
  const ReceiptGatedLayout L = receipt_gated_layout(N, D, nq, settle, full);
  const GatedLayout P = gated_layout(N, D, nq);
  if (L.panel.total != P.total || L.panel.X != P.X || L.panel.n_live != P.n_live) return fail("panel differs", N, nq);
  const long long spq = gated_slabs_per_query(D), cols = (long long)nq * spq * 32, panel = N * cols * 4;
  const long long qs = L.qs, cell = N * qs, parts = receipt_gated_sum_parts(N), groups = receipt_gated_sum_groups(N);
  if (qs < nq || qs % 4 != 0 || qs - nq >= 4) return fail("pitch", qs, nq);
  if (parts < 1 || parts > kReceiptGatedSumParts) return fail("sum parts", N, parts);
  if (groups * kReceiptGatedFinishRows < parts || groups < 1) return fail("sum groups", groups, parts);
  std::vector<Block> b;
  if (settle) b.push_back({L.U, panel});
  b.push_back({L.dh, nq * 8LL});
  if (full) {
    b.push_back({L.comp, 3 * cell * 8});
    b.push_back({L.z, cell * 4});
    b.push_back({L.j, cell * 4});
    b.push_back({L.r, cell * 4});
    b.push_back({L.zt, N * nq * 4});
    b.push_back({L.sumpart, 3 * parts * nq * 8});
    b.push_back({L.sumfin, groups * nq * 8});
    b.push_back({L.sums, 3 * nq * 8LL});
  }
  long long end = P.total;
  for (size_t i = 0; i < b.size(); ++i) {
    if (b[i].at % 256 != 0) return fail("alignment", (long long)i, b[i].at);
    if (b[i].at < end) return fail("blocks overlap", (long long)i, b[i].at);  // (the blocks are laid out in this order)
    if (b[i].bytes <= 0) return fail("empty block", (long long)i, b[i].bytes);
    end = b[i].at + b[i].bytes;
  }
  if (end > L.total) return fail("block passes total", end, L.total);
  if (settle && L.panel.R - L.panel.X < panel) return fail("settle panel smaller than X", L.U, panel);
  return 0;
}

int main() {
  const long long Ns[] = {1, 2, 31, 32, 33, 97, 4096, 65537, 1000000};
  const int Ds[] = {1, 32, 33, 768, 1536};
  const int reqs[] = {-3, 0, 1, 2, 255, 256, 10000};
  const long long budgets[] = {kGatedBudgetBytes, (long long)1 << 28, (long long)1 << 24, (long long)1 << 16, 4096, 1};
  const int Qs[] = {1, 2, 5, 255, 256, 257, 600};
  long long cases = 0;
  for (long long N : Ns)
    for (int D : Ds)
      for (int mode = 0; mode < 4; ++mode) {
        const bool settle = mode & 1, full = mode & 2;
        const int spq = gated_slabs_per_query(D);
        for (int req : reqs)
          for (long long budget : budgets) {
            const int chunk = receipt_gated_chunk(N, D, settle, full, req, budget);
            const int want = std::min(std::max(req, 1), kGatedMaxChunk);
            if (chunk < 1 || chunk > kGatedMaxChunk) return fail("chunk range", chunk, req);
            if (chunk > want) return fail("chunk above the request", chunk, req);
            if (chunk > gated_chunk(N, D, req, budget)) return fail("chunk above the bundle's", chunk, req);
            const long long total = receipt_gated_layout(N, D, chunk, settle, full).total;
            if (chunk > 1 && total > budget) return fail("budget", chunk, total);
            if (chunk > 1 && budget == kGatedBudgetBytes && total > ((long long)1 << 30)) return fail("1 GiB", chunk, total);
            if (chunk < want && receipt_gated_layout(N, D, chunk + 1, settle, full).total <= budget)
              return fail("chunk lowered further than the budget asks", chunk, req);
            for (int Q : Qs) {
              const int nc = gates_chunk_count(Q, chunk);
              int next = 0;
              for (int c = 0; c < nc; ++c) {
                const int q0 = gates_chunk_begin(c, chunk), nq = gates_chunk_size(Q, c, chunk);
                if (q0 != next || nq < 1 || nq > chunk) return fail("chunks do not tile", q0, nq);
                next = q0 + nq;
                // a query's slabs [t spq, (t + 1) spq) lie inside the chunk's panel: none straddles a chunk
                if (gated_slab_begin(nq - 1, D) + spq != (long long)nq * spq) return fail("slab range", nq, spq);
                if (receipt_gated_layout(N, D, nq, settle, full).total > total) return fail("narrow chunk larger", nq, chunk);
                ++cases;
              }
              if (next != Q) return fail("chunks do not end at Q", next, Q);
            }
            if (check_layout(N, D, chunk, settle, full)) return 1;
            if (check_layout(N, D, 1, settle, full)) return 1;
          }
      }
  // a settling query costs one panel more: 5 against 4
  {
    const ReceiptGatedLayout a = receipt_gated_layout(20000, 128, 8, false, false), s = receipt_gated_layout(20000, 128, 8, true, false);
    if (s.total - a.total != a.panel.R - a.panel.X) return fail("fifth panel", s.total, a.total);
  }
  // config 3's size: one query passes the budget on its own, and the chunk is one query
  if (receipt_gated_chunk(100000, 768, true, true, kGatedMaxChunk, kGatedBudgetBytes) != 1) return fail("config 3 chunk", 0, 0);
  // walk small chunks through a real block as the kernels index them
  for (long long N : {1LL, 33LL, 97LL})
    for (int D : {1, 33, 40, 64})
      for (int nq : {1, 3, 5}) {
        const ReceiptGatedLayout L = receipt_gated_layout(N, D, nq, true, true);
        std::vector<unsigned char> block((size_t)L.total, 0);
        const int spq = gated_slabs_per_query(D), slabs = nq * spq, qs = L.qs;
        const int parts = receipt_gated_sum_parts(N), groups = receipt_gated_sum_groups(N);
        float* X = reinterpret_cast<float*>(block.data() + L.panel.X);
        float* U = reinterpret_cast<float*>(block.data() + L.U);
        double* dh = reinterpret_cast<double*>(block.data() + L.dh);
        double* comp = reinterpret_cast<double*>(block.data() + L.comp);
        float* z = reinterpret_cast<float*>(block.data() + L.z);
        int* j = reinterpret_cast<int*>(block.data() + L.j);
        float* r = reinterpret_cast<float*>(block.data() + L.r);
        float* zt = reinterpret_cast<float*>(block.data() + L.zt);
        double* sumpart = reinterpret_cast<double*>(block.data() + L.sumpart);
        double* sumfin = reinterpret_cast<double*>(block.data() + L.sumfin);
        double* sums = reinterpret_cast<double*>(block.data() + L.sums);
        for (int s = 0; s < slabs; ++s)
          for (long long row = 0; row < N; ++row)
            for (int c = 0; c < 32; ++c) {
              X[((size_t)s * N + row) * 32 + c] = 1.f;
              U[((size_t)s * N + row) * 32 + c] = (float)(row + c);
            }
        for (int t = 0; t < nq; ++t) {
          dh[t] = 1.0;
          for (long long row = 0; row < N; ++row) {
            const size_t o = (size_t)row * qs + t;
            for (int k = 0; k < 3; ++k) comp[(size_t)k * N * qs + o] = 1.0;
            z[o] = 1.f;
            j[o] = 1;
            r[o] = 1.f;
            zt[(size_t)t * N + row] = 1.f;
          }
          for (int k = 0; k < 3; ++k) {
            for (int b = 0; b < parts; ++b) sumpart[((size_t)k * parts + b) * nq + t] = 1.0;
            sums[(size_t)k * nq + t] = 1.0;
          }
          for (int g = 0; g < groups; ++g) sumfin[(size_t)g * nq + t] = 1.0;
        }
        const int t = nq - 1, d = D - 1;
        if (U[((size_t)(t * spq + d / 32) * N + (N - 1)) * 32 + d % 32] != (float)(N - 1 + d % 32)) return fail("walk", N, D);
        ++cases;
      }
  std::printf("receipt gated plan sweep ok (%lld cases)\n", cases);
  return 0;
}

// Sweep of bundle_gated_plan.hpp (osc_bundle_gated_many) over N from 1 to 1 000 000, D from 1 to
// 1536, requested chunks from 0 to 10 000 and budgets from 1 GiB down to one byte (too small for one query): the chunk is in
// [1, 256], at most the request, fits the budget unless it is the floor of one query, and is not lowered further than the
// budget asks; the chunks tile [0, Q); a query's slab range lies inside its chunk's panel and the ranges of a chunk's queries
// tile the panel; the arrays of a chunk are 256-byte aligned, pairwise disjoint and inside `total`, each large enough for
// what the kernels index; a narrower chunk fits the block allocated for the widest; the part count and the part rows are
// functions of N alone (called beside every chunk size and compared).  The driver then walks a real scratch block of small
// cases the way the kernels index it, so the sanitizers see the indexing.  Run under -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../oscillink_amd/csrc/bundle_gated_plan.hpp"

using namespace osc::host;

static int fail(const char* what, long long a, long long b) {
  std::printf("ERROR %s (%lld, %lld)\n", what, a, b);
  return 1;
}

struct Block {
  long long at, bytes;
};

static int check_layout(long long N, int D, int nq) {
  const GatedLayout L = gated_layout(N, D, nq);
  const long long spq = gated_slabs_per_query(D), slabs = nq * spq, cols = slabs * 32, parts = gates_parts(N);
  const long long panel = N * cols * 4;
  const Block b[] = {{L.X, panel},           {L.R, panel},       {L.P, panel},        {L.AP, panel},
                     {L.gate_api, nq * N * 4}, {L.gate, nq * N * 4}, {L.psi, cols * 4},
                     {L.part_a, slabs * parts * 32 * 8},          {L.part_b, slabs * parts * 32 * 8},
                     {L.rz, cols * 8},       {L.alpha, cols * 4}, {L.beta, cols * 4},  {L.res, nq * 4LL},
                     {L.live, nq * 4LL},     {L.iters, nq * 4LL}, {L.n_live, 8}};
  const int n = (int)(sizeof b / sizeof b[0]);
  long long end = 0;
  for (int i = 0; i < n; ++i) {
    if (b[i].at % 256 != 0) return fail("alignment", i, b[i].at);
    if (b[i].at < end) return fail("blocks overlap", i, b[i].at);  // (the blocks are laid out in this order)
    if (b[i].bytes <= 0) return fail("empty block", i, b[i].bytes);
    end = b[i].at + b[i].bytes;
  }
  if (end > L.total) return fail("block passes total", end, L.total);
  if (spq * 32 < D || spq * 32 - D >= 32) return fail("slabs per query", spq, D);
  return 0;
}

int main() {
  const long long Ns[] = {1, 2, 31, 32, 33, 97, 65536, 65537, 1000000};
  const int Ds[] = {1, 32, 33, 768, 1536};
  const int reqs[] = {-3, 0, 1, 2, 255, 256, 10000};
  const long long budgets[] = {kGatedBudgetBytes, (long long)1 << 28, (long long)1 << 24, (long long)1 << 16, 4096, 1};
  const int Qs[] = {1, 2, 5, 255, 256, 257, 600};
  long long cases = 0;
  for (long long N : Ns) {
    const int pr = gates_part_rows(N), parts = gates_parts(N);
    if (pr < kGatesStepRows || pr % kGatesStepRows != 0) return fail("part rows", N, pr);
    if (parts < 1 || parts > kGatesMaxParts) return fail("parts", N, parts);
    if ((long long)parts * pr < N || (long long)(parts - 1) * pr >= N) return fail("partition does not cover the rows", N, parts);
    for (int D : Ds) {
      const int spq = gated_slabs_per_query(D);
      for (int req : reqs)
        for (long long budget : budgets) {
          const int chunk = gated_chunk(N, D, req, budget);
          const int want = std::min(std::max(req, 1), kGatedMaxChunk);
          if (chunk < 1 || chunk > kGatedMaxChunk) return fail("chunk range", chunk, req);
          if (chunk > want) return fail("chunk above the request", chunk, req);
          const long long total = gated_layout(N, D, chunk).total;
          if (chunk > 1 && total > budget) return fail("budget", chunk, total);
          if (chunk < want && gated_layout(N, D, chunk + 1).total <= budget)
            return fail("chunk lowered further than the budget asks", chunk, req);
          for (int Q : Qs) {
            const int nc = gates_chunk_count(Q, chunk);
            int next = 0;
            for (int c = 0; c < nc; ++c) {
              const int q0 = gates_chunk_begin(c, chunk), nq = gates_chunk_size(Q, c, chunk);
              if (q0 != next || nq < 1 || nq > chunk) return fail("chunks do not tile", q0, nq);
              next = q0 + nq;
              // the queries' slab ranges tile the chunk's panel: none straddles a chunk
              long long slab = 0;
              for (int t = 0; t < nq; ++t) {
                if (gated_slab_begin(t, D) != slab) return fail("slab ranges do not tile the panel", t, slab);
                slab += spq;
              }
              if (slab != (long long)nq * spq) return fail("panel slabs", slab, nq);
              if (gated_layout(N, D, nq).total > total) return fail("narrow chunk larger", nq, chunk);
              if (gates_part_rows(N) != pr || gates_parts(N) != parts) return fail("partition changed with the chunk", nq, N);
              ++cases;
            }
            if (next != Q) return fail("chunks do not end at Q", next, Q);
          }
          if (check_layout(N, D, chunk)) return 1;
          if (check_layout(N, D, 1)) return 1;
        }
    }
  }
  if (gates_chunk_count(0, 256) != 0) return fail("Q = 0", 0, 0);
  // config 3's size: one query passes the budget on its own, and the chunk is one query
  if (gated_layout(100000, 768, 1).total <= kGatedBudgetBytes) return fail("config 3 fits", 0, 0);
  if (gated_chunk(100000, 768, kGatedMaxChunk, kGatedBudgetBytes) != 1) return fail("config 3 chunk", 0, 0);
  // walk small panels through a real block as the kernels index them: element (row, col) of query t, the partials at
  // (slab, part), the gates at (query, row), the queries at (query, col)
  for (long long N : {1LL, 33LL, 97LL})
    for (int D : {1, 33, 40, 64})
      for (int nq : {1, 3}) {
        const GatedLayout L = gated_layout(N, D, nq);
        std::vector<unsigned char> block((size_t)L.total, 0);
        const int spq = gated_slabs_per_query(D), slabs = nq * spq, parts = gates_parts(N), pr = gates_part_rows(N);
        float* X = reinterpret_cast<float*>(block.data() + L.X);
        float* AP = reinterpret_cast<float*>(block.data() + L.AP);
        float* gate = reinterpret_cast<float*>(block.data() + L.gate);
        float* psi = reinterpret_cast<float*>(block.data() + L.psi);
        double* pb = reinterpret_cast<double*>(block.data() + L.part_b);
        double* rz = reinterpret_cast<double*>(block.data() + L.rz);
        int* iters = reinterpret_cast<int*>(block.data() + L.iters);
        std::vector<int> seen((size_t)N, 0);
        for (int s = 0; s < slabs; ++s) {
          const int t = s / spq;
          for (int p = 0; p < parts; ++p) {
            const long long r0 = (long long)p * pr, r1 = std::min<long long>(N, r0 + pr);
            for (long long r = r0; r < r1; ++r) {
              if (s == 0) ++seen[(size_t)r];
              gate[(size_t)t * N + r] = 1.f;
              for (int c = 0; c < 32; ++c) {
                X[((size_t)s * N + r) * 32 + c] = (float)(r + c);
                AP[((size_t)s * N + r) * 32 + c] = 1.f;
              }
            }
            for (int c = 0; c < 32; ++c) pb[((size_t)s * parts + p) * 32 + c] = 1.0;
          }
          for (int c = 0; c < 32; ++c) {
            rz[(size_t)s * 32 + c] = 1.0;
            psi[(size_t)t * spq * 32 + (s % spq) * 32 + c] = 1.f;
          }
          iters[t] = 1;
        }
        for (long long r = 0; r < N; ++r)
          if (seen[(size_t)r] != 1) return fail("a row is in no part or in two", r, seen[(size_t)r]);
        // the read-out of query nq - 1: column d of row r
        const int t = nq - 1, d = D - 1;
        if (X[((size_t)(t * spq + d / 32) * N + (N - 1)) * 32 + d % 32] != (float)(N - 1 + d % 32)) return fail("walk", N, D);
        ++cases;
      }
  std::printf("bundle gated plan sweep ok (%lld cases)\n", cases);
  return 0;
}

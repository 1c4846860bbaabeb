// Sweep of chain_many.hpp (the host side of osc_chain_receipt_many): the checks on the caller's chains, where a query's edges
// land in the flat outputs, and a chunk's (query, edge) units with their path ranges.  Every chunk is checked against a dense
// restatement: unit u of query q, edge t is (dev(chain[t]), dev(chain[t + 1])), its path range lists exactly the nonzero
// entries of row i of the dense A_path -- of the query's own chain, or of the lattice's chain when it has one -- in ascending
// column order, and a chain seen twice is packed once.  Batches cross the chunk size, chains have 2 to 1024 nodes with
// repeats, self-steps and revisited edges, rows go through a permutation.  The unit, offset and entry arrays are read at
// exactly their sizes, so an index past an end is an AddressSanitizer report.  Run under -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <vector>

#include "../../oscillink_amd/csrc/chain_many.hpp"

using namespace osc::host;

static int fail(const char* what, long long a, long long b) {
  std::printf("ERROR %s (%lld, %lld)\n", what, a, b);
  return 1;
}

// dense A_path (graph.py:96-111) of a chain in device rows
static std::vector<float> dense_path(const std::vector<int32_t>& rows, const float* w, int N) {
  std::vector<float> A((size_t)N * N, 0.f);
  for (size_t t = 0; t + 1 < rows.size(); ++t) {
    const int i = rows[t], j = rows[t + 1];
    const float v = w ? w[t] : 1.0f;
    A[(size_t)i * N + j] = std::max(A[(size_t)i * N + j], v);
    A[(size_t)j * N + i] = std::max(A[(size_t)j * N + i], v);
  }
  return A;
}

static int check_batch(std::mt19937& rng, int N, int Q, int chunk, int max_len, bool permute, bool own_chain, bool shared,
                       long long* units_seen) {
  std::vector<int32_t> dev((size_t)N);
  std::iota(dev.begin(), dev.end(), 0);
  if (permute) std::shuffle(dev.begin(), dev.end(), rng);
  std::vector<int64_t> off((size_t)Q + 1, 0);
  std::vector<int32_t> nodes;
  std::vector<int32_t> first;
  for (int q = 0; q < Q; ++q) {
    const int len = shared && q ? (int)first.size() : (max_len >= kCorpusMaxChain ? max_len : 2 + (int)(rng() % (unsigned)(max_len - 1)));
    for (int t = 0; t < len; ++t) {
      int32_t v = (int32_t)(rng() % (unsigned)std::min(N, 1 + (int)(rng() % (unsigned)N)));
      if (t && rng() % 5 == 0) v = nodes.back();  // a self-step
      if (shared && q) v = first[(size_t)t];
      nodes.push_back(v);
      if (!q) first.push_back(v);
    }
    off[(size_t)q + 1] = (int64_t)nodes.size();
  }
  int32_t where = -1;
  if (chain_many_check(off.data(), nodes.data(), Q, N, &where) != 0) return fail("a valid batch is refused", where, Q);
  // the edge offsets are the running edge count
  int64_t edges = 0;
  for (int q = 0; q <= Q; ++q) {
    if (chain_many_edge_at(off.data(), q) != edges) return fail("edge offset", q, edges);
    if (q < Q) edges += off[(size_t)q + 1] - off[(size_t)q] - 1;
  }
  ChainManyPaths paths;
  int32_t own = -1;
  std::vector<float> own_dense;
  if (own_chain) {
    std::vector<int32_t> rows(2 + rng() % 9);
    std::vector<float> w(rows.size() - 1);
    for (auto& v : rows) v = dev[rng() % (unsigned)N];
    for (auto& v : w) v = rng() % 6 == 0 ? -0.5f : 0.25f * (float)(1 + rng() % 8);
    own = paths.add(rows.data(), w.data(), (int32_t)rows.size(), N);
    own_dense = dense_path(rows, w.data(), N);
  }
  std::vector<ChainManyUnit> units;
  std::vector<int32_t> eoff;
  for (int c0 = 0; c0 < Q; c0 += chunk) {
    const int nq = std::min(chunk, Q - c0);
    if (own < 0) paths.clear();
    chain_many_units(off.data(), nodes.data(), c0, nq, permute ? dev.data() : nullptr, N, own, paths, units, eoff);
    // exact-size copies: what the driver uploads
    const std::vector<ChainManyUnit> U(units.begin(), units.end());
    const std::vector<int32_t> E(eoff.begin(), eoff.end()), pcol(paths.pcol.begin(), paths.pcol.end());
    const std::vector<float> pa(paths.pa.begin(), paths.pa.end());
    if ((int)E.size() != nq + 1 || E[0] != 0 || E[(size_t)nq] != (int32_t)U.size()) return fail("eoff ends", nq, (long long)U.size());
    if ((int64_t)U.size() != chain_many_edge_at(off.data(), c0 + nq) - chain_many_edge_at(off.data(), c0))
      return fail("the chunk's units are not its queries' edges", c0, (long long)U.size());
    if (own < 0 && shared && paths.paths.size() != 1) return fail("a shared chain is packed more than once", c0, (long long)paths.paths.size());
    if (own >= 0 && paths.paths.size() != 1) return fail("a chain was packed beside the lattice's own", c0, (long long)paths.paths.size());
    for (int t = 0; t < nq; ++t) {
      const int64_t b = off[(size_t)(c0 + t)];
      const int len = (int)(off[(size_t)(c0 + t) + 1] - b);
      if (E[(size_t)t + 1] - E[(size_t)t] != len - 1) return fail("units of a query", c0 + t, len);
      std::vector<int32_t> rows((size_t)len);
      for (int s = 0; s < len; ++s) rows[(size_t)s] = dev[(size_t)nodes[(size_t)(b + s)]];
      const std::vector<float> A = own >= 0 ? own_dense : dense_path(rows, nullptr, N);
      for (int s = 0; s + 1 < len; ++s) {
        const ChainManyUnit& u = U[(size_t)E[(size_t)t] + s];
        if (u.q != t || u.i != rows[(size_t)s] || u.j != rows[(size_t)s + 1]) return fail("unit", c0 + t, s);
        if (u.pb < 0 || u.pb > u.pe || u.pe > (int32_t)pcol.size()) return fail("path range", u.pb, u.pe);
        int listed = 0, dense = 0;
        for (int c = 0; c < N; ++c) dense += A[(size_t)u.i * N + c] != 0.f;
        for (int e = u.pb; e < u.pe; ++e) {
          const int c = pcol[(size_t)e];
          if (c < 0 || c >= N || (e > u.pb && pcol[(size_t)e - 1] >= c)) return fail("path columns", u.i, c);
          if (pa[(size_t)e] != A[(size_t)u.i * N + c]) return fail("A_path entry", u.i, c);
          listed += pa[(size_t)e] != 0.f;
        }
        if (listed != dense) return fail("a dense path entry is not listed", listed, dense);
        if (own < 0 && u.pb == u.pe) return fail("a chain node without a path row", u.i, s);
        ++*units_seen;
      }
    }
  }
  return 0;
}

static int sweep_checks() {
  const int32_t nodes[] = {0, 1, 2, 3, 4, 5};
  int32_t where = -1;
  const int64_t good[] = {0, 2, 6};
  if (chain_many_check(good, nodes, 2, 6, &where) != 0) return fail("good chains refused", where, 0);
  if (chain_many_check(good, nodes, 0, 6, &where) != 0) return fail("Q = 0 refused", where, 0);
  if (chain_many_check(good, nodes, 2, 5, &where) != 2 || where != 1) return fail("node == N accepted", where, 0);
  const int32_t neg[] = {0, -1};
  if (chain_many_check(good, neg, 1, 6, &where) != 2 || where != 0) return fail("node -1 accepted", where, 0);
  const int64_t from1[] = {1, 3}, single[] = {0, 2, 3}, back[] = {0, 4, 2};
  if (chain_many_check(from1, nodes, 1, 6, &where) != 1) return fail("offsets from 1 accepted", where, 0);
  if (chain_many_check(single, nodes, 2, 6, &where) != 1 || where != 1) return fail("a one-node chain accepted", where, 0);
  if (chain_many_check(back, nodes, 2, 6, &where) != 1 || where != 1) return fail("descending offsets accepted", where, 0);
  std::vector<int32_t> big((size_t)kCorpusMaxChain + 1, 0);
  const int64_t most[] = {0, kCorpusMaxChain}, over[] = {0, kCorpusMaxChain + 1};
  if (chain_many_check(most, big.data(), 1, 1, &where) != 0) return fail("1024 nodes refused", where, 0);
  if (chain_many_check(over, big.data(), 1, 1, &where) != 1) return fail("1025 nodes accepted", where, 0);
  return 0;
}

int main() {
  if (sweep_checks()) return 1;
  std::mt19937 rng(2468);
  long long batches = 0, units = 0;
  for (int N : {2, 7, 61})
    for (int Q : {1, 3, 9})
      for (int chunk : {1, 4, 256})
        for (int mode = 0; mode < 8; ++mode) {
          if (check_batch(rng, N, Q, chunk, N == 61 ? 40 : 9, (mode & 1) != 0, (mode & 2) != 0, (mode & 4) != 0, &units))
            return fail("batch", N, Q);
          ++batches;
        }
  // the longest chain, and a batch across the real chunk size
  if (check_batch(rng, 5, 2, 256, 1024, true, false, false, &units)) return 1;
  if (check_batch(rng, 33, 300, 256, 9, true, false, false, &units)) return 1;
  if (check_batch(rng, 33, 300, 256, 9, false, true, true, &units)) return 1;
  batches += 3;
  std::printf("chain many sweep ok (%lld batches, %lld units)\n", batches, units);
  return 0;
}

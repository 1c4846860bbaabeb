// Sweep of the balanced source-block order's host reference (oscillink_amd/csrc/block_balance.hpp), built with a plain host
// compiler by tests/test_block_balance_host.py (once plain, once under -fsanitize=address,undefined).  Over generated
// symmetric graphs (N 1..1500, 1..32 blocks, 1..4 slots, degrees 0..40, isolated rows, rows above nb x slots) it checks:
// the output is a permutation; every block holds the contiguous range of stored rows the blocked copy cuts
// (blocked_rows_per_block, ragged last block and empty blocks included), in ascending API id; the displaced edges counted
// independently on the returned order equal the reported count and are no more than the API order's; two calls agree.
// Edge cases: nb = 1, N below nb, an already balanced graph (no swap, identity).  argv[1]: the fixture graph
// (tests/golden/block_balance_knn4096.bin), on which the displaced share must fall as far as the runner's docstring says
// (argv[2]: that fraction).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>

#include "../../oscillink_amd/csrc/block_balance.hpp"

using namespace osc::host;

static int g_fail = 0;
static long g_cases = 0;
#define CHECK(cond, ...)                                                  \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::fprintf(stderr, "FAIL %s:%d %s  ", __FILE__, __LINE__, #cond); \
      std::fprintf(stderr, __VA_ARGS__);                                  \
      std::fprintf(stderr, "\n");                                         \
      if (++g_fail > 20) std::exit(1);                                    \
    }                                                                     \
  } while (0)

struct Ell {
  int32_t N = 0, width = 1;
  std::vector<int32_t> col, deg;
};

static Ell from_sets(const std::vector<std::set<int32_t>>& adj) {
  Ell g;
  g.N = (int32_t)adj.size();
  for (auto& s : adj) g.width = std::max<int32_t>(g.width, (int32_t)s.size());
  g.col.assign((size_t)g.N * g.width, 0);
  g.deg.assign((size_t)g.N, 0);
  for (int32_t i = 0; i < g.N; ++i)
    for (int32_t j : adj[(size_t)i]) g.col[(size_t)i * g.width + g.deg[(size_t)i]++] = j;
  return g;
}

static uint64_t g_rng = 0x2545F4914F6CDD1Dull;
static uint32_t rnd() {
  g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17;
  return (uint32_t)(g_rng >> 20);
}

// about `mean` edges per row, the first `isolated` rows without any, row N - 1 joined to `hub` others
static Ell random_graph(int32_t N, int mean, int isolated, int hub) {
  std::vector<std::set<int32_t>> adj((size_t)N);
  const int32_t lo = std::min(isolated, N);
  if (N - lo >= 2)
    for (int64_t e = 0; e < (int64_t)(N - lo) * mean / 2; ++e) {
      const int32_t i = lo + (int32_t)(rnd() % (uint32_t)(N - lo)), j = lo + (int32_t)(rnd() % (uint32_t)(N - lo));
      if (i != j) adj[(size_t)i].insert(j), adj[(size_t)j].insert(i);
    }
  for (int32_t j = lo; j < std::min(N - 1, lo + hub); ++j) adj[(size_t)N - 1].insert(j), adj[(size_t)j].insert(N - 1);
  return from_sets(adj);
}

static void check_graph(const Ell& g, int nb, int slots, const char* what, BalanceStats* out = nullptr, std::vector<int32_t>* perm_out = nullptr) {
  ++g_cases;
  BalanceStats st, st2;
  std::vector<int32_t> pos;
  balance_assign(g.col.data(), g.deg.data(), g.width, g.N, nb, slots, pos, &st);
  const std::vector<int32_t> perm = balance_blocks(g.col.data(), g.deg.data(), g.width, g.N, nb, slots, &st2);
  const std::vector<int32_t> again = balance_blocks(g.col.data(), g.deg.data(), g.width, g.N, nb, slots);
  CHECK(perm == again, "%s N %d nb %d: two calls differ", what, g.N, nb);
  CHECK(st.displaced_after == st2.displaced_after && st.rounds == st2.rounds && st.swaps == st2.swaps, "%s: statistics differ", what);
  CHECK((int32_t)perm.size() == g.N && (int32_t)pos.size() == g.N, "%s: sizes", what);
  std::vector<int32_t> inv((size_t)g.N, -1);
  for (int32_t p = 0; p < g.N; ++p) {
    CHECK(perm[(size_t)p] >= 0 && perm[(size_t)p] < g.N && inv[(size_t)perm[(size_t)p]] < 0, "%s N %d nb %d: not a permutation at %d", what, g.N, nb, p);
    if (perm[(size_t)p] >= 0 && perm[(size_t)p] < g.N) inv[(size_t)perm[(size_t)p]] = p;
  }
  // blocks: the stored range [b rpb, (b + 1) rpb) holds exactly the rows assigned to block b, ascending
  const int32_t rpb = blocked_rows_per_block(g.N, nb);
  CHECK((int64_t)rpb * nb >= g.N && rpb >= 1, "%s: rpb %d", what, rpb);
  for (int32_t r = 0; r < g.N; ++r)
    CHECK(blk_of(inv[(size_t)r], rpb, nb) == blk_of(pos[(size_t)r], rpb, nb), "%s N %d nb %d: row %d stored in block %d, assigned %d", what,
          g.N, nb, r, blk_of(inv[(size_t)r], rpb, nb), blk_of(pos[(size_t)r], rpb, nb));
  for (int32_t p = 1; p < g.N; ++p)
    if (p / rpb == (p - 1) / rpb) CHECK(perm[(size_t)p] > perm[(size_t)p - 1], "%s: block %d not ascending at %d", what, p / rpb, p);
  CHECK(st.displaced_before == balance_displaced(g.col.data(), g.deg.data(), g.width, g.N, nb, slots, nullptr), "%s: displaced before", what);
  CHECK(st.displaced_after == balance_displaced(g.col.data(), g.deg.data(), g.width, g.N, nb, slots, inv.data()),
        "%s N %d nb %d: displaced after %lld, counted %lld", what, g.N, nb, (long long)st.displaced_after,
        (long long)balance_displaced(g.col.data(), g.deg.data(), g.width, g.N, nb, slots, inv.data()));
  CHECK(st.displaced_after <= st.displaced_before, "%s N %d nb %d: %lld -> %lld", what, g.N, nb, (long long)st.displaced_before,
        (long long)st.displaced_after);
  CHECK(st.rounds >= 1 && st.rounds <= kBalanceRounds && (int)st.swaps.size() == st.rounds, "%s: rounds %d", what, st.rounds);
  for (int32_t s : st.swaps) CHECK(s >= 0 && s <= g.N && (s & 1) == 0, "%s: %d rows moved in a round", what, s);
  if (out) *out = st;
  if (perm_out) *perm_out = perm;
}

int main(int argc, char** argv) {
  for (int32_t N : {1, 2, 3, 5, 7, 8, 9, 31, 64, 100, 257, 1000, 1500})
    for (int nb : {1, 2, 3, 5, 8, 9, 32})
      for (int slots : {1, 4})
        for (int mean : {0, 3, 12, 40}) {
          if (N > 300 && (slots == 1) != (mean == 12)) continue;
          const Ell g = random_graph(N, mean, N / 10, nb * slots + 3);  // the hub row: more edges than nb x slots where N allows
          check_graph(g, nb, slots, "random");
        }
  {  // nb = 1: one block, nothing to trade
    const Ell g = random_graph(200, 10, 3, 0);
    BalanceStats st;
    std::vector<int32_t> perm;
    check_graph(g, 1, 4, "one block", &st, &perm);
    for (int32_t p = 0; p < g.N; ++p) CHECK(perm[(size_t)p] == p, "one block: not the identity at %d", p);
    CHECK(st.rounds == 1 && st.swaps[0] == 0, "one block: rounds %d", st.rounds);
  }
  {  // N below nb: blocks of one row, the last ones empty
    const Ell g = random_graph(5, 3, 0, 4);
    check_graph(g, 8, 4, "N below nb");
    check_graph(g, 32, 1, "N below nb");
  }
  {  // already balanced: row i's neighbours i + 8 k (mod 64), one in each of the other blocks of 8 rows
    std::vector<std::set<int32_t>> adj(64);
    for (int32_t i = 0; i < 64; ++i)
      for (int k = 1; k < 8; ++k) adj[(size_t)i].insert((i + 8 * k) % 64);
    const Ell g = from_sets(adj);
    for (int slots : {1, 4}) {
      BalanceStats st;
      std::vector<int32_t> perm;
      check_graph(g, 8, slots, "balanced", &st, &perm);
      CHECK(st.displaced_before == 0 && st.displaced_after == 0 && st.rounds == 1 && st.swaps[0] == 0, "balanced: %lld displaced, %d rounds",
            (long long)st.displaced_before, st.rounds);
      for (int32_t p = 0; p < 64; ++p) CHECK(perm[(size_t)p] == p, "balanced: not the identity at %d", p);
    }
  }
  {  // bad input is refused before anything is read through it
    Ell g = random_graph(10, 3, 0, 0);
    bool threw = false;
    if (g.deg[0] > 0) {
      g.col[0] = 10;
      try {
        balance_blocks(g.col.data(), g.deg.data(), g.width, g.N, 2, 4);
      } catch (const InvalidArg&) {
        threw = true;
      }
      CHECK(threw, "neighbour id N accepted");
    }
  }
  if (argc > 2) {  // the fixture graph: int32 N, int32 nnz, int32 rowptr[N + 1], uint16 col[nnz]
    FILE* f = std::fopen(argv[1], "rb");
    CHECK(f != nullptr, "cannot open %s", argv[1]);
    if (f) {
      int32_t hdr[2] = {0, 0};
      CHECK(std::fread(hdr, 4, 2, f) == 2 && hdr[0] > 0 && hdr[0] <= 65536 && hdr[1] >= 0, "fixture header");
      std::vector<int32_t> rowptr((size_t)hdr[0] + 1);
      std::vector<uint16_t> col((size_t)hdr[1]);
      CHECK(std::fread(rowptr.data(), 4, rowptr.size(), f) == rowptr.size(), "fixture rowptr");
      CHECK(std::fread(col.data(), 2, col.size(), f) == col.size(), "fixture col");
      std::fclose(f);
      std::vector<std::set<int32_t>> adj((size_t)hdr[0]);
      for (int32_t i = 0; i < hdr[0]; ++i)
        for (int32_t q = rowptr[(size_t)i]; q < rowptr[(size_t)i + 1]; ++q) adj[(size_t)i].insert(col[(size_t)q]);
      const Ell g = from_sets(adj);
      BalanceStats st;
      check_graph(g, 8, 4, "fixture", &st);
      const double frac = std::atof(argv[2]);
      std::printf("fixture: N %d nnz %d displaced %lld -> %lld (%.4f of the API order's) in %d rounds\n", g.N, hdr[1], (long long)st.displaced_before,
                  (long long)st.displaced_after, (double)st.displaced_after / (double)std::max<int64_t>(1, st.displaced_before), st.rounds);
      CHECK((double)st.displaced_after <= frac * (double)st.displaced_before, "fixture: %lld -> %lld, allowed fraction %.3f",
            (long long)st.displaced_before, (long long)st.displaced_after, frac);
    }
  }
  if (g_fail) {
    std::fprintf(stderr, "%d failures\n", g_fail);
    return 1;
  }
  std::printf("block balance sweep ok (%ld cases)\n", g_cases);
  return 0;
}

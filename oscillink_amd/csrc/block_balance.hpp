// Balanced source blocks: a row order under which every row's neighbours spread over the source blocks of the blocked
// matvec with at most `slots` of them in each, so that fewer edges are displaced into another block's free slot
// (common.hpp: BlockedView; DESIGN.md section 4, "Balanced source blocks").  HIP-free: osc_graph.hip runs the final
// ordering step and, with OSC_BALANCE_HOST=1, the whole of it; balance_kernels.hip runs the rounds on the device and must
// return the same assignment to the element; tests/host_logic/sweep_block_balance.cpp sweeps it under the sanitizers.
//
// A block is the contiguous range of stored positions [b rpb, (b + 1) rpb), rpb = blocked_rows_per_block(N, nb) -- the
// ranges k_blk_fill cuts -- so the block sizes are fixed and rows can only trade places.  The scheme is synchronous and
// deterministic.  Per round t (at most kBalanceRounds):
//   counts    cnt[i][b] = neighbours of row i stored in block b, recounted from scratch; the objective is
//             sum_i sum_b max(0, cnt[i][b] - slots), the displaced edges;
//   proposals a quarter of the rows is active (balance_active: a fixed hash of (row, t)); an active row j of block a
//             computes for every other block b   g = #{i in adj(j): cnt[i][a] > slots} - #{i in adj(j): cnt[i][b] >= slots}
//             (the graph is symmetric: adj(j) is also the set of rows that gather j) and proposes the b with the largest
//             g > 0, the smallest such b on a tie;
//   exchange  for every pair a < b the k-th proposer a -> b and the k-th proposer b -> a, by ascending stored position,
//             trade positions for k < min of the two counts; the other proposers stay;
//   stop      after a round that moved fewer than N / kBalanceStopDiv rows.
// The rounds are not monotone, so the assignment with the fewest displaced edges seen at any round start (the first such)
// is the one kept: never worse than the order it started from.  The result is block-major with ascending API id inside
// a block, so it depends on the kept assignment alone.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "host_logic.hpp"

#if defined(__HIPCC__)
#define OSC_BAL_HD __host__ __device__
#else
#define OSC_BAL_HD
#endif

namespace osc {
namespace host {

constexpr int kBalanceRounds = 40;
constexpr int64_t kBalanceStopDiv = 4000;

// is row `row` active in round t?  (a quarter of the rows, another quarter every round)
OSC_BAL_HD inline bool balance_active(uint32_t row, uint32_t t) {
  uint32_t h = row * 0x9E3779B1u + t * 0x85EBCA6Bu;
  h ^= h >> 15;
  h *= 0x2C1B3C6Du;
  h ^= h >> 12;
  h *= 0x297A2D39u;
  h ^= h >> 15;
  return (h & 3u) == 0u;
}
// does a round that moved `swaps` rows end the search?
OSC_BAL_HD inline bool balance_stops(int64_t swaps, int64_t N) { return swaps * kBalanceStopDiv < N; }

struct BalanceStats {
  int64_t displaced_before = 0, displaced_after = 0;
  int rounds = 0;               // rounds run
  std::vector<int32_t> swaps;   // rows moved per round
};

// The stored order of a block assignment: pos[r] = stored position of API row r under it (only its block matters).
// perm[new] = old, block-major, ascending API id inside a block.
inline std::vector<int32_t> balance_order(const int32_t* pos, int32_t N, int nb) {
  const int32_t rpb = blocked_rows_per_block(N, nb);
  std::vector<int32_t> start((size_t)nb + 1, 0), perm((size_t)std::max(N, 0));
  for (int32_t r = 0; r < N; ++r) ++start[(size_t)blk_of(pos[r], rpb, nb) + 1];
  for (int b = 0; b < nb; ++b) start[(size_t)b + 1] += start[(size_t)b];
  for (int32_t r = 0; r < N; ++r) perm[(size_t)start[(size_t)blk_of(pos[r], rpb, nb)]++] = r;
  return perm;
}

// displaced edges of the graph when API row r is stored at pos[r] (pos == nullptr: the API order)
inline int64_t balance_displaced(const int32_t* col, const int32_t* deg, int32_t width, int32_t N, int nb, int slots, const int32_t* pos) {
  const int32_t rpb = blocked_rows_per_block(N, nb);
  std::vector<int32_t> c((size_t)nb);
  int64_t d = 0;
  for (int32_t i = 0; i < N; ++i) {
    std::fill(c.begin(), c.end(), 0);
    for (int e = 0; e < deg[i]; ++e) {
      const int32_t j = col[(size_t)i * width + e];
      ++c[(size_t)blk_of(pos ? pos[j] : j, rpb, nb)];
    }
    for (int b = 0; b < nb; ++b) d += std::max(0, c[(size_t)b] - slots);
  }
  return d;
}

// The block assignment itself: pos_out[r] = stored position of API row r (N entries).  ELL graph: col [N][width], deg [N].
inline void balance_assign(const int32_t* col, const int32_t* deg, int32_t width, int32_t N, int nb, int slots, std::vector<int32_t>& pos_out,
                           BalanceStats* stats) {
  if (N < 0 || nb < 1 || nb > OSC_MAX_SRC_BLOCKS || slots < 1 || width < 0) throw InvalidArg("balance_assign: bad sizes");
  for (int32_t i = 0; i < N; ++i) {
    if (deg[i] < 0 || deg[i] > width) throw InvalidArg("balance_assign: degree out of range");
    for (int e = 0; e < deg[i]; ++e)
      if (col[(size_t)i * width + e] < 0 || col[(size_t)i * width + e] >= N) throw InvalidArg("balance_assign: neighbour id out of range");
  }
  const int32_t rpb = blocked_rows_per_block(N, nb);
  std::vector<int32_t> pos((size_t)N), rowat((size_t)N), prop((size_t)N), best;
  for (int32_t r = 0; r < N; ++r) pos[(size_t)r] = rowat[(size_t)r] = r;
  std::vector<uint32_t> gt((size_t)N), ge((size_t)N);  // bit b: cnt[i][b] > slots / >= slots
  std::vector<int32_t> c((size_t)nb);
  auto blk = [&](int32_t r) { return blk_of(pos[(size_t)r], rpb, nb); };
  auto recount = [&]() {
    int64_t d = 0;
    for (int32_t i = 0; i < N; ++i) {
      std::fill(c.begin(), c.end(), 0);
      for (int e = 0; e < deg[i]; ++e) ++c[(size_t)blk(col[(size_t)i * width + e])];
      uint32_t g = 0, q = 0;
      for (int b = 0; b < nb; ++b) {
        d += std::max(0, c[(size_t)b] - slots);
        if (c[(size_t)b] > slots) g |= 1u << b;
        if (c[(size_t)b] >= slots) q |= 1u << b;
      }
      gt[(size_t)i] = g, ge[(size_t)i] = q;
    }
    return d;
  };
  BalanceStats st;
  int64_t best_d = 0;
  auto keep = [&](int64_t d, bool first) {
    if (first || d < best_d) best_d = d, best = pos;
  };
  std::vector<std::vector<int32_t>> lists((size_t)nb * nb);
  for (int t = 0; t < kBalanceRounds; ++t) {
    const int64_t d = recount();
    if (t == 0) st.displaced_before = d;
    keep(d, t == 0);
    for (int32_t j = 0; j < N; ++j) {
      prop[(size_t)j] = -1;
      if (!balance_active((uint32_t)j, (uint32_t)t)) continue;
      const int a = blk(j);
      int out = 0;
      std::fill(c.begin(), c.end(), 0);
      for (int e = 0; e < deg[j]; ++e) {
        const int32_t i = col[(size_t)j * width + e];
        out += (int)((gt[(size_t)i] >> a) & 1u);
        for (int b = 0; b < nb; ++b) c[(size_t)b] += (int)((ge[(size_t)i] >> b) & 1u);
      }
      int best_g = 0, best_b = -1;
      for (int b = 0; b < nb; ++b)
        if (b != a && out - c[(size_t)b] > best_g) best_g = out - c[(size_t)b], best_b = b;
      prop[(size_t)j] = best_b;
    }
    for (auto& l : lists) l.clear();
    for (int32_t p = 0; p < N; ++p) {
      const int32_t r = rowat[(size_t)p];
      if (prop[(size_t)r] >= 0) lists[(size_t)blk_of(p, rpb, nb) * nb + prop[(size_t)r]].push_back(r);
    }
    int64_t swaps = 0;
    for (int a = 0; a < nb; ++a)
      for (int b = a + 1; b < nb; ++b) {
        const auto &ab = lists[(size_t)a * nb + b], &ba = lists[(size_t)b * nb + a];
        const size_t m = std::min(ab.size(), ba.size());
        for (size_t k = 0; k < m; ++k) {
          const int32_t r = ab[k], s = ba[k];
          std::swap(pos[(size_t)r], pos[(size_t)s]);
          rowat[(size_t)pos[(size_t)r]] = r;
          rowat[(size_t)pos[(size_t)s]] = s;
        }
        swaps += 2 * (int64_t)m;
      }
    st.swaps.push_back((int32_t)swaps);
    st.rounds = t + 1;
    if (balance_stops(swaps, N)) break;
  }
  keep(recount(), false);
  st.displaced_after = best_d;
  pos_out = best;
  if (stats) *stats = st;
}

// perm[new] = old
inline std::vector<int32_t> balance_blocks(const int32_t* col, const int32_t* deg, int32_t width, int32_t N, int nb, int slots,
                                           BalanceStats* stats = nullptr) {
  std::vector<int32_t> pos;
  balance_assign(col, deg, width, N, nb, slots, pos, stats);
  return balance_order(pos.data(), N, nb);
}

}  // namespace host
}  // namespace osc

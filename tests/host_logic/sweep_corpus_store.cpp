// Sweep of corpus_store.hpp (the row-store arithmetic of a mutable corpus): capacity growth from 1 row to the id limit and
// past it, bitmap word counts and tail masks for every N mod 32, popcounts of live & allow against a bit-by-bit loop, and
// compaction maps of random tombstone sets.  Run under -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../oscillink_amd/csrc/corpus_store.hpp"

using namespace osc::host;

static int fail(const char* what, long long a, long long b) {
  std::printf("ERROR %s (%lld, %lld)\n", what, a, b);
  return 1;
}

static uint32_t rnd(uint64_t& s) {  // splitmix64
  s += 0x9e3779b97f4a7c15ull;
  uint64_t z = s;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return (uint32_t)((z ^ (z >> 31)) >> 16);
}

int main() {
  long long cases = 0;
  // growth: one row at a time from an empty store, then by need = cap + 1 up to the limit; beyond it, -1
  for (long long step : {1LL, 7LL, 1000LL, 1LL << 20}) {
    long long cap = 0, n = 0, moves = 0;
    while (n < kCorpusMaxRows) {
      n = std::min<long long>(kCorpusMaxRows, n + (n < 100000 ? step : std::max(step, cap / 3)));
      if (n <= cap) continue;
      const long long c1 = store_capacity(cap, n);
      if (c1 < n) return fail("capacity below need", c1, n);
      if (c1 % kCorpusCapStep != 0) return fail("capacity not a whole tile", c1, n);
      if (cap > 0 && c1 < cap + cap / 2 && c1 < kCorpusMaxRows) return fail("growth below 1.5x", c1, cap);
      if (c1 > kCorpusMaxRows + kCorpusCapStep) return fail("capacity far past the id limit", c1, n);
      if (c1 > std::max(n, cap + cap / 2) + kCorpusCapStep) return fail("capacity above the policy", c1, n);
      cap = c1;
      ++moves;
      ++cases;
    }
    if (step >= 1000 && moves > 200) return fail("growth is not geometric", moves, step);
    if (store_capacity(cap, kCorpusMaxRows + 1) != -1) return fail("need past the id limit accepted", cap, 0);
    if (store_capacity(cap, (long long)1 << 40) != -1) return fail("huge need accepted", cap, 0);
    if (store_capacity(cap, -1) != -1) return fail("negative need accepted", cap, 0);
  }
  if (store_capacity(0, 0) != 0 || store_capacity(0, 1) != 128 || store_capacity(128, 129) != 256 ||
      store_capacity(1024, 1025) != 1536 || store_capacity(333, 428) != 512)
    return fail("capacity examples", store_capacity(1024, 1025), store_capacity(333, 428));
  // tail masks and word counts
  for (long long n = 0; n <= 200; ++n) {
    const long long nw = store_words(n);
    if (nw * 32 < n || (nw > 0 && (nw - 1) * 32 >= n)) return fail("words", n, nw);
    uint32_t want = 0u;
    for (long long i = (nw - 1) * 32; nw > 0 && i < n; ++i) want |= 1u << (i & 31);
    if (store_tail_mask(n) != want) return fail("tail mask", n, store_tail_mask(n));
    ++cases;
  }
  if (store_tail_mask(kCorpusMaxRows) != 0x7fffffffu) return fail("tail mask at the limit", 0, 0);
  // popcounts and compaction maps
  uint64_t seed = 1;
  for (long long n : {1LL, 2LL, 31LL, 32LL, 33LL, 63LL, 64LL, 65LL, 600LL, 1100LL, 4099LL})
    for (int density : {0, 1, 50, 99, 100})
      for (int rep = 0; rep < 4; ++rep) {
        const long long nw = store_words(n);
        std::vector<uint32_t> live((size_t)nw, 0u), allow((size_t)nw, 0u);
        std::vector<char> lb((size_t)n), ab((size_t)n);
        for (long long i = 0; i < n; ++i) {
          lb[(size_t)i] = (int)(rnd(seed) % 100) < density;
          ab[(size_t)i] = (rnd(seed) & 1u) != 0u;
          if (lb[(size_t)i]) store_set(live.data(), i);
          if (ab[(size_t)i]) store_set(allow.data(), i);
        }
        std::vector<uint32_t> dirty = allow;  // a filter may carry bits beyond N: they must not count
        if (nw > 0) dirty.back() |= ~store_tail_mask(n);
        long long both = 0, alive = 0;
        for (long long i = 0; i < n; ++i) {
          if (store_get(live.data(), i) != (bool)lb[(size_t)i]) return fail("get", n, i);
          alive += lb[(size_t)i];
          both += lb[(size_t)i] && ab[(size_t)i];
        }
        if (store_count(live.data(), nullptr, n) != alive) return fail("count live", n, alive);
        if (store_count(live.data(), allow.data(), n) != both) return fail("count live & allow", n, both);
        if (store_count(live.data(), dirty.data(), n) != both) return fail("count with bits beyond N", n, both);
        std::vector<uint32_t> ones((size_t)nw, 0xffffffffu);
        if (store_count(ones.data(), dirty.data(), n) != store_count(allow.data(), nullptr, n))
          return fail("count of a full word past N", n, 0);
        std::vector<int32_t> map((size_t)n, 7), kept;
        const long long k = store_compact_map(live.data(), n, map.data(), kept);
        if (k != alive || (long long)kept.size() != alive) return fail("kept count", k, alive);
        long long next = 0;
        for (long long i = 0; i < n; ++i) {
          if (lb[(size_t)i]) {
            if (map[(size_t)i] != next || kept[(size_t)next] != i) return fail("map", i, map[(size_t)i]);
            ++next;
          } else if (map[(size_t)i] != -1) {
            return fail("map of a removed row", i, map[(size_t)i]);
          }
        }
        std::vector<int32_t> kept2;
        if (store_compact_map(live.data(), n, nullptr, kept2) != k || kept2 != kept) return fail("map without output", n, k);
        // clearing every live row one by one leaves an empty bitmap
        for (long long i = 0; i < n; ++i)
          if (lb[(size_t)i]) store_clear(live.data(), i);
        if (store_count(live.data(), nullptr, n) != 0) return fail("clear", n, 0);
        ++cases;
      }
  for (uint32_t v : {0u, 1u, 0x80000000u, 0xffffffffu, 0x55555555u, 0x12345678u}) {
    int c = 0;
    for (int b = 0; b < 32; ++b) c += (v >> b) & 1u;
    if (store_popcount(v) != c) return fail("popcount", v, c);
  }
  std::printf("corpus store sweep ok (%lld cases)\n", cases);
  return 0;
}

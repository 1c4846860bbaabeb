// Sweep of derived_state.hpp (which of the handle's caches is computed from what): from every combination of held and
// dropped caches, every input drops exactly the caches whose dependency set names it; the cached row sums never outlive
// the anchors' image or the graph copy they were formed from; the epoch moves by one exactly where the epoch-keyed caches
// depend on the input; a second report of the same input drops nothing more.  The expected dependency sets are written out
// here, independently of the header: an edit there that loses a dependency fails.  Run under -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>

#include "../../oscillink_amd/csrc/derived_state.hpp"

using namespace osc::host;

static int fail(const char* what, long long a, long long b) {
  std::printf("ERROR %s (%lld, %lld)\n", what, a, b);
  return 1;
}

enum { ANCHORS, WINDOW, ROW_ORDER, GRAPH, CHAIN, COMM, QUERY, LAMS, NIN };
enum { ELL_T, BLOCKED, SLAB, WY, USTAR, EPOCH, NCACHE };
static const Input kInputs[NIN] = {Input::anchors, Input::window, Input::row_order, Input::graph,
                                   Input::chain,   Input::comm,   Input::query,     Input::lams};
static const Cache kCaches[NCACHE] = {Cache::ell_t,     Cache::blocked_copy, Cache::anchor_slab,
                                      Cache::anchor_wy, Cache::ustar,        Cache::epoch_keyed};
// what each cache is computed from
static const bool kExpect[NCACHE][NIN] = {
    //            anchors window row_order graph chain comm query lams
    /* ell_t   */ {false, false, true, true, false, false, false, false},
    /* blocked */ {false, false, true, true, false, false, false, false},
    /* slab    */ {true, true, true, false, false, false, false, false},
    /* wy      */ {true, true, true, true, false, false, false, false},
    /* ustar   */ {true, false, true, true, true, true, true, true},
    /* epoch   */ {false, false, true, true, true, true, false, false},
};

// the caches of `a` that `b` no longer holds, as a bit set (the epoch is compared apart)
static unsigned lost(const Derived& a, const Derived& b) {
  unsigned m = 0;
  if (a.ell_t && !b.ell_t) m |= 1u << ELL_T;
  if (a.blk_nb != 0 && b.blk_nb == 0) m |= 1u << BLOCKED;
  if (a.ys && !b.ys) m |= 1u << SLAB;
  if (held(a, Level::wy) && !held(b, Level::wy)) m |= 1u << WY;
  if (a.ustar && !b.ustar) m |= 1u << USTAR;
  return m;
}

int main() {
  if ((int)Input::count != NIN || (int)Cache::count != NCACHE) return fail("enumeration sizes", (int)Input::count, (int)Cache::count);
  for (int c = 0; c < NCACHE; ++c) {
    if ((int)kCaches[c] != c) return fail("cache order", c, (int)kCaches[c]);
    for (int i = 0; i < NIN; ++i) {
      if ((int)kInputs[i] != i) return fail("input order", i, (int)kInputs[i]);
      if (depends_on(kCaches[c], kInputs[i]) != kExpect[c][i]) return fail("dependency table", c, i);
    }
  }
  const int nbs[] = {0, 2, 5};
  const uint64_t epochs[] = {1, 77};
  long long cases = 0;
  for (int ell_t = 0; ell_t < 2; ++ell_t)
    for (int blk : nbs)
      for (int ys = 0; ys < 2; ++ys)
        for (int wy : nbs)
          for (int ustar = 0; ustar < 2; ++ustar)
            for (uint64_t epoch : epochs)
              for (int i = 0; i < NIN; ++i) {
                Derived d0;
                d0.ell_t = ell_t != 0;
                d0.blk_nb = blk;
                d0.ys = ys != 0;
                if (wy != 0) built(d0, Level::wy, wy);
                d0.ustar = ustar != 0;
                d0.epoch = epoch;
                Derived d1 = d0;
                changed(d1, kInputs[i]);
                // 1. dropped if and only if the dependency set holds the input; nothing is ever gained or altered
                const bool now[NCACHE - 1] = {d1.ell_t, d1.blk_nb != 0, d1.ys, held(d1, Level::wy), d1.ustar};
                const bool was[NCACHE - 1] = {d0.ell_t, d0.blk_nb != 0, d0.ys, held(d0, Level::wy), d0.ustar};
                for (int c = 0; c < NCACHE - 1; ++c)
                  if (now[c] != (was[c] && !kExpect[c][i])) return fail("dropped iff dependent", c, i);
                if (d1.blk_nb != 0 && d1.blk_nb != d0.blk_nb) return fail("block count altered", d0.blk_nb, d1.blk_nb);
                if (held(d1, Level::wy) && !held(d1, Level::wy, wy)) return fail("sum block count altered", wy, 0);
                // 2. the row sums go with the image and with the graph copy
                const bool ys_dropped = kExpect[SLAB][i], blk_dropped = kExpect[BLOCKED][i];
                if ((ys_dropped || blk_dropped) && held(d1, Level::wy)) return fail("row sums outlive their sources", i, wy);
                // 3. the epoch
                if (d1.epoch != d0.epoch + (kExpect[EPOCH][i] ? 1 : 0)) return fail("epoch", i, (long long)d1.epoch);
                // 4. the same input again: only the epoch moves
                Derived d2 = d1;
                changed(d2, kInputs[i]);
                if (lost(d1, d2) != 0) return fail("second report dropped more", i, lost(d1, d2));
                // (the sums' count is the same number: held at all alike, and held at the count they were given alike)
                if (d2.blk_nb != d1.blk_nb || held(d2, Level::wy) != held(d1, Level::wy) || held(d2, Level::wy, wy) != held(d1, Level::wy, wy)) return fail("second report altered a count", i, d2.blk_nb);
                if (d2.epoch != d1.epoch + (kExpect[EPOCH][i] ? 1 : 0)) return fail("epoch, second report", i, (long long)d2.epoch);
                ++cases;
              }
  std::printf("derived state sweep ok (%lld cases)\n", cases);
  return 0;
}

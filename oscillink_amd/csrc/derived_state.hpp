// Which of the handle's derived device arrays is computed from what, and the one function that drops them: plain host
// code, free of every HIP type (the style of host_logic.hpp and knn_plan.hpp), swept by
// tests/host_logic/sweep_derived_state.cpp under -fsanitize=address,undefined.
//   Input / Cache : what can change on a handle / what is computed from it and kept
//   kDependsOn    : per cache, the inputs it is computed from (the one place that says so)
//   Derived       : the validity of every cache (osc_lattice::derived)
//   changed       : an input changed -- every cache computed from it is dropped
//   Level         : the chain of arrays an anchor start keeps, each computed from the ones before it (Cache::anchor_wy is
//                   the whole chain); held / begin_build / built are the only way a level's validity is read or written
// Every other cache is marked as built by assigning its field where it is built (osc_solve.hip, osc_api.hip: osc_solve_ustar).
#pragma once
#include <cstdint>

namespace osc {
namespace host {

enum class Input : unsigned {
  anchors,    // Y's device content
  window,     // the handle's column window [c0, c1)
  row_order,  // the internal row order
  graph,      // the ELL arrays
  chain,      // the chain prior
  comm,       // the communicator
  query,      // psi or the gates
  lams,       // lamG, lamC, lamQ
  count
};

enum class Cache : unsigned {
  ell_t,         // ell_col_t / ell_w_t: the transposed ELL of the one-launch solve
  blocked_copy,  // blk_slots / blk_rest / blk_over: the block-major graph copy (Derived::blk_nb blocks)
  anchor_slab,   // Ys: the slab-major image of the anchors over the window
  anchor_wy,     // WYs and every Level above it: the anchors' row sums W.Y, in the slot placement of the graph copy
  ustar,         // Ustar
  epoch_keyed,   // the halo plan, the query basis, query.Yn: each keeps the epoch it was built for and compares on use
  count
};

constexpr unsigned bit(Input i) { return 1u << (unsigned)i; }
template <typename... More>
constexpr unsigned inputs(Input first, More... more) {
  return (bit(first) | ... | bit(more));
}

constexpr unsigned kGraphCopy = inputs(Input::graph, Input::row_order);
constexpr unsigned kAnchorSlab = inputs(Input::anchors, Input::row_order, Input::window);
// indexed by Cache
constexpr unsigned kDependsOn[(unsigned)Cache::count] = {
    kGraphCopy,                // ell_t
    kGraphCopy,                // blocked_copy
    kAnchorSlab,               // anchor_slab
    kAnchorSlab | kGraphCopy,  // anchor_wy: sums of the slab's values in the copy's placement
    inputs(Input::anchors, Input::graph, Input::row_order, Input::chain, Input::comm, Input::query, Input::lams),  // ustar
    inputs(Input::graph, Input::row_order, Input::chain, Input::comm),                                             // epoch_keyed
};

constexpr bool depends_on(Cache c, Input i) { return (kDependsOn[(unsigned)c] & bit(i)) != 0; }

// The anchor-start chain, in the order it is built.  Each level is computed from the levels before it and from the block-major
// graph copy, so it is current exactly while all of them are and were formed with the same block count:
//   wy     WYs: the anchors' row sums W.Y, slab-major, in the slot placement of the copy
//   wwy    WWs / Wsum: W.(W.Y) and W.1
//   w3     W3s / Wsum2 (and the T array): W.(W.(W.Y)) and W.(W.1)
//   gram   gram: the Gram sums of Ys, WYs, WWs, W3s, Wsum, Wsum2 (anchor_gram.hpp)
//   gram3  gram3 / Wsum3: the third step's sums, over W.W3s and W.Wsum2 as well
//   gram4  gram4: the fourth step's sums, over W.W.W3s and W.Wsum3 as well
//   w4     W4s: W.W3s, kept from the pass that forms gram4 (the polynomial last form)
enum class Level : unsigned { wy, wwy, w3, gram, gram3, gram4, w4, count };
constexpr unsigned kLevels = (unsigned)Level::count;

struct Derived {
  bool ell_t = false;
  int blk_nb = 0;  // blocks of the copy held (0 = none)
  bool ys = false;
  int level_nb[kLevels] = {};  // per Level, the block count it was built with (0 = not held): held, begin_build, built
  bool ustar = false;
  uint64_t epoch = 1;  // what an epoch_keyed cache was built for (its own 0 = never built)
};

// `level` and every level below it were built with `nb` blocks
inline bool held(const Derived& d, Level level, int nb) {
  if (nb <= 0) return false;
  for (unsigned l = 0; l <= (unsigned)level; ++l)
    if (d.level_nb[l] != nb) return false;
  return true;
}
// ... with whatever block count the chain was begun with (what a reader of the arrays asks)
inline bool held(const Derived& d, Level level) { return held(d, level, d.level_nb[0]); }
// `level` is about to be formed anew: it and every level above it are dropped
inline void begin_build(Derived& d, Level level) {
  for (unsigned l = (unsigned)level; l < kLevels; ++l) d.level_nb[l] = 0;
}
inline void built(Derived& d, Level level, int nb) { d.level_nb[(unsigned)level] = nb; }

inline void drop(Derived& d, Cache c) {
  switch (c) {
    case Cache::ell_t: d.ell_t = false; break;
    case Cache::blocked_copy: d.blk_nb = 0; break;
    case Cache::anchor_slab: d.ys = false; break;
    case Cache::anchor_wy: begin_build(d, Level::wy); break;
    case Cache::ustar: d.ustar = false; break;
    case Cache::epoch_keyed: ++d.epoch; break;
    case Cache::count: break;
  }
}

// `what` changed: every cache computed from it is dropped.  The only way a cache is dropped.
inline void changed(Derived& d, Input what) {
  for (unsigned c = 0; c < (unsigned)Cache::count; ++c)
    if (depends_on((Cache)c, what)) drop(d, (Cache)c);
}

}  // namespace host
}  // namespace osc

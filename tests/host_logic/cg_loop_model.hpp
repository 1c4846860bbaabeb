// The ops of the library's CG host loop (oscillink_amd/csrc/host_logic.hpp: cg_host_loop) for a sweep's device model, which
// is written as lambdas over the sweep's state: four references, called by the names cg_host_loop uses.
#pragma once

template <class E, class I, class W, class G>
struct CgLoopModel {
  E& enqueue;           // (it, speculative)
  I& idle_before_wait;  // (it)
  W& wait;              // (it) -> residual
  G& go_on;             // (it)
};
template <class E, class I, class W, class G>
static CgLoopModel<E, I, W, G> cg_loop_model(E& e, I& i, W& w, G& g) {
  return {e, i, w, g};
}

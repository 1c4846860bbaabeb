// Chunk, layout and partition arithmetic of osc_bundle_gated_many.  HIP-free: osc_query.hip runs
// it, tests/host_logic/sweep_bundle_gated_plan.cpp sweeps it under the sanitizers.
//
// A chunk of nq queries is one slab-major panel (gates_many_plan.hpp: slab s is a contiguous N x 32 array).  Query t of the
// chunk owns the spq = ceil(D / 32) consecutive slabs [t spq, (t + 1) spq): its N x D solve, the last slab padded with zero
// columns.  The rows are cut by gates_many_plan.hpp's rule of N alone, so a column's arithmetic and the order of every
// reduction are the same whatever else shares its chunk.
#pragma once
#include <algorithm>
#include <cstdint>

#include "gates_many_plan.hpp"

namespace osc {
namespace host {

constexpr int32_t kGatedMaxChunk = 256;                  // queries per chunk without OSC_GATED_CHUNK (and at most)
constexpr int64_t kGatedBudgetBytes = (int64_t)1 << 30;  // scratch of one chunk

inline int32_t gated_slabs_per_query(int32_t D) { return (std::max(D, 1) + kGatesSlab - 1) / kGatesSlab; }
inline int64_t gated_slab_begin(int32_t t, int32_t D) { return (int64_t)t * gated_slabs_per_query(D); }

// byte offsets of one chunk's arrays: nq queries, cols = nq spq 32 panel columns
struct GatedLayout {
  int64_t X, R, P, AP;      // float  [nq spq][N][32]
  int64_t gate_api;         // float  [nq][N]  the gates as they arrive, API row order
  int64_t gate;             // float  [nq][N]  the gates in device row order
  int64_t psi;              // float  [nq][spq 32]  the queries, zero past D
  int64_t part_a, part_b;   // double [nq spq][parts][32] per-part column sums
  int64_t rz;               // double [cols]
  int64_t alpha, beta;      // float  [cols]
  int64_t res;              // float  [nq] the query's largest column residual after its last iteration
  int64_t live, iters;      // int32  [nq]
  int64_t n_live;           // int32  [2] live queries of the panel, by iteration parity
  int64_t total;
};

inline GatedLayout gated_layout(int64_t N, int32_t D, int32_t nq) {
  GatedLayout L{};
  int64_t o = 0;
  auto take = [&](int64_t bytes) {
    const int64_t at = o;
    o += gates_align(bytes);
    return at;
  };
  const int64_t q = std::max(nq, 1), slabs = q * gated_slabs_per_query(D), cols = slabs * kGatesSlab;
  const int64_t rows = std::max<int64_t>(N, 1), panel = rows * cols * 4, parts = gates_parts(N);
  L.X = take(panel);
  L.R = take(panel);
  L.P = take(panel);
  L.AP = take(panel);
  L.gate_api = take(q * rows * 4);
  L.gate = take(q * rows * 4);
  L.psi = take(cols * 4);
  L.part_a = take(slabs * parts * kGatesSlab * 8);
  L.part_b = take(slabs * parts * kGatesSlab * 8);
  L.rz = take(cols * 8);
  L.alpha = take(cols * 4);
  L.beta = take(cols * 4);
  L.res = take(q * 4);
  L.live = take(q * 4);
  L.iters = take(q * 4);
  L.n_live = take(2 * 4);
  L.total = o;
  return L;
}

// queries per chunk: the requested count (OSC_GATED_CHUNK, else kGatedMaxChunk) in [1, 256], lowered until one chunk's
// scratch fits the budget; never below 1 (one query's solve is as large as it is)
inline int32_t gated_chunk(int64_t N, int32_t D, int32_t requested, int64_t budget) {
  int32_t c = std::min(std::max(requested, 1), kGatedMaxChunk);
  if (c > 1 && gated_layout(N, D, c).total > budget) {
    // the layout grows with the chunk: the largest chunk that fits, by bisection over [1, c)
    int32_t lo = 1, hi = c;  // lo fits or is the floor, hi does not fit
    while (hi - lo > 1) {
      const int32_t mid = lo + (hi - lo) / 2;
      if (gated_layout(N, D, mid).total > budget) hi = mid; else lo = mid;
    }
    c = lo;
  }
  return c;
}

// the chunks tile [0, Q) like the gates' (gates_chunk_count / gates_chunk_begin / gates_chunk_size)

}  // namespace host
}  // namespace osc

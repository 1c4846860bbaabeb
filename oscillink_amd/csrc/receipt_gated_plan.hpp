// Chunk and layout arithmetic of osc_receipt_gated_many.  HIP-free: osc_query.hip runs it,
// tests/host_logic/sweep_receipt_gated_plan.cpp sweeps it under the sanitizers.
//
// A chunk is bundle_gated_plan.hpp's panel -- query t owns the slabs [t spq, (t + 1) spq), the rows cut by
// gates_many_plan.hpp's rule of N alone -- with one more panel when the request settles: the settled U_q, kept beside the
// U* solve's X, R, P and AP (20 N Dp bytes a query instead of 16 N Dp).  Behind the panels lie deltaH per query and, in full
// detail, the per-(row, query) components, the null-point candidates and the partials of the three sums.
#pragma once
#include "bundle_gated_plan.hpp"

namespace osc {
namespace host {

constexpr int32_t kReceiptGatedSumParts = 512;  // row partials of the three sums at most (query.hpp: rm_col_parts)
constexpr int32_t kReceiptGatedFinishRows = 64; // partials one finish group adds (query.hpp: kRmFinishRows)

inline int32_t receipt_gated_qs(int32_t nq) { return (std::max(nq, 1) + 3) & ~3; }  // query.hpp: query_qs
inline int32_t receipt_gated_sum_parts(int64_t N) {
  return (int32_t)std::max<int64_t>(1, std::min<int64_t>((N + 63) / 64, kReceiptGatedSumParts));
}
inline int32_t receipt_gated_sum_groups(int64_t N) {
  return (receipt_gated_sum_parts(N) + kReceiptGatedFinishRows - 1) / kReceiptGatedFinishRows;
}

struct ReceiptGatedLayout {
  GatedLayout panel;       // X, R, P, AP, the gates, psi and the solve's scalars, from offset 0
  bool settle = false, full = false;
  int32_t qs = 0;          // pitch of the N x qs arrays
  int64_t U = 0;           // float  [nq spq][N][32] the settled states (settle)
  int64_t dh = 0;          // double [nq]
  int64_t comp = 0;        // double [3][N][qs]: coh, anchor, query (full)
  int64_t z = 0, j = 0, r = 0;  // float / int32 / float [N][qs] (full)
  int64_t zt = 0;          // float  [nq][N] (full)
  int64_t sumpart = 0;     // double [3][sum parts][nq] (full)
  int64_t sumfin = 0;      // double [sum groups][nq] (full)
  int64_t sums = 0;        // double [3][nq] (full)
  int64_t total = 0;
};

inline ReceiptGatedLayout receipt_gated_layout(int64_t N, int32_t D, int32_t nq, bool settle, bool full) {
  ReceiptGatedLayout L{};
  L.panel = gated_layout(N, D, nq);
  L.settle = settle;
  L.full = full;
  L.qs = receipt_gated_qs(nq);
  int64_t o = L.panel.total;
  auto take = [&](int64_t bytes) {
    const int64_t at = o;
    o += gates_align(bytes);
    return at;
  };
  const int64_t q = std::max(nq, 1), rows = std::max<int64_t>(N, 1);
  if (settle) L.U = take(L.panel.R - L.panel.X);
  L.dh = take(q * 8);
  if (full) {
    const int64_t cell = rows * L.qs;
    L.comp = take(3 * cell * 8);
    L.z = take(cell * 4);
    L.j = take(cell * 4);
    L.r = take(cell * 4);
    L.zt = take(rows * q * 4);
    L.sumpart = take(3 * (int64_t)receipt_gated_sum_parts(N) * q * 8);
    L.sumfin = take((int64_t)receipt_gated_sum_groups(N) * q * 8);
    L.sums = take(3 * q * 8);
  }
  L.total = o;
  return L;
}

// queries per chunk: gated_chunk's rule on this layout -- the requested count (OSC_GATED_CHUNK, else kGatedMaxChunk) in
// [1, 256], lowered until one chunk's scratch fits the budget; never below 1
inline int32_t receipt_gated_chunk(int64_t N, int32_t D, bool settle, bool full, int32_t requested, int64_t budget) {
  int32_t c = std::min(std::max(requested, 1), kGatedMaxChunk);
  if (c > 1 && receipt_gated_layout(N, D, c, settle, full).total > budget) {
    int32_t lo = 1, hi = c;  // lo fits or is the floor, hi does not fit
    while (hi - lo > 1) {
      const int32_t mid = lo + (hi - lo) / 2;
      if (receipt_gated_layout(N, D, mid, settle, full).total > budget) hi = mid; else lo = mid;
    }
    c = lo;
  }
  return c;
}

}  // namespace host
}  // namespace osc

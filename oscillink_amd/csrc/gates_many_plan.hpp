// Chunk, partition and offset arithmetic of osc_gates_many.  HIP-free: osc_query.hip runs it,
// tests/host_logic/sweep_gates_many_plan.cpp sweeps it under the sanitizers.
//
// A chunk of nq queries is a panel of N rows and qc = nq rounded up to 32 columns, stored slab-major: slab s holds the
// columns [32 s, 32 s + 32) of every row as one contiguous N x 32 array (a row of a slab is one 128-byte line), so element
// (row, col) sits at ((col / 32) * N + row) * 32 + col % 32.  Every kernel works on one slab at a time and never sees the
// panel's width; the rows are cut into parts by a rule that knows N alone.  A column's arithmetic -- its GEMM outputs, its
// row partition, the order of every reduction -- is therefore the same whatever else shares its call.
#pragma once
#include <algorithm>
#include <cstdint>

namespace osc {
namespace host {

constexpr int32_t kGatesSlab = 32;                       // columns of a slab
constexpr int32_t kGatesMaxChunk = 256;                  // queries per chunk without OSC_GATES_CHUNK (and at most)
constexpr int64_t kGatesBudgetBytes = (int64_t)1 << 30;  // scratch of one chunk
constexpr int32_t kGatesStepRows = 32;                   // rows a workgroup (4 waves x 8 rows) works on at a time
constexpr int32_t kGatesMaxParts = 2048;                 // row parts (workgroups per slab) at most

inline int64_t gates_align(int64_t b) { return (b + 255) / 256 * 256; }
inline int32_t gates_width(int32_t nq) { return (std::max(nq, 1) + kGatesSlab - 1) / kGatesSlab * kGatesSlab; }

// the row partition: parts of part_rows rows (a multiple of kGatesStepRows), the last one shorter; functions of N alone
inline int32_t gates_part_rows(int64_t N) {
  const int64_t per = (std::max<int64_t>(N, 1) + kGatesMaxParts - 1) / kGatesMaxParts;
  return (int32_t)((per + kGatesStepRows - 1) / kGatesStepRows * kGatesStepRows);
}
inline int32_t gates_parts(int64_t N) {
  const int64_t pr = gates_part_rows(N);
  return (int32_t)((std::max<int64_t>(N, 1) + pr - 1) / pr);
}

// byte offsets of one chunk's arrays for a panel of qc columns (a multiple of 32)
struct GatesLayout {
  int64_t X, R, P, AP;      // float  [qc / 32][N][32]  the solve; AP first holds the GEMM's N x qc cosines, row-major
  int64_t out;              // float  [qc][N]           the gates, query-major, API row order
  int64_t Bt;               // float  [bt_floats]       the GEMM's query operand
  int64_t part_a, part_b;   // double [qc / 32][parts][32] per-part column sums (later: float minima / maxima)
  int64_t rz;               // double [qc]
  int64_t tol, alpha, beta, res, lo, hi;  // float [qc]
  int64_t live, iters;      // int32  [qc]
  int64_t slab_live;        // int32  [qc / 32] live columns per slab
  int64_t n_live;           // int32  [2]       live columns of the panel, by iteration parity
  int64_t total;
};

inline GatesLayout gates_layout(int64_t N, int32_t qc, int64_t bt_floats) {
  GatesLayout L{};
  int64_t o = 0;
  auto take = [&](int64_t bytes) {
    const int64_t at = o;
    o += gates_align(bytes);
    return at;
  };
  const int64_t panel = N * (int64_t)qc * 4, slabs = qc / kGatesSlab, parts = gates_parts(N);
  L.X = take(panel);
  L.R = take(panel);
  L.P = take(panel);
  L.AP = take(panel);
  L.out = take(panel);
  L.Bt = take(bt_floats * 4);
  L.part_a = take(slabs * parts * kGatesSlab * 8);
  L.part_b = take(slabs * parts * kGatesSlab * 8);
  L.rz = take((int64_t)qc * 8);
  L.tol = take((int64_t)qc * 4);
  L.alpha = take((int64_t)qc * 4);
  L.beta = take((int64_t)qc * 4);
  L.res = take((int64_t)qc * 4);
  L.lo = take((int64_t)qc * 4);
  L.hi = take((int64_t)qc * 4);
  L.live = take((int64_t)qc * 4);
  L.iters = take((int64_t)qc * 4);
  L.slab_live = take(slabs * 4);
  L.n_live = take(2 * 4);
  L.total = o;
  return L;
}

// the GEMM operand of a qc-column panel: query_qpad(qc) rows of kpad floats (query.hpp: 128-row tiles, K padded to 32)
inline int64_t gates_bt_floats(int32_t qc, int32_t D) {
  const int64_t qpad = ((int64_t)qc + 127) / 128 * 128, kpad = ((int64_t)D + 31) / 32 * 32;
  return qpad * kpad;
}

// queries per chunk: the requested count (OSC_GATES_CHUNK, else kGatesMaxChunk) as a multiple of 32 in [32, 256], lowered
// in steps of 32 until one chunk's scratch fits the budget; never below 32 (such a panel is as large as it is)
inline int32_t gates_chunk(int64_t N, int32_t D, int32_t requested, int64_t budget) {
  int32_t qc = gates_width(std::min(std::max(requested, 1), kGatesMaxChunk));
  while (qc > kGatesSlab && gates_layout(N, qc, gates_bt_floats(qc, D)).total > budget) qc -= kGatesSlab;
  return qc;
}

inline int32_t gates_chunk_count(int32_t Q, int32_t qc) { return Q <= 0 ? 0 : (Q + qc - 1) / qc; }
inline int32_t gates_chunk_begin(int32_t c, int32_t qc) { return c * qc; }
inline int32_t gates_chunk_size(int32_t Q, int32_t c, int32_t qc) { return std::min(qc, Q - c * qc); }

}  // namespace host
}  // namespace osc

// Chunk, layout and path arithmetic of osc_chain_gated_many.  HIP-free: osc_query.hip runs it,
// tests/host_logic/sweep_chain_gated_plan.cpp sweeps it under the sanitizers.
//
// A chunk is receipt_gated_plan.hpp's block with the chain prior's arrays behind it: the path rows of the chunk's distinct
// (chain, weights) pairs back to back (ChainManyPaths' order; their columns and A_path are that structure's own arrays), the
// normalised weights beside the columns, per query the range of its path's rows, and the partial sums of the path kernels.
// A query's path rows are cut into fix units of kChainFixRows rows by a rule that knows the path's row count alone, so its
// arithmetic and the order of its reductions do not depend on what shares its chunk.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "chain_many.hpp"
#include "receipt_gated_plan.hpp"

namespace osc {
namespace host {

constexpr int32_t kChainFixRows = 128;  // path rows of one fix unit (one workgroup per (unit, slab): 4 steps of 32 rows)

// a chain of len nodes on N rows: its path owns at most min(len, N) rows and 2 (len - 1) entries
inline int32_t chain_gated_rows_max(int32_t len, int64_t N) { return (int32_t)std::min<int64_t>(std::max(len, 1), std::max<int64_t>(N, 1)); }
inline int32_t chain_gated_entries_max(int32_t len) { return 2 * std::max(len - 1, 1); }

// the cut of a path's rows into fix units: unit u holds the rows [u kChainFixRows, min((u + 1) kChainFixRows, rows))
inline int32_t chain_fix_units(int32_t rows) { return (std::max(rows, 0) + kChainFixRows - 1) / kChainFixRows; }
inline int32_t chain_fix_begin(int32_t u) { return u * kChainFixRows; }
inline int32_t chain_fix_end(int32_t rows, int32_t u) { return std::min(rows, (u + 1) * kChainFixRows); }

struct ChainGatedLayout {
  ReceiptGatedLayout rg;   // from offset 0
  int32_t max_units = 0;   // fix units of a query at most: the pitch of cpart
  int64_t prow = 0;        // int32  [rows]     device row of every packed path row
  int64_t pbeg = 0;        // int32  [rows]     the row's entries [pbeg, pend) in the chunk's columns / weights
  int64_t pend = 0;        // int32  [rows]
  int64_t pw = 0;          // float  [entries]  the normalised path weights, beside ChainManyPaths' pcol
  int64_t q_row0 = 0;      // int32  [nq]       first packed row of the query's path
  int64_t q_rows = 0;      // int32  [nq]       rows of the query's path
  int64_t cpart = 0;       // double [nq spq][max_units][32]  the path kernels' column sums per fix unit
  int64_t total = 0;
};

// the layout of nq queries whose chains have max_len nodes at most (every query's path counted as distinct)
inline ChainGatedLayout chain_gated_layout(int64_t N, int32_t D, int32_t nq, bool settle, bool full, int32_t max_len) {
  ChainGatedLayout L{};
  L.rg = receipt_gated_layout(N, D, nq, settle, full);
  int64_t o = L.rg.total;
  auto take = [&](int64_t bytes) {
    const int64_t at = o;
    o += gates_align(bytes);
    return at;
  };
  const int64_t q = std::max(nq, 1), rows = q * chain_gated_rows_max(max_len, N), entries = q * chain_gated_entries_max(max_len);
  L.max_units = std::max(chain_fix_units(chain_gated_rows_max(max_len, N)), 1);
  L.prow = take(rows * 4);
  L.pbeg = take(rows * 4);
  L.pend = take(rows * 4);
  L.pw = take(entries * 4);
  L.q_row0 = take(q * 4);
  L.q_rows = take(q * 4);
  L.cpart = take(q * gated_slabs_per_query(D) * L.max_units * kGatesSlab * 8);
  L.total = o;
  return L;
}

// queries per chunk: receipt_gated_chunk's rule on this layout
inline int32_t chain_gated_chunk(int64_t N, int32_t D, bool settle, bool full, int32_t max_len, int32_t requested,
                                 int64_t budget) {
  int32_t c = std::min(std::max(requested, 1), kGatedMaxChunk);
  if (c > 1 && chain_gated_layout(N, D, c, settle, full, max_len).total > budget) {
    int32_t lo = 1, hi = c;  // lo fits or is the floor, hi does not fit
    while (hi - lo > 1) {
      const int32_t mid = lo + (hi - lo) / 2;
      if (chain_gated_layout(N, D, mid, settle, full, max_len).total > budget) hi = mid; else lo = mid;
    }
    c = lo;
  }
  return c;
}

// the most nodes of any chain of queries [0, Q)
inline int32_t chain_gated_max_len(const int64_t* off, int32_t Q) {
  int64_t m = 2;
  for (int32_t q = 0; q < Q; ++q) m = std::max(m, off[q + 1] - off[q]);
  return (int32_t)m;
}

// what a chunk uploads beside ChainManyPaths' pcol / pa: the rows of its distinct paths, back to back in the paths' order
struct ChainGatedPack {
  std::vector<int32_t> prow, pbeg, pend, q_row0, q_rows;
  std::vector<float> pw;
  int32_t max_units = 0;  // of the chunk's queries
};

// path_of[t]: the path of the chunk's query t (chain_many_units_weighted's)
inline void chain_gated_pack(const ChainManyPaths& paths, const std::vector<int32_t>& path_of, ChainGatedPack& k) {
  k.prow.clear();
  k.pbeg.clear();
  k.pend.clear();
  k.pw.clear();
  std::vector<int32_t> row0(paths.paths.size(), 0);
  for (size_t id = 0; id < paths.paths.size(); ++id) {
    const ChainPath& p = paths.paths[id];
    row0[id] = (int32_t)k.prow.size();
    for (size_t t = 0; t < p.rows.size(); ++t) {
      k.prow.push_back(p.rows[t]);
      k.pbeg.push_back(paths.base[id] + p.ptr[t]);
      k.pend.push_back(paths.base[id] + p.ptr[t + 1]);
    }
    k.pw.insert(k.pw.end(), p.w.begin(), p.w.end());
  }
  k.q_row0.assign(path_of.size(), 0);
  k.q_rows.assign(path_of.size(), 0);
  k.max_units = 0;
  for (size_t t = 0; t < path_of.size(); ++t) {
    const size_t id = (size_t)path_of[t];
    k.q_row0[t] = row0[id];
    k.q_rows[t] = (int32_t)paths.paths[id].rows.size();
    k.max_units = std::max(k.max_units, chain_fix_units(k.q_rows[t]));
  }
}

}  // namespace host
}  // namespace osc

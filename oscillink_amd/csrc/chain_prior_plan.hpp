// The host plan of osc_chain_prior_many: per-query chain priors on a resident lattice by a
// low-rank update.  Query q's operator is M' - S_q K_q S_q^T with M' = M + lamP I; one Green's column G e = M'^-1 e per
// distinct chain node serves every query that touches the node.  HIP-free: osc_query.hip runs it,
// tests/host_logic/sweep_chain_prior_plan.cpp sweeps it under the sanitizers.
//
// A pass is a run of consecutive queries whose distinct chain nodes -- one panel column each, in the order they are first
// seen -- are solved together: four slab-major N x qc panels (gates_many_plan.hpp's layout and row partition) beside the
// per-column scalars.  A query's nodes never straddle two passes.  A pass takes queries while it fits the budget and the
// column limit; a pass of one query is as wide as that query needs, whatever the budget says.  ChainPriorPass and
// chain_prior_pack are also the pass and the packer of bundle_prior_plan.hpp and receipt_prior_plan.hpp, which differ in the
// layout whose bytes the budget bounds.
#pragma once
#include <algorithm>
#include <cstdint>
#include <map>
#include <vector>

#include "gates_many_plan.hpp"

namespace osc {
namespace host {

constexpr int32_t kChainPriorMaxNodes = 64;                   // distinct nodes of one chain: the m x m solve is one workgroup's LDS
constexpr int64_t kChainPriorBudgetBytes = (int64_t)1 << 30;  // scratch of one pass
constexpr float kChainPriorTolFloor = 2e-7f;                  // where fp32 stops lowering a unit right-hand side's residual

// byte offsets of one pass's solve arrays for a panel of qc columns (a multiple of 32)
struct ChainPriorLayout {
  int64_t X, R, P, AP;     // float  [qc / 32][N][32]; X ends as G
  int64_t part_a, part_b;  // double [qc / 32][parts][32]
  int64_t rz;              // double [qc]
  int64_t tol, alpha, beta, res;  // float [qc]
  int64_t live, iters;     // int32 [qc]
  int64_t node;            // int32 [qc] device row of column c (-1 past the pass's columns)
  int64_t slab_live;       // int32 [qc / 32]
  int64_t n_live;          // int32 [2]
  int64_t total;
};

inline ChainPriorLayout chain_prior_layout(int64_t N, int32_t qc) {
  ChainPriorLayout L{};
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
  L.part_a = take(slabs * parts * kGatesSlab * 8);
  L.part_b = take(slabs * parts * kGatesSlab * 8);
  L.rz = take((int64_t)qc * 8);
  L.tol = take((int64_t)qc * 4);
  L.alpha = take((int64_t)qc * 4);
  L.beta = take((int64_t)qc * 4);
  L.res = take((int64_t)qc * 4);
  L.live = take((int64_t)qc * 4);
  L.iters = take((int64_t)qc * 4);
  L.node = take((int64_t)qc * 4);
  L.slab_live = take(slabs * 4);
  L.n_live = take(2 * 4);
  L.total = o;
  return L;
}

// the distinct nodes of nodes[0 .. len), ascending
inline std::vector<int32_t> chain_prior_distinct(const int32_t* nodes, int64_t len) {
  std::vector<int32_t> d(nodes, nodes + len);
  std::sort(d.begin(), d.end());
  d.erase(std::unique(d.begin(), d.end()), d.end());
  return d;
}

// -1, or the first query whose chain has more than kChainPriorMaxNodes distinct nodes
inline int32_t chain_prior_check(const int64_t* off, const int32_t* nodes, int32_t Q) {
  for (int32_t q = 0; q < Q; ++q)
    if ((int32_t)chain_prior_distinct(nodes + off[q], off[q + 1] - off[q]).size() > kChainPriorMaxNodes) return q;
  return -1;
}

struct ChainPriorPass {
  int32_t q0 = 0, nq = 0;      // queries [q0, q0 + nq)
  int32_t qc = 0;              // panel columns: cols.size() rounded up to 32
  int64_t msum = 0, msq = 0;   // sums of the queries' distinct node counts and of their squares
  int32_t mmax = 0;            // the largest of them
  std::vector<int32_t> cols;   // the node (as given: an API id) of every panel column, first seen first
};

// The one packer of the three per-query-prior calls: passes over queries [0, Q), at most max_queries queries (floored at 1)
// and max_cols distinct nodes each (max_cols <= 0: no limit beside the budget).  fits(qc, msum, msq, nq) says whether a pass
// of that shape is within the caller's budget; it is asked about the pass as it would be after taking the next query, and a
// pass of one query is taken whatever it says.
template <class Fits>
std::vector<ChainPriorPass> chain_prior_pack(const int64_t* off, const int32_t* nodes, int32_t Q, int32_t max_queries,
                                             int32_t max_cols, Fits fits) {
  std::vector<ChainPriorPass> out;
  std::map<int32_t, int32_t> at;  // node -> column of the open pass
  ChainPriorPass cur;
  auto close = [&]() {
    if (cur.nq == 0) return;
    cur.qc = gates_width((int32_t)cur.cols.size());
    out.push_back(std::move(cur));
    cur = ChainPriorPass{};
    at.clear();
  };
  for (int32_t q = 0; q < Q; ++q) {
    const std::vector<int32_t> d = chain_prior_distinct(nodes + off[q], off[q + 1] - off[q]);
    const int64_t m = (int64_t)d.size();
    int32_t fresh = 0;
    for (int32_t v : d) fresh += at.count(v) ? 0 : 1;
    const int32_t want = (int32_t)cur.cols.size() + fresh;
    const bool take = cur.nq < std::max(max_queries, 1) && (max_cols <= 0 || want <= max_cols) &&
                      fits(gates_width(want), cur.msum + m, cur.msq + m * m, cur.nq + 1);
    if (cur.nq > 0 && !take) close();
    if (cur.nq == 0) cur.q0 = q;
    for (int32_t v : d)
      if (at.emplace(v, (int32_t)cur.cols.size()).second) cur.cols.push_back(v);
    cur.msum += m;
    cur.msq += m * m;
    cur.mmax = std::max(cur.mmax, (int32_t)m);
    ++cur.nq;
  }
  close();
  return out;
}

// osc_chain_prior_many's passes: the panel within `budget` bytes unless the pass holds one query
inline std::vector<ChainPriorPass> chain_prior_passes(const int64_t* off, const int32_t* nodes, int32_t Q, int64_t N,
                                                      int32_t max_queries, int32_t max_cols, int64_t budget) {
  return chain_prior_pack(off, nodes, Q, max_queries, max_cols, [&](int32_t qc, int64_t, int64_t, int32_t) {
    return chain_prior_layout(N, qc).total <= budget;
  });
}

// The per-chain systems of a pass: chain c (a path of ChainManyPaths) has m[c] distinct rows, ascending; its panel columns
// start at col_at[c] in `cols`, its T (m x m doubles, row-major) at t_at[c] in the pass's T block, its K entries
// (local row, local column, normalised path weight) at [k_at[c], k_at[c + 1]).
struct ChainPriorSystems {
  std::vector<int32_t> m, col_at, k_at;
  std::vector<int64_t> t_at;
  std::vector<int32_t> cols;   // panel column per (chain, local node)
  std::vector<int32_t> rows;   // device row per (chain, local node)
  std::vector<int32_t> kr, kc;
  std::vector<float> kw;
  int64_t t_doubles = 0;

  void clear() { *this = ChainPriorSystems{}; }
  // rows / ptr / col / w: one path's structure (corpus_chain.hpp: ChainPath, device rows); column_of: device row -> panel column
  void add(const std::vector<int32_t>& prow, const std::vector<int32_t>& ptr, const std::vector<int32_t>& pcol,
           const std::vector<float>& pw, const std::map<int32_t, int32_t>& column_of) {
    const int32_t mm = (int32_t)prow.size();
    if (k_at.empty()) k_at.push_back(0);
    m.push_back(mm);
    col_at.push_back((int32_t)cols.size());
    t_at.push_back(t_doubles);
    t_doubles += (int64_t)mm * mm;
    for (int32_t a = 0; a < mm; ++a) {
      rows.push_back(prow[(size_t)a]);
      cols.push_back(column_of.at(prow[(size_t)a]));
      for (int32_t e = ptr[(size_t)a]; e < ptr[(size_t)a + 1]; ++e) {
        const auto it = std::lower_bound(prow.begin(), prow.end(), pcol[(size_t)e]);
        kr.push_back(a);
        kc.push_back((int32_t)(it - prow.begin()));  // (every column of a path owns a row: the path is symmetric)
        kw.push_back(pw[(size_t)e]);
      }
    }
    k_at.push_back((int32_t)kr.size());
  }
};

// The Green's columns' stop: tol_g * 64 * tau * vmax <= tol / 2 with tau = lamP (lamG + lamP) / lamG >= |T_q|_2 and
// vmax >= max |U'0|; a function of the handle's state and the call's settings alone, floored where fp32 goes no lower.
inline float chain_prior_tol_g(float tol, float lamG, float lamP, float vmax) {
  const double tau = (double)lamP * ((double)lamG + (double)lamP) / (double)lamG;
  const double t = 0.5 * (double)tol / std::max((double)kChainPriorMaxNodes * tau * std::max((double)vmax, 1e-30), 1e-30);
  return (float)std::max(std::min(t, 0.5 * (double)tol), (double)kChainPriorTolFloor);
}

}  // namespace host
}  // namespace osc

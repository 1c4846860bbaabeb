// Sweep of chain_prior_plan.hpp (osc_chain_prior_many) for N from 1 to 2 000 000 and Q from 1 to 1000:
// the passes tile [0, Q) in order; no query is split -- every distinct node of a query is a column of its pass; a node is a
// column once per pass, so a chain many queries share is solved once; a pass of more than one query keeps its panel within
// the budget, its queries within the chunk and its columns within the forced limit; the arrays of a layout are 256-byte
// aligned, pairwise disjoint and inside the block; the passes are the greedy ones and their columns stand in first-seen
// order (sweep_prior_common.hpp); chains of 1 and 64 distinct nodes pass the check and 65 do not; the
// per-chain systems index inside their arrays (walked here the way the kernels walk them, so the sanitizers see it); the
// weighted path key keeps chains with different weights apart.  Run under -fsanitize=address,undefined.
#include <cstdlib>
#include <map>

#include "../../oscillink_amd/csrc/chain_many.hpp"
#include "sweep_prior_common.hpp"

static int check_layout(long long N, int qc) {
  const ChainPriorLayout L = chain_prior_layout(N, qc);
  const long long slabs = qc / kGatesSlab, parts = gates_parts(N), panel = N * (long long)qc * 4;
  return check_blocks({{L.X, panel},       {L.R, panel},       {L.P, panel},        {L.AP, panel},
                       {L.part_a, slabs * parts * 32 * 8},     {L.part_b, slabs * parts * 32 * 8},
                       {L.rz, qc * 8LL},   {L.tol, qc * 4LL},  {L.alpha, qc * 4LL}, {L.beta, qc * 4LL},
                       {L.res, qc * 4LL},  {L.live, qc * 4LL}, {L.iters, qc * 4LL}, {L.node, qc * 4LL},
                       {L.slab_live, slabs * 4},               {L.n_live, 8}},
                      L.total);
}

// kind 0 one chain shared by all, 1 a chain per query (2..9 nodes, repeats), 2 chains of 64 distinct nodes
static int check_passes(long long N, int Q, int kind, int max_queries, int max_cols, long long budget) {
  std::vector<int64_t> off;
  std::vector<int> nodes;
  make_chains(N, Q, kind == 0, kind == 2 ? 64 : 0, off, nodes);
  const std::vector<ChainPriorPass> ps = chain_prior_passes(off.data(), nodes.data(), Q, N, max_queries, max_cols, budget);
  if (check_packing(ps, off, nodes, Q, max_queries, max_cols,
                    [&](int qc, long long, long long, int) { return chain_prior_layout(N, qc).total > budget; }))
    return 1;
  for (const ChainPriorPass& p : ps)
    if (check_layout(N, p.qc)) return 1;
  if (kind == 0 && max_cols <= 0 && chain_prior_layout(N, 32).total <= budget && (int)ps.size() != (Q + std::max(max_queries, 1) - 1) / std::max(max_queries, 1))
    return fail("a shared chain splits passes beyond the chunk", (long long)ps.size(), Q);
  return 0;
}

// the systems of a small pass, walked as k_cp_systems / k_cp_tv / k_cm_edges walk them, on real arrays
static int check_systems() {
  const int N = 97;
  const int chainA[] = {5, 9, 2, 9, 40}, chainB[] = {7, 7}, chainC[] = {5, 9, 2, 9, 40};
  const float wC[] = {1.0f, 0.5f, 2.0f, 0.25f};
  std::vector<int64_t> off = {0, 5, 7, 12, 17};
  std::vector<int> nodes;
  nodes.insert(nodes.end(), chainA, chainA + 5);
  nodes.insert(nodes.end(), chainB, chainB + 2);
  nodes.insert(nodes.end(), chainC, chainC + 5);
  nodes.insert(nodes.end(), chainA, chainA + 5);
  std::vector<float> w(13, 1.0f);
  std::copy(wC, wC + 4, w.begin() + 5);  // query 2's edges start at off[2] - 2 = 5
  ChainManyPaths paths;
  std::vector<ChainManyUnit> units;
  std::vector<int32_t> eoff, path_of;
  chain_many_units_weighted(off.data(), nodes.data(), w.data(), 0, 4, nullptr, N, paths, units, eoff, path_of);
  if (paths.paths.size() != 3) return fail("distinct (chain, weights)", (long long)paths.paths.size(), 3);
  if (path_of[0] != path_of[3] || path_of[0] == path_of[2]) return fail("weights are part of a chain's identity", path_of[0], path_of[2]);
  if ((int)units.size() != 13 || eoff[4] != 13) return fail("units", (long long)units.size(), eoff[4]);
  const std::vector<ChainPriorPass> ps = chain_prior_passes(off.data(), nodes.data(), 4, N, 256, 0, kChainPriorBudgetBytes);
  if (ps.size() != 1 || ps[0].cols.size() != 5 || ps[0].qc != 32) return fail("one pass of five columns", (long long)ps.size(), 0);
  std::map<int32_t, int32_t> column_of;
  for (size_t c = 0; c < ps[0].cols.size(); ++c) column_of[ps[0].cols[c]] = (int32_t)c;
  ChainPriorSystems sys;
  for (const ChainPath& cp : paths.paths) sys.add(cp.rows, cp.ptr, cp.col, cp.w, column_of);
  std::vector<float> G((size_t)N * 32, 0.5f);
  std::vector<double> T((size_t)sys.t_doubles, 0.0);
  for (size_t c = 0; c < sys.m.size(); ++c) {
    const int m = sys.m[c];
    if (m < 1 || m > kChainPriorMaxNodes) return fail("system size", (long long)c, m);
    std::vector<double> K((size_t)m * m, 0.0);
    for (int e = sys.k_at[c]; e < sys.k_at[c + 1]; ++e) {
      if (sys.kr[(size_t)e] < 0 || sys.kr[(size_t)e] >= m || sys.kc[(size_t)e] < 0 || sys.kc[(size_t)e] >= m) return fail("entry outside its system", (long long)c, e);
      K[(size_t)sys.kr[(size_t)e] * m + sys.kc[(size_t)e]] = sys.kw[(size_t)e];
    }
    for (int a = 0; a < m; ++a)
      for (int b = 0; b < m; ++b) {
        if (K[(size_t)a * m + b] != K[(size_t)b * m + a]) return fail("K is not symmetric", a, b);
        const int row = sys.rows[(size_t)sys.col_at[c] + a], col = sys.cols[(size_t)sys.col_at[c] + b];
        if (row < 0 || row >= N || col < 0 || col >= ps[0].qc) return fail("gather outside the panel", row, col);
        T[(size_t)sys.t_at[c] + (size_t)a * m + b] = G[((size_t)(col >> 5) * N + row) * 32 + (col & 31)];
      }
  }
  if (sys.m[(size_t)path_of[1]] != 1) return fail("[7, 7] is one node", sys.m[(size_t)path_of[1]], 1);
  return 0;
}

int main() {
  const long long Ns[] = {1, 2, 31, 33, 64, 65, 1000, 4097, 65536, 100000, 500000, 1999999, 2000000};
  const int Qs[] = {1, 2, 31, 32, 33, 255, 256, 257, 513, 1000};
  const int colss[] = {0, 1, 8, 31, 32, 33, 64, 200};
  long long cases = 0;
  for (long long N : Ns) {
    for (int qc = 32; qc <= 512; qc += 32) {
      if (check_layout(N, qc)) return 1;
      ++cases;
    }
    for (int Q : Qs)
      for (int kind = 0; kind < 3; ++kind)
        for (int max_cols : colss) {
          if (kind == 2 && Q > 257) continue;  // (64-node chains: the small counts cover the seams)
          if (check_passes(N, Q, kind, 256, max_cols, kChainPriorBudgetBytes)) return 1;
          if (check_passes(N, Q, kind, 7, max_cols, (long long)1 << 24)) return 1;
          cases += 2;
        }
  }
  // m = 1, 64 and 65 distinct nodes
  {
    std::vector<int> n1 = {4, 4, 4}, n64, n65;
    for (int t = 0; t < 64; ++t) n64.push_back(t);
    n64.push_back(0);
    n64.push_back(63);
    for (int t = 0; t < 65; ++t) n65.push_back(t);
    const int64_t o1[] = {0, 3}, o64[] = {0, 66}, o65[] = {0, 65};
    if (chain_prior_distinct(n1.data(), 3).size() != 1) return fail("m = 1", 0, 0);
    if (chain_prior_check(o1, n1.data(), 1) != -1 || chain_prior_check(o64, n64.data(), 1) != -1) return fail("m = 1 / 64 refused", 0, 0);
    if (chain_prior_check(o65, n65.data(), 1) != 0) return fail("m = 65 accepted", 0, 0);
    std::vector<int> both = n64;
    both.insert(both.end(), n65.begin(), n65.end());
    const int64_t ob[] = {0, 66, 131};
    if (chain_prior_check(ob, both.data(), 2) != 1) return fail("the query of the 65-node chain", 0, 0);
  }
  // the Green's columns' stop: within (floor, tol / 2], falling with lamP and vmax, a function of its arguments alone
  {
    const float a = chain_prior_tol_g(1e-4f, 1.0f, 0.2f, 1.0f), b = chain_prior_tol_g(1e-4f, 1.0f, 0.5f, 1.0f);
    const float c = chain_prior_tol_g(1e-4f, 1.0f, 0.5f, 1e6f), d = chain_prior_tol_g(1e-4f, 1.0f, 1e-9f, 1.0f);
    if (!(a >= b && b >= c && c == kChainPriorTolFloor && d == 0.5e-4f && a <= 0.5e-4f)) return fail("tol_g", 0, 0);
    if (!(64.0 * 0.2 * 1.2 * a <= 0.5e-4 * 1.0001)) return fail("tol_g misses its bound", 0, 0);
  }
  if (check_systems()) return 1;
  std::printf("chain prior plan sweep ok (%lld cases)\n", cases);
  return 0;
}

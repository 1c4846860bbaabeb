// Sweep of bundle_prior_plan.hpp (osc_bundle_prior_many) for N from 1 to 2 000 000, Q from 1 to 1000 and
// chains of 1 to 64 distinct nodes: the passes tile [0, Q) in order; no query is split -- every distinct node of a query is a
// column of its pass, once; msum is the sum of the queries' distinct node counts; a pass of more than one query keeps its
// resident bytes within the budget, its queries within the chunk and its columns within the forced limit; the arrays of a
// layout are 256-byte aligned, pairwise disjoint, inside the block and large enough for what the kernels index (kappa's
// last column of the last query, the GEMM operand's last padded row); the passes are the greedy ones and their columns stand
// in first-seen order (sweep_prior_common.hpp).  Run under -fsanitize=address,undefined.
#include <cstdlib>

#include "../../oscillink_amd/csrc/bundle_prior_plan.hpp"
#include "sweep_prior_common.hpp"

static int check_layout(long long N, int qc, long long msum, int nq, int kpad) {
  const BundlePriorLayout L = bundle_prior_layout(N, qc, msum, nq, kpad);
  if (L.ks % 4 != 0 || L.ks < msum || L.ks >= msum + 4) return fail("kappa pitch", L.ks, msum);
  if (L.qs % 4 != 0 || L.qs < nq || L.qs >= nq + 4) return fail("query pitch", L.qs, nq);
  const long long rows_pad = (msum + 127) / 128 * 128;
  if (check_blocks({{0, L.panel.total},
                    {L.kappa, N * (long long)L.ks * 4},
                    {L.nu, N * (long long)L.qs * 8},
                    {L.bt, rows_pad * kpad * 4},
                    {L.e, nq * 64LL * 8},
                    {L.H, nq * 4096LL * 8}},
                   L.total))
    return 1;
  if (L.resident < L.total + 3 * N * (long long)L.qs * 4) return fail("resident bytes leave out section 11's arrays", L.resident, L.total);
  // the panel's own offsets are chain_prior_layout's: osc_chain_prior_many's stage addresses them from the block's start
  const ChainPriorLayout P = chain_prior_layout(N, qc);
  if (P.total != L.panel.total || P.X != L.panel.X || P.node != L.panel.node) return fail("panel offsets", P.total, L.panel.total);
  // the last element the row kernels read of kappa: row N - 1, the last query's last node
  if (((N - 1) * L.ks + msum - 1) * 4 + 4 > N * (long long)L.ks * 4) return fail("kappa index", N, msum);
  return 0;
}

// kind 0 one chain of m distinct nodes shared by all, 1 a chain per query (2..9 nodes, repeats), 2 a chain of m distinct nodes
// per query
static int check_passes(long long N, int Q, int kind, int m, int kpad, int max_queries, int max_cols, long long budget) {
  std::vector<int64_t> off;
  std::vector<int> nodes;
  make_chains(N, Q, kind == 0, kind == 1 ? 0 : m, off, nodes);
  if (chain_prior_check(off.data(), nodes.data(), Q) != -1) return fail("a chain of at most 64 distinct nodes refused", N, m);
  const std::vector<ChainPriorPass> ps = bundle_prior_passes(off.data(), nodes.data(), Q, N, kpad, max_queries, max_cols, budget);
  if (check_packing(ps, off, nodes, Q, max_queries, max_cols, [&](int qc, long long msum, long long, int nq) {
        return bundle_prior_layout(N, qc, msum, nq, kpad).resident > budget;
      }))
    return 1;
  for (const ChainPriorPass& p : ps) {
    const int gs = bundle_prior_group(p.mmax);
    if (gs < p.mmax || gs > 64 || (gs & (gs - 1)) != 0 || (gs > 1 && gs / 2 >= p.mmax)) return fail("group size", gs, p.mmax);
    if (check_layout(N, p.qc, p.msum, p.nq, kpad)) return 1;
  }
  return 0;
}

int main() {
  const long long Ns[] = {1, 2, 31, 33, 64, 65, 1000, 4097, 65536, 100000, 500000, 1999999, 2000000};
  const int Qs[] = {1, 2, 31, 32, 33, 255, 256, 257, 513, 1000};
  const int ms[] = {1, 2, 8, 31, 32, 33, 63, 64};
  const int colss[] = {0, 8, 33};
  const int kpads[] = {32, 64, 768};
  long long cases = 0;
  for (long long N : Ns) {
    for (int qc = 32; qc <= 512; qc += 96)
      for (int m : ms) {
        if (check_layout(N, qc, (long long)m * 7, 7, 768)) return 1;
        ++cases;
      }
    for (int Q : Qs)
      for (int kind = 0; kind < 3; ++kind)
        for (int m : ms) {
          if (kind == 1 && m != 8) continue;          // (its chains draw their own lengths)
          if (kind == 2 && Q > 257 && m > 8) continue;  // (wide chains: the small counts cover the seams)
          const int max_cols = colss[(size_t)(cases % 3)], kpad = kpads[(size_t)(cases % 3)];
          if (check_passes(N, Q, kind, m, kpad, 256, max_cols, kChainPriorBudgetBytes)) return 1;
          if (check_passes(N, Q, kind, m, kpad, 7, max_cols, (long long)1 << 24)) return 1;
          cases += 2;
        }
  }
  // a lone query may exceed the budget: 64 nodes at N = 2 000 000
  {
    std::vector<int64_t> off;
    std::vector<int> nodes;
    make_chains(2000000, 3, false, 64, off, nodes);
    const std::vector<ChainPriorPass> ps = bundle_prior_passes(off.data(), nodes.data(), 3, 2000000, 768, 256, 0, kChainPriorBudgetBytes);
    if (ps.size() != 3) return fail("three lone queries", (long long)ps.size(), 3);
    if (bundle_prior_layout(2000000, ps[0].qc, ps[0].msum, 1, 768).resident <= kChainPriorBudgetBytes) return fail("expected a pass over the budget", 0, 0);
  }
  std::printf("bundle prior plan sweep ok (%lld cases)\n", cases);
  return 0;
}

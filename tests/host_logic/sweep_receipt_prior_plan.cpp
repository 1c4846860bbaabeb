// Sweep of receipt_prior_plan.hpp (osc_receipt_prior_many) for N from 1 to 2 000 000, Q from 1 to 1000 and
// chains of 1 to 64 distinct nodes, in both detail modes: the passes tile [0, Q) in order; no query is split -- every
// distinct node of a query is a column of its pass, once; msum and msq are the sums of the queries' distinct node counts and
// of their squares; a pass of more than one query keeps its resident bytes within the budget, its queries within the chunk and
// its columns within the forced limit; the arrays of a layout are 256-byte aligned, pairwise disjoint, inside the block and
// large enough for what the kernels index; the light layout is no larger than the full one and holds no N x Q array; the row
// partition, the Gram sums' groups and the panel's offsets are functions of N (and qc) alone; the passes are the greedy ones
// and their columns stand in first-seen order (sweep_prior_common.hpp).  Run under
// -fsanitize=address,undefined.
#include <cstdlib>

#include "../../oscillink_amd/csrc/receipt_prior_plan.hpp"
#include "sweep_prior_common.hpp"

// osc_query.hip's partials of the coherence column sums (query.hpp: rm_col_parts, rm_finish_groups)
static int col_parts(long long N) { return (int)std::max<long long>(1, std::min<long long>((N + 63) / 64, 512)); }
static int fin_groups(int nb) { return (nb + 63) / 64; }

static int check_layout(long long N, int qc, long long msum, long long msq, int nq, int kpad, int ld) {
  const int cp = col_parts(N), cg = fin_groups(cp);
  const ReceiptPriorLayout F = receipt_prior_layout(N, qc, msum, msq, nq, kpad, ld, true, cp, cg);
  const ReceiptPriorLayout L = receipt_prior_layout(N, qc, msum, msq, nq, kpad, ld, false, cp, cg);
  const ChainPriorLayout P = chain_prior_layout(N, qc);
  for (const ReceiptPriorLayout* l : {&F, &L})
    if (P.total != l->panel.total || P.X != l->panel.X || P.node != l->panel.node) return fail("panel offsets", P.total, l->panel.total);
  if (L.total > F.total || L.resident > F.resident) return fail("the light layout is larger than the full one", L.total, F.total);
  if (L.resident != L.total) return fail("the light layout counts N x Q arrays", L.resident, L.total);
  // light: the panel and per-query scalars only
  if (check_blocks({{0, P.total}, {L.e, nq * 64LL * 8}, {L.H, nq * 4096LL * 8}, {L.J, nq * 4096LL * 8}, {L.Z, nq * 4096LL * 8},
                    {L.scal, nq * 32LL + nq * 8LL}},
                   L.total))
    return 1;
  if (L.total - P.total > nq * (3 * 4096LL + 64 + 5) * 8 + 6 * 256) return fail("light bytes beyond the per-query scalars", L.total, P.total);
  const BundlePriorLayout Bp = bundle_prior_layout(N, qc, msum, nq, kpad);
  if (F.kappa != Bp.kappa || F.nu != Bp.nu || F.bt != Bp.bt || F.e != Bp.e || F.H != Bp.H || F.ks != Bp.ks || F.qs != Bp.qs)
    return fail("bundle_prior_layout's arrays moved", F.kappa, Bp.kappa);
  const long long parts = gates_parts(N), slabs = qc / kGatesSlab;
  if (F.wout != 2 * ld + 2) return fail("moment row", F.wout, ld);
  if (F.mom_slabs < 1 || F.mom_slabs > slabs) return fail("moment slabs", F.mom_slabs, slabs);
  if (F.mom_slabs > 1 && (long long)F.mom_slabs * parts * 32 * F.wout * 4 > kReceiptPriorMomentBytes) return fail("moment partials over their limit", F.mom_slabs, parts);
  if (F.groups < 1 || F.groups > kReceiptPriorGramGroups || F.groups != receipt_prior_gram_groups(N)) return fail("gram groups", F.groups, N);
  if ((long long)receipt_prior_gram_group_parts(N) * F.groups < parts) return fail("gram groups leave parts out", F.groups, parts);
  if (check_blocks({{0, Bp.total},
                    {F.J, nq * 4096LL * 8},
                    {F.Z, nq * 4096LL * 8},
                    {F.scal, nq * 32LL + nq * 8LL},
                    {F.mom_part, (long long)F.mom_slabs * parts * 32 * F.wout * 4},
                    {F.mom, (long long)qc * F.wout * 8},
                    {F.gram_part, (long long)F.groups * 2 * msq * 8},
                    {F.z, N * (long long)F.qs * 4},
                    {F.j, N * (long long)F.qs * 4},
                    {F.r, N * (long long)F.qs * 4},
                    {F.zt, N * (long long)nq * 4},
                    {F.coh, N * (long long)F.qs * 8},
                    {F.cohpart, (long long)cp * nq * 8},
                    {F.cohfin, (long long)cg * nq * 8}},
                   F.total))
    return 1;
  if (F.resident < F.total + 2 * N * (long long)F.qs * 4) return fail("resident bytes leave out section 11's arrays", F.resident, F.total);
  return 0;
}

// kind 0 one chain of m distinct nodes shared by all, 1 a chain per query (2..9 nodes, repeats), 2 a chain of m distinct nodes
// per query
static int check_passes(long long N, int Q, int kind, int m, int kpad, int ld, bool full, int max_queries, int max_cols,
                        long long budget) {
  std::vector<int64_t> off;
  std::vector<int> nodes;
  make_chains(N, Q, kind == 0, kind == 1 ? 0 : m, off, nodes);
  const int cp = col_parts(N), cg = fin_groups(cp);
  const std::vector<ChainPriorPass> ps =
      receipt_prior_passes(off.data(), nodes.data(), Q, N, kpad, ld, full, cp, cg, max_queries, max_cols, budget);
  if (check_packing(ps, off, nodes, Q, max_queries, max_cols, [&](int qc, long long msum, long long msq, int nq) {
        return receipt_prior_layout(N, qc, msum, msq, nq, kpad, ld, full, cp, cg).resident > budget;
      }))
    return 1;
  for (const ChainPriorPass& p : ps)
    if (check_layout(N, p.qc, p.msum, p.msq, p.nq, kpad, ld)) return 1;
  return 0;
}

int main() {
  const long long Ns[] = {1, 2, 31, 33, 64, 65, 1000, 4097, 65536, 100000, 500000, 1999999, 2000000};
  const int Qs[] = {1, 2, 31, 32, 33, 255, 256, 257, 513, 1000};
  const int ms[] = {1, 2, 8, 31, 32, 33, 63, 64};
  const int colss[] = {0, 8, 33};
  const int lds[] = {20, 64, 768};
  long long cases = 0;
  for (long long N : Ns) {
    // the row partition is a function of N alone: whole parts of a multiple of 32 rows that cover [0, N)
    const long long pr = gates_part_rows(N), parts = gates_parts(N);
    if (pr % kGatesStepRows != 0 || parts < 1 || parts > kGatesMaxParts || (parts - 1) * pr >= N || parts * pr < N)
      return fail("row partition", N, parts);
    for (int qc = 32; qc <= 512; qc += 96)
      for (int m : ms) {
        if (check_layout(N, qc, (long long)m * 7, (long long)m * m * 7, 7, 768, 768)) return 1;
        if (gates_parts(N) != parts || receipt_prior_gram_groups(N) != std::min<long long>(parts, kReceiptPriorGramGroups)) return fail("partition moved", N, qc);
        ++cases;
      }
    for (int Q : Qs)
      for (int kind = 0; kind < 3; ++kind)
        for (int m : ms) {
          if (kind == 1 && m != 8) continue;          // (its chains draw their own lengths)
          if (kind == 2 && Q > 257 && m > 8) continue;  // (wide chains: the small counts cover the seams)
          const int max_cols = colss[(size_t)(cases % 3)], ld = lds[(size_t)(cases % 3)], kpad = (ld + 31) / 32 * 32;
          const bool full = (cases / 3) % 2 == 0;
          if (check_passes(N, Q, kind, m, kpad, ld, full, 256, max_cols, kChainPriorBudgetBytes)) return 1;
          if (check_passes(N, Q, kind, m, kpad, ld, !full, 7, max_cols, (long long)1 << 24)) return 1;
          cases += 2;
        }
  }
  // a lone query may exceed the budget: 64 nodes at N = 2 000 000
  {
    std::vector<int64_t> off;
    std::vector<int> nodes;
    make_chains(2000000, 3, false, 64, off, nodes);
    const int cp = col_parts(2000000), cg = fin_groups(cp);
    const std::vector<ChainPriorPass> ps =
        receipt_prior_passes(off.data(), nodes.data(), 3, 2000000, 768, 768, true, cp, cg, 256, 0, kChainPriorBudgetBytes);
    if (ps.size() != 3) return fail("three lone queries", (long long)ps.size(), 3);
    if (receipt_prior_layout(2000000, ps[0].qc, ps[0].msum, ps[0].msq, 1, 768, 768, true, cp, cg).resident <= kChainPriorBudgetBytes)
      return fail("expected a pass over the budget", 0, 0);
  }
  std::printf("receipt prior plan sweep ok (%lld cases)\n", cases);
  return 0;
}

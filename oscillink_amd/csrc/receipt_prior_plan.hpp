// The host plan of osc_receipt_prior_many: receipt() of Q (query, chain prior) pairs on a resident
// lattice.  HIP-free: osc_query.hip runs it, tests/host_logic/sweep_receipt_prior_plan.cpp sweeps it under the sanitizers.
//
// A pass is chain_prior_plan.hpp's ChainPriorPass, cut by its packer: a run of consecutive queries, one panel column per
// distinct chain node of the pass, a query never split.  Its block holds, behind bundle_prior_layout's arrays, the per-query Gram blocks and scalars of deltaH
// and -- full detail only -- the moments of the Green's columns (partials per (part, slab) for mom_slabs slabs at a time,
// then one row of wout doubles per column), the chains' Gram partials and the per-(row, query) arrays of the row pass and
// the null-point stage.  A light pass holds the panel and the per-query scalars alone.  The rows are cut by section 17's
// partition (gates_parts / gates_part_rows: functions of N alone); the Gram sums add runs of consecutive parts.
#pragma once
#include "bundle_prior_plan.hpp"

namespace osc {
namespace host {

constexpr int32_t kReceiptPriorGramGroups = 16;                 // runs of parts a chain's Gram sums are split into at most
constexpr int64_t kReceiptPriorMomentBytes = (int64_t)256 << 20;  // moment partials held at a time (at least one slab's)
constexpr int32_t kReceiptPriorScalars = 5;                     // doubles a query leaves: deltaH, anchor sum, query sum, spare;
                                                                // then a float (the bound) and an int32 (the iterations)

// columns of a moment row: [X' - Y | B X'] at pitch ld each, then x' and B (x' - 1)
inline int32_t receipt_prior_wout(int32_t ld) { return 2 * ld + 2; }

// runs of consecutive parts of the Gram sums: functions of N alone
inline int32_t receipt_prior_gram_groups(int64_t N) { return std::min(gates_parts(N), kReceiptPriorGramGroups); }
inline int32_t receipt_prior_gram_group_parts(int64_t N) {
  const int32_t g = receipt_prior_gram_groups(N);
  return (gates_parts(N) + g - 1) / g;
}

// slabs whose moment partials are held at a time
inline int32_t receipt_prior_moment_slabs(int64_t N, int32_t qc, int32_t ld) {
  const int64_t per = (int64_t)gates_parts(N) * kGatesSlab * receipt_prior_wout(ld) * 4;
  return (int32_t)std::max<int64_t>(1, std::min<int64_t>(qc / kGatesSlab, kReceiptPriorMomentBytes / std::max<int64_t>(per, 1)));
}

struct ReceiptPriorLayout {
  ChainPriorLayout panel;
  bool full = false;
  int32_t ks = 0, qs = 0;     // bundle_prior_layout's pitches (full)
  int32_t wout = 0, mom_slabs = 0, groups = 0;
  int64_t kappa = 0, nu = 0, bt = 0;   // bundle_prior_layout's arrays (full)
  int64_t e = 0, H = 0;       // double [nq][64], [nq][64][64]
  int64_t J = 0, Z = 0;       // double [nq][64][64] each: F0 C^T and F0 F0^T
  int64_t scal = 0;           // double [nq][4], then float [nq] and int32 [nq]
  int64_t mom_part = 0;       // float  [mom_slabs][parts][32][wout]
  int64_t mom = 0;            // double [qc][wout]
  int64_t gram_part = 0;      // double [groups][2][msq]
  int64_t z = 0, j = 0, r = 0;  // float / int32 / float [N][qs]
  int64_t zt = 0;             // float  [nq][N]
  int64_t coh = 0;            // double [N][qs]
  int64_t cohpart = 0;        // double [cparts][nq], then the finish's groups
  int64_t cohfin = 0;
  int64_t total = 0;
  int64_t resident = 0;       // total + the two N x qs float arrays of section 11 the row pass reads and writes (align, p)
};

// msq: the sum of m_q^2 over the pass's queries (a bound on the chains' Gram entries); cparts / cgroups: the partials of the
// coherence column sums and of their finish (query.hpp: rm_col_parts, rm_finish_groups)
inline ReceiptPriorLayout receipt_prior_layout(int64_t N, int32_t qc, int64_t msum, int64_t msq, int32_t nq, int32_t kpad,
                                               int32_t ld, bool full, int32_t cparts, int32_t cgroups) {
  ReceiptPriorLayout L{};
  L.full = full;
  L.panel = chain_prior_layout(N, qc);
  int64_t o = L.panel.total;
  auto take = [&](int64_t bytes) {
    const int64_t at = o;
    o += gates_align(bytes);
    return at;
  };
  const int64_t nodes = kChainPriorMaxNodes;
  if (full) {
    const BundlePriorLayout b = bundle_prior_layout(N, qc, msum, nq, kpad);
    L.ks = b.ks;
    L.qs = b.qs;
    L.kappa = b.kappa;
    L.nu = b.nu;
    L.bt = b.bt;
    L.e = b.e;
    L.H = b.H;
    o = b.total;
  } else {
    L.e = take((int64_t)nq * nodes * 8);
    L.H = take((int64_t)nq * nodes * nodes * 8);
  }
  L.J = take((int64_t)nq * nodes * nodes * 8);
  L.Z = take((int64_t)nq * nodes * nodes * 8);
  L.scal = take((int64_t)nq * kReceiptPriorScalars * 8);
  if (full) {
    L.wout = receipt_prior_wout(ld);
    L.mom_slabs = receipt_prior_moment_slabs(N, qc, ld);
    L.groups = receipt_prior_gram_groups(N);
    L.mom_part = take((int64_t)L.mom_slabs * gates_parts(N) * kGatesSlab * L.wout * 4);
    L.mom = take((int64_t)qc * L.wout * 8);
    L.gram_part = take((int64_t)L.groups * 2 * msq * 8);
    L.z = take(N * (int64_t)L.qs * 4);
    L.j = take(N * (int64_t)L.qs * 4);
    L.r = take(N * (int64_t)L.qs * 4);
    L.zt = take(N * (int64_t)nq * 4);
    L.coh = take(N * (int64_t)L.qs * 8);
    L.cohpart = take((int64_t)cparts * nq * 8);
    L.cohfin = take((int64_t)std::max(cgroups, 1) * nq * 8);
  }
  L.total = o;
  L.resident = o + (full ? 2 * gates_align(N * (int64_t)L.qs * 4) : 0);
  return L;
}

// Passes over queries [0, Q) by chain_prior_pack: layout.resident within `budget` bytes unless the pass holds one query.
inline std::vector<ChainPriorPass> receipt_prior_passes(const int64_t* off, const int32_t* nodes, int32_t Q, int64_t N,
                                                        int32_t kpad, int32_t ld, bool full, int32_t cparts, int32_t cgroups,
                                                        int32_t max_queries, int32_t max_cols, int64_t budget) {
  return chain_prior_pack(off, nodes, Q, max_queries, max_cols, [&](int32_t qc, int64_t msum, int64_t msq, int32_t nq) {
    return receipt_prior_layout(N, qc, msum, msq, nq, kpad, ld, full, cparts, cgroups).resident <= budget;
  });
}

}  // namespace host
}  // namespace osc

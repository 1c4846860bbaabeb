// The host plan of osc_bundle_prior_many: bundle() of Q (query, chain prior) pairs on a resident
// lattice.  HIP-free: osc_query.hip runs it, tests/host_logic/sweep_bundle_prior_plan.cpp sweeps it under the sanitizers.
//
// A pass is chain_prior_plan.hpp's ChainPriorPass, cut by its packer -- a run of consecutive queries, one panel column per
// distinct chain node of the pass, a query never split -- whose block also holds, for its queries' m_q distinct nodes (msum
// their sum, mmax the largest), kappa (N x sum m_q floats, row pitch ks), nu
// (N x qs doubles), the kappa GEMM's operand and section 11's three N x qs float arrays.  The pass takes queries while all of
// that fits the budget; a pass of one query is as large as that query needs.
#pragma once
#include "chain_prior_plan.hpp"

namespace osc {
namespace host {

// one pass's block: chain_prior_layout's arrays at its own offsets from 0, then the arrays of the bundle
struct BundlePriorLayout {
  ChainPriorLayout panel;
  int32_t ks = 0;      // row pitch of kappa: msum rounded up to 4
  int32_t qs = 0;      // row pitch of the N x nq arrays: nq rounded up to 4
  int64_t kappa = 0;   // float  [N][ks]
  int64_t nu = 0;      // double [N][qs]
  int64_t bt = 0;      // float  [msum rounded up to 128][kpad]
  int64_t e = 0;       // double [nq][64]
  int64_t H = 0;       // double [nq][64][64]
  int64_t total = 0;   // bytes of the block
  int64_t resident = 0;  // total + the three N x qs float arrays of section 11 (align, p, coh)
};

inline BundlePriorLayout bundle_prior_layout(int64_t N, int32_t qc, int64_t msum, int32_t nq, int32_t kpad) {
  BundlePriorLayout L{};
  L.panel = chain_prior_layout(N, qc);
  L.ks = (int32_t)((msum + 3) / 4 * 4);
  L.qs = (nq + 3) / 4 * 4;
  int64_t o = L.panel.total;
  auto take = [&](int64_t bytes) {
    const int64_t at = o;
    o += gates_align(bytes);
    return at;
  };
  L.kappa = take(N * (int64_t)L.ks * 4);
  L.nu = take(N * (int64_t)L.qs * 8);
  L.bt = take((msum + 127) / 128 * 128 * (int64_t)kpad * 4);
  L.e = take((int64_t)nq * kChainPriorMaxNodes * 8);
  L.H = take((int64_t)nq * kChainPriorMaxNodes * kChainPriorMaxNodes * 8);
  L.total = o;
  L.resident = o + 3 * gates_align(N * (int64_t)L.qs * 4);
  return L;
}

// Passes over queries [0, Q) by chain_prior_pack: layout.resident within `budget` bytes unless the pass holds one query.
inline std::vector<ChainPriorPass> bundle_prior_passes(const int64_t* off, const int32_t* nodes, int32_t Q, int64_t N,
                                                       int32_t kpad, int32_t max_queries, int32_t max_cols, int64_t budget) {
  return chain_prior_pack(off, nodes, Q, max_queries, max_cols, [&](int32_t qc, int64_t msum, int64_t, int32_t nq) {
    return bundle_prior_layout(N, qc, msum, nq, kpad).resident <= budget;
  });
}

// lanes a (row, query) pair takes in the row kernels: mmax rounded up to a power of two, 1 to 64
inline int32_t bundle_prior_group(int32_t mmax) {
  int32_t gs = 1;
  while (gs < mmax && gs < kChainPriorMaxNodes) gs *= 2;
  return gs;
}

}  // namespace host
}  // namespace osc

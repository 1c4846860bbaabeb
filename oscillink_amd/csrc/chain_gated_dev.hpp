// Device helper of the chain prior under per-query gates, shared by the kernels that read the path
// kernels' sums (bundle_gated_kernels.hip, receipt_gated_kernels.hip) and the ones that write them (chain_gated_kernels.hip).
#pragma once
#include "bundle_gated_dev.hpp"
#include "chain_gated.hpp"

namespace osc {
namespace {

// the path kernels' share of a slab's column sums: the fix units of the slab's query in order.  Valid in threads 0..31
// (column = thread), like gm_part_sum's total, to which the caller adds it.
__device__ __forceinline__ double cg_unit_sum(const CgChain& ch, int slab, int q) {
  double s = 0.0;
  if (threadIdx.x < 32) {
    const int nu = (ch.q_rows[q] + host::kChainFixRows - 1) / host::kChainFixRows;
    const double* part = ch.part + (size_t)slab * ch.max_units * 32 + threadIdx.x;
    for (int u = 0; u < nu; ++u) s += part[(size_t)u * 32];
  }
  return s;
}

}  // namespace
}  // namespace osc

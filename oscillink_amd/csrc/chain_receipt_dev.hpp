// chain_receipt's per-edge and per-chain rules (lattice.py:466-528), shared by the candidate lattices of a corpus refine
// (k_cq_chain_receipt, corpus_chain_kernels.hip) and the built lattice's batched call (chain_many_kernels.hip).  Device code:
// include from .hip translation units only.
#pragma once
#include <hip/hip_runtime.h>

namespace osc {

// z of the entry r of a dense residual row of n entries, zeros included, from the row's sums s1 = sum R, s2 = sum R^2:
// mu = s1 / n, sigma = sqrt(s2 / n - mu^2) + 1e-12
__device__ __forceinline__ double chain_row_z(double s1, double s2, float r, double n) {
  const double mu = s1 / n;
  const double var = fmax(s2 / n - mu * mu, 0.0);
  return ((double)r - mu) / (sqrt(var) + 1e-12);
}

// Python's max(z_struct, z_path)
__device__ __forceinline__ double chain_zmax(double z_s, double z_p) { return z_p > z_s ? z_p : z_s; }

// One chain from its E edges' gain terms and max(z): the gain added in fp64 in edge order, the first edge whose max(z) is
// strictly greater than every earlier one, from -1 (lattice.py:489, 506; k = -1 when none is), the verdict
// all(max(z) <= z_th)
struct ChainVerdict {
  double gain, worst;
  int weak_k, ok;
};
__device__ __forceinline__ ChainVerdict chain_finish(const double* term, const double* zmax, int E, float z_th) {
  ChainVerdict v{0.0, -1.0, -1, 1};
  for (int t = 0; t < E; ++t) {
    v.gain += term[t];
    if (zmax[t] > v.worst) {
      v.worst = zmax[t];
      v.weak_k = t;
    }
    if (!(zmax[t] <= (double)z_th)) v.ok = 0;
  }
  return v;
}

}  // namespace osc

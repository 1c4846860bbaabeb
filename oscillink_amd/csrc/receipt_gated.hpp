// Receipts under per-query gates: the kernels behind osc_receipt_gated_many
// (receipt_gated_kernels.hip).  The solves are bundle_gated.hpp's panel PCG -- the settle's (I + dt M_q) is the same
// operator with lamG' = 1 + dt lamG, lamC' = dt lamC, lamQ' = dt lamQ -- and everything here works on its slab-major panels
// in device row order: query t owns the slabs [t spq, (t + 1) spq).
#pragma once
#include "bundle_gated.hpp"
#include "receipt_gated_plan.hpp"

namespace osc {

// The settle's start (lattice.py:184-196, solver.py:18-22 with x0 = U): ps carries the primed lambdas and the settle's
// tol; x = U (N x ld, device rows), r = dt [lamG (y - u) + lamQ g (psi - u) + lamC (W u - u)] with the true lambdas,
// p = z = r / (lamG' + lamQ' g + 1e-12); part_a: r . z (prior: chain_gated.hpp's form with -dt lamP u on every row)
void launch_rg_settle_init(const BgPanel& ps, const GmGraph& g, const float* U, const float* Y, int32_t ld, float dt, float lamG,
                           float lamC, float lamQ, hipStream_t s, const CgPrior* prior = nullptr);
// P = Us - X over every slab, Us the settled panel or (Us == nullptr) the state U (N x ld) for every query; every query live
void launch_rg_diff(const BgPanel& p, const float* Us, const float* U, int32_t ld, hipStream_t s);
// dh[q] = sum over the query's columns of part_a (launch_bg_apply's p . M_q p): parts, then columns, then slabs, in order
// (with chain: and the fix units' share of each column, chain_gated.hpp)
void launch_rg_deltah(const BgPanel& p, double* dh, hipStream_t s, const CgChain* chain = nullptr);

// per (row, query) on the solved panel p.X, one wave each, fp64 (receipts.py:28-83 on the capped adjacency):
//   anchor = lamG |U*_i - Y_i|^2, query = lamQ g_i |U*_i - psi|^2, coh = 1/2 lamC (ysum_i - sum_j A_ij |Un_i - Un_j|^2),
//   R_ij = lamC A_ij |Un_i - Un_j|^2 with Un = U* / (sqrt_deg + 1e-12): S1, S2 and the first argmax in API column order,
//   z = (R_max - S1 / N) / (sqrt(S2 / N - (S1 / N)^2) + 1e-12); a null point when R_max > 0 and z > z_th.
// comp: [3][N][qs] doubles (coh, anchor, query); z / j / r as RmRowsArgs' (j an API id, z = -inf without a null point)
struct RgRowsArgs {
  const int32_t* col;   // ELL, device rows
  const float* adj;     // capped adjacency
  const int32_t* deg;
  int32_t width;
  const float* sqrt_deg;
  const float* Y;       // N x ld
  int32_t ld, qs;
  const double* ysum;   // [N] launch_bg_ysum's
  const int32_t* api_id;  // nullptr = identity
  float z_th;
  double* comp;
  float* z;
  int32_t* j;
  float* r;
};
void launch_rg_components(const BgPanel& p, const RgRowsArgs& a, hipStream_t s);

}  // namespace osc

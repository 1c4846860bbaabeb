// Per-query gates with per-query chain priors: the kernels behind osc_chain_gated_many
// (chain_gated_kernels.hip).  With gates every query is its own N x D panel solve already (bundle_gated.hpp), so query q's
// chain prior is a term of its own operator,
//   M_q = (lamG + lamP) I + lamC L_sym + lamQ diag(g_q) - lamP W_path,q,
// and no low-rank machinery: the panel runs with lamG + lamP in lamG's place (the Jacobi diagonal is then the reference's flat
// lamG + lamQ g + lamP, lattice.py:186-192, 257-259), and W_path,q -- entries on the chain's few rows only -- is applied by
// a small kernel behind launch_bg_apply, per (fix unit of the query's path rows, slab of the query).
#pragma once
#include "bundle_gated.hpp"
#include "chain_gated_plan.hpp"
#include "query.hpp"

namespace osc {

// a chunk's paths on the device (chain_gated_plan.hpp: ChainGatedLayout; pcol is ChainManyPaths' column array)
struct CgChain {
  static constexpr bool active = true;
  const int32_t* prow;    // device row of every packed path row
  const int32_t* pbeg;    // the row's entries [pbeg, pend) in pcol / pw
  const int32_t* pend;
  const int32_t* pcol;    // device rows
  const float* pw;        // W_path
  const int32_t* q_row0;  // [nq] first packed row of the query's path
  const int32_t* q_rows;  // [nq] its rows
  double* part;           // [slabs][max_units][32] column sums per fix unit
  int32_t max_units;      // the pitch of part: the most units a chain of the call's longest length can have
  int32_t grid_units;     // the most units of any query of this chunk: the path kernels' grid
};
// in the chain's place for a call without one: the kernels that fold the units' sums compile to the code they were
struct CgNoChain {
  static constexpr bool active = false;
};

// The prior form of the init kernels (launch_bg_init, launch_rg_settle_init), an instantiation of its own: L_path is the
// identity off the chain, so every row's start residual carries -cP x0_i (cP = lamP with x0 = Y for the U* solve, dt lamP with
// x0 = U for the settle).  CgNoPrior compiles to the kernels the calls without a chain launch.
struct CgPrior {
  static constexpr bool active = true;
  float cP;
};
struct CgNoPrior {
  static constexpr bool active = false;
};

// The start residual's chain rows (L_path = I - W_path; the identity's share is the init kernels' own, on every row):
// r += cP sum_e w_e src_col(e) over the query's path rows, src the anchors (U* solve) or the state U (settle), N x ld;
// p = z = r / (lamG + lamQ g + 1e-12) with the panel's lamG; ch.part: the change of r . z per fix unit
void launch_cg_path_init(const BgPanel& p, const CgChain& ch, const float* src, int32_t ld, float cP, hipStream_t s);
// behind launch_bg_apply, over the live queries' slabs: AP_i -= cP sum_e w_e P_col(e) on the query's path rows;
// ch.part: the unit's share of p . Ap
void launch_cg_path_apply(const BgPanel& p, const CgChain& ch, float cP, hipStream_t s);
// launch_cm_edges' computation with U*_q read from the solved slab-major panel a.X (query t of the chunk: the slabs
// [t spq, (t + 1) spq) of N x 32 floats); a.x4 and a.psi are not read
void launch_cg_edges(const CmEdgesArgs& a, hipStream_t s);

}  // namespace osc

// Bundles under per-query gates: the kernels behind osc_bundle_gated_many
// (bundle_gated_kernels.hip).  With gates g_q the operator M_q = lamG I + lamC L_sym + lamQ diag(g_q) differs per query, so a
// chunk is nq honest N x D solves of the reference's solve_Ustar (lattice.py:245-263, solver.py:6-37) run as ONE Jacobi-PCG
// over the handle's ELL graph: alpha / beta per column, the stop per query.  Arrays are slab-major panels in device row
// order (bundle_gated_plan.hpp); query t owns the slabs [t spq, (t + 1) spq).
#pragma once
#include "../../include/oscillink_hip.h"
#include "bundle_gated_plan.hpp"
#include "common.hpp"
#include "gates_many.hpp"

namespace osc {

struct CgChain;  // chain_gated.hpp: a chunk's chain priors; nullptr for a call without them
struct CgPrior;

// one chunk's arrays (pointers into the scratch block at GatedLayout's offsets)
struct BgPanel {
  float* X;
  float* R;
  float* P;
  float* AP;
  const float* gate;   // [nq][N] device row order
  const float* psi;    // [nq][spq 32], zero past D
  double* part_a;      // [slabs][parts][32]
  double* part_b;
  double* rz;          // [slabs 32] r . z of the last iteration
  float* alpha;
  float* beta;
  float* res;          // [nq] max over the query's columns of |r_c| after its last iteration
  int32_t* live;       // [nq] 1 while the query iterates
  int32_t* iters;      // [nq]
  int32_t* n_live;     // [2]
  int32_t N, slabs, parts, part_rows, nq, spq, D;
  float lamG, lamC, lamQ, tol;
};

// gate[q][device row] = gate_api[q][API row of that device row] (api_id: device row -> API row, nullptr = identity)
void launch_bg_gates(const float* gate_api, const int32_t* api_id, int32_t N, int32_t nq, float* gate, hipStream_t s);
// x = Y, r = RHS - M_q Y = lamQ g (psi - y) + lamC (W y - y) formed on the fly from the anchors (N x ld, device rows),
// p = z = r / (lamG + lamQ g + 1e-12); part_a: r . z
// (prior: chain_gated.hpp's form with -cP y on every row)
void launch_bg_init(const BgPanel& p, const GmGraph& g, const float* Y, int32_t ld, hipStream_t s, const CgPrior* prior = nullptr);
// rz per column from those sums (with chain: and the fix units' behind them); every query live, iters = 0; n_live = 0
void launch_bg_start(const BgPanel& p, hipStream_t s, const CgChain* chain = nullptr);
// AP = (lamG + lamC + lamQ g) p - lamC W p over the live queries' slabs; part_a: p . Ap
void launch_bg_apply(const BgPanel& p, const GmGraph& g, hipStream_t s);
// alpha = rz / (p . Ap + 1e-18) per column of a live query (with chain: p . Ap with the fix units' share, added in unit order)
void launch_bg_alpha(const BgPanel& p, hipStream_t s, const CgChain* chain = nullptr);
// x += alpha p, r -= alpha Ap over the live queries' slabs; part_a: r . r, part_b: r . z
void launch_bg_update(const BgPanel& p, hipStream_t s);
// per live query: res = max over its columns of sqrt(r . r), slabs and columns in order (a NaN stays); records (it, res) and
// freezes when res <= tol, else beta = rz' / (rz + 1e-18) per column; n_live[it & 1] = queries still live,
// n_live[(it + 1) & 1] = 0
void launch_bg_beta(const BgPanel& p, int it, hipStream_t s);
// p = r / (lamG + lamQ g + 1e-12) + beta p over the live queries' slabs
void launch_bg_direction(const BgPanel& p, hipStream_t s);

// the bundle's two columns from the solved panel (lattice.py:557-562, receipts.py:28-38 on the capped adjacency):
//   ysum_i = sum_j A_ij |Y_i / d_i - Y_j / d_j|^2, d = sqrt_deg + 1e-12, once per call (fp64, slot order)
//   align[i][q] = U_i . psi_q / ((|U_i| + 1e-12) (|psi_q| + 1e-12)),  coh[i][q] = 1/2 lamC (ysum_i - sum_j A_ij |U_i / d_i - U_j / d_j|^2)
// written into N x qs arrays (query.hpp's layout) for launch_query_score, the batched MMR and launch_query_pack
struct BgBundleArgs {
  const int32_t* col;   // ELL, device rows
  const float* adj;     // capped adjacency
  const int32_t* deg;
  int32_t width;
  const float* sqrt_deg;
  const float* Y;       // N x ld
  int32_t ld, qs;
  double* ysum;         // [N]
  float* align;         // N x qs
  float* coh;           // N x qs
};
void launch_bg_ysum(const BgPanel& p, const BgBundleArgs& a, hipStream_t s);
void launch_bg_bundle(const BgPanel& p, const BgBundleArgs& a, hipStream_t s);

}  // namespace osc

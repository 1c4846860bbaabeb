// Screened-diffusion gates for many queries on one lattice: the kernels behind osc_gates_many
// (gates_many_kernels.hip).  One CG with a right-hand side per query over the handle's ELL graph, every column stopped by
// its own residual.  Arrays are slab-major panels in device row order (gates_many_plan.hpp).
#pragma once
#include "../../include/oscillink_hip.h"
#include "common.hpp"
#include "gates_many_plan.hpp"

namespace osc {

// one chunk's arrays (pointers into the scratch block at GatesLayout's offsets)
struct GmPanel {
  float* X;
  float* R;
  float* P;
  float* AP;
  double* part_a;      // [slabs][parts][32]
  double* part_b;
  double* rz;          // [qc] r . z of the last iteration
  float* tol;          // [qc] the column's own stop tolerance
  float* alpha;
  float* beta;
  float* res;          // [qc] |r_q| after the column's last iteration
  float* lo;
  float* hi;
  int32_t* live;       // [qc] 1 while the column iterates
  int32_t* iters;      // [qc] iterations the column took
  int32_t* slab_live;  // [slabs]
  int32_t* n_live;     // [2]
  int32_t N, slabs, parts, part_rows, nq;
};

// the handle's graph: normalised weights W_ij (GraphView::w)
struct GmGraph {
  const int32_t* col;
  const float* w;
  const int32_t* deg;
  int32_t width;
};

// a per-row diagonal and the graph term's factor: the operator diag(d) - lamC W of the Green's columns
struct GmRowOp {
  const float* d = nullptr;  // [N]
  float lamC = 0.f;
};

// S = beta max(0, C) from the GEMM's cosines C (N x qc, row-major; columns >= nq count as 0); x = 0, r = S, p = z = r inv_md;
// part_a / part_b: the parts' column sums of r . z and s . s
void launch_gm_source(const GmPanel& p, const float* C, float beta, float inv_md, hipStream_t s);
// rz and tol per column from those sums (direct != 0: tol_q = 1e-7 max(1, |s_q|), else tol); live = the real columns
void launch_gm_init(const GmPanel& p, int direct, float tol, hipStream_t s);
// AP = cs p - W p over the live slabs; part_a: p . Ap
void launch_gm_apply(const GmPanel& p, const GmGraph& g, float cs, hipStream_t s);
// alpha = rz / (p . Ap + 1e-18) for live columns, 0 for frozen ones
void launch_gm_alpha(const GmPanel& p, hipStream_t s);
// x += alpha p, r -= alpha Ap on live columns (a frozen column's x and r are not written); part_a: r . r, part_b: r . z
void launch_gm_update(const GmPanel& p, float inv_md, hipStream_t s);
// per column: res = sqrt(r . r); a live column records (it, res) and freezes when res <= tol, else beta = rz' / (rz + 1e-18);
// n_live[it & 1] = columns still live, n_live[(it + 1) & 1] = 0
void launch_gm_beta(const GmPanel& p, int it, hipStream_t s);
// p = r inv_md + beta p over the live slabs
void launch_gm_direction(const GmPanel& p, float inv_md, hipStream_t s);
// lo / hi per column (two stages, fixed order, NaN kept), then out[q][api row] = clip((x - lo) / (hi - lo)) -- ones when
// hi - lo < 1e-12 -- or clip(x) with clamp == 0; inv: API row -> device row, nullptr = identity
void launch_gm_finish(const GmPanel& p, int clamp, const int32_t* inv, float* out, hipStream_t s);

// The same solve over M' = diag(d) - lamC W for unit right-hand sides (osc_chain_prior_many): d_i = c + lamQ B_i; column c
// starts from the unit vector of row node[c] (x = 0, r = e, p = r / d; node[c] < 0: a zero column); then launch_gm_init
// (direct = 0), and per iteration apply_rows / launch_gm_alpha / update_rows / launch_gm_beta / direction_rows, the Jacobi
// preconditioner being 1 / d_i.  The panel's lo / hi are not used.
void launch_gm_row_diag(const float* B, float c, float lamQ, int32_t N, float* d, hipStream_t s);
void launch_gm_unit_source(const GmPanel& p, const int32_t* node, const GmRowOp& op, hipStream_t s);
void launch_gm_apply_rows(const GmPanel& p, const GmGraph& g, const GmRowOp& op, hipStream_t s);
void launch_gm_update_rows(const GmPanel& p, const GmRowOp& op, hipStream_t s);
void launch_gm_direction_rows(const GmPanel& p, const GmRowOp& op, hipStream_t s);

}  // namespace osc

// Settle and receipt of the candidate lattices of a corpus refine chunk (osc_corpus_refine_receipts, DESIGN.md section
// 13.2): argument blocks and launchers of corpus_receipt_kernels.hip.  The kernels live in a translation unit of their
// own; the settle's iteration is corpus_pcg.hpp's cq_pcg, the one k_cq_solve of osc_corpus.hip runs.
#pragma once
#include "corpus_pcg.hpp"

namespace osc {

struct CqReceiptArgs {
  CqLattice lat;
  const float* Us;      // U* (union rows x ldn)
  const float* Up;      // the settled state U+ (union rows x ldn)
  int32_t full, cap, slots;
  float z_th;
  double* sums;         // nq x 4: deltaH, coh_drop, anchor_pen, query_term
  int32_t* n_total;     // nq
  int32_t* n_kept;      // nq
  int32_t* n_i;         // nq x slots (local row), and likewise below
  int32_t* n_j;
  float* n_z;
  float* n_r;
};

// one workgroup per lattice, nq lattices
void launch_cq_settle(const CqPcgArgs& a, int32_t nq, hipStream_t s);
void launch_cq_receipt(const CqReceiptArgs& a, int32_t nq, hipStream_t s);

}  // namespace osc

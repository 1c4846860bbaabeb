// Settle and receipt of the candidate lattices of a corpus refine chunk (osc_corpus_refine_receipts, DESIGN.md section
// 13.2): argument blocks and launchers of corpus_receipt_kernels.hip.  The kernels live in a translation unit of their
// own, so that the code object of osc_corpus.hip -- every kernel of a refine without receipts -- is the one it was.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

#include "corpus_plan.hpp"

namespace osc {

constexpr int kCqMaxRows = host::kCorpusMaxTopK;  // rows of a candidate lattice
constexpr int kCqMaxCols = 1536;                  // columns (Corpus: D <= 1536)

struct CqSettleArgs {
  const float* Y;     // union rows x ldn
  const float* psi;   // nq x ldn
  const int32_t* col;  // union ELL (width k, union row ids)
  const float* w;
  const int32_t* deg;
  float* X;           // out: the settled state U+ (starts as Y)
  float* R;
  float* P;
  float* AP;
  int32_t* iters;
  float* res;
  int32_t K, k, ldn, max_iters;
  float lamG, lamC, lamQ, dt, tol;
  const float* B;     // union rows: the gates, or nullptr (B = 1)
};

struct CqReceiptArgs {
  const float* Y;       // union rows x ldn
  const float* Us;      // U* (union rows x ldn)
  const float* Up;      // the settled state U+ (union rows x ldn)
  const float* psi;     // nq x ldn
  const int32_t* col;   // union ELL (width k, union row ids)
  const float* w;       // normalised weights (the operator's)
  const float* adj;     // capped adjacency (the receipt's)
  const int32_t* deg;
  const float* sd;
  const float* B;       // union rows: the gates, or nullptr (B = 1)
  int32_t K, k, ldn, full, cap, slots;
  float lamG, lamC, lamQ, z_th;
  double* sums;         // nq x 4: deltaH, coh_drop, anchor_pen, query_term
  int32_t* n_total;     // nq
  int32_t* n_kept;      // nq
  int32_t* n_i;         // nq x slots (local row), and likewise below
  int32_t* n_j;
  float* n_z;
  float* n_r;
};

// one workgroup per lattice, nq lattices
void launch_cq_settle(const CqSettleArgs& a, int32_t nq, hipStream_t s);
void launch_cq_receipt(const CqReceiptArgs& a, int32_t nq, hipStream_t s);

}  // namespace osc

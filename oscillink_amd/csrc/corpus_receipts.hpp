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

// a call with chains (osc_corpus_refine_chains): the same blocks with the chunk's chain records
struct CqChainPcgArgs {
  CqPcgArgs pcg;
  CqChain chain;
};
struct CqChainReceiptArgs {
  CqReceiptArgs rec;
  CqChain chain;
};

constexpr int kCqMaxChainEdges = 1023;  // a chain has at most 1024 nodes

// k_cq_chain_receipt: chain_receipt() of the lattice's own chain from U*
struct CqChainEdgesArgs {
  CqLattice lat;
  CqChain chain;
  const float* Us;      // U* (union rows x ldn)
  float z_th;
  float* edge;          // nq x 4 x cap: z_struct, z_path, r_struct, r_path per chain edge
  double* gain;         // nq
  int32_t* verdict;     // nq
  int32_t* weak_k;      // nq: -1 without a chain (or when no edge's z exceeds -1: lattice.py:489)
  float* weak_z;        // nq
};

// one workgroup per lattice, nq lattices
void launch_cq_settle(const CqPcgArgs& a, int32_t nq, hipStream_t s);
void launch_cq_receipt(const CqReceiptArgs& a, int32_t nq, hipStream_t s);
// the chain instantiations (corpus_chain_kernels.hip, corpus_receipt_kernels.hip); only calls with chains launch them
void launch_cq_solve_chain(const CqChainPcgArgs& a, int32_t nq, hipStream_t s);
void launch_cq_settle_chain(const CqChainPcgArgs& a, int32_t nq, hipStream_t s);
void launch_cq_receipt_chain(const CqChainReceiptArgs& a, int32_t nq, hipStream_t s);
void launch_cq_chain_receipt(const CqChainEdgesArgs& a, int32_t nq, hipStream_t s);

}  // namespace osc

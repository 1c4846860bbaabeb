// The chain prior of one candidate lattice of a corpus refine (osc_corpus_refine_chains) as a
// compact path structure: install_chain's arithmetic (osc_graph.hip) without the handle.  HIP-free: osc_corpus.hip runs it,
// tests/host_logic/sweep_corpus_chain.cpp sweeps it under the sanitizers.
//
// build_path_laplacian (graph.py:96-111): A_path[i][j] = A_path[j][i] = max(A_path[i][j], w) over the chain's steps, from
// zero -- so a weight below zero leaves a zero entry, a revisited edge keeps its largest weight and a self-step puts its
// weight on the diagonal.  normalized_laplacian (graph.py:86-93): W_p = (A_path / sd(r)) / sd(c) with
// sd = sqrt(max(rowsum, 1e-12)); L_path = I - W_p, so only rows that own an entry differ from the identity.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <map>
#include <utility>
#include <vector>

#include "corpus_plan.hpp"

namespace osc {
namespace host {

constexpr int32_t kCorpusMaxChain = 1024;  // nodes of one query's chain

struct ChainPath {
  std::vector<int32_t> rows;  // the rows that own a path entry, ascending
  std::vector<int32_t> ptr;   // rows.size() + 1: row t's entries are [ptr[t], ptr[t + 1])
  std::vector<int32_t> col;   // ascending within a row
  std::vector<float> a;       // A_path (the chain receipt's R_p)
  std::vector<float> w;       // (a * 1 / sd(r)) * 1 / sd(c) (the operators')
};

// nodes: len >= 2 local row ids in [0, K); weights: len - 1 values, or nullptr for ones
inline ChainPath build_chain_path(const int32_t* nodes, const float* weights, int32_t len, int32_t K) {
  ChainPath p;
  std::map<std::pair<int32_t, int32_t>, float> adj;
  for (int32_t t = 0; t + 1 < len; ++t) {
    const int32_t i = nodes[t], j = nodes[t + 1];
    if (i < 0 || i >= K || j < 0 || j >= K) continue;  // graph.py:107
    const float w = weights ? weights[t] : 1.0f;
    auto put = [&](int32_t r, int32_t c) {
      auto it = adj.find({r, c});
      if (it == adj.end()) adj[{r, c}] = std::max(0.0f, w);
      else it->second = std::max(it->second, w);
    };
    put(i, j);
    put(j, i);
  }
  std::map<int32_t, float> dsum;
  for (auto& kv : adj) dsum[kv.first.first] += kv.second;
  auto sd = [&](int32_t r) {
    auto it = dsum.find(r);
    return std::sqrt(std::max(it == dsum.end() ? 0.0f : it->second, 1e-12f));
  };
  for (auto& kv : adj) {  // (row, column) ascending
    const int32_t r = kv.first.first, c = kv.first.second;
    if (p.rows.empty() || p.rows.back() != r) {
      p.rows.push_back(r);
      p.ptr.push_back((int32_t)p.col.size());
    }
    p.col.push_back(c);
    p.a.push_back(kv.second);
    p.w.push_back((kv.second * (1.0f / sd(r))) * (1.0f / sd(c)));
  }
  p.ptr.push_back((int32_t)p.col.size());
  return p;
}

// One query's chain block on the device: int32 record [n_edges, n_rows, nodes[E + 1], rows[R], ptr[R + 1], col[2 E]] and
// float record [a[2 E], w[2 E]], E = the call's largest edge count (chain_cap), R = chain_rows(K, E).  n_edges = 0: no chain.
inline int32_t chain_rows(int32_t K, int32_t cap) { return std::min(K, cap + 1); }
inline int64_t chain_int_words(int32_t K, int32_t cap) { return corpus_chain_int_words(K, cap); }
inline int64_t chain_flt_words(int32_t cap) { return 4 * (int64_t)cap; }
inline int64_t chain_nodes_at() { return 2; }
inline int64_t chain_rows_at(int32_t cap) { return 2 + (int64_t)cap + 1; }
inline int64_t chain_ptr_at(int32_t K, int32_t cap) { return chain_rows_at(cap) + chain_rows(K, cap); }
inline int64_t chain_col_at(int32_t K, int32_t cap) { return chain_ptr_at(K, cap) + chain_rows(K, cap) + 1; }

// fills one query's records (zeroed by the caller); len = 0: no chain
inline void pack_chain(const int32_t* nodes, const float* weights, int32_t len, int32_t K, int32_t cap, int32_t* ints,
                       float* flts) {
  if (len < 2) return;
  const ChainPath p = build_chain_path(nodes, weights, len, K);
  ints[0] = len - 1;
  ints[1] = (int32_t)p.rows.size();
  std::copy(nodes, nodes + len, ints + chain_nodes_at());
  std::copy(p.rows.begin(), p.rows.end(), ints + chain_rows_at(cap));
  std::copy(p.ptr.begin(), p.ptr.end(), ints + chain_ptr_at(K, cap));
  std::copy(p.col.begin(), p.col.end(), ints + chain_col_at(K, cap));
  std::copy(p.a.begin(), p.a.end(), flts);
  std::copy(p.w.begin(), p.w.end(), flts + 2 * (int64_t)cap);
}

}  // namespace host
}  // namespace osc

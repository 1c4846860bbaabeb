// The host side of osc_chain_receipt_many: the checks on the caller's chains, where a query's
// edges land in the flat outputs, and one chunk's work units -- a (query, chain edge) pair each, with the range of its
// row's path entries -- over the path structures host::build_chain_path packs (corpus_chain.hpp).  HIP-free: osc_query.hip
// runs it, tests/host_logic/sweep_chain_many.cpp sweeps it under the sanitizers.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <vector>

#include "corpus_chain.hpp"

namespace osc {
namespace host {

// chain_offsets holds Q + 1 node offsets from 0; query q has len_q = off[q + 1] - off[q] nodes and len_q - 1 edges, so its
// edge t lands at off[q] - q + t of the flat per-edge outputs
inline int64_t chain_many_edge_at(const int64_t* off, int64_t q) { return off[q] - q; }

// 0, or what is wrong with the caller's chains: 1 the offsets (not from 0 / a chain outside 2..kCorpusMaxChain nodes),
// 2 a node outside [0, N).  *where receives the query.
inline int chain_many_check(const int64_t* off, const int32_t* nodes, int32_t Q, int64_t N, int32_t* where) {
  *where = 0;
  if (Q > 0 && off[0] != 0) return 1;
  for (int32_t q = 0; q < Q; ++q) {
    *where = q;
    const int64_t len = off[q + 1] - off[q];
    if (len < 2 || len > kCorpusMaxChain) return 1;
    for (int64_t t = off[q]; t < off[q + 1]; ++t)
      if (nodes[t] < 0 || (int64_t)nodes[t] >= N) return 2;
  }
  return 0;
}

// one (query, chain edge) pair in device rows; [pb, pe) are row i's path entries in the chunk's pcol / pa
struct ChainManyUnit {
  int32_t q;  // query of the chunk
  int32_t i, j;
  int32_t pb, pe;
};

// the path structures a chunk's units point into, one per distinct chain, entries back to back
struct ChainManyPaths {
  std::vector<ChainPath> paths;
  std::vector<int32_t> base;  // first entry of path p in pcol / pa
  std::vector<int32_t> pcol;  // device rows
  std::vector<float> pa;      // A_path
  std::map<std::vector<int32_t>, int32_t> seen;

  void clear() {
    paths.clear();
    base.clear();
    pcol.clear();
    pa.clear();
    seen.clear();
  }
  // the path of these nodes (device rows; weights or nullptr for ones), packed on first sight
  int32_t add(const int32_t* nodes, const float* weights, int32_t len, int32_t N) {
    std::vector<int32_t> key(nodes, nodes + len);
    auto it = seen.find(key);
    if (it != seen.end()) return it->second;
    const int32_t id = (int32_t)paths.size();
    paths.push_back(build_chain_path(nodes, weights, len, N));
    base.push_back((int32_t)pcol.size());
    pcol.insert(pcol.end(), paths.back().col.begin(), paths.back().col.end());
    pa.insert(pa.end(), paths.back().a.begin(), paths.back().a.end());
    seen.emplace(std::move(key), id);
    return id;
  }
  // ... with weights in the key as well (osc_chain_prior_many): a chain is the same path only with the same weights.  The
  // weighted key is the nodes, -1, then the weights' bits; without weights it is add's own.
  int32_t add_weighted(const int32_t* nodes, const float* weights, int32_t len, int32_t N) {
    if (!weights) return add(nodes, nullptr, len, N);
    std::vector<int32_t> key(nodes, nodes + len);
    key.push_back(-1);
    for (int32_t t = 0; t + 1 < len; ++t) {
      int32_t bits;
      static_assert(sizeof bits == sizeof weights[t], "float is 32 bits");
      std::memcpy(&bits, weights + t, sizeof bits);
      key.push_back(bits);
    }
    auto it = seen.find(key);
    if (it != seen.end()) return it->second;
    const int32_t id = (int32_t)paths.size();
    paths.push_back(build_chain_path(nodes, weights, len, N));
    base.push_back((int32_t)pcol.size());
    pcol.insert(pcol.end(), paths.back().col.begin(), paths.back().col.end());
    pa.insert(pa.end(), paths.back().a.begin(), paths.back().a.end());
    seen.emplace(std::move(key), id);
    return id;
  }
  // row's entries of path id: [*pb, *pe), empty when the row owns none
  void range(int32_t id, int32_t row, int32_t* pb, int32_t* pe) const {
    const ChainPath& p = paths[(size_t)id];
    const auto it = std::lower_bound(p.rows.begin(), p.rows.end(), row);
    if (it == p.rows.end() || *it != row) {
      *pb = *pe = 0;
      return;
    }
    const size_t t = (size_t)(it - p.rows.begin());
    *pb = base[(size_t)id] + p.ptr[t];
    *pe = base[(size_t)id] + p.ptr[t + 1];
  }
};

// The units of queries [c0, c0 + nq) in (query, edge) order and eoff[nq + 1], each query's first unit.  dev maps an API id
// to its device row (nullptr = identity).  own >= 0: every unit reads that path of `paths` (the lattice's own chain);
// own < 0: each query's chain is packed into `paths` (once per distinct chain) and read as its own path.
inline void chain_many_units(const int64_t* off, const int32_t* nodes, int32_t c0, int32_t nq, const int32_t* dev, int32_t N,
                             int32_t own, ChainManyPaths& paths, std::vector<ChainManyUnit>& units,
                             std::vector<int32_t>& eoff) {
  units.clear();
  eoff.assign((size_t)nq + 1, 0);
  std::vector<int32_t> rows;
  for (int32_t t = 0; t < nq; ++t) {
    const int64_t b = off[c0 + t];
    const int32_t len = (int32_t)(off[c0 + t + 1] - b);
    rows.resize((size_t)len);
    for (int32_t s = 0; s < len; ++s) rows[(size_t)s] = dev ? dev[nodes[b + s]] : nodes[b + s];
    const int32_t id = own >= 0 ? own : paths.add(rows.data(), nullptr, len, N);
    for (int32_t s = 0; s + 1 < len; ++s) {
      ChainManyUnit u{t, rows[(size_t)s], rows[(size_t)s + 1], 0, 0};
      paths.range(id, u.i, &u.pb, &u.pe);
      units.push_back(u);
    }
    eoff[(size_t)t + 1] = (int32_t)units.size();
  }
}

// chain_many_units for chains with weights of their own (osc_chain_prior_many): weights is flat over the chains' edges like
// the per-edge outputs (query q's at chain_many_edge_at(off, q)), or nullptr for ones.  Every query's chain is packed once per
// distinct (chain, weights); path_of[t] receives the path of the chunk's query t.
inline void chain_many_units_weighted(const int64_t* off, const int32_t* nodes, const float* weights, int32_t c0, int32_t nq,
                                      const int32_t* dev, int32_t N, ChainManyPaths& paths, std::vector<ChainManyUnit>& units,
                                      std::vector<int32_t>& eoff, std::vector<int32_t>& path_of) {
  units.clear();
  eoff.assign((size_t)nq + 1, 0);
  path_of.assign((size_t)nq, 0);
  std::vector<int32_t> rows;
  for (int32_t t = 0; t < nq; ++t) {
    const int64_t b = off[c0 + t];
    const int32_t len = (int32_t)(off[c0 + t + 1] - b);
    rows.resize((size_t)len);
    for (int32_t s = 0; s < len; ++s) rows[(size_t)s] = dev ? dev[nodes[b + s]] : nodes[b + s];
    const int32_t id = paths.add_weighted(rows.data(), weights ? weights + chain_many_edge_at(off, c0 + t) : nullptr, len, N);
    path_of[(size_t)t] = id;
    for (int32_t s = 0; s + 1 < len; ++s) {
      ChainManyUnit u{t, rows[(size_t)s], rows[(size_t)s + 1], 0, 0};
      paths.range(id, u.i, &u.pb, &u.pe);
      units.push_back(u);
    }
    eoff[(size_t)t + 1] = (int32_t)units.size();
  }
}

}  // namespace host
}  // namespace osc

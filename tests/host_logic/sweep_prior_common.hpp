// What the sweeps of chain_prior_plan.hpp, bundle_prior_plan.hpp and receipt_prior_plan.hpp share: the chains they draw, the
// walk over a layout's blocks and the checks that pin chain_prior_pack's passes.  Each sweep stays a program of its own.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#include "../../oscillink_amd/csrc/chain_prior_plan.hpp"

using namespace osc::host;

static int fail(const char* what, long long a, long long b) {
  std::printf("ERROR %s (%lld, %lld)\n", what, a, b);
  return 1;
}

struct Block {
  long long at, bytes;
};

// the blocks in order: 256-byte aligned, pairwise disjoint, not empty, inside `total`
static int check_blocks(const std::vector<Block>& b, long long total) {
  long long end = 0;
  for (size_t i = 0; i < b.size(); ++i) {
    if (b[i].at % 256 != 0) return fail("alignment", (long long)i, b[i].at);
    if (b[i].at < end) return fail("blocks overlap", (long long)i, b[i].at);
    if (b[i].bytes <= 0) return fail("empty block", (long long)i, b[i].bytes);
    end = b[i].at + b[i].bytes;
  }
  if (end > total) return fail("block passes total", end, total);
  return 0;
}

static unsigned long long rng_state = 88172645463325252ULL;
static unsigned rnd(unsigned n) {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (unsigned)(rng_state % n);
}

// Q chains on N rows, one per query or the first `shared` by all: m > 0 a run of m distinct nodes closed on its first, m == 0
// 2..9 drawn nodes with a revisit
static void make_chains(long long N, int Q, bool shared, int m, std::vector<int64_t>& off, std::vector<int>& nodes) {
  off.assign(1, 0);
  nodes.clear();
  std::vector<int> ch;
  for (int q = 0; q < Q; ++q) {
    if (!shared || q == 0) {
      ch.clear();
      if (m == 0) {
        const int len = 2 + (int)rnd(8);
        for (int t = 0; t < len; ++t) ch.push_back((int)rnd((unsigned)std::min<long long>(N, 1 << 30)));
        if (len > 3) ch[3] = ch[1];  // a revisit
      } else {
        const long long mm = std::min<long long>(N, m);
        const long long start = N > mm ? rnd((unsigned)(N - mm)) : 0;
        for (long long t = 0; t < mm; ++t) ch.push_back((int)(start + t));
        ch.push_back(ch[0]);
      }
    }
    nodes.insert(nodes.end(), ch.begin(), ch.end());
    off.push_back((int64_t)nodes.size());
  }
}

static std::set<int> query_nodes(const std::vector<int64_t>& off, const std::vector<int>& nodes, int q) {
  return std::set<int>(nodes.begin() + off[(size_t)q], nodes.begin() + off[(size_t)q + 1]);
}

// The passes of chain_prior_pack over the chains (off, nodes), from the chains alone.  over(qc, msum, msq, nq): a pass of that
// shape is beyond the caller's budget.  The passes tile [0, Q) in order; no query is split -- every distinct node of a query
// is a column of its pass, once, in first-seen order with each query's nodes ascending; msum, msq and mmax are the sum of the
// queries' distinct node counts, of their squares and the largest; a pass of more than one query is within the budget, the
// chunk and the column limit; and every pass but the last is greedy: its successor's first query did not fit.
template <class Over>
static int check_packing(const std::vector<ChainPriorPass>& ps, const std::vector<int64_t>& off, const std::vector<int>& nodes,
                         int Q, int max_queries, int max_cols, Over over) {
  const int chunk = std::max(max_queries, 1);
  int next = 0;
  for (size_t i = 0; i < ps.size(); ++i) {
    const ChainPriorPass& p = ps[i];
    if (p.q0 != next || p.nq < 1) return fail("passes do not tile the queries", p.q0, next);
    next = p.q0 + p.nq;
    if (p.nq > chunk) return fail("pass over the chunk", p.nq, max_queries);
    const std::set<int> cols(p.cols.begin(), p.cols.end());
    if (cols.size() != p.cols.size()) return fail("a node is two columns of one pass", (long long)cols.size(), (long long)p.cols.size());
    if (p.qc % kGatesSlab != 0 || p.qc < (int)p.cols.size() || p.qc >= (int)p.cols.size() + kGatesSlab) return fail("panel width", p.qc, (long long)p.cols.size());
    std::set<int> want;
    std::vector<int> order;
    long long msum = 0, msq = 0, mmax = 0;
    for (int q = p.q0; q < p.q0 + p.nq; ++q) {
      const std::set<int> mine = query_nodes(off, nodes, q);
      if (mine.size() < 1 || mine.size() > 64) return fail("a query's distinct nodes", q, (long long)mine.size());
      msum += (long long)mine.size();
      msq += (long long)(mine.size() * mine.size());
      mmax = std::max<long long>(mmax, (long long)mine.size());
      for (int v : mine)
        if (want.insert(v).second) order.push_back(v);
    }
    if (want != cols) return fail("a pass's columns are not its queries' nodes: a query was split", (long long)want.size(), (long long)cols.size());
    if (order != p.cols) return fail("columns are not in first-seen order", p.q0, p.nq);
    if (msum != p.msum || msq != p.msq || mmax != p.mmax) return fail("msum / msq / mmax", msum, p.msum);
    if (p.nq > 1) {
      if (over(p.qc, msum, msq, p.nq)) return fail("pass over budget", p.q0, p.qc);
      if (max_cols > 0 && (int)p.cols.size() > max_cols) return fail("pass over the column limit", (long long)p.cols.size(), max_cols);
    }
    if (i + 1 < ps.size()) {  // greedy: the next query was refused by the chunk, the column limit or the budget
      const std::set<int> mine = query_nodes(off, nodes, next);
      long long width = (long long)cols.size();
      for (int v : mine) width += cols.count(v) ? 0 : 1;
      const long long m = (long long)mine.size();
      const bool refused = p.nq >= chunk || (max_cols > 0 && width > max_cols) ||
                           over((int)((width + kGatesSlab - 1) / kGatesSlab * kGatesSlab), msum + m, msq + m * m, p.nq + 1);
      if (!refused) return fail("a pass closed before a query that fits", p.q0, p.nq);
    }
  }
  if (next != Q) return fail("passes end early", next, Q);
  return 0;
}

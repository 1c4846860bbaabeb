// Sweep of chain_gated_plan.hpp (osc_chain_gated_many) over N from 1 to 1 000 000, D from 1 to 1536,
// with and without the settle's panel, light and full detail, chain lengths from 2 to 1024, requested chunks from 0 to 10 000
// and budgets from 1 GiB down to one byte: the chunk is in [1, 256], at most the request and at most
// receipt_gated_plan.hpp's, fits the budget unless it is the floor of one query, and is not lowered further than the budget
// asks; the chain arrays are 256-byte aligned, pairwise disjoint, behind receipt_gated_plan.hpp's block (which is the layout's
// own, unchanged) and inside `total`, each large enough for the worst chunk -- every query a path of its own with the most
// rows and entries a chain of that length can have; a narrower chunk fits the block allocated for the widest.  The fix
// units of a path tile its rows, in order, kChainFixRows at most each, and are a function of the path's row count alone: the
// same chain packed into chunks of different composition is cut the same way.  The driver then packs real chains
// (ChainManyPaths, chain_gated_pack) and walks a real block the way the kernels index it, so the sanitizers see the
// indexing.  Run under -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../oscillink_amd/csrc/chain_gated_plan.hpp"

using namespace osc::host;

static int fail(const char* what, long long a, long long b) {
  std::printf("ERROR %s (%lld, %lld)\n", what, a, b);
  return 1;
}

struct Block {
  long long at, bytes;
};

static int check_layout(long long N, int D, int nq, bool settle, bool full, int len) {
  const ChainGatedLayout L = chain_gated_layout(N, D, nq, settle, full, len);
  const ReceiptGatedLayout R = receipt_gated_layout(N, D, nq, settle, full);
  if (L.rg.total != R.total || L.rg.panel.X != R.panel.X || L.rg.dh != R.dh || L.rg.sums != R.sums || L.rg.U != R.U)
    return fail("receipt block differs", N, nq);
  const long long rows = (long long)nq * chain_gated_rows_max(len, N), entries = (long long)nq * chain_gated_entries_max(len);
  if (chain_gated_rows_max(len, N) > N || chain_gated_rows_max(len, N) > len) return fail("rows bound", N, len);
  if (L.max_units < 1 || (long long)L.max_units * kChainFixRows < chain_gated_rows_max(len, N)) return fail("max units", N, len);
  const long long slabs = (long long)nq * gated_slabs_per_query(D);
  const Block b[] = {{L.prow, rows * 4}, {L.pbeg, rows * 4}, {L.pend, rows * 4}, {L.pw, entries * 4},
                     {L.q_row0, nq * 4LL}, {L.q_rows, nq * 4LL}, {L.cpart, slabs * L.max_units * 32 * 8}};
  long long end = R.total;
  for (size_t i = 0; i < sizeof b / sizeof b[0]; ++i) {
    if (b[i].at % 256 != 0) return fail("alignment", (long long)i, b[i].at);
    if (b[i].at < end) return fail("blocks overlap", (long long)i, b[i].at);  // (the blocks are laid out in this order)
    if (b[i].bytes <= 0) return fail("empty block", (long long)i, b[i].bytes);
    end = b[i].at + b[i].bytes;
  }
  if (end > L.total) return fail("block passes total", end, L.total);
  return 0;
}

// the units of a path of `rows` rows tile [0, rows) in order
static int check_units(int rows) {
  const int nu = chain_fix_units(rows);
  int next = 0;
  for (int u = 0; u < nu; ++u) {
    const int b = chain_fix_begin(u), e = chain_fix_end(rows, u);
    if (b != next || e <= b || e - b > kChainFixRows) return fail("unit range", rows, u);
    next = e;
  }
  if (next != rows) return fail("units do not end at the last row", next, rows);
  if (chain_fix_end(rows, nu) > rows || chain_fix_begin(nu) < rows) return fail("a unit past the last", rows, nu);
  return 0;
}

int main() {
  const long long Ns[] = {1, 2, 33, 97, 4096, 65537, 1000000};
  const int Ds[] = {1, 32, 33, 768, 1536};
  const int lens[] = {2, 3, 128, 129, 257, 1024};
  const int reqs[] = {-3, 0, 1, 2, 255, 256, 10000};
  const long long budgets[] = {kGatedBudgetBytes, (long long)1 << 28, (long long)1 << 24, (long long)1 << 16, 4096, 1};
  long long cases = 0;
  for (int rows = 0; rows <= 1024; ++rows)
    if (check_units(rows)) return 1;
  for (long long N : Ns)
    for (int D : Ds)
      for (int len : lens)
        for (int mode = 0; mode < 4; ++mode) {
          const bool settle = mode & 1, full = mode & 2;
          for (int req : reqs)
            for (long long budget : budgets) {
              const int chunk = chain_gated_chunk(N, D, settle, full, len, req, budget);
              const int want = std::min(std::max(req, 1), kGatedMaxChunk);
              if (chunk < 1 || chunk > kGatedMaxChunk) return fail("chunk range", chunk, req);
              if (chunk > want) return fail("chunk above the request", chunk, req);
              if (chunk > receipt_gated_chunk(N, D, settle, full, req, budget)) return fail("chunk above the receipts'", chunk, req);
              const long long total = chain_gated_layout(N, D, chunk, settle, full, len).total;
              if (chunk > 1 && total > budget) return fail("budget", chunk, total);
              if (chunk < want && chain_gated_layout(N, D, chunk + 1, settle, full, len).total <= budget)
                return fail("chunk lowered further than the budget asks", chunk, req);
              for (int nq : {1, chunk / 2 + 1, chunk})
                if (chain_gated_layout(N, D, nq, settle, full, len).total > total) return fail("narrow chunk larger", nq, chunk);
              if (check_layout(N, D, chunk, settle, full, len)) return 1;
              if (check_layout(N, D, 1, settle, full, len)) return 1;
              ++cases;
            }
        }
  // real chains through the pack and a real block, as the kernels index them
  for (long long N : {2LL, 33LL, 97LL, 1500LL})
    for (int D : {1, 33, 40})
      for (int len : {2, 7, 300, 1024}) {
        // chains over the rows in steps of 7 with revisits: one shared by two queries, one with weights, a self-step
        std::vector<int> a((size_t)len), b((size_t)len), c = {(int)(N - 1), (int)(N - 1)};
        std::vector<float> wb((size_t)len - 1);
        for (int t = 0; t < len; ++t) {
          a[(size_t)t] = (int)((7LL * t) % N);
          b[(size_t)t] = (int)((11LL * t + 3) % N);
          if (t + 1 < len) wb[(size_t)t] = (float)((t % 5) - 1);  // (a weight below zero and a zero among them)
        }
        const std::vector<std::vector<int>> chains = {a, b, a, c};
        std::vector<long long> off = {0};
        std::vector<int> nodes;
        std::vector<float> weights;
        for (size_t q = 0; q < chains.size(); ++q) {
          nodes.insert(nodes.end(), chains[q].begin(), chains[q].end());
          off.push_back((long long)nodes.size());
          for (size_t t = 0; t + 1 < chains[q].size(); ++t) weights.push_back(q == 1 ? wb[t] : 1.0f);
        }
        const int Q = (int)chains.size();
        std::vector<int64_t> off64(off.begin(), off.end());
        const int max_len = chain_gated_max_len(off64.data(), Q);
        if (max_len != std::max(len, 2)) return fail("max len", max_len, len);
        std::vector<std::vector<int>> cuts;  // per query, its units' first rows (device rows), from whichever chunk held it
        for (int chunk : {4, 1, 3}) {
          for (int q0 = 0; q0 < Q; q0 += chunk) {
            const int nq = std::min(chunk, Q - q0);
            const ChainGatedLayout L = chain_gated_layout(N, D, nq, true, true, max_len);
            std::vector<unsigned char> block((size_t)L.total, 0);
            ChainManyPaths paths;
            std::vector<ChainManyUnit> units;
            std::vector<int32_t> eoff, path_of;
            chain_many_units_weighted(off64.data(), nodes.data(), weights.data(), q0, nq, nullptr, (int32_t)N, paths, units, eoff,
                                      path_of);
            ChainGatedPack k;
            chain_gated_pack(paths, path_of, k);
            if (k.max_units > L.max_units) return fail("pack units pass the layout's", k.max_units, L.max_units);
            if ((long long)k.prow.size() * 4 > L.pbeg - L.prow || (long long)k.pw.size() * 4 > L.q_row0 - L.pw)
              return fail("pack passes the layout", (long long)k.prow.size(), (long long)k.pw.size());
            if (k.pw.size() != paths.pcol.size() || k.prow.size() != k.pbeg.size()) return fail("pack sizes", 0, 0);
            std::memcpy(block.data() + L.prow, k.prow.data(), k.prow.size() * 4);
            std::memcpy(block.data() + L.pbeg, k.pbeg.data(), k.pbeg.size() * 4);
            std::memcpy(block.data() + L.pend, k.pend.data(), k.pend.size() * 4);
            std::memcpy(block.data() + L.pw, k.pw.data(), k.pw.size() * 4);
            std::memcpy(block.data() + L.q_row0, k.q_row0.data(), k.q_row0.size() * 4);
            std::memcpy(block.data() + L.q_rows, k.q_rows.data(), k.q_rows.size() * 4);
            const int32_t* prow = reinterpret_cast<const int32_t*>(block.data() + L.prow);
            const int32_t* pbeg = reinterpret_cast<const int32_t*>(block.data() + L.pbeg);
            const int32_t* pend = reinterpret_cast<const int32_t*>(block.data() + L.pend);
            const float* pw = reinterpret_cast<const float*>(block.data() + L.pw);
            const int32_t* q_row0 = reinterpret_cast<const int32_t*>(block.data() + L.q_row0);
            const int32_t* q_rows = reinterpret_cast<const int32_t*>(block.data() + L.q_rows);
            double* cpart = reinterpret_cast<double*>(block.data() + L.cpart);
            const int spq = gated_slabs_per_query(D);
            for (int t = 0; t < nq; ++t) {
              std::vector<int> cut;
              int last_row = -1;
              for (int u = 0; u < L.max_units; ++u) {  // the grid's units, the empty ones past the query's own included
                const int rb = chain_fix_begin(u), re = chain_fix_end(q_rows[t], u);
                for (int r = rb; r < re; ++r) {
                  const int pr = q_row0[t] + r;
                  if (prow[pr] <= last_row || prow[pr] >= N) return fail("path rows not ascending inside N", pr, prow[pr]);
                  last_row = prow[pr];
                  if (r == rb) cut.push_back(prow[pr]);
                  if (pbeg[pr] >= pend[pr]) return fail("a path row without entries", pr, pbeg[pr]);
                  for (int e = pbeg[pr]; e < pend[pr]; ++e) {
                    if (paths.pcol[(size_t)e] < 0 || paths.pcol[(size_t)e] >= N) return fail("column", e, paths.pcol[(size_t)e]);
                    if (!(pw[e] >= 0.f)) return fail("weight", e, 0);
                  }
                }
                for (int s = 0; s < spq; ++s)
                  for (int col = 0; col < 32; ++col) cpart[((size_t)(t * spq + s) * L.max_units + u) * 32 + col] += 1.0;
              }
              if ((int)cut.size() != chain_fix_units(q_rows[t])) return fail("units of the query", (long long)cut.size(), q_rows[t]);
              const size_t q = (size_t)(q0 + t);
              if (cuts.size() <= q) cuts.resize(q + 1);
              if (cuts[q].empty()) cuts[q] = cut;
              else if (cuts[q] != cut) return fail("a chain's units differ between chunks", (long long)q, chunk);
            }
            ++cases;
          }
        }
        if (cuts[0] != cuts[2]) return fail("the same chain cut differently", 0, 2);
        if (len > kChainFixRows && N > kChainFixRows && cuts[0].size() < 2) return fail("a long chain in one unit", len, N);
      }
  std::printf("chain gated plan sweep ok (%lld cases)\n", cases);
  return 0;
}

// Sweep of corpus_chain.hpp (the chain prior of one candidate lattice as a compact path structure) and of the chain blocks of
// corpus_plan.hpp.  Every chain is checked against a dense restatement of build_path_laplacian + normalized_laplacian
// (graph.py:96-111, 86-93): random chains, repeated nodes, self-steps, weights of 0 and below, chain length 2 and 1024,
// K = 2 and 1024.  pack_chain writes into buffers of exactly chain_int_words / chain_flt_words, so a record that outgrows
// its slot is an AddressSanitizer report.  Layouts: without chains every offset and the chunk are EQUAL to what the older
// calls give; with chains every older block is where it was and the new blocks are aligned, in order, disjoint, large enough
// and inside total.  Run under -fsanitize=address,undefined.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../oscillink_amd/csrc/corpus_chain.hpp"

using namespace osc::host;

static int fail(const char* what, long long a, long long b) {
  std::printf("ERROR %s (%lld, %lld)\n", what, a, b);
  return 1;
}

static int check_chain(const std::vector<int32_t>& nodes, const std::vector<float>* weights, int K) {
  const int len = (int)nodes.size();
  // dense restatement
  std::vector<float> A((size_t)K * K, 0.f), d((size_t)K, 0.f), sd((size_t)K);
  for (int t = 0; t + 1 < len; ++t) {
    const int i = nodes[t], j = nodes[t + 1];
    const float w = weights ? (*weights)[t] : 1.0f;
    A[(size_t)i * K + j] = std::max(A[(size_t)i * K + j], w);
    A[(size_t)j * K + i] = std::max(A[(size_t)j * K + i], w);
  }
  for (int r = 0; r < K; ++r) {
    for (int c = 0; c < K; ++c) d[r] += A[(size_t)r * K + c];
    sd[r] = std::sqrt(std::max(d[r], 1e-12f));
  }
  const ChainPath p = build_chain_path(nodes.data(), weights ? weights->data() : nullptr, len, K);
  const int R = (int)p.rows.size();
  if ((int)p.ptr.size() != R + 1 || p.ptr[0] != 0 || p.ptr[R] != (int)p.col.size()) return fail("ptr ends", R, len);
  if (p.a.size() != p.col.size() || p.w.size() != p.col.size()) return fail("entry arrays", R, len);
  if (R > std::min(K, len) || (int)p.col.size() > 2 * (len - 1)) return fail("more rows or entries than the chain allows", R, len);
  long long listed_nonzero = 0, dense_nonzero = 0;
  for (float v : A) dense_nonzero += v != 0.f;
  for (int t = 0; t < R; ++t) {
    const int r = p.rows[t];
    if (r < 0 || r >= K || (t && p.rows[t - 1] >= r)) return fail("rows not ascending", t, r);
    if (p.ptr[t] >= p.ptr[t + 1]) return fail("empty path row", t, r);
    for (int e = p.ptr[t]; e < p.ptr[t + 1]; ++e) {
      const int c = p.col[e];
      if (c < 0 || c >= K || (e > p.ptr[t] && p.col[e - 1] >= c)) return fail("columns not ascending", r, c);
      if (std::memcmp(&p.a[e], &A[(size_t)r * K + c], 4) != 0) return fail("A_path entry", r, c);
      const float w = (A[(size_t)r * K + c] * (1.0f / sd[r])) * (1.0f / sd[c]);
      if (std::memcmp(&p.w[e], &w, 4) != 0) return fail("W_path entry", r, c);
      listed_nonzero += p.a[e] != 0.f;
    }
  }
  if (listed_nonzero != dense_nonzero) return fail("a dense entry is not listed", listed_nonzero, dense_nonzero);
  // the packed record, in buffers of exactly its size
  for (int cap : {len - 1, len + 5, 1023}) {
    if (cap < len - 1) continue;
    std::vector<int32_t> ints((size_t)chain_int_words(K, cap), 0);
    std::vector<float> flts((size_t)chain_flt_words(cap), 0.f);
    pack_chain(nodes.data(), weights ? weights->data() : nullptr, len, K, cap, ints.data(), flts.data());
    if (ints[0] != len - 1 || ints[1] != R) return fail("record header", ints[0], ints[1]);
    if (chain_col_at(K, cap) + 2LL * cap != chain_int_words(K, cap)) return fail("record size", K, cap);
    if (std::memcmp(ints.data() + chain_nodes_at(), nodes.data(), (size_t)len * 4) != 0) return fail("record nodes", K, cap);
    if (R && std::memcmp(ints.data() + chain_rows_at(cap), p.rows.data(), (size_t)R * 4) != 0) return fail("record rows", K, cap);
    if (std::memcmp(ints.data() + chain_ptr_at(K, cap), p.ptr.data(), (size_t)(R + 1) * 4) != 0) return fail("record ptr", K, cap);
    if (std::memcmp(ints.data() + chain_col_at(K, cap), p.col.data(), p.col.size() * 4) != 0) return fail("record col", K, cap);
    if (std::memcmp(flts.data(), p.a.data(), p.a.size() * 4) != 0) return fail("record a", K, cap);
    if (std::memcmp(flts.data() + 2 * (size_t)cap, p.w.data(), p.w.size() * 4) != 0) return fail("record w", K, cap);
  }
  return 0;
}

static int sweep_chains(long long* cases) {
  std::mt19937 rng(12345);
  for (int K : {2, 3, 7, 100, 1024})
    for (int len : {2, 3, 8, 57, 1024})
      for (int mode = 0; mode < 5; ++mode) {
        std::vector<int32_t> nodes((size_t)len);
        std::vector<float> w((size_t)len - 1);
        const int span = mode == 1 ? std::min(K, 3) : K;  // mode 1: few nodes, many repeats and revisited edges
        for (int t = 0; t < len; ++t) nodes[t] = (int32_t)(rng() % span);
        if (mode == 2)  // self-steps
          for (int t = 1; t < len; t += 2) nodes[t] = nodes[t - 1];
        if (mode == 3)  // a simple path where K allows
          for (int t = 0; t < len; ++t) nodes[t] = t % K;
        for (int t = 0; t + 1 < len; ++t) {
          const unsigned r = rng() % 8;
          w[t] = r == 0 ? 0.f : (r == 1 ? -0.5f : 0.1f + 0.01f * (float)(rng() % 300));
        }
        if (check_chain(nodes, mode == 4 ? nullptr : &w, K)) return fail("chain case", K, len);
        ++*cases;
      }
  // no chain: the records stay zero
  std::vector<int32_t> ints((size_t)chain_int_words(7, 4), 0);
  std::vector<float> flts((size_t)chain_flt_words(4), 0.f);
  pack_chain(nullptr, nullptr, 0, 7, 4, ints.data(), flts.data());
  for (int32_t v : ints)
    if (v != 0) return fail("record of a lattice without a chain", v, 0);
  return 0;
}

static int sweep_layouts(long long* cases) {
  const long long Ns[] = {1, 7, 1000, 1000000};
  const int Ds[] = {1, 128, 1536};
  const int Ks[] = {1, 2, 7, 100, 1024};
  for (long long N : Ns)
    for (int D : Ds)
      for (int Kr : Ks)
        for (int req : {1, 64, 256, 100000})
          for (int rec = 0; rec < 2; ++rec) {
            const int K = (int)std::min<long long>(Kr, N), knn = K > 1 ? corpus_knn(6, K) : 0, k = std::max(1, knn);
            const int kk = std::max(1, std::min(8, K)), ldn = corpus_ldn(D), slots = rec ? K : 0;
            const int nq0 = corpus_chunk(N, ldn, K, k, kk, req, kCorpusBudgetBytes, rec != 0, slots);
            if (corpus_chunk(N, ldn, K, k, kk, req, kCorpusBudgetBytes, rec != 0, slots, 0) != nq0) return fail("chunk moved", nq0, 0);
            const CorpusLayout L0 = corpus_layout(N, ldn, K, k, kk, nq0, rec != 0, slots);
            const CorpusLayout Lz = corpus_layout(N, ldn, K, k, kk, nq0, rec != 0, slots, 0);
            if (std::memcmp(&Lz, &L0, sizeof L0) != 0) return fail("layout moved without chains", nq0, rec);
            if (L0.c_int || L0.c_flt || L0.c_edge || L0.c_gain || L0.c_verdict || L0.c_weak_k || L0.c_weak_z)
              return fail("chain offsets set without chains", L0.c_int, L0.c_edge);
            for (int cap : {1, 7, 1023}) {
              const int nq = corpus_chunk(N, ldn, K, k, kk, req, kCorpusBudgetBytes, rec != 0, slots, cap);
              if (nq < 1 || nq > nq0) return fail("chunk range", nq, nq0);
              const CorpusLayout L = corpus_layout(N, ldn, K, k, kk, nq, rec != 0, slots, cap);
              if (nq > 1 && L.total > kCorpusBudgetBytes) return fail("budget", nq, L.total);
              CorpusLayout B = corpus_layout(N, ldn, K, k, kk, nq, rec != 0, slots);
              const long long old_end = B.total;
              B.total = L.total;
              if (std::memcmp(&L, &B, offsetof(CorpusLayout, c_int)) != 0) return fail("an older block moved", nq, cap);
              const long long iw = chain_int_words(K, cap);
              if (iw != corpus_chain_int_words(K, cap) || iw < 2 + (cap + 1) + 2 * chain_rows(K, cap) + 1 + 2 * cap)
                return fail("int record words", iw, cap);
              const long long off[] = {L.c_int, L.c_flt, L.c_edge, L.c_gain, L.c_verdict, L.c_weak_k, L.c_weak_z, L.total};
              const long long need[] = {nq * iw * 4, nq * 16LL * cap, nq * 16LL * cap, nq * 8LL, nq * 4LL, nq * 4LL, nq * 4LL};
              if (off[0] != old_end) return fail("chain blocks do not follow the older ones", off[0], old_end);
              for (int i = 0; i < 7; ++i) {
                if (off[i] % 256 != 0) return fail("alignment", i, off[i]);
                if (off[i] + need[i] > off[i + 1]) return fail("block overlaps its successor", i, off[i]);
              }
              // growth per query: the two records, the edge outputs and 20 bytes of scalars, plus padding
              if (L.total - old_end > nq * (iw * 4 + 32LL * cap + 20) + 7 * 256) return fail("growth", L.total - old_end, nq);
              ++*cases;
            }
          }
  return 0;
}

int main() {
  long long chains = 0, layouts = 0;
  if (sweep_chains(&chains) || sweep_layouts(&layouts)) return 1;
  std::printf("corpus chain sweep ok (%lld chains, %lld layouts)\n", chains, layouts);
  return 0;
}

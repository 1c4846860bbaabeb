// Sweep of gates_many_plan.hpp (osc_gates_many) for N from 1 to 2 000 000 and Q from 1 to 1000: the
// chunks tile [0, Q); a chunk's width is a multiple of 32 in [32, 256] that fits the budget unless it is the floor of 32;
// the arrays of a panel are 256-byte aligned, pairwise disjoint and inside the block, each large enough for what the
// kernels index; the row partition covers [0, N) in whole 32-row steps, stays within the part limit, and -- like the
// length of the partials -- is the same for every width (the functions are called beside every width and compared).
// The driver walks a real scratch block of a small case the way the kernels do, so the sanitizers see the indexing.
// Run under -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../oscillink_amd/csrc/gates_many_plan.hpp"

using namespace osc::host;

static int fail(const char* what, long long a, long long b) {
  std::printf("ERROR %s (%lld, %lld)\n", what, a, b);
  return 1;
}

struct Block {
  long long at, bytes;
};

static int check_layout(long long N, int D, int qc) {
  const long long btn = gates_bt_floats(qc, D);
  const GatesLayout L = gates_layout(N, qc, btn);
  const long long slabs = qc / kGatesSlab, parts = gates_parts(N), panel = N * (long long)qc * 4;
  const Block b[] = {{L.X, panel},       {L.R, panel},        {L.P, panel},
                     {L.AP, panel},      {L.out, panel},      {L.Bt, btn * 4},
                     {L.part_a, slabs * parts * 32 * 8},      {L.part_b, slabs * parts * 32 * 8},
                     {L.rz, qc * 8LL},   {L.tol, qc * 4LL},   {L.alpha, qc * 4LL},
                     {L.beta, qc * 4LL}, {L.res, qc * 4LL},   {L.lo, qc * 4LL},
                     {L.hi, qc * 4LL},   {L.live, qc * 4LL},  {L.iters, qc * 4LL},
                     {L.slab_live, slabs * 4},                {L.n_live, 8}};
  const int n = (int)(sizeof b / sizeof b[0]);
  long long end = 0;
  for (int i = 0; i < n; ++i) {
    if (b[i].at % 256 != 0) return fail("alignment", i, b[i].at);
    if (b[i].at < end) return fail("blocks overlap", i, b[i].at);  // (the blocks are laid out in this order)
    if (b[i].bytes <= 0) return fail("empty block", i, b[i].bytes);
    end = b[i].at + b[i].bytes;
  }
  if (end > L.total) return fail("block passes total", end, L.total);
  // the GEMM operand: whole 128-row tiles of kpad floats, kpad >= D
  if (btn % 128 != 0 || btn < (long long)qc * D) return fail("Bt size", btn, qc);
  return 0;
}

int main() {
  const long long Ns[] = {1,    2,     31,    32,     33,     63,     64,      65,      1000,    2000,
                          4097, 65535, 65536, 65537, 100000, 131072, 500000, 1000000, 1999999, 2000000};
  const int Ds[] = {1, 96, 128, 768, 1536};
  const int reqs[] = {-5, 0, 1, 31, 32, 33, 64, 100, 255, 256, 257, 100000};
  const int Qs[] = {1, 2, 31, 32, 33, 64, 65, 70, 255, 256, 257, 511, 512, 513, 999, 1000};
  long long cases = 0;
  for (long long N : Ns) {
    // the row partition: a rule of N alone
    const int pr = gates_part_rows(N), parts = gates_parts(N);
    if (pr < kGatesStepRows || pr % kGatesStepRows != 0) return fail("part rows", N, pr);
    if (parts < 1 || parts > kGatesMaxParts) return fail("parts", N, parts);
    if ((long long)parts * pr < N || (long long)(parts - 1) * pr >= N) return fail("partition does not cover the rows", N, parts);
    for (int D : Ds)
      for (int req : reqs) {
        const int qc = gates_chunk(N, D, req, kGatesBudgetBytes);
        if (qc < kGatesSlab || qc > kGatesMaxChunk || qc % kGatesSlab != 0) return fail("chunk width", qc, req);
        if (req >= 1 && req <= kGatesMaxChunk && qc > gates_width(req)) return fail("chunk above the request", qc, req);
        const long long total = gates_layout(N, qc, gates_bt_floats(qc, D)).total;
        if (qc > kGatesSlab && total > kGatesBudgetBytes) return fail("budget", qc, total);
        if (qc < gates_width(std::min(std::max(req, 1), kGatesMaxChunk)) &&
            gates_layout(N, qc + kGatesSlab, gates_bt_floats(qc + kGatesSlab, D)).total <= kGatesBudgetBytes)
          return fail("chunk lowered further than the budget asks", qc, req);
        for (int Q : Qs) {
          const int nc = gates_chunk_count(Q, qc);
          int next = 0;
          for (int c = 0; c < nc; ++c) {
            const int q0 = gates_chunk_begin(c, qc), nq = gates_chunk_size(Q, c, qc);
            if (q0 != next || nq < 1 || nq > qc) return fail("chunks do not tile", q0, nq);
            next = q0 + nq;
            const int w = gates_width(nq);  // the panel this chunk runs in
            if (w % kGatesSlab != 0 || w < nq || w - nq >= kGatesSlab || w > qc) return fail("panel width", w, nq);
            // a narrower panel's arrays fit the block allocated for the widest
            if (gates_layout(N, w, gates_bt_floats(w, D)).total > total) return fail("narrow panel larger", w, qc);
            if (gates_part_rows(N) != pr || gates_parts(N) != parts) return fail("partition changed with the width", w, N);
            ++cases;
          }
          if (next != Q) return fail("chunks do not end at Q", next, Q);
        }
        for (int w = kGatesSlab; w <= qc; w += kGatesSlab)
          if (check_layout(N, D, w)) return 1;
      }
  }
  if (gates_chunk_count(0, 256) != 0) return fail("Q = 0", 0, 0);
  // walk one small panel through a real block as the kernels index it: element (row, col) of a slab-major array, the
  // partials at (slab, part), the transposed output
  for (long long N : {1LL, 33LL, 2000LL})
    for (int qc : {32, 96}) {
      const GatesLayout L = gates_layout(N, qc, gates_bt_floats(qc, 96));
      std::vector<unsigned char> block((size_t)L.total, 0);
      const int slabs = qc / kGatesSlab, parts = gates_parts(N), pr = gates_part_rows(N);
      float* X = reinterpret_cast<float*>(block.data() + L.X);
      float* out = reinterpret_cast<float*>(block.data() + L.out);
      double* pa = reinterpret_cast<double*>(block.data() + L.part_a);
      std::vector<int> seen((size_t)N, 0);
      for (int s = 0; s < slabs; ++s)
        for (int p = 0; p < parts; ++p) {
          const long long r0 = (long long)p * pr, r1 = std::min<long long>(N, r0 + pr);
          for (long long r = r0; r < r1; ++r) {
            if (s == 0) ++seen[(size_t)r];
            for (int c = 0; c < 32; ++c) X[((size_t)s * N + r) * 32 + c] = (float)(r + c);
          }
          for (int c = 0; c < 32; ++c) pa[((size_t)s * parts + p) * 32 + c] = 1.0;
        }
      for (long long r = 0; r < N; ++r)
        if (seen[(size_t)r] != 1) return fail("a row is in no part or in two", r, seen[(size_t)r]);
      for (int q = 0; q < qc; ++q)
        for (long long r = 0; r < N; ++r) out[(size_t)q * N + r] = X[((size_t)(q / 32) * N + r) * 32 + q % 32];
      if (out[(size_t)(qc - 1) * N + (N - 1)] != (float)(N - 1 + 31)) return fail("walk", N, qc);
      ++cases;
    }
  std::printf("gates many plan sweep ok (%lld cases)\n", cases);
  return 0;
}

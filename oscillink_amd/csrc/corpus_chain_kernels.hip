// Chain priors on the candidate lattices of a corpus refine chunk (osc_corpus_refine_chains): the U*
// solve with lamP L_path (k_cq_solve_chain) and chain_receipt() of every lattice's own chain (k_cq_chain_receipt), one
// workgroup per lattice each.  The settle and the receipt of such a call are corpus_receipt_kernels.hip's chain instances.
// Only a call with chains launches any of them; no workgroup waits on another.
#include "chain_receipt_dev.hpp"
#include "common.hpp"
#include "corpus_receipts.hpp"

namespace osc {
namespace {

// k_cq_solve's gated operator (osc_corpus.hip) with the path hook; B = 1 where there are no gates
struct CqChainSolveOp {
  const float* s_cs;
  const float* s_inv;
  const float* B;
  int64_t r0;
  float cW, lamG, lamQ;
  CqPathRows path;
  static constexpr bool kFromY = false, kPath = true;
  __device__ __forceinline__ float cs(int64_t i) const { return s_cs[i - r0]; }
  __device__ __forceinline__ float inv_diag(int64_t i) const { return s_inv[i - r0]; }
  __device__ __forceinline__ float qb(int64_t i) const { return B ? lamQ * B[i] : lamQ; }
  __device__ __forceinline__ float rhs(float y, float qbi, float p) const { return lamG * y + qbi * p; }
};

// Jacobi-PCG for U* of a lattice with a chain prior (lattice.py:245-263): M gains lamP L_path = lamP (I - W_p) while
// lamP > 0 -- lamP in the rows' constants, -lamP W_p through cq_pcg's path hook -- and the Jacobi diagonal gains lamP
// whenever a chain is present (lattice.py:257-259).  Each is added to k_cq_solve's expression, so a lattice without a chain,
// or with one at lamP = 0, gets k_cq_solve's bytes.
template <int NC>
__global__ __launch_bounds__(256) void k_cq_solve_chain(const CqChainPcgArgs ca) {
  __shared__ float red[4];
  __shared__ float s_cs[host::kCorpusMaxTopK], s_inv[host::kCorpusMaxTopK];
  __shared__ int32_t s_slot[host::kCorpusMaxTopK];
  const CqPcgArgs& a = ca.pcg;
  const CqLattice& g = a.lat;
  const int tid = threadIdx.x, lat = blockIdx.x;
  const int64_t r0 = (int64_t)lat * g.K;
  const int n = g.rows(lat);
  const float lamG = g.lamG(lat), lamC = g.lamC(lat), lamQ = g.lamQ(lat);  // (uniform: the lattice's own, or the launch's)
  const float lamP = g.lamP(lat, ca.chain.lamP);
  const bool present = ca.chain.rec(lat)[0] > 0, active = present && lamP > 0.f;
  const float cP = active ? lamP : 0.f;
  cq_path_slots(ca.chain, lat, n, active, s_slot);
  for (int r = tid; r < n; r += 256) {
    const float Bi = g.B ? g.B[r0 + r] : 1.0f;
    const float cs = fmaf(lamQ, Bi, lamG + lamC);
    s_cs[r] = active ? cs + cP : cs;
    s_inv[r] = 1.f / (fmaf(lamQ, Bi, present ? lamG + lamP : lamG) + 1e-12f);
  }
  __syncthreads();
  cq_pcg<NC>(a, CqChainSolveOp{s_cs, s_inv, g.B, r0, lamC, lamG, lamQ, cq_path_rows(ca.chain, lat, s_slot, cP)}, red,
             a.max_iters, a.tol);
}

// chain_receipt(chain, z_th) of the lattice's own chain (lattice.py:466-528), one workgroup per lattice, a wave per chain
// edge t = (i, j), k_cq_receipt's arithmetic (cq_sdiff, fp32 dot products by wave_sum_f, row statistics over the K dense
// entries in fp64):
//   R_s = lamC a_ie |Un_i - Un_e|^2 over row i's structural entries, R_p = max(lamC, 1e-6) A_path[i][e] |Un_i - Un_e|^2 over its
//   path entries; mu = sum R / K, sigma = sqrt(sum R^2 / K - mu^2) + 1e-12; z = (R_ij - mu) / sigma with R_ij = 0 when j is not
//   an entry of the row; gain term 0.5 lamC max(a_ij, 0) (|Yn_i - Yn_j|^2 - |Un_i - Un_j|^2).
// One thread then adds the gain in fp64 in edge order, takes the first edge whose max(z) is strictly greater than every
// earlier one, from -1 (lattice.py:489, 506), and forms the verdict all(max(z) <= z_th): chain_receipt_dev.hpp's rules, which
// the built lattice's batched call (chain_many_kernels.hip) runs as well.
__global__ __launch_bounds__(256) void k_cq_chain_receipt(const CqChainEdgesArgs a) {
  __shared__ double s_term[kCqMaxChainEdges], s_zmax[kCqMaxChainEdges];
  __shared__ int32_t s_slot[kCqMaxRows];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const CqLattice& g = a.lat;
  const int lat = blockIdx.x, K = g.rows(lat);  // (the lattice's own row count; its slot is g.K rows)
  const int64_t r0 = (int64_t)lat * g.K;
  const int32_t* rec = a.chain.rec(lat);
  const int E = min(rec[0], min(a.chain.cap, kCqMaxChainEdges));
  if (E <= 0) {  // (uniform) no chain
    if (tid == 0) {
      a.gain[lat] = 0.0;
      a.verdict[lat] = 0;
      a.weak_k[lat] = -1;
      a.weak_z[lat] = 0.f;
    }
    return;
  }
  cq_path_slots(a.chain, lat, K, true, s_slot);
  __syncthreads();
  const int32_t* nodes = rec + 2;
  const int32_t* pptr = rec + a.chain.ptr_at;
  const int32_t* pcol = rec + a.chain.col_at;
  const float* pa = a.chain.a(lat);
  const float lamC = g.lamC(lat);  // (uniform: the lattice's own, or the launch's)
  const float lam_p = fmaxf(lamC, 1e-6f);
  float* out = a.edge + (size_t)lat * 4 * a.chain.cap;
  for (int t = wave; t < E; t += 4) {
    const int li = nodes[t], lj = nodes[t + 1];
    const int64_t i = r0 + li, j = r0 + lj;
    const size_t io = (size_t)i * g.ldn;
    const float inv_i = 1.0f / (g.sd[i] + 1e-12f);
    auto du_to = [&](int64_t jj) {
      const float inv_j = 1.0f / (g.sd[jj] + 1e-12f);
      const size_t jo = (size_t)jj * g.ldn;
      float du = 0.f;
      for (int c = lane; c < g.ldn; c += 64) {
        const float u = cq_sdiff(a.Us[io + c], inv_i, a.Us[jo + c], inv_j);
        du = fmaf(u, u, du);
      }
      return wave_sum_f(du);
    };
    // structural row i
    float rs = 0.f, rp = 0.f;
    double s1 = 0.0, s2 = 0.0, term = 0.0;
    const int d = g.deg[i];
    for (int e = 0; e < d; ++e) {
      const int64_t jj = g.col[i * g.k + e];
      const float wij = g.adj[i * g.k + e];
      const float du = du_to(jj);
      if (!(wij > 0.f)) continue;
      const float R = lamC * wij * du;
      s1 += (double)R;
      s2 += (double)R * (double)R;
      if (jj != j) continue;
      rs = R;
      const float inv_j = 1.0f / (g.sd[j] + 1e-12f);
      const size_t jo = (size_t)j * g.ldn;
      float dy = 0.f;
      for (int c = lane; c < g.ldn; c += 64) {
        const float y = cq_sdiff(g.Y[io + c], inv_i, g.Y[jo + c], inv_j);
        dy = fmaf(y, y, dy);
      }
      dy = wave_sum_f(dy);
      term = 0.5 * (double)lamC * (double)wij * ((double)dy - (double)du);
    }
    const double z_s = chain_row_z(s1, s2, rs, (double)K);
    // path row i (every chain node owns one)
    s1 = s2 = 0.0;
    const int ps = s_slot[li];
    if (ps >= 0)
      for (int e = pptr[ps]; e < pptr[ps + 1]; ++e) {
        const float R = lam_p * pa[e] * du_to(r0 + pcol[e]);
        s1 += (double)R;
        s2 += (double)R * (double)R;
        if (pcol[e] == lj) rp = R;
      }
    const double z_p = chain_row_z(s1, s2, rp, (double)K);
    if (lane == 0) {
      out[t] = (float)z_s;
      out[a.chain.cap + t] = (float)z_p;
      out[2 * a.chain.cap + t] = rs;
      out[3 * a.chain.cap + t] = rp;
      s_term[t] = term;
      s_zmax[t] = chain_zmax(z_s, z_p);
    }
  }
  __syncthreads();
  if (tid == 0) {
    const ChainVerdict v = chain_finish(s_term, s_zmax, E, a.z_th);
    a.gain[lat] = v.gain;
    a.verdict[lat] = v.ok;
    a.weak_k[lat] = v.weak_k;
    a.weak_z[lat] = (float)v.worst;
  }
}

}  // namespace

void launch_cq_solve_chain(const CqChainPcgArgs& a, int32_t nq, hipStream_t s) {
  cq_with_nc(a.pcg.lat.ldn, [&](auto nc) {
    hipLaunchKernelGGL((k_cq_solve_chain<decltype(nc)::value>), dim3((unsigned)nq), dim3(256), 0, s, a);
  });
  HIP_CHECK(hipGetLastError());
}

void launch_cq_chain_receipt(const CqChainEdgesArgs& a, int32_t nq, hipStream_t s) {
  hipLaunchKernelGGL(k_cq_chain_receipt, dim3((unsigned)nq), dim3(256), 0, s, a);
  HIP_CHECK(hipGetLastError());
}

}  // namespace osc

// Kernels of osc_create_updated and osc_corpus_update: rows of a lattice or a corpus replaced in place.
//
//   k_update_scatter_rows : the uploaded new rows onto their ids, in the handle's row pitch
//   k_update_lists        : the base's lists with the replaced members emptied and the replaced rows' lists empty
//   k_update_merge        : every kept row scans its column of the replaced rows' score block; an equal score can win
//   k_corpus_update_rows  : a corpus' Y and Yn rows rewritten from the uploaded rows
#include "update.hpp"
#include "append.hpp"

namespace osc {
namespace {

__global__ __launch_bounds__(256) void k_update_scatter_rows(float* __restrict__ dst, int32_t ld_dst, const float* __restrict__ src,
                                                             int32_t D, int32_t cols, const int32_t* __restrict__ ids, int64_t M) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= M * cols) return;
  const int64_t j = t / cols;
  const int32_t c = (int32_t)(t - j * cols);
  dst[(int64_t)ids[j] * ld_dst + c] = c < D ? src[j * D + c] : 0.f;
}

// k_remove_lists' shape (remove_kernels.hip) without the move: one thread per V consecutive entries of the flat n x k list
// arrays (V = 4 where k is a multiple of 4, so a thread's entries share a row and both sides move 16 bytes per lane; else
// 1).  The map lookups are element gathers from a table of 4 bytes a row, which the caches hold.
template <int V>
__global__ __launch_bounds__(256) void k_update_lists(const float* __restrict__ kval, const int32_t* __restrict__ kidx, int64_t n,
                                                      int32_t k, const int32_t* __restrict__ keep, float* __restrict__ out_val,
                                                      int32_t* __restrict__ out_idx) {
  const int64_t t = ((int64_t)blockIdx.x * 256 + threadIdx.x) * V;
  if (t >= n * k) return;
  const int64_t i = t / k;
  const bool gone = keep[i] < 0;  // a replaced row: its list is the select's to write, empty until then
  int32_t id[V];
  float v[V];
  if constexpr (V == 4) {
    const int4 a = *reinterpret_cast<const int4*>(kidx + t);
    const float4 b = *reinterpret_cast<const float4*>(kval + t);
    id[0] = a.x, id[1] = a.y, id[2] = a.z, id[3] = a.w;
    v[0] = b.x, v[1] = b.y, v[2] = b.z, v[3] = b.w;
  } else {
    id[0] = kidx[t];
    v[0] = kval[t];
  }
#pragma unroll
  for (int u = 0; u < V; ++u) {
    const int32_t m = (!gone && id[u] >= 0 && id[u] < n) ? keep[id[u]] : -1;
    id[u] = m;
    if (m < 0) v[u] = 0.f;
  }
  if constexpr (V == 4) {
    *reinterpret_cast<int4*>(out_idx + t) = make_int4(id[0], id[1], id[2], id[3]);
    *reinterpret_cast<float4*>(out_val + t) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    out_idx[t] = id[0];
    out_val[t] = v[0];
  }
}

// a is a worse list entry than b  <=>  smaller score, or equal score and larger index
__device__ __forceinline__ bool worse(float av, int ai, float bv, int bi) { return av < bv || (av == bv && ai > bi); }

// k_append_merge's shape (append_kernels.hip): one thread per row, adjacent threads read adjacent columns of a score row,
// so the scan -- all the kernel does for most rows -- is one coalesced stream over the block; the replaced columns' ids
// are the same for every thread (uniform loads).  A row outside the redo set has k members with scores > 0 (stored values
// are true scores then), none of them a replaced row, in any order: its list is the k best of the columns that did not
// change.  A replaced column j may lie BELOW a member's index, so it enters iff (score, j) precedes the worst member
// (wv, wi): s > wv, or s == wv and j < wi.  NaN compares false both ways and never enters.  The worst member is found
// again after every hit.
__global__ __launch_bounds__(256) void k_update_merge(const float* __restrict__ Sm, int64_t lds_, int32_t qb, int32_t qe,
                                                      const int32_t* __restrict__ cols, int32_t n, const uint8_t* __restrict__ flags,
                                                      int32_t k, float* __restrict__ kval, int32_t* __restrict__ kidx,
                                                      int32_t* __restrict__ changed) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n || (flags[i] & kAppendRedo)) return;
  float* v = kval + i * k;
  int32_t* id = kidx + i * k;
  float wv = v[0];
  int wi = id[0], wp = 0;
  for (int e = 1; e < k; ++e)
    if (worse(v[e], id[e], wv, wi)) wv = v[e], wi = id[e], wp = e;
  int hits = 0;
  auto offer = [&](float s, int32_t col) {
    if (!(s > wv || (s == wv && col < wi))) return;
    v[wp] = fmaxf(s, 0.f);
    id[wp] = col;
    ++hits;
    wv = v[0], wi = id[0], wp = 0;
    for (int e = 1; e < k; ++e)
      if (worse(v[e], id[e], wv, wi)) wv = v[e], wi = id[e], wp = e;
  };
  const float* col = Sm + i;
  int q = qb;
  for (; q + 8 <= qe; q += 8) {  // eight loads in flight
    float s[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) s[u] = col[(int64_t)(q + u) * lds_];
#pragma unroll
    for (int u = 0; u < 8; ++u) offer(s[u], cols[q + u]);
  }
  for (; q < qe; ++q) offer(col[(int64_t)q * lds_], cols[q]);
  if (hits == 0) return;
  for (int e = 1; e < k; ++e) {  // rewritten lists are sorted (score desc, index asc)
    const float ev = v[e];
    const int ei = id[e];
    int p = e;
    while (p > 0 && worse(v[p - 1], id[p - 1], ev, ei)) {
      v[p] = v[p - 1];
      id[p] = id[p - 1];
      --p;
    }
    v[p] = ev;
    id[p] = ei;
  }
  atomicAdd(changed, hits);
}

// one wave per replaced row; the sums are k_normalize_rows' (knn_kernels.hip): lane l adds the squares of columns l, l + 64,
// ... in that order by fma, the 64 sums meet in the xor butterfly 32, 16, .. 1, and a column is scaled by one multiply
__global__ __launch_bounds__(256) void k_corpus_update_rows(const float* __restrict__ src, int32_t D, const int32_t* __restrict__ ids,
                                                            int64_t M, float* __restrict__ Y, float* __restrict__ Yn, int32_t ldn) {
  const int lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= M) return;
  const float* x = src + j * D;
  float* y = Y + (int64_t)ids[j] * ldn;
  float* yn = Yn + (int64_t)ids[j] * ldn;
  float ss = 0.f;
  for (int c = lane; c < D; c += 64) ss = fmaf(x[c], x[c], ss);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
  const float inv = 1.f / (sqrtf(ss) + 1e-12f);
  for (int c = lane; c < ldn; c += 64) {
    const float a = c < D ? x[c] : 0.f;
    y[c] = a;
    yn[c] = c < D ? a * inv : 0.f;
  }
}

}  // namespace

void launch_update_scatter_rows(float* dst, int32_t ld_dst, const float* src, int32_t D, int32_t cols, const int32_t* ids, int64_t M,
                                hipStream_t s) {
  if (M <= 0 || cols <= 0) return;
  if (cols > ld_dst || D > cols) throw std::runtime_error("launch_update_scatter_rows: need D <= cols <= ld_dst");
  const int64_t blocks = (M * cols + 255) / 256;
  if (blocks >= ((int64_t)1 << 31)) throw std::runtime_error("launch_update_scatter_rows: too many elements for one launch");
  hipLaunchKernelGGL(k_update_scatter_rows, dim3((unsigned)blocks), dim3(256), 0, s, dst, ld_dst, src, D, cols, ids, M);
  HIP_CHECK(hipGetLastError());
}

void launch_update_lists(const float* kval, const int32_t* kidx, int64_t n, int32_t k, const int32_t* keep, float* out_val,
                         int32_t* out_idx, hipStream_t s) {
  if (n <= 0 || k <= 0) return;
  const int v = k % 4 == 0 ? 4 : 1;
  const int64_t blocks = ((n * k + v - 1) / v + 255) / 256;
  if (blocks >= ((int64_t)1 << 31)) throw std::runtime_error("launch_update_lists: too many list entries for one launch");
  if (v == 4) hipLaunchKernelGGL(k_update_lists<4>, dim3((unsigned)blocks), dim3(256), 0, s, kval, kidx, n, k, keep, out_val, out_idx);
  else hipLaunchKernelGGL(k_update_lists<1>, dim3((unsigned)blocks), dim3(256), 0, s, kval, kidx, n, k, keep, out_val, out_idx);
  HIP_CHECK(hipGetLastError());
}

void launch_update_merge(const float* Sm, int64_t lds_, int32_t qb, int32_t qe, const int32_t* cols, int32_t n, const uint8_t* flags,
                         int32_t k, float* kval, int32_t* kidx, int32_t* changed, hipStream_t s) {
  if (qe <= qb || n <= 0) return;
  hipLaunchKernelGGL(k_update_merge, dim3((unsigned)(((int64_t)n + 255) / 256)), dim3(256), 0, s, Sm, lds_, qb, qe, cols, n, flags, k, kval,
                     kidx, changed);
  HIP_CHECK(hipGetLastError());
}

void launch_corpus_update_rows(const float* src, int32_t D, const int32_t* ids, int64_t M, float* Y, float* Yn, int32_t ldn,
                               hipStream_t s) {
  if (M <= 0) return;
  hipLaunchKernelGGL(k_corpus_update_rows, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, src, D, ids, M, Y, Yn, ldn);
  HIP_CHECK(hipGetLastError());
}

}  // namespace osc

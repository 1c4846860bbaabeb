// The per-query top-K select of the corpus search (DESIGN.md sections 13 and 13.6): what k_cq_select (osc_corpus.hip) and
// k_cq_select_masked (corpus_store_kernels.hip) share, and the launchers of corpus_store_kernels.hip.
#pragma once
#include "common.hpp"
#include "corpus_plan.hpp"

namespace osc {

constexpr int kSelT = host::kCorpusMaxTopK;  // threads of a select workgroup: one key per thread in the final sort

__device__ __forceinline__ uint32_t fkey(float v) {  // ascending float order == ascending key order; finite keys are > 0
  const uint32_t u = v == 0.f ? 0u : __float_as_uint(v);  // (-0 and +0 are one value)
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ int block_scan(bool flag, int* wsum, int* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long m = __ballot(flag);
  const int pre = __popcll(m & ((1ull << lane) - 1ull));
  if (lane == 0) wsum[w] = __popcll(m);
  __syncthreads();
  int wpre = 0, tot = 0;
#pragma unroll
  for (int t = 0; t < kSelT / 64; ++t) {
    const int v = wsum[t];
    wpre += t < w ? v : 0;
    tot += v;
  }
  __syncthreads();
  *total = tot;
  return wpre + pre;
}

// k_cq_select over the eligible rows only: row i of query q takes part iff bit i & 31 of live[i >> 5] and (allow != nullptr)
// of allow[q allow_stride + (i >> 5)] are set.  allow_stride = 0: one filter for every query.  The caller guarantees K
// eligible rows per query.
void launch_cq_select_masked(const float* dots, int64_t N, int32_t K, const uint32_t* live, const uint32_t* allow,
                             int64_t allow_stride, int32_t* cand, float* ccos, int32_t nq, hipStream_t s);
// the ragged form: a query with n < K eligible rows keeps all n, sorted as always; nrows[q] =
// min(K, eligible rows), cand is -1 and ccos 0 behind it.  The caller guarantees one eligible row per query.
void launch_cq_select_ragged(const float* dots, int64_t N, int32_t K, const uint32_t* live, const uint32_t* allow,
                             int64_t allow_stride, int32_t* cand, float* ccos, int32_t* nrows, int32_t nq, hipStream_t s);
// dst row g <- src row kept[g], for Y and Yn at once (rows of ldn floats, ldn a multiple of 4)
void launch_cq_compact(const float* Y, const float* Yn, int32_t ldn, const int32_t* kept, int64_t rows, float* Yd, float* Ynd,
                       hipStream_t s);

}  // namespace osc

// Kernels of the mutable corpus:
//   k_cq_select_masked : k_cq_select (osc_corpus.hip) over the eligible rows of a corpus with tombstones and / or a filter
//   k_cq_compact       : the kept rows of Y and Yn, in order, into fresh buffers
// A search on a corpus without tombstones and without a filter launches k_cq_select, never the masked kernel.
#include "corpus_select.hpp"

namespace osc {
namespace {

// Row i of query q is eligible iff its live bit and (with a filter) its allow bit are set.  A thread reads word i >> 5 of
// each bitmap for its row: 32 neighbouring lanes share a word, so a wave's loads are two words per bitmap.  The score is
// loaded beside the words, not behind a branch on them: the loop is bound by load latency (one workgroup per query), and a
// score load that waits for the word's would double it.  A row that is not eligible takes no part at all: it is in no histogram, it is not collected, and it is not counted by the scan that
// numbers the rows of the K-th key's tie class (counted there, a masked row in front of a live one with the same key would
// push the live one out).
// RAGGED (the reference's filtered loop keeps whichever rows pass, proof_hallucination.py:203-221):
// a query may have fewer than K eligible rows.  The first histogram pass counts them; with fewer than K the radix walk has no
// K-th key to find (its `cum + h >= k` never fires), so the walk is skipped, every eligible key is collected (T = 0: finite
// keys are > 0) and sorted as always, n = the count goes to nrows[q], and cand / ccos behind n are -1 / 0.  Only tid < n
// indexes d[].  The uniform instance is the kernel as it was.
template <bool RAGGED>
__global__ __launch_bounds__(kSelT) void k_cq_select_masked(const float* dots, int64_t N, int32_t K, const uint32_t* live,
                                                            const uint32_t* allow, int64_t allow_stride, int32_t* cand,
                                                            float* ccos, int32_t* nrows) {
  __shared__ uint32_t hist[256];
  __shared__ uint32_t skey[kSelT];
  __shared__ int32_t sid[kSelT];
  __shared__ int wsum[kSelT / 64];
  __shared__ uint32_t st_prefix, st_mask, st_k;
  __shared__ int st_n;
  __shared__ int st_rows;  // (RAGGED only)
  const int q = blockIdx.x, tid = threadIdx.x;
  const float* d = dots + (size_t)q * N;
  const uint32_t* arow = allow ? allow + (size_t)q * allow_stride : nullptr;
  auto eligible = [&](int64_t i) {
    uint32_t w = live[i >> 5];
    if (arow) w &= arow[i >> 5];
    return ((w >> (i & 31)) & 1u) != 0u;
  };
  uint32_t prefix = 0u, mask = 0u, k = (uint32_t)K;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    if (tid < 256) hist[tid] = 0u;
    __syncthreads();
    for (int64_t i = tid; i < N; i += kSelT) {
      const float v = d[i];
      const bool on = eligible(i);
      const uint32_t kk = fkey(v);
      if (on && (kk & mask) == prefix) atomicAdd(&hist[(kk >> shift) & 255u], 1u);
    }
    __syncthreads();
    if constexpr (RAGGED) {
      if (pass == 0) {
        if (tid == 0) {
          uint32_t tot = 0u;
          for (int b = 0; b < 256; ++b) tot += hist[b];
          st_rows = (int)(tot < (uint32_t)K ? tot : (uint32_t)K);
        }
        __syncthreads();
      }
      if (st_rows < K) break;  // (uniform) fewer than K eligible rows: all of them are kept
    }
    if (tid == 0) {
      uint32_t cum = 0u;
      for (int b = 255; b >= 0; --b) {
        const uint32_t h = hist[b];
        if (cum + h >= k) {
          prefix |= (uint32_t)b << shift;
          k -= cum;
          break;
        }
        cum += h;
      }
      mask |= 255u << shift;
      st_prefix = prefix;
      st_mask = mask;
      st_k = k;
    }
    __syncthreads();
    prefix = st_prefix;
    mask = st_mask;
    k = st_k;
  }
  const uint32_t T = prefix;  // the K-th largest eligible key; k = how many keys equal to T are kept (the smallest ids)
  if (tid == 0) st_n = 0;
  sid[tid] = 0x7fffffff;
  skey[tid] = 0u;
  __syncthreads();
  int eqrun = 0;
  for (int64_t i0 = 0; i0 < N; i0 += kSelT) {  // (every thread runs every round: block_scan has barriers)
    const int64_t i = i0 + tid;
    const float v = i < N ? d[i] : 0.f;
    const bool on = i < N && eligible(i);
    const uint32_t kk = on ? fkey(v) : 0u;
    int tot = 0;
    const int eqpos = eqrun + block_scan(on && kk == T, wsum, &tot);
    if (on && (kk > T || (kk == T && eqpos < (int)k))) {
      const int slot = atomicAdd(&st_n, 1);
      if (slot < kSelT) {
        skey[slot] = kk;
        sid[slot] = (int32_t)i;
      }
    }
    eqrun += tot;
  }
  __syncthreads();
  for (int size = 2; size <= kSelT; size <<= 1) {  // key descending, then id ascending
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      const int l = tid ^ stride;
      if (l > tid) {
        const uint32_t ki = skey[tid], kl = skey[l];
        const int ai = sid[tid], al = sid[l];
        const bool l_first = kl > ki || (kl == ki && al < ai);
        const bool i_first = ki > kl || (ki == kl && ai < al);
        if ((tid & size) == 0 ? l_first : i_first) {
          skey[tid] = kl;
          skey[l] = ki;
          sid[tid] = al;
          sid[l] = ai;
        }
      }
      __syncthreads();
    }
  }
  if constexpr (RAGGED) {
    const int n = st_rows;
    if (tid == 0) nrows[q] = n;
    if (tid < K) {
      const int32_t i = sid[tid];
      const bool real = tid < n && i >= 0 && i < N;  // (tid < n implies the rest: n keys were collected)
      cand[(size_t)q * K + tid] = real ? i : -1;
      ccos[(size_t)q * K + tid] = real ? d[i] : 0.f;
    }
  } else if (tid < K) {
    const int32_t i = sid[tid];
    cand[(size_t)q * K + tid] = i;
    ccos[(size_t)q * K + tid] = i < N ? d[i] : 0.f;  // (i < N always: the host checked K <= eligible rows)
  }
}

// a wave per kept row, float4 per lane
__global__ __launch_bounds__(256) void k_cq_compact(const float* __restrict__ Y, const float* __restrict__ Yn, int32_t ldn,
                                                    const int32_t* __restrict__ kept, int64_t rows, float* __restrict__ Yd,
                                                    float* __restrict__ Ynd) {
  const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= rows) return;
  const int lane = threadIdx.x & 63;
  const size_t src = (size_t)kept[g] * ldn, dst = (size_t)g * ldn;
  for (int c = lane * 4; c < ldn; c += 256) {
    *reinterpret_cast<float4*>(Yd + dst + c) = *reinterpret_cast<const float4*>(Y + src + c);
    *reinterpret_cast<float4*>(Ynd + dst + c) = *reinterpret_cast<const float4*>(Yn + src + c);
  }
}

}  // namespace

void launch_cq_select_masked(const float* dots, int64_t N, int32_t K, const uint32_t* live, const uint32_t* allow,
                             int64_t allow_stride, int32_t* cand, float* ccos, int32_t nq, hipStream_t s) {
  hipLaunchKernelGGL(k_cq_select_masked<false>, dim3((unsigned)nq), dim3(kSelT), 0, s, dots, N, K, live, allow, allow_stride,
                     cand, ccos, (int32_t*)nullptr);
  HIP_CHECK(hipGetLastError());
}

void launch_cq_select_ragged(const float* dots, int64_t N, int32_t K, const uint32_t* live, const uint32_t* allow,
                             int64_t allow_stride, int32_t* cand, float* ccos, int32_t* nrows, int32_t nq, hipStream_t s) {
  hipLaunchKernelGGL(k_cq_select_masked<true>, dim3((unsigned)nq), dim3(kSelT), 0, s, dots, N, K, live, allow, allow_stride,
                     cand, ccos, nrows);
  HIP_CHECK(hipGetLastError());
}

void launch_cq_compact(const float* Y, const float* Yn, int32_t ldn, const int32_t* kept, int64_t rows, float* Yd, float* Ynd,
                       hipStream_t s) {
  if (rows <= 0) return;
  hipLaunchKernelGGL(k_cq_compact, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, Y, Yn, ldn, kept, rows, Yd, Ynd);
  HIP_CHECK(hipGetLastError());
}

}  // namespace osc

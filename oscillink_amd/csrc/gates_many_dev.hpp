// Device helpers of the slab-major panel kernels (gates_many_kernels.hip, bundle_gated_kernels.hip): 16-byte accesses, the
// workgroup's fp64 fold of its 32 row classes, the sum of a slab's parts in a fixed order, and a workgroup's rows.  A panel
// is any struct with N, parts and part_rows (gates_many.hpp: GmPanel; bundle_gated.hpp: BgPanel).
#pragma once
#include "common.hpp"

namespace osc {
namespace {

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, const float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float4 f4(float v) { return make_float4(v, v, v, v); }
__device__ __forceinline__ float4 mulacc4(const float4 a, const float4 b, const float4 c) {
  return make_float4(fmaf(a.x, b.x, c.x), fmaf(a.y, b.y, c.y), fmaf(a.z, b.z, c.z), fmaf(a.w, b.w, c.w));
}

// column sums of a workgroup's 32 row classes (thread t: class t >> 3, columns 4 (t & 7) ..): classes in order, in fp64
__device__ __forceinline__ void gm_fold(const float4 v, double* sh, double* out) {
  const int t = threadIdx.x;
  double* s = sh + (t >> 3) * 32 + (t & 7) * 4;
  s[0] = (double)v.x;
  s[1] = (double)v.y;
  s[2] = (double)v.z;
  s[3] = (double)v.w;
  __syncthreads();
  if (t < 32) {
    double a = 0.0;
#pragma unroll
    for (int c = 0; c < 32; ++c) a += sh[c * 32 + t];
    out[t] = a;
  }
  __syncthreads();
}

// one slab's column partials summed over the parts by a 1024-thread workgroup: 32 thread groups take parts g, g + 32, ... in
// order, then the groups in order.  The total is valid in threads 0..31 (column = thread).
constexpr int kGmSumThreads = 1024, kGmSumGroups = kGmSumThreads / 32;
__device__ __forceinline__ double gm_part_sum(const double* part, int parts, double* sh) {
  const int c = threadIdx.x & 31, g = threadIdx.x >> 5;
  double s = 0.0;
#pragma unroll 8
  for (int b = g; b < parts; b += kGmSumGroups) s += part[(size_t)b * 32 + c];
  sh[g * 32 + c] = s;
  __syncthreads();
  double tot = 0.0;
  if (threadIdx.x < 32) {
#pragma unroll
    for (int k = 0; k < kGmSumGroups; ++k) tot += sh[k * 32 + c];
  }
  __syncthreads();
  return tot;
}

// np.minimum / np.maximum: a NaN stays
__device__ __forceinline__ float nan_min(float a, float v) { return (v < a || v != v) ? v : a; }
__device__ __forceinline__ float nan_max(float a, float v) { return (v > a || v != v) ? v : a; }

struct GmRows {  // the rows of this workgroup's part
  int64_t r0, r1;
};
template <class Panel>
__device__ __forceinline__ GmRows gm_rows(const Panel& p) {
  const int64_t r0 = (int64_t)blockIdx.x * p.part_rows;
  const int64_t r1 = r0 + p.part_rows < (int64_t)p.N ? r0 + p.part_rows : (int64_t)p.N;
  return GmRows{r0, r1};
}
template <class Panel>
__device__ __forceinline__ size_t gm_part_at(const Panel& p) {
  return ((size_t)blockIdx.y * p.parts + blockIdx.x) * 32;
}

}  // namespace
}  // namespace osc

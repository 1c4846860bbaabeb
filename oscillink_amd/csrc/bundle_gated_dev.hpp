// Device helpers shared by the gated panel kernels (bundle_gated_kernels.hip, receipt_gated_kernels.hip): the Jacobi
// diagonal of M_q, masked loads of a row-major N x ld array, the wave's fixed fp64 butterfly and the squared difference of
// two scaled float4s in fp64.
#pragma once
#include "bundle_gated.hpp"
#include "gates_many_dev.hpp"

namespace osc {
namespace {

// the reference's Jacobi diagonal lamG + lamQ g (+ 1e-12), inverted (lattice.py:257-259, solver.py:20)
__device__ __forceinline__ float bg_inv_md(const BgPanel& p, float g) { return 1.0f / (fmaf(p.lamQ, g, p.lamG) + 1e-12f); }

__device__ __forceinline__ float4 scale4(const float4 v, float s) { return make_float4(v.x * s, v.y * s, v.z * s, v.w * s); }

// four anchor columns of a row (pitch ld), zero past D
__device__ __forceinline__ float4 ld_anchor(const float* __restrict__ Y, int64_t row, int32_t ld, int c, int32_t D) {
  if (c >= D) return f4(0.f);
  float4 v = ld4(Y + (size_t)row * ld + c);  // c < D and c % 4 == 0: the four floats lie inside the row's pitch (>= D rounded up to 4)
  if (c + 1 >= D) v.y = 0.f;
  if (c + 2 >= D) v.z = 0.f;
  if (c + 3 >= D) v.w = 0.f;
  return v;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ double sqdiff4(const float4 a, double sa, const float4 b, double sb) {
  const double dx = (double)a.x * sa - (double)b.x * sb, dy = (double)a.y * sa - (double)b.y * sb;
  const double dz = (double)a.z * sa - (double)b.z * sb, dw = (double)a.w * sa - (double)b.w * sb;
  return dx * dx + dy * dy + dz * dz + dw * dw;
}

}  // namespace
}  // namespace osc

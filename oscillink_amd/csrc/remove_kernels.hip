// Kernels of osc_create_removed: a lattice's top-k lists shrunk from the base's kept lists.
//
//   k_remove_gather_index : where each kept row's anchors live in the base's stored order
//   k_remove_lists        : the kept rows' lists at their new rows, member ids renumbered, removed members emptied
#include "remove.hpp"

namespace osc {
namespace {

__global__ __launch_bounds__(256) void k_remove_gather_index(const int32_t* __restrict__ old_of_new, const int32_t* __restrict__ inv,
                                                             int64_t rows_left, int32_t* __restrict__ from) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= rows_left) return;
  const int32_t o = old_of_new[j];
  from[j] = inv ? inv[o] : o;
}

// One thread per V consecutive entries of the flat n_base x k list arrays (V = 4 where k is a multiple of 4, so a
// thread's entries share a row and both sides move 16 bytes per lane; else 1): adjacent lanes read adjacent entries of
// the source and -- a row's entries stay together, kept rows keep their order -- write adjacent entries of the
// destination.  The map lookups are element gathers from a table of 4 bytes a row, which the caches hold.
template <int V>
__global__ __launch_bounds__(256) void k_remove_lists(const float* __restrict__ kval, const int32_t* __restrict__ kidx, int64_t n_base,
                                                      int32_t k, const int32_t* __restrict__ new_id, float* __restrict__ out_val,
                                                      int32_t* __restrict__ out_idx) {
  const int64_t t = ((int64_t)blockIdx.x * 256 + threadIdx.x) * V;
  if (t >= n_base * k) return;
  const int64_t i = t / k;
  const int32_t e = (int32_t)(t - i * k);
  const int32_t ni = new_id[i];
  if (ni < 0) return;  // a removed row: its list goes nowhere
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
    const int32_t m = (id[u] >= 0 && id[u] < n_base) ? new_id[id[u]] : -1;
    id[u] = m;
    if (m < 0) v[u] = 0.f;
  }
  const int64_t at = (int64_t)ni * k + e;
  if constexpr (V == 4) {
    *reinterpret_cast<int4*>(out_idx + at) = make_int4(id[0], id[1], id[2], id[3]);
    *reinterpret_cast<float4*>(out_val + at) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    out_idx[at] = id[0];
    out_val[at] = v[0];
  }
}

}  // namespace

void launch_remove_gather_index(const int32_t* old_of_new, const int32_t* inv, int64_t rows_left, int32_t* from, hipStream_t s) {
  if (rows_left <= 0) return;
  hipLaunchKernelGGL(k_remove_gather_index, dim3((unsigned)((rows_left + 255) / 256)), dim3(256), 0, s, old_of_new, inv, rows_left, from);
  HIP_CHECK(hipGetLastError());
}

void launch_remove_lists(const float* kval, const int32_t* kidx, int64_t n_base, int32_t k, const int32_t* new_id, float* out_val,
                         int32_t* out_idx, hipStream_t s) {
  if (n_base <= 0 || k <= 0) return;
  const int v = k % 4 == 0 ? 4 : 1;
  const int64_t blocks = ((n_base * k + v - 1) / v + 255) / 256;
  if (blocks >= ((int64_t)1 << 31)) throw std::runtime_error("launch_remove_lists: too many list entries for one launch");
  if (v == 4) hipLaunchKernelGGL(k_remove_lists<4>, dim3((unsigned)blocks), dim3(256), 0, s, kval, kidx, n_base, k, new_id, out_val, out_idx);
  else hipLaunchKernelGGL(k_remove_lists<1>, dim3((unsigned)blocks), dim3(256), 0, s, kval, kidx, n_base, k, new_id, out_val, out_idx);
  HIP_CHECK(hipGetLastError());
}

}  // namespace osc

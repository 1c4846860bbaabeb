// Sweep of k_init_two_steps_stream's launch shapes at the headline size (N = 100 000, D = 768; --n / --d for others): float4
// chunks per lane (a 768-column window as one tile of three chunks or three tiles of one), row groups per wave and trip, and
// the grid as a multiple of the CU count.  Every variant's r2, p3 and x2 are compared with the first one's, byte for byte.
// The kernels are the library's own: this file includes cg_kernels.hip.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I oscillink_amd/csrc scripts/exp/two_steps_stream_sweep.hip -o two_steps_stream_sweep
//   ./two_steps_stream_sweep > profiles/two_steps_stream_sweep.txt
#include "cg_kernels.hip"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace osc;

namespace {

__global__ void k_count_diff(const uint32_t* a, const uint32_t* b, size_t n, unsigned long long* out) {
  unsigned long long c = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) c += a[i] != b[i];
  if (c) atomicAdd(out, c);
}

struct Bufs {
  BlkArgs a{};
  BlkInit ii{};
  BlkInitAp ap{};
  BlkInitAp2 ap2{};
  BlkTwoSteps ts{};
  float *refR = nullptr, *refZ = nullptr, *refX = nullptr;
  unsigned long long* diff = nullptr;
  size_t n = 0;
};

float* dev_random(size_t n, uint32_t seed, float lo, float hi) {
  std::vector<float> h(n);
  uint32_t s = seed * 2654435761u + 12345u;
  for (size_t i = 0; i < n; ++i) {
    s = s * 1664525u + 1013904223u;
    h[i] = lo + (hi - lo) * (float)(s >> 8) * (1.f / 16777216.f);
  }
  float* d = nullptr;
  HIP_CHECK(hipMalloc(&d, n * 4));
  HIP_CHECK(hipMemcpy(d, h.data(), n * 4, hipMemcpyHostToDevice));
  return d;
}
float* dev_zero(size_t n) {
  float* d = nullptr;
  HIP_CHECK(hipMalloc(&d, n * 4));
  HIP_CHECK(hipMemset(d, 0, n * 4));
  return d;
}

template <int LPR, int NCH, int RPT>
void run(Bufs& b, int cus, int per_cu, bool first) {
  const int tile = LPR * 4 * NCH, tiles = (b.a.c1 - b.a.c0 + tile - 1) / tile;
  const dim3 g((unsigned)std::max(1, cus * per_cu / tiles), (unsigned)tiles);
  hipEvent_t e0, e1;
  HIP_CHECK(hipEventCreate(&e0));
  HIP_CHECK(hipEventCreate(&e1));
  auto launch = [&]() { hipLaunchKernelGGL((k_init_two_steps_stream<LPR, NCH, RPT>), g, dim3(256), 0, 0, b.a, b.ii, b.ap, b.ap2, b.ts); };
  for (int i = 0; i < 3; ++i) launch();
  HIP_CHECK(hipDeviceSynchronize());
  std::vector<float> ms(20);
  for (float& m : ms) {
    HIP_CHECK(hipEventRecord(e0, 0));
    launch();
    HIP_CHECK(hipEventRecord(e1, 0));
    HIP_CHECK(hipEventSynchronize(e1));
    HIP_CHECK(hipEventElapsedTime(&m, e0, e1));
  }
  HIP_CHECK(hipGetLastError());
  std::sort(ms.begin(), ms.end());
  unsigned long long nd = 0;
  if (first) {
    HIP_CHECK(hipMemcpy(b.refR, b.ii.R, b.n * 4, hipMemcpyDeviceToDevice));
    HIP_CHECK(hipMemcpy(b.refZ, b.ii.Z, b.n * 4, hipMemcpyDeviceToDevice));
    HIP_CHECK(hipMemcpy(b.refX, b.ii.Xcopy, b.n * 4, hipMemcpyDeviceToDevice));
  } else {
    HIP_CHECK(hipMemset(b.diff, 0, 8));
    for (auto pr : {std::make_pair(b.refR, b.ii.R), std::make_pair(b.refZ, b.ii.Z), std::make_pair(b.refX, b.ii.Xcopy)})
      hipLaunchKernelGGL(k_count_diff, dim3(1024), dim3(256), 0, 0, reinterpret_cast<const uint32_t*>(pr.first),
                         reinterpret_cast<const uint32_t*>(pr.second), b.n, b.diff);
    HIP_CHECK(hipMemcpy(&nd, b.diff, 8, hipMemcpyDeviceToHost));
  }
  HIP_CHECK(hipMemset(b.ii.R, 0xff, b.n * 4));  // (the next variant has to write everything itself)
  HIP_CHECK(hipMemset(b.ii.Z, 0xff, b.n * 4));
  HIP_CHECK(hipMemset(b.ii.Xcopy, 0xff, b.n * 4));
  const double gb = 7.0 * (double)(b.a.N) * (double)(b.a.c1 - b.a.c0) * 4.0 / 1e9;
  printf("<%2d,%d,%d> tiles %d grid %4u x %d (%2d per CU)  median %7.1f us  p10 %7.1f  p90 %7.1f  %5.2f TB/s  %s\n", LPR, NCH, RPT, tiles, g.x,
         tiles, per_cu, ms[10] * 1e3, ms[2] * 1e3, ms[18] * 1e3, gb / ms[10], first ? "reference" : nd ? "DIFFERS" : "same bytes");
  fflush(stdout);
  HIP_CHECK(hipEventDestroy(e0));
  HIP_CHECK(hipEventDestroy(e1));
}

}  // namespace

int main(int argc, char** argv) {
  int N = 100000, D = 768;
  for (int i = 1; i + 1 < argc; i += 2) {
    if (!strcmp(argv[i], "--n")) N = atoi(argv[i + 1]);
    if (!strcmp(argv[i], "--d")) D = atoi(argv[i + 1]);
  }
  if (N < 1 || D < 32 || (D & 31) != 0) return 2;
  hipDeviceProp_t prop;
  HIP_CHECK(hipGetDeviceProperties(&prop, 0));
  const int cus = prop.multiProcessorCount;
  Bufs b;
  b.n = (size_t)N * D;
  b.a.X = dev_random(b.n, 1, -1.f, 1.f);
  b.a.B = dev_random(N, 2, 1.f, 1.f);  // (uniform gates)
  b.a.N = N;
  b.a.ld = D;
  b.a.c0 = 0;
  b.a.c1 = D;
  b.a.cs_const = 1.5f;
  b.a.cs_B = 4.f;
  b.a.cW = 1.f;
  b.ii.R = dev_zero(b.n);
  b.ii.Z = dev_zero(b.n);
  b.ii.Xcopy = dev_zero(b.n);
  b.ii.psi = dev_random(D, 3, -0.05f, 0.05f);
  b.ii.rbU = 1.f;
  b.ii.rbY = 0.5f;
  b.ii.rbB = 4.f;
  b.ii.md_B = 4.f;
  b.ii.md_const = 2.5f;
  b.ii.WY = dev_random(b.n, 4, -0.3f, 0.3f);
  b.ap.WW = dev_random(b.n, 5, -0.1f, 0.1f);
  b.ap.wsum = dev_random(N, 6, 0.9f, 1.1f);
  b.ap2.W3 = dev_random(b.n, 7, -0.05f, 0.05f);
  b.ap2.wsum2 = dev_random(N, 8, 0.9f, 1.1f);
  b.ts.alpha1 = dev_random(D, 9, 0.1f, 0.2f);
  b.ts.alpha2 = dev_random(D, 10, 0.1f, 0.2f);
  b.ts.beta1 = dev_random(D, 11, 0.01f, 0.05f);
  b.ts.beta2 = dev_random(D, 12, 0.01f, 0.05f);
  uint32_t* go = nullptr;
  const uint32_t one = 1u;
  HIP_CHECK(hipMalloc(&go, 4));
  HIP_CHECK(hipMemcpy(go, &one, 4, hipMemcpyHostToDevice));
  b.ts.go = go;
  b.ts.row0 = 0;
  b.refR = dev_zero(b.n);
  b.refZ = dev_zero(b.n);
  b.refX = dev_zero(b.n);
  HIP_CHECK(hipMalloc(&b.diff, 8));
  printf("# k_init_two_steps_stream<LPR, NCH, RPT>, N = %d, D = %d, %s, %d CUs; %.2f GB per launch (4 arrays read, 3 written)\n", N, D,
         prop.gcnArchName, cus, 7.0 * (double)b.n * 4.0 / 1e9);
  bool first = true;
  for (int per_cu : {4, 2, 3, 6, 8, 16}) {
    run<64, 3, 1>(b, cus, per_cu, first);
    first = false;
    run<64, 3, 2>(b, cus, per_cu, false);
    run<64, 1, 1>(b, cus, per_cu, false);
    run<64, 1, 2>(b, cus, per_cu, false);
    run<64, 1, 4>(b, cus, per_cu, false);
    run<64, 2, 1>(b, cus, per_cu, false);
    run<64, 2, 2>(b, cus, per_cu, false);
    run<8, 1, 1>(b, cus, per_cu, false);  // (the blocked form's footprint: a wave is eight rows of one slab)
    run<8, 1, 2>(b, cus, per_cu, false);
    run<8, 1, 4>(b, cus, per_cu, false);
    run<32, 1, 2>(b, cus, per_cu, false);
  }
  // the yardstick under the same conditions: k_update_x_ring<64, 3, 2> in place on x2, two slab-major directions
  {
    XRingArgs xa{};
    xa.X = b.ii.Xcopy;
    xa.P[0] = b.a.X;
    xa.P[1] = b.ii.WY;
    xa.alpha[0] = b.ts.alpha1;
    xa.alpha[1] = b.ts.alpha2;
    xa.M = 2;
    xa.N = N;
    xa.ld = D;
    xa.c1 = D;
    xa.pblk = N;
    hipEvent_t e0, e1;
    HIP_CHECK(hipEventCreate(&e0));
    HIP_CHECK(hipEventCreate(&e1));
    for (int per_cu : {4, 8}) {
      std::vector<float> ms(20);
      for (int i = 0; i < 23; ++i) {
        HIP_CHECK(hipEventRecord(e0, 0));
        hipLaunchKernelGGL((k_update_x_ring<64, 3, 2>), dim3(cus * per_cu), dim3(256), 0, 0, xa);
        HIP_CHECK(hipEventRecord(e1, 0));
        HIP_CHECK(hipEventSynchronize(e1));
        HIP_CHECK(hipEventElapsedTime(&ms[std::max(0, i - 3)], e0, e1));
      }
      std::sort(ms.begin(), ms.end());
      printf("k_update_x_ring<64,3,2> grid %d (%d per CU)  median %7.1f us  %5.2f TB/s (%.2f GB)\n", cus * per_cu, per_cu, ms[10] * 1e3,
             4.0 * (double)b.n * 4.0 / 1e9 / ms[10], 4.0 * (double)b.n * 4.0 / 1e9);
    }
  }
  return 0;
}

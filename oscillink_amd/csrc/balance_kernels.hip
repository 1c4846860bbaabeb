// The rounds of the balanced source-block order ON THE DEVICE (block_balance.hpp has the scheme and the host reference; the
// assignment returned here equals balance_assign's to the element).  Nothing depends on the arrival order of an atomic:
// the only atomics add integers (the displaced-edge count of a round, LDS counters), ranks come from ballots and prefix
// sums in stored-position order.
//
// The whole search is enqueued at once, 5 launches per round, and read back once.  A round that the stop rule cuts off
// is a no-op: every kernel derives "is round t live" from swaps[0 .. t - 1], the rows moved by the rounds before it
// (written by k_bal_exchange), so the host never waits for a round to decide about the next.
//   k_bal_count     cnt[i][.] of every row from scratch (one byte per block in LDS) -> the masks gt / ge, disp[t]
//   k_bal_propose   keeps the best assignment so far (disp[t] below every earlier round's), then the active rows' proposals
//   k_bal_rank      one workgroup per source block walks its stored positions in order: the rank of every proposer
//                   within its (block, target) list, the lists themselves and their lengths
//   k_bal_exchange  the k-th proposers of a -> b and b -> a take each other's position (into newpos); swaps[t]
//   k_bal_commit    pos <- newpos, rowat <- its inverse
#include "block_balance.hpp"
#include "perm.hpp"

#include <vector>

namespace osc {
namespace {

constexpr int kCntStride = 36;  // bytes of LDS per thread for OSC_MAX_SRC_BLOCKS one-byte counters (9 words: no bank conflicts)
constexpr int kRankThreads = 1024;
static_assert(OSC_MAX_SRC_BLOCKS <= 32, "block masks are 32-bit words, the counters 32 bytes per thread");

// round t runs iff no earlier round stopped the search; the recount in front of round t runs iff round t - 1 ran
__device__ inline bool bal_live(const int32_t* swaps, int t, int32_t N) {
  for (int s = 0; s < t; ++s)
    if (host::balance_stops(swaps[s], N)) return false;
  return true;
}
__device__ inline bool bal_recount_live(const int32_t* swaps, int t, int32_t N) { return t == 0 || bal_live(swaps, t - 1, N); }

__global__ void k_bal_init(int32_t* pos, int32_t* rowat, int32_t N) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < N) pos[r] = rowat[r] = r;
}

__global__ void __launch_bounds__(256) k_bal_count(const int32_t* col, const int32_t* deg, int32_t width, int32_t N, int32_t nb, int32_t rpb,
                                                   int32_t slots, const int32_t* pos, uint32_t* gt, uint32_t* ge,
                                                   unsigned long long* disp, const int32_t* swaps, int t) {
  if (!bal_recount_live(swaps, t, N)) return;
  __shared__ uint32_t cw[256 * kCntStride / 4];
  __shared__ unsigned red;
  if (threadIdx.x == 0) red = 0;
  uint32_t* mine = cw + threadIdx.x * (kCntStride / 4);
  for (int q = 0; q < kCntStride / 4; ++q) mine[q] = 0;
  unsigned char* c = reinterpret_cast<unsigned char*>(mine);
  __syncthreads();
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < N) {
    const int32_t* ci = col + (size_t)i * width;
    const int d = deg[i];
    for (int e = 0; e < d; ++e) ++c[min(nb - 1, pos[ci[e]] / rpb)];  // (width <= 255: device_balance_assign)
    uint32_t g = 0, q = 0;
    unsigned excess = 0;
    for (int b = 0; b < nb; ++b) {
      const int v = c[b];
      excess += (unsigned)max(0, v - slots);
      g |= v > slots ? 1u << b : 0u;
      q |= v >= slots ? 1u << b : 0u;
    }
    gt[i] = g;
    ge[i] = q;
    if (excess) atomicAdd(&red, excess);
  }
  __syncthreads();
  if (threadIdx.x == 0 && red) atomicAdd(&disp[t], (unsigned long long)red);
}

__global__ void __launch_bounds__(256) k_bal_propose(const int32_t* col, const int32_t* deg, int32_t width, int32_t N, int32_t nb, int32_t rpb,
                                                     const int32_t* pos, const uint32_t* gt, const uint32_t* ge, int32_t* prop,
                                                     int32_t* best_pos, const unsigned long long* disp, const int32_t* swaps, int t,
                                                     int rounds) {
  if (!bal_recount_live(swaps, t, N)) return;
  __shared__ uint32_t cw[256 * kCntStride / 4];
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= N) return;
  const int32_t pj = pos[j];
  bool better = t == 0;
  if (!better) {
    unsigned long long m = disp[0];
    for (int s = 1; s < t; ++s) m = disp[s] < m ? disp[s] : m;
    better = disp[t] < m;
  }
  if (better) best_pos[j] = pj;
  if (t >= rounds || (t > 0 && host::balance_stops(swaps[t - 1], N))) return;  // no round t
  int32_t choice = -1;
  if (host::balance_active((uint32_t)j, (uint32_t)t)) {
    uint32_t* mine = cw + threadIdx.x * (kCntStride / 4);
    for (int q = 0; q < kCntStride / 4; ++q) mine[q] = 0;
    unsigned char* c = reinterpret_cast<unsigned char*>(mine);
    const int a = min(nb - 1, pj / rpb);
    const int32_t* cj = col + (size_t)j * width;
    const int d = deg[j];
    int out = 0;
    for (int e = 0; e < d; ++e) {
      const int32_t i = cj[e];
      out += (int)((gt[i] >> a) & 1u);
      for (uint32_t m = ge[i]; m; m &= m - 1) ++c[__ffs((int)m) - 1];
    }
    int best_g = 0;
    for (int b = 0; b < nb; ++b)
      if (b != a && out - (int)c[b] > best_g) best_g = out - (int)c[b], choice = b;
  }
  prop[j] = choice;
}

__global__ void __launch_bounds__(kRankThreads) k_bal_rank(int32_t N, int32_t nb, int32_t rpb, const int32_t* rowat, const int32_t* prop,
                                                           int32_t* list, int32_t* rankof, int32_t* cm, const int32_t* swaps, int t) {
  if (!bal_live(swaps, t, N)) return;
  constexpr int kWaves = kRankThreads / 64;
  __shared__ int32_t wcnt[kWaves][OSC_MAX_SRC_BLOCKS];
  __shared__ int32_t run[OSC_MAX_SRC_BLOCKS];
  const int a = blockIdx.x, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int64_t p0 = (int64_t)a * rpb, p1 = min<int64_t>(N, p0 + rpb);
  if (tid < OSC_MAX_SRC_BLOCKS) run[tid] = 0;
  __syncthreads();
  for (int64_t base = p0; base < p1; base += kRankThreads) {  // (uniform trip count: p0, p1 are the workgroup's)
    const int64_t p = base + tid;
    int32_t r = -1, tgt = -1;
    if (p < p1) {
      r = rowat[p];
      tgt = prop[r];
    }
    int myrank = 0;
    for (int b = 0; b < nb; ++b) {
      const unsigned long long m = __ballot(tgt == b);
      if (tgt == b) myrank = __popcll(m & ((1ull << lane) - 1ull));
      if (lane == 0) wcnt[w][b] = __popcll(m);
    }
    __syncthreads();
    if (tgt >= 0) {
      int k = run[tgt] + myrank;
      for (int v = 0; v < w; ++v) k += wcnt[v][tgt];
      list[((size_t)a * nb + tgt) * rpb + k] = r;  // k < rows of block a <= rpb
      rankof[r] = k;
    }
    __syncthreads();
    if (tid < nb) {
      int s = 0;
      for (int v = 0; v < kWaves; ++v) s += wcnt[v][tid];
      run[tid] += s;
    }
    __syncthreads();
  }
  if (tid < nb) cm[a * nb + tid] = run[tid];
}

__global__ void __launch_bounds__(256) k_bal_exchange(int32_t N, int32_t nb, int32_t rpb, const int32_t* pos, const int32_t* prop,
                                                      const int32_t* list, const int32_t* rankof, const int32_t* cm, int32_t* newpos,
                                                      int32_t* swaps, int t) {
  if (!bal_live(swaps, t, N)) return;
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r < N) {
    int32_t np = pos[r];
    const int32_t tgt = prop[r];
    if (tgt >= 0) {
      const int a = min(nb - 1, np / rpb), k = rankof[r];
      if (k < min(cm[a * nb + tgt], cm[tgt * nb + a])) np = pos[list[((size_t)tgt * nb + a) * rpb + k]];
    }
    newpos[r] = np;
  }
  if (blockIdx.x == 0) {  // rows moved by this round (read by the later rounds' kernels only)
    __shared__ int32_t moved;
    if (threadIdx.x == 0) moved = 0;
    __syncthreads();
    for (int q = threadIdx.x; q < nb * nb; q += 256) {
      const int a = q / nb, b = q % nb;
      if (a < b) atomicAdd(&moved, 2 * min(cm[a * nb + b], cm[b * nb + a]));
    }
    __syncthreads();
    if (threadIdx.x == 0) swaps[t] = moved;
  }
}

// (swaps[t] is written by now: live-ness of round t reads the rounds before it only)
__global__ void k_bal_commit(int32_t N, int32_t* pos, int32_t* rowat, const int32_t* newpos, const int32_t* swaps, int t) {
  if (!bal_live(swaps, t, N)) return;
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < N) {
    const int32_t np = newpos[r];
    pos[r] = np;
    rowat[np] = r;
  }
}

}  // namespace

bool device_balance_assign(const int32_t* col, const int32_t* deg, int32_t width, int32_t N, int32_t nb, int32_t slots,
                           std::vector<int32_t>& pos_out, host::BalanceStats& st, hipStream_t s) {
  constexpr int R = host::kBalanceRounds;
  if (N < 1 || nb < 1 || nb > OSC_MAX_SRC_BLOCKS || slots < 1 || width < 1 || width > 255) return false;
  const int32_t rpb = host::blocked_rows_per_block(N, nb);
  const size_t nlist = (size_t)nb * nb * rpb;
  if (nlist >= ((size_t)1 << 30)) return false;
  DevBuf<int32_t> pos, rowat, prop, best, list, rankof, cm, newpos, swaps;
  DevBuf<uint32_t> gt, ge;
  DevBuf<unsigned long long> disp;
  for (DevBuf<int32_t>* b : {&pos, &rowat, &prop, &best, &rankof, &newpos}) b->alloc((size_t)N);
  gt.alloc((size_t)N);
  ge.alloc((size_t)N);
  list.alloc(nlist);
  cm.alloc((size_t)nb * nb);
  swaps.alloc((size_t)R);
  disp.alloc((size_t)R + 1);
  HIP_CHECK(hipMemsetAsync(swaps.p, 0, (size_t)R * 4, s));
  HIP_CHECK(hipMemsetAsync(disp.p, 0, ((size_t)R + 1) * 8, s));
  const dim3 grid((N + 255) / 256), block(256);
  hipLaunchKernelGGL(k_bal_init, grid, block, 0, s, pos.p, rowat.p, N);
  for (int t = 0; t <= R; ++t) {
    hipLaunchKernelGGL(k_bal_count, grid, block, 0, s, col, deg, width, N, nb, rpb, slots, pos.p, gt.p, ge.p, disp.p, swaps.p, t);
    hipLaunchKernelGGL(k_bal_propose, grid, block, 0, s, col, deg, width, N, nb, rpb, pos.p, gt.p, ge.p, prop.p, best.p, disp.p, swaps.p, t, R);
    if (t == R) break;
    hipLaunchKernelGGL(k_bal_rank, dim3(nb), dim3(kRankThreads), 0, s, N, nb, rpb, rowat.p, prop.p, list.p, rankof.p, cm.p, swaps.p, t);
    hipLaunchKernelGGL(k_bal_exchange, grid, block, 0, s, N, nb, rpb, pos.p, prop.p, list.p, rankof.p, cm.p, newpos.p, swaps.p, t);
    hipLaunchKernelGGL(k_bal_commit, grid, block, 0, s, N, pos.p, rowat.p, newpos.p, swaps.p, t);
  }
  HIP_CHECK(hipGetLastError());
  std::vector<int32_t> hs((size_t)R);
  std::vector<unsigned long long> hd((size_t)R + 1);
  pos_out.assign((size_t)N, 0);
  HIP_CHECK(hipMemcpyAsync(hs.data(), swaps.p, (size_t)R * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(hd.data(), disp.p, ((size_t)R + 1) * 8, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipMemcpyAsync(pos_out.data(), best.p, (size_t)N * 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));  // (the buffers above are released behind this)
  st = host::BalanceStats{};
  st.rounds = R;
  for (int t = 0; t < R; ++t)
    if (host::balance_stops(hs[(size_t)t], N)) {
      st.rounds = t + 1;
      break;
    }
  st.swaps.assign(hs.begin(), hs.begin() + st.rounds);
  st.displaced_before = (int64_t)hd[0];
  st.displaced_after = (int64_t)hd[0];
  for (int t = 1; t <= st.rounds; ++t) st.displaced_after = std::min<int64_t>(st.displaced_after, (int64_t)hd[(size_t)t]);
  return true;
}

}  // namespace osc

// Kernels of osc_create_appended: an appended lattice's top-k lists grown from the base's kept lists.
//
//   k_append_gather_rows   : the base's anchors back in API order, into the new handle's row pitch (device to device)
//   k_append_flags         : which old rows cannot be merged (the redo set) and which rows are non-finite
//   k_append_scores_bfly   : scores of many query rows against all columns in the re-scoring's arithmetic
//   k_append_sanitize / k_append_fix_lists : NaN scores never enter a list
//   k_append_merge         : every old row scans its column of the score block for new columns that beat its worst member
#include "append.hpp"

namespace osc {
namespace {

constexpr float NEG = -3.0e38f;

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

__global__ __launch_bounds__(256) void k_append_gather_rows(float* __restrict__ dst, int32_t ld_dst, const float* __restrict__ src,
                                                            int32_t ld_src, const int32_t* __restrict__ from, int64_t rows,
                                                            int32_t cols4) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= rows * cols4) return;
  const int64_t i = t / cols4;
  const int32_t c = (int32_t)(t - i * cols4) * 4;
  const int64_t r = from ? (int64_t)from[i] : i;
  *reinterpret_cast<float4*>(dst + i * ld_dst + c) = ld4(src + r * ld_src + c);
}

// one wave per row
__global__ __launch_bounds__(256) void k_append_flags(const float* __restrict__ Yn, int32_t ldn, int64_t n_old, int64_t rows,
                                                      const float* __restrict__ kval, const int32_t* __restrict__ kidx, int32_t k,
                                                      uint8_t* __restrict__ flags, int32_t* __restrict__ redo_list,
                                                      int32_t* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  bool bad = false;
  const float* y = Yn + row * ldn;
  for (int c = lane * 4; c < ldn; c += 256) {
    const float4 v = ld4(y + c);
    const float t = v.x * 0.f + v.y * 0.f + v.z * 0.f + v.w * 0.f;  // NaN iff one of them is NaN or infinite
    bad = bad || (t != t);
  }
  bad = __ballot(bad) != 0ull;
  bool redo = false;
  if (row < n_old) {
    for (int e = lane; e < k; e += 64) redo = redo || !(kval[row * k + e] > 0.f) || kidx[row * k + e] < 0;
    redo = __ballot(redo) != 0ull || bad;
  }
  if (lane == 0) {
    flags[row] = (uint8_t)((redo ? kAppendRedo : 0) | (bad ? kAppendBad : 0));
    if (redo) redo_list[atomicAdd(counts, 1)] = (int32_t)row;
    if (bad) atomicAdd(counts + 1, 1);
  }
}

// NW waves of four query rows each share a tile of `tj` columns staged in LDS (tj <= 64, tj * ldn * 4 bytes).  The per-pair
// arithmetic is k_rows_scores' / k_knn_rescore's: lane l multiplies the float4 chunks at l * 4 + ch * 256 in order of ch, x y z
// w, by fma into one sum, and the 64 sums are added by the xor butterfly 32, 16, .. 1 (folded over the wave's four rows, see
// below).  A lane keeps the scores of up to four of the tile's columns for one query row, so the tile's scores leave in
// 64-byte runs.
template <int NCH, int NW>
__global__ __launch_bounds__(NW * 64) void k_append_scores_bfly(const float* __restrict__ Yn, int32_t ldn, int32_t cols,
                                                                const int32_t* __restrict__ qrows, int32_t nq,
                                                                float* __restrict__ Sm, int64_t lds_, int32_t tj,
                                                                int32_t cols_per_block) {
  extern __shared__ __attribute__((aligned(16))) float tile[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int q0 = ((int)blockIdx.y * NW + wave) * 4;
  float4 yq[4][NCH];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const float* yi = Yn + (size_t)qrows[min(q0 + u, nq - 1)] * ldn;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int c = lane * 4 + ch * 256;
      yq[u][ch] = c < ldn ? ld4(yi + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  const int jbeg = (int)blockIdx.x * cols_per_block, jend = min(cols, jbeg + cols_per_block);
  for (int j0 = jbeg; j0 < jend; j0 += tj) {
    const int nt = min(tj, jend - j0);
    __syncthreads();  // (the previous tile has been read)
    const int n4 = nt * (ldn / 4);  // the tile's rows are contiguous in Yn: one flat copy
    const float4* src = reinterpret_cast<const float4*>(Yn + (size_t)j0 * ldn);
    for (int t = tid; t < n4; t += NW * 64) reinterpret_cast<float4*>(tile)[t] = src[t];
    __syncthreads();
    float keep[4] = {0.f, 0.f, 0.f, 0.f};  // slot sl: column 16 sl + (lane & 15) of the tile, for query row q0 + (lane >> 4)
#pragma unroll
    for (int sl = 0; sl < 4; ++sl) {
      for (int j16 = 0; j16 < 16 && 16 * sl + j16 < nt; ++j16) {
        const float* yj = tile + (size_t)(16 * sl + j16) * ldn;
        float4 b[NCH];
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
          const int c = lane * 4 + ch * 256;
          b[ch] = c < ldn ? ld4(yj + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        float ss[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          float s = 0.f;
#pragma unroll
          for (int ch = 0; ch < NCH; ++ch) {
            const int c = lane * 4 + ch * 256;
            if (c < ldn) {
              const float4 a = yq[u][ch];
              s = fmaf(a.x, b[ch].x, s);
              s = fmaf(a.y, b[ch].y, s);
              s = fmaf(a.z, b[ch].z, s);
              s = fmaf(a.w, b[ch].w, s);
            }
          }
          ss[u] = s;
        }
        // The four butterflies in 7 exchanges instead of 24: at xor 32 a lane keeps two of the four sums and sends the other
        // two, at xor 16 it keeps one; every addition pairs the same two partial sums as the plain butterfly does on that
        // lane pair (a + b == b + a bit for bit), so each row's total is the plain butterfly's.  Lane l ends with the
        // total of query row q0 + (l >> 4).
        const bool hi = (lane & 32) != 0, mid = (lane & 16) != 0;
        float s0 = hi ? ss[2] : ss[0], s1 = hi ? ss[3] : ss[1];
        const float o0 = hi ? ss[0] : ss[2], o1 = hi ? ss[1] : ss[3];
        s0 += __shfl_xor(o0, 32, 64);
        s1 += __shfl_xor(o1, 32, 64);
        float t = mid ? s1 : s0;
        const float o = mid ? s0 : s1;
        t += __shfl_xor(o, 16, 64);
#pragma unroll
        for (int x = 8; x > 0; x >>= 1) t += __shfl_xor(t, x, 64);
        if ((lane & 15) == j16) keep[sl] = t;
      }
    }
    const int u = lane >> 4;
    if (q0 + u < nq) {
#pragma unroll
      for (int sl = 0; sl < 4; ++sl) {
        const int col = 16 * sl + (lane & 15);
        if (col < nt) Sm[(size_t)(q0 + u) * lds_ + j0 + col] = keep[sl];
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_append_sanitize(float* __restrict__ Sm, int64_t lds_, int32_t nq, int32_t cols) {
  for (int64_t q = blockIdx.y; q < nq; q += gridDim.y)
    for (int c = blockIdx.x * 256 + threadIdx.x; c < cols; c += gridDim.x * 256) {
      const float v = Sm[q * lds_ + c];
      if (v != v) Sm[q * lds_ + c] = NEG;
    }
}

__global__ __launch_bounds__(256) void k_append_fix_lists(const float* __restrict__ Sm, int64_t lds_, const int32_t* __restrict__ qrows,
                                                          int32_t nq, int32_t k, float* __restrict__ kval, int32_t* __restrict__ kidx) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (int64_t)nq * k) return;
  const int64_t q = t / k;
  const size_t at = (size_t)qrows[q] * k + (size_t)(t - q * k);
  const int32_t c = kidx[at];
  if (c >= 0 && !(Sm[q * lds_ + c] > NEG)) {
    kidx[at] = -1;
    kval[at] = 0.f;
  }
}

// a is a worse list entry than b  <=>  smaller score, or equal score and larger index
__device__ __forceinline__ bool worse(float av, int ai, float bv, int bi) { return av < bv || (av == bv && ai > bi); }

// One thread per old row: adjacent threads read adjacent columns of a score row, so the scan -- all the kernel does for
// most rows, M k / N hits are expected per row -- is one coalesced stream over the block.  A row outside the redo set has k
// members with scores > 0 (stored values are true scores then), in any order; a new column's index is above every member's,
// so it enters iff its score is strictly above the worst member's, which it replaces.  NaN compares false and never enters.
__global__ __launch_bounds__(256) void k_append_merge(const float* __restrict__ Sm, int64_t lds_, int32_t qb, int32_t qe,
                                                      int32_t first_col, int32_t n_old, const uint8_t* __restrict__ flags,
                                                      int32_t k, float* __restrict__ kval, int32_t* __restrict__ kidx,
                                                      int32_t* __restrict__ changed) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_old || (flags[i] & kAppendRedo)) return;
  float* v = kval + i * k;
  int32_t* id = kidx + i * k;
  float wv = v[0];
  int wi = id[0], wp = 0;
  for (int e = 1; e < k; ++e)
    if (worse(v[e], id[e], wv, wi)) wv = v[e], wi = id[e], wp = e;
  int hits = 0;
  auto offer = [&](float s, int32_t col) {
    if (!(s > wv)) return;
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
    for (int u = 0; u < 8; ++u) offer(s[u], first_col + (q + u - qb));
  }
  for (; q < qe; ++q) offer(col[(int64_t)q * lds_], first_col + (q - qb));
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

}  // namespace

void launch_append_gather_rows(float* dst, int32_t ld_dst, const float* src, int32_t ld_src, const int32_t* from, int64_t rows,
                               int32_t cols, hipStream_t s) {
  if (rows <= 0 || cols <= 0) return;
  if (cols % 4 != 0 || ld_dst % 4 != 0 || ld_src % 4 != 0) throw std::runtime_error("launch_append_gather_rows: columns and pitches are multiples of 4");
  const int32_t cols4 = cols / 4;
  const int64_t blocks = (rows * cols4 + 255) / 256;
  if (blocks >= ((int64_t)1 << 31)) throw std::runtime_error("launch_append_gather_rows: too many elements for one launch");
  hipLaunchKernelGGL(k_append_gather_rows, dim3((unsigned)blocks), dim3(256), 0, s, dst, ld_dst, src, ld_src, from, rows, cols4);
  HIP_CHECK(hipGetLastError());
}

void launch_append_flags(const float* Yn, int32_t ldn, int64_t n_old, int64_t rows, const float* kval, const int32_t* kidx,
                         int32_t k, uint8_t* flags, int32_t* redo_list, int32_t* counts, hipStream_t s) {
  if (rows <= 0) return;
  hipLaunchKernelGGL(k_append_flags, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, Yn, ldn, n_old, rows, kval, kidx, k, flags,
                     redo_list, counts);
  HIP_CHECK(hipGetLastError());
}

void launch_append_scores_butterfly(const float* Yn, int32_t ldn, int32_t cols, const int32_t* qrows, int32_t nq, float* Sm,
                                    int64_t lds_, int cus, hipStream_t s) {
  if (nq <= 0 || cols <= 0) return;
  const int nch = (ldn + 255) / 256;
  if (nch > 6 || ldn % 4 != 0) throw std::runtime_error("launch_append_scores_butterfly: unit rows wider than 1536 floats");
  const int nw = nch <= 3 ? 16 : 8;  // waves per workgroup: the query rows' registers leave room for 16 up to 768 columns
  const int32_t tj = std::max(1, std::min(64, 12288 / ldn));  // a tile of at most 48 KB
  const int qblocks = (nq + 4 * nw - 1) / (4 * nw);
  const int max_gx = (cols + tj - 1) / tj;
  const int gx = std::max(1, std::min(max_gx, (4 * std::max(1, cus) + qblocks - 1) / qblocks));
  const int32_t cols_per_block = (((cols + gx - 1) / gx + tj - 1) / tj) * tj;
  const dim3 grid((unsigned)((cols + cols_per_block - 1) / cols_per_block), (unsigned)qblocks);
  const size_t shmem = (size_t)tj * ldn * 4;
#define OSC_AS(NN, WW) \
  hipLaunchKernelGGL((k_append_scores_bfly<NN, WW>), grid, dim3(WW * 64), shmem, s, Yn, ldn, cols, qrows, nq, Sm, lds_, tj, cols_per_block)
  if (nch <= 1) OSC_AS(1, 16);
  else if (nch == 2) OSC_AS(2, 16);
  else if (nch == 3) OSC_AS(3, 16);
  else if (nch == 4) OSC_AS(4, 8);
  else OSC_AS(6, 8);
#undef OSC_AS
  HIP_CHECK(hipGetLastError());
}

void launch_append_sanitize(float* Sm, int64_t lds_, int32_t nq, int32_t cols, hipStream_t s) {
  if (nq <= 0 || cols <= 0) return;
  hipLaunchKernelGGL(k_append_sanitize, dim3((unsigned)std::min(1024, (cols + 255) / 256), (unsigned)std::min(nq, 32768)), dim3(256), 0, s, Sm, lds_, nq,
                     cols);
  HIP_CHECK(hipGetLastError());
}

void launch_append_fix_lists(const float* Sm, int64_t lds_, const int32_t* qrows, int32_t nq, int32_t k, float* kval,
                             int32_t* kidx, hipStream_t s) {
  if (nq <= 0) return;
  hipLaunchKernelGGL(k_append_fix_lists, dim3((unsigned)(((int64_t)nq * k + 255) / 256)), dim3(256), 0, s, Sm, lds_, qrows, nq, k, kval,
                     kidx);
  HIP_CHECK(hipGetLastError());
}

void launch_append_merge(const float* Sm, int64_t lds_, int32_t qb, int32_t qe, int32_t first_col, int32_t n_old,
                         const uint8_t* flags, int32_t k, float* kval, int32_t* kidx, int32_t* changed, hipStream_t s) {
  if (qe <= qb || n_old <= 0) return;
  hipLaunchKernelGGL(k_append_merge, dim3((unsigned)(((int64_t)n_old + 255) / 256)), dim3(256), 0, s, Sm, lds_, qb, qe, first_col, n_old, flags,
                     k, kval, kidx, changed);
  HIP_CHECK(hipGetLastError());
}

}  // namespace osc

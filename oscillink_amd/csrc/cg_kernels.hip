// CG hot loop of the lattice settle path, hand-written for gfx950 (wave64, HBM-bound).
//
//   k_spmm      : operator apply  out = (cs_i) x_i - cW sum_j W_ij x_j - cP sum_j Wp_ij x_j   (lattice.py:173-182, 247-255)
//                 fused with the per-column dot product the CG needs next (solver.py:21,25) and, in INIT mode,
//                 with the right-hand side, residual, Jacobi scaling and first search direction (solver.py:19-22).
//   k_update_xr : x += alpha p ; r -= alpha Ap ; column sums of r.r and r.z   (solver.py:27-29, 32-33)
//   k_update_p  : p = z + beta p with z = r / (Md + 1e-12) recomputed          (solver.py:32, 35)
//   k_update_x_ring : x += alpha_1 p_1 + ... + alpha_M p_M from a ring of kept directions, the x update of the solves that
//                 keep one (solver.py:27 applied M iterations at a time, same roundings)
//   k_reduce_*  : deterministic second stage of the column reductions -> alpha, beta, residual
//
// Layout: every N x D array is row-major with pitch ld (multiple of 4 floats) so one wave reads a row as
// 16-byte-per-lane coalesced segments.  LPR lanes cover one row's column window (LPR*4*NCH floats); a wave
// carries 64/LPR rows.  Neighbour ids/weights are read one entry per lane and broadcast with v_readlane
// (LPR == 64: wave-uniform row base -> scalar address + lane offset) or ds_bpermute (LPR < 64).
// Column sums never use atomics: each block keeps per-lane partials in registers over its grid-stride rows,
// folds its 4 waves through LDS and writes one row of part[grid][ld]; a small second kernel finishes in fp64.
#include "common.hpp"
#include "anchor_gram.hpp"
#include <type_traits>

namespace osc {

namespace {

// max that PROPAGATES NaN (fmaxf drops it): a column that diverged to NaN / Inf must reach the stop test as NaN, like
// np.linalg.norm(...).max() of the reference (solver.py:29) -- the solve then runs to max_iters and reports res = NaN.
// The canonical NaN's bit pattern (0x7FC00000) is above every non-negative float's, so the uint atomicMax keeps it.
__device__ __forceinline__ float nanmax(float a, float b) {
  return (a != a || b != b) ? __uint_as_float(0x7FC00000u) : fmaxf(a, b);
}


__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
// streaming store (written once, not re-read by this kernel): keeps the gathered operand's lines in the caches
// (measured on config 3: nontemporal streams took the settle from 8.71 to 8.37 ms)
using v4f = __attribute__((ext_vector_type(4))) float;
__device__ __forceinline__ void st4_stream(float* p, float4 v) {
  const v4f t = {v.x, v.y, v.z, v.w};
  __builtin_nontemporal_store(t, reinterpret_cast<v4f*>(p));
}
using v2f = __attribute__((ext_vector_type(2))) float;
__device__ __forceinline__ void st2_stream(float* p, float a, float b) {
  const v2f t = {a, b};
  __builtin_nontemporal_store(t, reinterpret_cast<v2f*>(p));
}
// streaming load (read once per kernel)
__device__ __forceinline__ float4 ld4_stream(const float* p) {
  const v4f t = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(p));
  return make_float4(t.x, t.y, t.z, t.w);
}
// ... or an ordinary one, by a kernel-uniform flag (UpdateArgs::temporal)
__device__ __forceinline__ float4 ld4_sel(const float* p, bool temporal) { return temporal ? ld4(p) : ld4_stream(p); }
__device__ __forceinline__ void st4_sel(float* p, float4 v, bool temporal) {
  if (temporal) st4(p, v);
  else st4_stream(p, v);
}
__device__ __forceinline__ float4 f4(float v) { return make_float4(v, v, v, v); }
__device__ __forceinline__ float4 fma4(float s, float4 a, float4 c) {
  return make_float4(fmaf(s, a.x, c.x), fmaf(s, a.y, c.y), fmaf(s, a.z, c.z), fmaf(s, a.w, c.w));
}
__device__ __forceinline__ float4 mulacc4(float4 a, float4 b, float4 c) {
  return make_float4(fmaf(a.x, b.x, c.x), fmaf(a.y, b.y, c.y), fmaf(a.z, b.z, c.z), fmaf(a.w, b.w, c.w));
}

// offset of (row, col) in a slab-major array of `rows` rows (32-column slabs)
__device__ __forceinline__ size_t blk_off(int64_t rows, int row, int col) {
  return ((size_t)(col >> 5) * (size_t)rows + (size_t)row) * 32 + (size_t)(col & 31);
}
// offset of the float4 at (row, col) of the search direction P of an update kernel
__device__ __forceinline__ size_t p_off(const UpdateArgs& a, int row, int col) {
  return a.pblk ? blk_off(a.pblk, row, col) : (size_t)row * a.ld + col;
}

template <int LPR>
__device__ __forceinline__ int bcast_i(int v, int sub, int t) {
  if constexpr (LPR == 64) {
    return __builtin_amdgcn_readlane(v, t);
  } else {
    return __shfl(v, sub * LPR + t, 64);
  }
}
template <int LPR>
__device__ __forceinline__ float bcast_f(float v, int sub, int t) {
  return __int_as_float(bcast_i<LPR>(__float_as_int(v), sub, t));
}

// fold per-lane column partials of the 4 waves of a block and write one row of part[grid][ld]
template <int LPR, int NCH>
__device__ __forceinline__ void block_fold(float4 (&dot)[NCH], float* red /*[4][CPW]*/, float* part, int32_t ld,
                                           int32_t c0, int32_t c1) {
  constexpr int CPW = NCH * LPR * 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane / LPR, lr = lane % LPR;
  if constexpr (LPR < 64) {
#pragma unroll
    for (int o = LPR; o < 64; o <<= 1) {
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        dot[ch].x += __shfl_xor(dot[ch].x, o, 64);
        dot[ch].y += __shfl_xor(dot[ch].y, o, 64);
        dot[ch].z += __shfl_xor(dot[ch].z, o, 64);
        dot[ch].w += __shfl_xor(dot[ch].w, o, 64);
      }
    }
  }
  __syncthreads();  // red may still be read by a previous fold
  if (sub == 0) {
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) st4(red + wave * CPW + (ch * LPR + lr) * 4, dot[ch]);
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < CPW; idx += 256) {
    const int col = c0 + idx;
    if (col < c1) part[(size_t)blockIdx.x * ld + col] = (red[idx] + red[CPW + idx]) + (red[2 * CPW + idx] + red[3 * CPW + idx]);
  }
}

constexpr int OSC_SPMM_U1 = 2;
constexpr int OSC_SPMM_U8 = 2;  // 8 lanes per row (xs mode): 8 rows per wave, 2 neighbour rows of each in flight (4 and 8: slower)
template <int NCH>
struct Unroll {  // neighbour rows fetched per batch (all loads in flight together)
  static constexpr int U = NCH == 1 ? OSC_SPMM_U1 : (NCH <= 3 ? 4 : (NCH <= 6 ? 2 : 1));
};

// ---------------------------------------------------------------------------------------------
// UDEEP > 0: that many neighbour rows in flight per row instead (lattices stored in a local row order: their gathers hit
// the XCD's L2, so the apply is bound by how many hits a wave keeps in flight, not by misses -- measured on 1000
// clusters x 100 rows, N = 100k, D = 768: 0.595 ms per apply at 2, 0.490 at 4, 0.450 at 8; on an unstructured lattice
// the extra registers only cost occupancy: 7.81 -> 8.17 ms per settle on the plain path of config 3)
constexpr int OSC_SPMM_UDEEP = 8;
template <int LPR, int NCH, int MODE, int UDEEP = 0>
__global__ __launch_bounds__(256) void k_spmm(const SpmmArgs a) {
  constexpr int RPW = 64 / LPR;
  constexpr int CPW = NCH * LPR * 4;
  constexpr int U = UDEEP > 0 ? UDEEP : (LPR == 8 ? OSC_SPMM_U8 : Unroll<NCH>::U);
  __shared__ __attribute__((aligned(16))) float red[4 * CPW];
  if (a.gate != nullptr && *a.gate <= a.gate_tol) return;  // converged earlier: speculative launch is a no-op
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane / LPR, lr = lane % LPR;
  const int32_t ld = a.ld;
  const bool xs = a.xs != 0;  // workgroup-uniform
  if (xs) {  // this workgroup's row of part[][] is summed over every column by the reduce kernels: clear the columns
             // of the slabs other XCDs own (block_fold's leading barrier orders this against the folds below)
    for (int c = a.c0 + threadIdx.x; c < a.c1; c += 256) a.part[(size_t)blockIdx.x * ld + c] = 0.f;
    if ((int)(blockIdx.x >> 3) >= a.xs) return;  // a.xs workgroups per XCD do the work
  }
  // slab loop: one pass over [c0, c1) normally; in xs mode the slabs x, x+8, ... of this workgroup's XCD
  const int xgroups = xs ? a.xs_groups : 1, xgrp = (int)(blockIdx.x & 7) % xgroups, xpart = (int)(blockIdx.x & 7) / xgroups;
  for (int32_t sc0 = xs ? a.c0 + xgrp * CPW : a.c0; sc0 < a.c1; sc0 += xs ? xgroups * CPW : (1 << 30)) {
  const int32_t sc1 = xs ? min(a.c1, sc0 + CPW) : a.c1;
  int coff[NCH];
  bool cok[NCH];
  float4 psi4[NCH];
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    coff[ch] = sc0 + (ch * LPR + lr) * 4;
    cok[ch] = coff[ch] < sc1;
    psi4[ch] = f4(0.f);
    if (MODE == SPMM_INIT && cok[ch]) psi4[ch] = ld4(a.psi + coff[ch]);
  }
  float4 dot[NCH];
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) dot[ch] = f4(0.f);

  // XCD-aware row order.  Workgroups b and b+8 share an XCD (round-robin dispatch): XCD x = b % 8 takes the x-th
  // eighth of the row range and its workgroups sweep that eighth together, 4*RPW rows per workgroup per step, so at any
  // moment the rows in flight on one XCD form a narrow contiguous window.  On lattices whose row order has locality
  // (clustered anchors) the neighbours of the window are inside it and their rows are re-read from that XCD's 4 MB L2
  // instead of from the fabric; on unstructured graphs the order is irrelevant.  (gridDim.x is a multiple of 8 or < 8.)
  const int64_t span = a.N - a.row0;
  int64_t rbeg, rend, rstep;
  if (xs) {  // the rows of this XCD's part, shared among its workgroups
    const int64_t parts = 8 / xgroups;
    rbeg = a.row0 + span * xpart / parts + (int64_t)(blockIdx.x >> 3) * 4 * RPW;
    rend = a.row0 + span * (xpart + 1) / parts;
    rstep = (int64_t)a.xs * 4 * RPW;
  } else if (gridDim.x >= 8 && (gridDim.x & 7) == 0) {
    const int64_t per_xcd = ((span + 7) / 8 + 4 * RPW - 1) / (4 * RPW) * (4 * RPW);
    const int64_t x0 = a.row0 + (int64_t)(blockIdx.x & 7) * per_xcd;
    rend = min(a.N, x0 + per_xcd);
    rbeg = x0 + (int64_t)(blockIdx.x >> 3) * 4 * RPW;
    rstep = (int64_t)(gridDim.x >> 3) * 4 * RPW;
  } else {
    rbeg = a.row0 + (int64_t)blockIdx.x * 4 * RPW;
    rend = a.N;
    rstep = (int64_t)gridDim.x * 4 * RPW;
  }
  for (int64_t rb = rbeg + (int64_t)wave * RPW; rb < rend; rb += rstep) {
    int row = (int)rb + sub;
    const bool rok = row < rend;
    if (!rok) row = (int)rend - 1;
    if constexpr (LPR == 64) row = __builtin_amdgcn_readfirstlane(row);
    int deg = rok ? a.g.deg[row] : 0;
    if constexpr (LPR == 64) deg = __builtin_amdgcn_readfirstlane(deg);
    int maxdeg = deg;
    if constexpr (LPR < 64) {
#pragma unroll
      for (int o = LPR; o < 64; o <<= 1) maxdeg = max(maxdeg, __shfl_xor(maxdeg, o, 64));
    }
    // operand addressing: row-major, or slab-major in xs mode (one slab per pass: the slab base is loop-invariant)
    const bool xb = LPR == 8 && a.xblk != 0;
    const float* xbase = xb ? a.X + (size_t)(sc0 >> 5) * (size_t)a.xblk * 32 + lr * 4 : a.X + coff[0];
    const size_t xpitch = xb ? 32 : (size_t)ld;
    const float* xrow = xbase + (size_t)row * xpitch;
    float4 xs[NCH], acc[NCH];
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      xs[ch] = cok[ch] ? ld4(xrow + (coff[ch] - coff[0])) : f4(0.f);
      acc[ch] = f4(0.f);
    }
    const int32_t* crow = a.g.col + (size_t)row * a.g.width;
    const float* wrow = a.g.w + (size_t)row * a.g.width;
    // edge lists are fetched NBF batches of LPR entries at a time (all index loads of a row in flight together: with
    // 8 lanes per row a 32-wide ELL row is four batches, and one exposed index latency instead of four)
    constexpr int NBF = LPR == 8 ? 4 : 1;
    for (int e0 = 0; e0 < maxdeg; e0 += LPR * NBF) {
      int cjb[NBF];
      float wjb[NBF];
#pragma unroll
      for (int b = 0; b < NBF; ++b) {
        const int e = e0 + b * LPR + lr;
        cjb[b] = row;
        wjb[b] = 0.f;
        if (e < deg) {
          cjb[b] = crow[e];
          wjb[b] = wrow[e];
        }
      }
#pragma unroll
      for (int b = 0; b < NBF; ++b) {
        const int cnt = min(LPR, maxdeg - e0 - b * LPR);  // <= 0: nothing left (the loop below does not run)
        const int cj = cjb[b];
        const float wj = wjb[b];
        for (int t = 0; t < cnt; t += U) {
          float4 v[U][NCH];
          float wv[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int j = bcast_i<LPR>(cj, sub, t + u);  // t+u <= LPR-1: cnt <= LPR and LPR % U == 0
            wv[u] = bcast_f<LPR>(wj, sub, t + u);
            const float* xj = xbase + (size_t)j * xpitch;
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) v[u][ch] = cok[ch] ? ld4(xj + (coff[ch] - coff[0])) : f4(0.f);
          }
#pragma unroll
          for (int u = 0; u < U; ++u)
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) acc[ch] = fma4(wv[u], v[u][ch], acc[ch]);
        }
      }
    }
    // chain prior rows (a handful): second tiny ELL addressed through path_slot
    float4 accp[NCH];
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) accp[ch] = f4(0.f);
    if (a.g.path_slot != nullptr) {
      const int ps = rok ? a.g.path_slot[row] : -1;
      if (ps >= 0) {
        const int pd = a.g.pdeg[ps];
        for (int e = 0; e < pd; ++e) {
          const int j = a.g.pcol[(size_t)ps * a.g.pwidth + e];
          const float w = a.g.pw[(size_t)ps * a.g.pwidth + e];
          const float* xj = xbase + (size_t)j * xpitch;
#pragma unroll
          for (int ch = 0; ch < NCH; ++ch)
            if (cok[ch]) accp[ch] = fma4(w, ld4(xj + (coff[ch] - coff[0])), accp[ch]);
        }
      }
    }
    if (rok) {
      const float Bi = a.B[row];
      const float cs = fmaf(a.op.cs_B, Bi, a.op.cs_const);
      float invMd = 1.f;
      if (MODE == SPMM_INIT && a.op.precond) invMd = 1.f / (fmaf(a.op.md_B, Bi, a.op.md_const) + 1e-12f);
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        if (!cok[ch]) continue;
        float4 o;
        o.x = cs * xs[ch].x - a.op.cW * acc[ch].x - a.op.cP * accp[ch].x;
        o.y = cs * xs[ch].y - a.op.cW * acc[ch].y - a.op.cP * accp[ch].y;
        o.z = cs * xs[ch].z - a.op.cW * acc[ch].z - a.op.cP * accp[ch].z;
        o.w = cs * xs[ch].w - a.op.cW * acc[ch].w - a.op.cP * accp[ch].w;
        const size_t off = (size_t)row * ld + coff[ch];
        if (MODE == SPMM_AP) {
          st4_stream(a.OUT + off, o);
          dot[ch] = mulacc4(xs[ch], o, dot[ch]);
        } else if (MODE == SPMM_DOT) {
          dot[ch] = mulacc4(xs[ch], o, dot[ch]);
        } else {  // INIT: r = b - A x0 ; z = r / (Md + eps) ; p = z ; rz = sum r.z   (solver.py:19-22)
          // warm-started settle: the rhs term U is the gathered operand itself (x0 = U), already in xs; the stationary
          // solve has no U term at all (rbU = 0) and starts from Y, which is then the gathered operand
          const float4 u = (a.U == a.X) ? xs[ch] : (a.op.rbU != 0.f ? ld4_stream(a.U + off) : f4(0.f));
          const float4 y = (a.Y == a.X) ? xs[ch] : ld4_stream(a.Y + off);
          const float qb = a.op.rbB * Bi;
          float4 r, z;
          r.x = (a.op.rbU * u.x + a.op.rbY * y.x + qb * psi4[ch].x) - o.x;
          r.y = (a.op.rbU * u.y + a.op.rbY * y.y + qb * psi4[ch].y) - o.y;
          r.z = (a.op.rbU * u.z + a.op.rbY * y.z + qb * psi4[ch].z) - o.z;
          r.w = (a.op.rbU * u.w + a.op.rbY * y.w + qb * psi4[ch].w) - o.w;
          z = make_float4(r.x * invMd, r.y * invMd, r.z * invMd, r.w * invMd);
          if (a.OUT != a.X) st4_stream(a.OUT + off, xs[ch]);  // in-place solve (x0 is the work array): nothing to copy
          st4_stream(a.R + off, r);
          st4(a.P + (LPR == 8 && a.pblk != 0 ? blk_off(a.pblk, row, coff[ch]) : off), z);
          dot[ch] = mulacc4(r, z, dot[ch]);
        }
      }
    }
  }
  block_fold<LPR, NCH>(dot, red, a.part, ld, sc0, sc1);
  }  // slab loop
}

// ---------------------------------------------------------------------------------------------
// Operator apply, source-blocked (the CG matvec wherever the XCD-affine slab mode runs: host_logic.hpp, plan_apply).  Measured (scripts/exp/gather_bench.hip, profiles/r02_gather_bench.txt): a CU completes a random
// 128-byte row gather every 2.4 clk when the rows come from <= 3.6 MB per XCD, every 7.0 clk from a 12.8 MB slab -- the
// request rate, not the bytes, is what the plain apply pays for.  Here the neighbour rows are visited block by block:
//   * source rows are cut into nb blocks, nb such that a row has ~3.3 edges into each (4 slots per row and block);
//   * every gathering wave owns a fixed set of row groups (8 rows each, dealt round-robin) per slice of the destination
//     rows and runs  for block b: for my groups: gather the edges that point into b,  the per-row sums staying in
//     registers across the blocks (no partial results through memory); the destination rows are cut into slices so that
//     the rows in flight on an XCD fit its waves' registers.  All waves of an XCD walk the same (slab, slice, block)
//     sequence from the same start, so what they gather from at any time is a few neighbouring blocks rather than the
//     whole slab (L2 hits 25 -> 56 M, misses 58 -> 26 M per launch at config 3);
//   * loads of one wave complete in issue order, so a miss in a gathering wave's stream holds up every L2 hit behind it.
//     Hence two roles per workgroup: waves 0-6 gather (LDS reads and slab rows only), wave 7 copies the next block's edge
//     lists (block-major copy of the graph, BlockedView: always misses) into the other half of an LDS staging area by
//     LDS-DMA while the others gather; one workgroup barrier per block.
// What was tried on top and did not pay (scripts/exp/blocked_apply/README.md): pulling the next block into the L2 with
// dword-per-line loads, gated or not by a progress counter in the XCD's L2 (no change: 877-890 us either way), and
// holding leaders back at that counter (stragglers fall out of the resident set and get later still: 1.8-2.3 ms).
// Same terms per row as k_spmm; the order of summation differs where a row has more than OSC_BLK_SLOTS edges into one
// block (those move to a later block's free slots, launch_blocked_fill): results agree with k_spmm's to fp32 rounding
// of the sums (3e-8 relative on the state).  The chain prior's few rows are applied by k_chain_fix behind this kernel.
// (its kernel shapes: host_logic.hpp, kBlkShapes)

__device__ __forceinline__ float4 ld4_at(const float* base, uint32_t byte_off) {
  return *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(base) + byte_off);
}
__device__ __forceinline__ float ld1_at(const float* base, uint32_t byte_off) {
  return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + byte_off);
}
__device__ __forceinline__ int2 ld2_at(const int2* base, uint32_t byte_off) {
  return *reinterpret_cast<const int2*>(reinterpret_cast<const char*>(base) + byte_off);
}
__device__ __forceinline__ int opaque(int v) {  // a wave-uniform value the optimiser must not fold into hoisted products
  asm volatile("" : "+s"(v));
  return v;
}

struct BlkPhase {  // sub-phase ph = (slab, slice, block): every wave of the XCD walks the same sequence
  int sc0, slice, b;
};

// the slab's column sums of one workgroup: every wave (the list wave with zeros) folds its 8 row lanes, then the waves'
// rows of 32 columns are added in wave order
template <int NW>
__device__ __forceinline__ void blk_fold(float4 dot, float (&red)[NW][32], float* part, int32_t ld, int32_t c0, int32_t c1,
                                         int wave, int lane) {
#pragma unroll
  for (int o = 8; o < 64; o <<= 1) {
    dot.x += __shfl_xor(dot.x, o, 64);
    dot.y += __shfl_xor(dot.y, o, 64);
    dot.z += __shfl_xor(dot.z, o, 64);
    dot.w += __shfl_xor(dot.w, o, 64);
  }
  __syncthreads();  // red may still be read by a previous fold
  if (lane < 8) st4(&red[wave][lane * 4], dot);
  __syncthreads();
  if (threadIdx.x < 32 && c0 + (int)threadIdx.x < c1) {
    float sacc = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) sacc += red[w][threadIdx.x];
    part[(size_t)blockIdx.x * ld + c0 + threadIdx.x] = sacc;
  }
}

// What one workgroup of a blocked launch works on (BlkArgs' geometry): k_init_cached must hand every row to the same
// workgroup, wave and lane as k_apply_blocked does, or its r . z partials would be other sums.  k_apply_blocked keeps the
// same lines in its own prologue: going through this struct there moves its scalar registers about (the loop form's code
// is to stay what three rounds of tuning left).  Change the two together.
struct BlkWork {
  int wgx;              // workgroup within its XCD
  int xgroups, xgrp;    // slab groups, this XCD's: it owns the slabs xgrp, xgrp + xgroups, ...
  int rlo, rhi;         // ... and of those the rows [rlo, rhi)
  int W8;               // rows one "deal" of groups covers (8 per gathering wave of the XCD)
  int slice_rows;       // rows of a destination slice
  int nslab;            // slabs of this XCD
};
template <int CW>
__device__ __forceinline__ BlkWork blk_work(const BlkArgs& a) {
  BlkWork k;
  const int xcd = (int)(blockIdx.x & 7);
  k.wgx = (int)(blockIdx.x >> 3);
  k.xgroups = a.xs_groups;
  k.xgrp = xcd % k.xgroups;
  const int xpart = xcd / k.xgroups, parts = 8 / k.xgroups;
  k.rlo = (int)((int64_t)a.N * xpart / parts);
  k.rhi = (int)((int64_t)a.N * (xpart + 1) / parts);
  k.W8 = a.xs * CW * 8;
  k.slice_rows = k.W8 * a.groups;
  k.nslab = a.c1 - a.c0 > k.xgrp * 32 ? ((a.c1 - a.c0 - k.xgrp * 32 + k.xgroups * 32 - 1) / (k.xgroups * 32)) : 0;
  return k;
}

// One float4 of the INIT pass: from x0's, the rhs anchor term's and the row sum's (acc = sum_j W_ij x0_j) values to
// r = rhs - A x0 and z = M^-1 r (k_init_finish's expressions).  Every product and sum is spelled out in the one form the
// compiler chose for the gathering kernel when the expressions were written infix (a x b - c x d contracts per call site):
// the gathering and the cached INIT pass must agree to the bit.
__device__ __forceinline__ void blk_init_row(const BlkArgs& a, const BlkInit& ii, float b, float4 x, float4 y, float4 acc,
                                             float4 psi4, float4& r, float4& z) {
  const float cs = fmaf(a.cs_B, b, a.cs_const);
  const float qb = __fmul_rn(ii.rbB, b);
  const float invMd = 1.f / (fmaf(ii.md_B, b, ii.md_const) + 1e-12f);  // (no preconditioner: md_B = 0, md_const = 1)
  auto one = [&](float xv, float yv, float av, float pv) {
    const float o = fmaf(cs, xv, -__fmul_rn(a.cW, av));                                  // (cs + ...) x - cW sum W x
    const float rhs = fmaf(pv, qb, fmaf(ii.rbU, xv, __fmul_rn(ii.rbY, yv)));             // rbU x + rbY y + rbB B psi
    return __fsub_rn(rhs, o);
  };
  r = make_float4(one(x.x, y.x, acc.x, psi4.x), one(x.y, y.y, acc.y, psi4.y), one(x.z, y.z, acc.z, psi4.z),
                  one(x.w, y.w, acc.w, psi4.w));
  z = make_float4(__fmul_rn(invMd, r.x), __fmul_rn(invMd, r.y), __fmul_rn(invMd, r.z), __fmul_rn(invMd, r.w));
}

// INIT (BlkInit): the solve's initial residual in the same launch.  X holds x0 slab-major, and where a row's sums are
// complete the epilogue forms r = rhs - A x0 with rhs = rbU x0 + rbY y + rbB B psi (y = ii.Y's row, or x0 itself: the
// warm-started settle, whose rhs state term IS x0, and the U* solve, which starts from Y and has no state term),
// z = M^-1 r, stores r row-major and z SLAB-MAJOR into ii.Z -- the first search direction, in the array the caller uses
// as P from here on --, copies x0 into the solution array where that is another one, and the column sums are those of
// r . z.  Saves the separate pass over A x0, x0, y, r, p (k_init_finish: five array passes) for one more row read or
// write here.
// PD: gather rounds a wave keeps in flight (round 5).  A wave's loads return in issue order and about a fifth of the gathers
// miss the L2, so a round of 32 lines practically always waits for one fabric round trip: with one round in flight the
// kernel is bound by bytes in flight / miss latency.  PD > 1 issues round g + PD - 1 before it consumes round g (the
// slots' weights and the gathered rows of PD rounds in registers).  WPE: waves per SIMD the register budget is set for.
// WY (INIT only): the pass also stores every row's sum (acc, as it enters the epilogue's arithmetic) slab-major into ii.WY:
// the operand of k_init_cached, which serves the later solves from the same x0 on the same graph copy.  That form takes
// no separate rhs term (ii.Y == nullptr: y is x0), so the y rows' registers pay for the store.
// FUSED (BlkFused in BlkInit's place; not with INIT): iteration 3 of an anchor start whose alpha3 and beta3 were known before the
// launch (k_anchor_gram_scalars, three_steps).  Gather rounds, list wave and phases are the loop form's; the epilogue also
// fetches the row of r2 (streamed, with the own-row loads), loads the slab's four alpha3 and beta3 per lane, forms o = A p3 as
// the loop form does, r3 = r2 - alpha3 o as k_update_xr does and p4 = z3 + beta3 p3 as k_update_p does (p3: the own row, in
// hand for the diagonal term), and stores r3 over r2 and p4 slab-major.  o is never stored, and with nothing to sum there is no
// fold: the two streaming passes and the two column reductions between matvec 3 and matvec 4 are gone.
// FMODE == 2 (FUSED_LAST): the same iteration where the solve is known to end in iteration 4 and alpha4 is out as well (four_steps).
// The epilogue fetches the row of x3 as a third stream, forms r3 and p4 with the FUSED form's expressions in registers only and
// stores x4 = x3 + alpha4 p4 (k_update_x_ring's fmaf) over x3: nothing else is written, and iteration 4 has no launch at all.
// FMODE == 3 (the folded last form, BlkFused::go_fold): that x4 is affine in the gathered row sum, and the INIT pass, which runs
// behind alpha3, beta3 and alpha4, has stored everything else of it as e in x's place (two_steps_elem).  The epilogue streams the
// row of e -- no own row of p3, no r2 -- and stores x4 = e + ((alpha4 alpha3) (M^-1 cW)) acc over it: one row in, one row out, as
// the loop form, and like it in batches of that form's width.
#ifndef OSC_FOLD_EC_WIDE
#define OSC_FOLD_EC_WIDE 4
#endif
#ifndef OSC_FOLD_EC_NARROW
#define OSC_FOLD_EC_NARROW 2
#endif
template <int GM, int CW, bool INIT = false, int PD = 1, int WPE = 4, bool WY = false, int FMODE = 0>
__global__ __launch_bounds__((CW + 1) * 64) __attribute__((amdgpu_waves_per_eu(WPE, WPE))) void k_apply_blocked(
    const BlkArgs a, const std::conditional_t<FMODE != 0, BlkFused, BlkInit> ii) {
  constexpr bool FUSED = FMODE != 0, LAST = FMODE == 2, FOLD = FMODE == 3;
  static_assert(INIT || !WY, "only the INIT pass stores the row sums");
  static_assert(!(INIT && FUSED), "the fused form is an iteration, not the INIT pass");
  constexpr int SL = OSC_BLK_SLOTS, NT = (CW + 1) * 64;
  __shared__ __attribute__((aligned(16))) float red[CW + 1][32];
  // per gathering wave: the slots of each of its rows in the current block, and (other half) in the next one
  __shared__ __attribute__((aligned(16))) int2 stage[2][GM][CW][8 * SL];
  if constexpr (!INIT) {  // (the INIT pass is never speculative)
    if (a.gate != nullptr && *a.gate <= a.gate_tol) return;
  }
  if constexpr (FUSED) {
    if (*ii.go != 1u) return;
  }
  if constexpr (FOLD) {
    if (*ii.go_fold != 1u) return;  // (the INIT pass stored e only under this word)
  }
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int sub = lane >> 3, lr = lane & 7;
  const int32_t ld = a.ld;
  if constexpr (!FUSED) {
    for (int c = a.c0 + threadIdx.x; c < a.c1; c += NT) a.part[(size_t)blockIdx.x * ld + c] = 0.f;
  }
  if ((int)(blockIdx.x >> 3) >= a.xs) return;
  const int xcd = (int)(blockIdx.x & 7), wgx = (int)(blockIdx.x >> 3);  // (blk_work's arithmetic, spelled out: see there)
  const int xgroups = a.xs_groups, xgrp = xcd % xgroups, xpart = xcd / xgroups, parts = 8 / xgroups;
  const int rlo = (int)((int64_t)a.N * xpart / parts), rhi = (int)((int64_t)a.N * (xpart + 1) / parts);
  const int nb = a.nb, ng = a.groups;
  const int W8 = a.xs * CW * 8;  // rows one "deal" of groups covers (8 per gathering wave of the XCD)
  const int slice_rows = W8 * ng;
  const int nslab = a.c1 - a.c0 > xgrp * 32 ? ((a.c1 - a.c0 - xgrp * 32 + xgroups * 32 - 1) / (xgroups * 32)) : 0;
  const int per_slab = a.slices * nb, nphase = nslab * per_slab;
  auto phase = [&](int ph) {
    BlkPhase p;
    const int q = ph / per_slab, r = ph - q * per_slab;
    p.sc0 = a.c0 + (xgrp + q * xgroups) * 32;
    p.slice = r / nb;
    p.b = r - p.slice * nb;
    return p;
  };
  auto slab_base = [&](int sc0) { return a.X + (size_t)(sc0 >> 5) * (size_t)a.N * 32; };

  if (wave == CW) {
    // ---- the last wave: the edge lists --------------------------------------------------------------------------------
    // For a fixed group index g the slot rows of the workgroup's CW gathering waves are 8 * CW consecutive lattice rows, i.e.
    // one contiguous piece of the block-major copy (and of the staging area, laid out [g][wave][row][slot]): it is copied
    // global -> LDS by LDS-DMA loads of 1 KB per instruction, no registers in between, ALL pieces of a sub-phase in flight
    // together (the loads always miss; under the gathers' traffic every dependent round trip costs several microseconds).
    // A group that starts inside the lattice but runs past its end (or past the slice) copies whatever follows in the
    // array -- other rows' valid slots, or the zeroed padding behind the last block (blocked_view: >= 8 * CW rows) -- and
    // the sums of such rows are never stored; a group that starts past the end is skipped here AND by the gathering waves.
    constexpr int GROUP_BYTES = CW * 8 * SL * 8, PIECES = (GROUP_BYTES + 1023) / 1024;
    static_assert(GM * PIECES <= 60, "outstanding vector-memory operations of one wave");
    const unsigned stage_lds = (unsigned)(size_t)&stage[0][0][0][0];
    auto fetch_slots = [&](int ph) {
      const BlkPhase p = phase(ph);
      const char* sb = reinterpret_cast<const char*>(a.slots + (size_t)p.b * (size_t)a.N * SL);
      const int row0 = rlo + p.slice * slice_rows + ((wgx * CW) << 3);
      const int w8 = opaque(W8);
#pragma unroll
      for (int g = 0; g < GM; ++g) {
        const bool inside = g < ng && row0 + g * w8 < a.N;
        if (PD == 1 && !inside) continue;  // (a group that starts past the lattice: nobody reads its area)
        // PD > 1: the gather rounds carry no tests at all, so every group's area is staged -- one that does not exist from the
        // zeroed padding behind the last block ({row 0, 0.0f}: one line for the whole wave, a product with zero)
        const char* src = inside ? sb + (size_t)(uint32_t)(row0 + g * w8) * (8u * SL)
                                 : reinterpret_cast<const char*>(a.slots + (size_t)nb * (size_t)a.N * SL);
        const unsigned dst = __builtin_amdgcn_readfirstlane(stage_lds + (unsigned)(((ph & 1) * GM + g) * GROUP_BYTES));
#pragma unroll
        for (int q = 0; q < PIECES; ++q) {
          if (q * 1024 + lane * 16 < GROUP_BYTES) {
            const char* lsrc = src + lane * 16;  // (the instruction's offset advances the global AND the LDS address)
            unsigned keep;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off offset:%3\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep)
                         : "v"(lsrc), "s"(dst), "n"(q * 1024)
                         : "memory");
          }
        }
      }
    };
    if (nphase > 0) fetch_slots(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int ph = 0; ph < nphase; ++ph) {
      if (ph + 1 < nphase) fetch_slots(ph + 1);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if constexpr (!FUSED) {
        if ((ph + 1) % per_slab == 0) {
          const int sc0 = phase(ph).sc0;
          blk_fold<CW + 1>(f4(0.f), red, a.part, ld, sc0, min(a.c1, sc0 + 32), wave, lane);
        }
      }
    }
    return;
  }

  // ---- the other waves: gather (L2 hits and LDS reads) ---------------------------------------------------------------
  const uint32_t lr16 = (uint32_t)lr * 16u;
  float4 acc[GM];
  float4 dot[1] = {f4(0.f)};
  __syncthreads();
  for (int ph = 0; ph < nphase; ++ph) {
    const BlkPhase p = phase(ph);
    const bool cok = p.sc0 + lr * 4 < a.c1;
    const float* xbase = slab_base(p.sc0);
    if (p.b == 0) {
#pragma unroll
      for (int g = 0; g < GM; ++g) acc[g] = f4(0.f);
    }
    const int2(*st)[CW][8 * SL] = stage[ph & 1];
    // One group per round: all slots of its 8 rows in flight together.  No tests in here: an unused slot holds {first row of
    // the block, 0.0f} (k_blk_fill, stage_slots), i.e. a gather of a line everybody has and a product with zero -- the
    // round is bound by instruction issue (four waves share a SIMD), and a compare + exec-mask + branch per slot cost
    // more than the fifth of the gathers they saved.
    const int wg_row0 = rlo + p.slice * slice_rows + ((wgx * CW) << 3);  // first row of this workgroup's group 0
    if constexpr (PD == 1) {
#pragma unroll
      for (int g = 0; g < GM; ++g) {
        if (g >= ng || wg_row0 + g * W8 >= a.N) continue;  // (same test as the list wave's: that area was not staged)
        int2 e[SL];
        float4 v[SL];
#pragma unroll
        for (int u = 0; u < SL; ++u) e[u] = st[g][wave][sub * SL + u];
#pragma unroll
        for (int u = 0; u < SL; ++u) v[u] = ld4_at(xbase, (uint32_t)e[u].x * 128u + lr16);
#pragma unroll
        for (int u = 0; u < SL; ++u) acc[g] = fma4(__int_as_float(e[u].y), v[u], acc[g]);
      }
    } else {
      // PD rounds in flight, straight-line: round g + PD - 1 is issued (slots from LDS, four row gathers per lane) before
      // round g is consumed, so the compiler's counted waits leave SL * (PD - 1) loads in flight in the steady state.
      // No test per group: the list wave staged every group's area (see there).
      typedef float f32x4 __attribute__((ext_vector_type(4)));  // (a native vector: one 128-bit operand of the asm below)
      f32x4 v[PD][SL];
      float w[PD][SL];
      auto issue = [&](int g, f32x4 (&vv)[SL], float (&ww)[SL]) {
        int2 e[SL];
#pragma unroll
        for (int u = 0; u < SL; ++u) e[u] = st[g][wave][sub * SL + u];
#pragma unroll
        for (int u = 0; u < SL; ++u)
          vv[u] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(xbase) + ((uint32_t)e[u].x * 128u + lr16));
#pragma unroll
        for (int u = 0; u < SL; ++u) ww[u] = __int_as_float(e[u].y);
      };
#pragma unroll
      for (int j = 0; j < PD - 1 && j < GM; ++j) issue(j, v[j % PD], w[j % PD]);
#pragma unroll
      for (int g = 0; g < GM; ++g) {
        if (g + PD - 1 < GM) issue(g + PD - 1, v[(g + PD - 1) % PD], w[(g + PD - 1) % PD]);
        // round g's rows pass through an empty asm with a memory clobber: its sums can start only here (behind the
        // issue of round g + PD - 1), and a later round's loads cannot be moved up past it
#pragma unroll
        for (int u = 0; u < SL; ++u) asm volatile("" : "+v"(v[g % PD][u])::"memory");
#pragma unroll
        for (int u = 0; u < SL; ++u) {
          const f32x4 t = v[g % PD][u];
          acc[g] = fma4(w[g % PD][u], make_float4(t.x, t.y, t.z, t.w), acc[g]);
        }
        // ... and end here (volatile asm statements keep their order): otherwise the compiler may postpone the sums of
        // all rounds and park the gathered rows in scratch memory meanwhile
        asm volatile("" : "+v"(acc[g].x), "+v"(acc[g].y), "+v"(acc[g].z), "+v"(acc[g].w));
      }
    }
    if (p.b == nb - 1) {  // the rows of this slice are complete: the rest of long lists, diagonal term, output, p.Ap
      const int w8 = opaque(W8);
      const int row_first = rlo + p.slice * slice_rows + ((wgx * CW + wave) << 3) + sub;
      // Own rows / gates / rest descriptors of EC groups at a time (these loads miss).  Loads and stores of a wave retire
      // in issue order, so the loads of batch k + 1 are issued BEFORE the stores of batch k: otherwise every batch would
      // also wait for the previous batch's stores to be acknowledged.
      // (FUSED: the r rows are a second stream per group, as the y rows are for INIT)
      // (FOLD: one stream, the loop form's width; OSC_FOLD_EC_WIDE / _NARROW: A/B builds of that choice)
      constexpr int EC = FOLD ? (WPE <= 2 ? OSC_FOLD_EC_WIDE : OSC_FOLD_EC_NARROW) : FUSED ? (WPE <= 2 ? 2 : 1) : WPE <= 2 ? 4 : INIT ? 1 : 2, NBATCH = (GM + EC - 1) / EC;  // (INIT: the y rows take the second group's registers; two groups: 72 spills)
      constexpr int YC = (INIT && !WY) || (FUSED && !FOLD) ? EC : 1;
      float4 xs[2][EC];    // (FOLD: the rows of e, not the own rows of the operand)
      float4 ys[2][YC];    // (FUSED: the rows of r2)
      [[maybe_unused]] float4 x3s[2][LAST ? EC : 1];  // (FUSED_LAST: the rows of x3)
      int2 rr[2][EC];
      float bv[2][EC];
      float4 psi4 = f4(0.f);
      float* zbase = nullptr;
      float* wybase = nullptr;
      const uint32_t ldb = (uint32_t)ld * 4u, cb = (uint32_t)(p.sc0 + lr * 4) * 4u;
      // (INIT: the 14 dwords of `ii` cost the kernel 22 scalar-register spills into vector lanes; reading them from the
      // kernel-argument segment here, per closing sub-phase, was tried -- 12 spills, the same 700 us at config 3)
      if constexpr (INIT) {
        if (cok) psi4 = ld4(ii.psi + p.sc0 + lr * 4);
        zbase = ii.Z + (size_t)(p.sc0 >> 5) * (size_t)a.N * 32;
        if constexpr (WY) wybase = ii.WY + (size_t)(p.sc0 >> 5) * (size_t)a.N * 32;
      }
      [[maybe_unused]] float4 al4 = f4(0.f), be4 = f4(0.f), aln = f4(0.f);
      if constexpr (FUSED) {
        if (cok) al4 = ld4(ii.alpha + p.sc0 + lr * 4);
        if constexpr (!FOLD) {
          if (cok) be4 = ld4(ii.beta + p.sc0 + lr * 4);
        }
        if constexpr (FOLD) {  // g = alpha4 alpha3 of the lane's four columns, in al4's registers
          if (cok) aln = ld4(ii.alpha_last + p.sc0 + lr * 4);
          al4 = make_float4(__fmul_rn(aln.x, al4.x), __fmul_rn(aln.y, al4.y), __fmul_rn(aln.z, al4.z), __fmul_rn(aln.w, al4.w));
        } else if constexpr (LAST) {
          if (cok) aln = ld4(ii.alpha_last + p.sc0 + lr * 4);
        } else {
          zbase = ii.Pout + (size_t)(p.sc0 >> 5) * (size_t)a.N * 32;
        }
      }
      auto fetch = [&](int k, float4 (&x)[EC], float4 (&y)[YC], int2 (&r)[EC], float (&bb)[EC],
                       float4 (&xl)[LAST ? EC : 1]) {
#pragma unroll
        for (int i = 0; i < EC; ++i) {
          const int g = k * EC + i, row = row_first + g * w8;
          x[i] = f4(0.f);
          r[i] = make_int2(0, 0);
          bb[i] = 0.f;
          if constexpr ((INIT && !WY) || (FUSED && !FOLD)) y[i] = f4(0.f);
          if constexpr (LAST) xl[i] = f4(0.f);
          if (g < GM && g < ng && row < rhi && cok) {
            if constexpr (FOLD) x[i] = ld4_stream(reinterpret_cast<const float*>(reinterpret_cast<const char*>(ii.X) + ((uint32_t)row * ldb + cb)));
            else x[i] = ld4_at(xbase, (uint32_t)row * 128u + lr16);
            r[i] = ld2_at(a.rest, (uint32_t)row * 8u);  // edges beyond SL per block: {first, count}, ascending columns
            bb[i] = ld1_at(a.B, (uint32_t)row * 4u);
            if constexpr (INIT && !WY) {  // (byte offsets of a row-major array fit 32 bits: launch_apply_blocked checks N * ld)
              if (ii.Y != nullptr) y[i] = ld4_stream(reinterpret_cast<const float*>(reinterpret_cast<const char*>(ii.Y) + ((uint32_t)row * ldb + cb)));
            }
            if constexpr (FUSED && !FOLD) y[i] = ld4_stream(reinterpret_cast<const float*>(reinterpret_cast<const char*>(ii.R) + ((uint32_t)row * ldb + cb)));
            if constexpr (LAST) xl[i] = ld4_stream(reinterpret_cast<const float*>(reinterpret_cast<const char*>(ii.X) + ((uint32_t)row * ldb + cb)));
          }
        }
      };
      fetch(0, xs[0], ys[0], rr[0], bv[0], x3s[0]);
#pragma unroll
      for (int k = 0; k < NBATCH; ++k) {
        if (k + 1 < NBATCH) fetch(k + 1, xs[(k + 1) & 1], ys[(k + 1) & 1], rr[(k + 1) & 1], bv[(k + 1) & 1], x3s[(k + 1) & 1]);
#pragma unroll
        for (int i = 0; i < EC; ++i) {
          const int g = k * EC + i, row = row_first + g * w8;
          if (g >= GM) continue;
          if (g >= ng || row >= rhi || !cok) continue;
          for (int e = 0; e < rr[k & 1][i].y; ++e) {
            const int2 en = ld2_at(a.over, (uint32_t)(rr[k & 1][i].x + e) * 8u);
            acc[g] = fma4(__int_as_float(en.y), ld4_at(xbase, (uint32_t)en.x * 128u + lr16), acc[g]);
          }
          if constexpr (INIT) {
            const float4 x = xs[k & 1][i];
            float4 y = x;
            if constexpr (!WY) y = ii.Y != nullptr ? ys[k & 1][i] : x;
            if constexpr (WY) {
              // in two halves: the sums live in register pairs, and one 16-byte store wants every group's moved into a quad first
              // (20+ registers, spills in the widest shapes).  The second offset is opaque so that the halves are not merged again.
              uint32_t lo = (uint32_t)row * 128u + lr16, hi = lo + 8u;
              asm volatile("" : "+v"(hi));
              st2_stream(reinterpret_cast<float*>(reinterpret_cast<char*>(wybase) + lo), acc[g].x, acc[g].y);
              st2_stream(reinterpret_cast<float*>(reinterpret_cast<char*>(wybase) + hi), acc[g].z, acc[g].w);
            }
            float4 r, z;
            blk_init_row(a, ii, bv[k & 1][i], x, y, acc[g], psi4, r, z);
            st4_stream(reinterpret_cast<float*>(reinterpret_cast<char*>(ii.R) + ((uint32_t)row * ldb + cb)), r);
            if (ii.Xcopy != nullptr) st4_stream(reinterpret_cast<float*>(reinterpret_cast<char*>(ii.Xcopy) + ((uint32_t)row * ldb + cb)), x);
            st4(reinterpret_cast<float*>(reinterpret_cast<char*>(zbase) + ((uint32_t)row * 128u + lr16)), z);
            dot[0] = mulacc4(r, z, dot[0]);
          } else if constexpr (FOLD) {
            const float invMd = 1.f / (fmaf(ii.md_B, bv[k & 1][i], ii.md_const) + 1e-12f);
            const float hq = __fmul_rn(invMd, a.cW);
            float4 xn = xs[k & 1][i];  // e
            xn.x = fmaf(__fmul_rn(al4.x, hq), acc[g].x, xn.x);
            xn.y = fmaf(__fmul_rn(al4.y, hq), acc[g].y, xn.y);
            xn.z = fmaf(__fmul_rn(al4.z, hq), acc[g].z, xn.z);
            xn.w = fmaf(__fmul_rn(al4.w, hq), acc[g].w, xn.w);
            st4_stream(reinterpret_cast<float*>(reinterpret_cast<char*>(ii.X) + ((uint32_t)row * ldb + cb)), xn);
          } else if constexpr (FUSED) {
            const float bq = bv[k & 1][i];
            const float cs = fmaf(a.cs_B, bq, a.cs_const);
            const float invMd = 1.f / (fmaf(ii.md_B, bq, ii.md_const) + 1e-12f);
            const float4 x = xs[k & 1][i];
            float4 r = ys[k & 1][i], pn;
            auto one = [&](float xv, float av, float al, float be, float& rv, float& pv) {
              const float o = fmaf(cs, xv, -__fmul_rn(a.cW, av));  // (the loop form's o, in the form blk_init_row records)
              rv = fmaf(-o, al, rv);                               // k_update_xr
              pv = fmaf(xv, be, __fmul_rn(rv, invMd));             // k_update_p
            };
            one(x.x, acc[g].x, al4.x, be4.x, r.x, pn.x);
            one(x.y, acc[g].y, al4.y, be4.y, r.y, pn.y);
            one(x.z, acc[g].z, al4.z, be4.z, r.z, pn.z);
            one(x.w, acc[g].w, al4.w, be4.w, r.w, pn.w);
            if constexpr (LAST) {
              float4 xn = x3s[k & 1][i];
              xn.x = fmaf(pn.x, aln.x, xn.x);  // k_update_x_ring
              xn.y = fmaf(pn.y, aln.y, xn.y);
              xn.z = fmaf(pn.z, aln.z, xn.z);
              xn.w = fmaf(pn.w, aln.w, xn.w);
              st4_stream(reinterpret_cast<float*>(reinterpret_cast<char*>(ii.X) + ((uint32_t)row * ldb + cb)), xn);
            } else {
              st4_stream(reinterpret_cast<float*>(reinterpret_cast<char*>(ii.R) + ((uint32_t)row * ldb + cb)), r);
              st4(reinterpret_cast<float*>(reinterpret_cast<char*>(zbase) + ((uint32_t)row * 128u + lr16)), pn);
            }
          } else {
            const float cs = fmaf(a.cs_B, bv[k & 1][i], a.cs_const);
            float4 o;
            o.x = cs * xs[k & 1][i].x - a.cW * acc[g].x;
            o.y = cs * xs[k & 1][i].y - a.cW * acc[g].y;
            o.z = cs * xs[k & 1][i].z - a.cW * acc[g].z;
            o.w = cs * xs[k & 1][i].w - a.cW * acc[g].w;
            st4_stream(a.OUT + ((size_t)(uint32_t)row * (uint32_t)ld + (uint32_t)(p.sc0 + lr * 4)), o);
            dot[0] = mulacc4(xs[k & 1][i], o, dot[0]);
          }
        }
      }
    }
    __syncthreads();
    if constexpr (!FUSED) {
      if ((ph + 1) % per_slab == 0) {  // the slab's column sums
        blk_fold<CW + 1>(dot[0], red, a.part, ld, p.sc0, min(a.c1, p.sc0 + 32), wave, lane);
        dot[0] = f4(0.f);
      }
    }
  }
}

// The INIT pass of a solve whose x0 has its row sums cached (BlkInit::WY, left by the storing form of
// k_apply_blocked<.., INIT> for the same x0, graph copy and block count): that kernel's epilogue with acc streamed in
// instead of gathered.  Same r, z, x0 copy and r . z partials to the bit, which takes the same arithmetic (blk_init_row),
// the same row -> (workgroup, wave, lane) mapping (blk_work) and the same order of every lane's sum: per slab its rows
// ascending -- the slices' groups are one arithmetic sequence of rows, slice_rows = W8 x groups, so slices and groups
// fold into one index here -- then blk_fold over the workgroup's waves.  The last wave, the gathering kernel's list
// wave, only takes part in the fold (with zeros, as there).  No x0 other than the rhs anchor term (ii.Y == nullptr).
// Every stream is read once: batches of EC groups per wave (EC KB each of x0 and of the sums), the next batch requested
// before the current one is consumed.
__device__ __forceinline__ float4 ld4_stream_at(const float* base, uint32_t byte_off) {
  return ld4_stream(reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + byte_off));
}
// AP (BlkInitAp, the anchor start under uniform gates): the pass also emits iteration 1's operator output.  The first
// direction is p1 = z0 = m (qb psi + u Y + cW WY) with per-row scalars m = 1 / Md, qb = rbB b, u = rbU + rbY - cs, so
// (W p1)_i = m (qb s_i psi + u WY_i + cW WWY_i) with s = W 1 and WWY = W (W Y), both cached (L::Wsum, L::WWs), and
// A p1 = cs z0 - cW W p1 is streamed here instead of gathered: one more row read (WWY, row-major), one more row written
// (A p1, row-major), the column sums of p1 . A p1 into ap.part beside those of r . z.  r, z, the x0 copy and the r . z sums
// are the other form's to the bit; the new products and sums are spelled out so that no call site contracts them its own way.
// AP == 2 (BlkInitAp2): ... and T = A (A p1) for iteration 2, by the same algebra one level up: with s2 = W s and W3Y = W WWY
// (L::Wsum2, L::W3s), (W W p1)_i = m (qb s2_i psi + u WWY_i + cW W3Y_i), W Q1 = cs W p1 - cW W W p1, T = cs Q1 - cW W Q1.
// One more row read (W3Y), one more row written (T, row-major); everything the AP == 1 form writes keeps its bits.
template <int CW, int AP>
__device__ __forceinline__ void init_cached_body(const BlkArgs& a, const BlkInit& ii, const BlkInitAp& ap, const BlkInitAp2& ap2) {
  constexpr int NT = (CW + 1) * 64, EC = AP == 2 ? 3 : 4;  // (AP == 2: batches of three rows keep the four streams in registers; a lane's sums keep their order)
  __shared__ __attribute__((aligned(16))) float red[CW + 1][32];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int sub = lane >> 3, lr = lane & 7;
  const int32_t ld = a.ld;
  for (int c = a.c0 + threadIdx.x; c < a.c1; c += NT) {
    a.part[(size_t)blockIdx.x * ld + c] = 0.f;
    if constexpr (AP) ap.part[(size_t)blockIdx.x * ld + c] = 0.f;
  }
  if ((int)(blockIdx.x >> 3) >= a.xs) return;
  const BlkWork wk = blk_work<CW>(a);
  const uint32_t lr16 = (uint32_t)lr * 16u, ldb = (uint32_t)ld * 4u;
  const int ngall = a.slices * a.groups, nbatch = (ngall + EC - 1) / EC;
  const int row_first = wk.rlo + ((wk.wgx * CW + wave) << 3) + sub;
  for (int q = 0; q < wk.nslab; ++q) {
    const int sc0 = a.c0 + (wk.xgrp + q * wk.xgroups) * 32;
    float4 dot = f4(0.f), dot_ap = f4(0.f);
    if (wave < CW) {
      const bool cok = sc0 + lr * 4 < a.c1;
      const size_t slab = (size_t)(sc0 >> 5) * (size_t)a.N * 32;
      const float* xbase = a.X + slab;
      const float* wybase = ii.WY + slab;
      float* zbase = ii.Z + slab;
      const uint32_t cb = (uint32_t)(sc0 + lr * 4) * 4u;
      const float4 psi4 = cok ? ld4(ii.psi + sc0 + lr * 4) : f4(0.f);
      float4 xs[2][EC], ws[2][EC];
      float4 vs[2][AP ? EC : 1];  // (AP: the rows of W W Y and the rows' weight sums)
      float ss[2][AP ? EC : 1];
      float4 ts[2][AP == 2 ? EC : 1];  // (AP == 2: the rows of W W W Y and the rows' second weight sums)
      float s2[2][AP == 2 ? EC : 1];
      float bv[2][EC];
      // No test around the loads: a lane without a row (past the part's rows, or a column past c1) reads the part's last row,
      // resp. the slab's first columns, and consume() drops what it got.  With the loads in straight-line code the compiler's
      // waits are counted ones and batch k + 1 stays in flight while batch k is consumed; under a test every wait is for all.
      const uint32_t lrc = cok ? lr16 : 0u;
      const uint32_t cbc = cok ? cb : (uint32_t)sc0 * 4u;
      const int row_last = max(wk.rhi - 1, 0);
      auto fetch = [&](int k, float4 (&x)[EC], float4 (&w)[EC], float (&bb)[EC], float4 (&v)[AP ? EC : 1], float (&sm)[AP ? EC : 1],
                       float4 (&t)[AP == 2 ? EC : 1], float (&sm2)[AP == 2 ? EC : 1]) {
#pragma unroll
        for (int i = 0; i < EC; ++i) {  // (byte offsets fit 32 bits: launch_init_cached checks as launch_apply_blocked does)
          const uint32_t row = (uint32_t)min(row_first + (k * EC + i) * wk.W8, row_last);
          x[i] = ld4_stream_at(xbase, row * 128u + lrc);
          w[i] = ld4_stream_at(wybase, row * 128u + lrc);
          bb[i] = ld1_at(a.B, row * 4u);
          if constexpr (AP) {
            v[i] = ld4_stream_at(ap.WW, row * ldb + cbc);
            sm[i] = ld1_at(ap.wsum, row * 4u);
          }
          if constexpr (AP == 2) {
            t[i] = ld4_stream_at(ap2.W3, row * ldb + cbc);
            sm2[i] = ld1_at(ap2.wsum2, row * 4u);
          }
        }
      };
      auto consume = [&](int k, const float4 (&x)[EC], const float4 (&w)[EC], const float (&bb)[EC], const float4 (&v)[AP ? EC : 1],
                         const float (&sm)[AP ? EC : 1], const float4 (&t)[AP == 2 ? EC : 1], const float (&sm2)[AP == 2 ? EC : 1]) {
#pragma unroll
        for (int i = 0; i < EC; ++i) {
          const int g = k * EC + i, row = row_first + g * wk.W8;
          if (g >= ngall || row >= wk.rhi || !cok) continue;
          float4 r, z;
          blk_init_row(a, ii, bb[i], x[i], x[i], w[i], psi4, r, z);
          st4_stream(reinterpret_cast<float*>(reinterpret_cast<char*>(ii.R) + ((uint32_t)row * ldb + cb)), r);
          if (ii.Xcopy != nullptr) st4_stream(reinterpret_cast<float*>(reinterpret_cast<char*>(ii.Xcopy) + ((uint32_t)row * ldb + cb)), x[i]);
          st4(reinterpret_cast<float*>(reinterpret_cast<char*>(zbase) + ((uint32_t)row * 128u + lr16)), z);
          dot = mulacc4(r, z, dot);
          if constexpr (AP) {
            const float cs = fmaf(a.cs_B, bb[i], a.cs_const);  // (blk_init_row's scalars)
            const float invMd = 1.f / (fmaf(ii.md_B, bb[i], ii.md_const) + 1e-12f);
            const float u = __fsub_rn(__fadd_rn(ii.rbU, ii.rbY), cs);
            const float qs = __fmul_rn(__fmul_rn(ii.rbB, bb[i]), sm[i]);
            auto one = [&](float zv, float wyv, float wwv, float pv) {
              const float wz = __fmul_rn(invMd, fmaf(a.cW, wwv, fmaf(u, wyv, __fmul_rn(qs, pv))));  // (W z0)_i
              return fmaf(cs, zv, -__fmul_rn(a.cW, wz));
            };
            const float4 o = make_float4(one(z.x, w[i].x, v[i].x, psi4.x), one(z.y, w[i].y, v[i].y, psi4.y),
                                         one(z.z, w[i].z, v[i].z, psi4.z), one(z.w, w[i].w, v[i].w, psi4.w));
            st4_stream(reinterpret_cast<float*>(reinterpret_cast<char*>(ap.AP) + ((uint32_t)row * ldb + cb)), o);
            dot_ap = mulacc4(z, o, dot_ap);
            if constexpr (AP == 2) {
              const float qs2 = __fmul_rn(__fmul_rn(ii.rbB, bb[i]), sm2[i]);
              auto two = [&](float ov, float wyv, float wwv, float w3v, float pv) {
                const float wz = __fmul_rn(invMd, fmaf(a.cW, wwv, fmaf(u, wyv, __fmul_rn(qs, pv))));    // (W z0)_i, as in one()
                const float wwz = __fmul_rn(invMd, fmaf(a.cW, w3v, fmaf(u, wwv, __fmul_rn(qs2, pv))));  // (W W z0)_i
                const float wq = fmaf(cs, wz, -__fmul_rn(a.cW, wwz));                                   // (W Q1)_i
                return fmaf(cs, ov, -__fmul_rn(a.cW, wq));
              };
              const float4 tt = make_float4(two(o.x, w[i].x, v[i].x, t[i].x, psi4.x), two(o.y, w[i].y, v[i].y, t[i].y, psi4.y),
                                            two(o.z, w[i].z, v[i].z, t[i].z, psi4.z), two(o.w, w[i].w, v[i].w, t[i].w, psi4.w));
              st4_stream(reinterpret_cast<float*>(reinterpret_cast<char*>(ap2.T) + ((uint32_t)row * ldb + cb)), tt);
            }
          }
        }
      };
      fetch(0, xs[0], ws[0], bv[0], vs[0], ss[0], ts[0], s2[0]);
      int k = 0;
      for (; k + 2 < nbatch; k += 2) {  // two batches per trip (the buffers keep their registers), no test around a fetch
        fetch(k + 1, xs[1], ws[1], bv[1], vs[1], ss[1], ts[1], s2[1]);
        consume(k, xs[0], ws[0], bv[0], vs[0], ss[0], ts[0], s2[0]);
        fetch(k + 2, xs[0], ws[0], bv[0], vs[0], ss[0], ts[0], s2[0]);
        consume(k + 1, xs[1], ws[1], bv[1], vs[1], ss[1], ts[1], s2[1]);
      }
      if (k + 1 < nbatch) {  // the last one or two batches (batch k is in xs[0])
        fetch(k + 1, xs[1], ws[1], bv[1], vs[1], ss[1], ts[1], s2[1]);
        consume(k, xs[0], ws[0], bv[0], vs[0], ss[0], ts[0], s2[0]);
        consume(k + 1, xs[1], ws[1], bv[1], vs[1], ss[1], ts[1], s2[1]);
      } else {
        consume(k, xs[0], ws[0], bv[0], vs[0], ss[0], ts[0], s2[0]);
      }
    }
    blk_fold<CW + 1>(dot, red, a.part, ld, sc0, min(a.c1, sc0 + 32), wave, lane);
    if constexpr (AP) blk_fold<CW + 1>(dot_ap, red, ap.part, ld, sc0, min(a.c1, sc0 + 32), wave, lane);
  }
}
template <int CW>
__global__ __launch_bounds__((CW + 1) * 64) void k_init_cached(const BlkArgs a, const BlkInit ii) {
  init_cached_body<CW, 0>(a, ii, BlkInitAp{}, BlkInitAp2{});
}
template <int CW>
__global__ __launch_bounds__((CW + 1) * 64) void k_init_cached_ap(const BlkArgs a, const BlkInit ii, const BlkInitAp ap) {
  init_cached_body<CW, 1>(a, ii, ap, BlkInitAp2{});
}
template <int CW>
__global__ __launch_bounds__((CW + 1) * 64) void k_init_cached_ap2(const BlkArgs a, const BlkInit ii, const BlkInitAp ap, const BlkInitAp2 ap2) {
  init_cached_body<CW, 2>(a, ii, ap, ap2);
}

// Iterations 1 and 2 in the INIT pass (BlkTwoSteps): with alpha1, beta1, alpha2, beta2 known before any N x D pass
// (k_anchor_gram_scalars) nothing of the two iterations has to reach memory but their outcome.  Geometry, row mapping and fetch
// pipeline of init_cached_body<CW, 2>; per element every value is formed with the operations and operand order of the kernel
// that forms it on the summed route -- r0, z0 = p1 (blk_init_row), Q1 = A p1 and T = A Q1 (init_cached_body), r1 = r0 - alpha1
// Q1 (k_update_xr), p2 = z1 + beta1 p1 and A p2 = (1 + beta1) Q1 - (m alpha1) T (k_update_p_ap2), r2 = r1 - alpha2 A p2, p3 =
// z2 + beta2 p2 (k_update_p), x2 = (x0 + alpha1 p1) + alpha2 p2 (k_update_x_ring) -- so the same scalars give the same bits.
// Stores r2 (row-major), p3 (slab-major) and x2 (row-major); no column sums, no fold: the list wave has nothing to do.
// Where the solve is known to end in iteration 4 (BlkTwoSteps::go_fold) it stores p3 and, in x's place, e -- x4 less the one term
// that needs the gathered row sum -- and no r2: the matvec's folded last form (k_apply_blocked, FMODE == 3) reads and writes e alone.
//
// One float4 of that pass (two_steps_elem): from the element's x0, W Y, W W Y, W W W Y, the row's b, s and s2 and the column's
// psi, alpha1, beta1, alpha2, beta2 to r2, p3 and x2.  Both forms of the pass call it -- the blocked one below (the reference
// form) and k_init_two_steps_stream -- and every output element depends on nothing else, so the launch geometry cannot
// change a bit.
__device__ __forceinline__ void two_steps_elem(const BlkArgs& a, const BlkInit& ii, float b, float sm, float sm2, float4 x, float4 w,
                                               float4 v, float4 t, float4 psi4, float4 al1, float4 be1, float4 al2, float4 be2,
                                               float4& r2, float4& p3, float4& x2, bool third = false, float4 al3 = float4{0.f, 0.f, 0.f, 0.f},
                                               bool fold = false, float4 be3 = float4{0.f, 0.f, 0.f, 0.f},
                                               float4 al4 = float4{0.f, 0.f, 0.f, 0.f}) {
  float4 r0, z0;
  blk_init_row(a, ii, b, x, x, w, psi4, r0, z0);
  const float cs = fmaf(a.cs_B, b, a.cs_const);  // (init_cached_body's scalars)
  const float invMd = 1.f / (fmaf(ii.md_B, b, ii.md_const) + 1e-12f);
  const float u = __fsub_rn(__fadd_rn(ii.rbU, ii.rbY), cs);
  const float qs = __fmul_rn(__fmul_rn(ii.rbB, b), sm);
  const float qs2 = __fmul_rn(__fmul_rn(ii.rbB, b), sm2);
  float r2v, p3v, x2v;
  auto one = [&](float xv, float rv, float zv, float wyv, float wwv, float w3v, float pv, float a1, float b1, float a2, float b2) {
    const float wz = __fmul_rn(invMd, fmaf(a.cW, wwv, fmaf(u, wyv, __fmul_rn(qs, pv))));    // (W z0)_i
    const float q1 = fmaf(cs, zv, -__fmul_rn(a.cW, wz));                                     // Q1 = A p1
    const float wwz = __fmul_rn(invMd, fmaf(a.cW, w3v, fmaf(u, wwv, __fmul_rn(qs2, pv))));  // (W W z0)_i
    const float wq = fmaf(cs, wz, -__fmul_rn(a.cW, wwz));                                    // (W Q1)_i
    const float tt = fmaf(cs, q1, -__fmul_rn(a.cW, wq));                                     // T = A Q1
    const float r1 = fmaf(-q1, a1, rv);
    const float p2 = fmaf(zv, b1, __fmul_rn(r1, invMd));
    const float ap2v = fmaf(__fadd_rn(1.f, b1), q1, -__fmul_rn(__fmul_rn(invMd, a1), tt));
    r2v = fmaf(-ap2v, a2, r1);
    p3v = fmaf(p2, b2, __fmul_rn(r2v, invMd));
    x2v = fmaf(p2, a2, fmaf(zv, a1, xv));
  };
  one(x.x, r0.x, z0.x, w.x, v.x, t.x, psi4.x, al1.x, be1.x, al2.x, be2.x); r2.x = r2v; p3.x = p3v; x2.x = x2v;
  one(x.y, r0.y, z0.y, w.y, v.y, t.y, psi4.y, al1.y, be1.y, al2.y, be2.y); r2.y = r2v; p3.y = p3v; x2.y = x2v;
  one(x.z, r0.z, z0.z, w.z, v.z, t.z, psi4.z, al1.z, be1.z, al2.z, be2.z); r2.z = r2v; p3.z = p3v; x2.z = x2v;
  one(x.w, r0.w, z0.w, w.w, v.w, t.w, psi4.w, al1.w, be1.w, al2.w, be2.w); r2.w = r2v; p3.w = p3v; x2.w = x2v;
  if (third) {  // (the three-step route: x3 = x2 + alpha3 p3, k_update_x_ring's operation on the same floats)
    x2.x = fmaf(p3.x, al3.x, x2.x);
    x2.y = fmaf(p3.y, al3.y, x2.y);
    x2.z = fmaf(p3.z, al3.z, x2.z);
    x2.w = fmaf(p3.w, al3.w, x2.w);
  }
  if (fold) {
    // (the folded last form, behind `third`: k_apply_blocked's FUSED_LAST epilogue on this element with a zero row sum -- its
    // operations in its operand order; fmaf(cs, p3, -(cW * 0)) is the rounded product -- so x4 = e + (alpha4 alpha3)(M^-1 cW) acc)
    auto last = [&](float pv, float rv, float xv, float a3, float b3, float a4) {
      const float o = __fmul_rn(cs, pv);
      const float r3 = fmaf(-o, a3, rv);
      const float p4 = fmaf(pv, b3, __fmul_rn(r3, invMd));
      return fmaf(p4, a4, xv);
    };
    x2.x = last(p3.x, r2.x, x2.x, al3.x, be3.x, al4.x);
    x2.y = last(p3.y, r2.y, x2.y, al3.y, be3.y, al4.y);
    x2.z = last(p3.z, r2.z, x2.z, al3.z, be3.z, al4.z);
    x2.w = last(p3.w, r2.w, x2.w, al3.w, be3.w, al4.w);
  }
}
template <int CW>
__global__ __launch_bounds__((CW + 1) * 64) void k_init_two_steps(const BlkArgs a, const BlkInit ii, const BlkInitAp ap, const BlkInitAp2 ap2,
                                                                  const BlkTwoSteps ts) {
  constexpr int EC = 3;  // (as init_cached_body<CW, 2>: batches of three rows keep the four streams in registers)
  if (*ts.go != 1u) return;
  const bool fold = ts.go_fold != nullptr && *ts.go_fold == 1u;  // (wave-uniform: the solve ends in iteration 4, BlkTwoSteps::go_fold)
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if ((int)(blockIdx.x >> 3) >= a.xs || wave >= CW) return;
  const int sub = lane >> 3, lr = lane & 7;
  const int32_t ld = a.ld;
  const BlkWork wk = blk_work<CW>(a);
  const uint32_t lr16 = (uint32_t)lr * 16u, ldb = (uint32_t)ld * 4u;
  const int ngall = a.slices * a.groups, nbatch = (ngall + EC - 1) / EC;
  const int row_first = wk.rlo + ((wk.wgx * CW + wave) << 3) + sub;
  for (int q = 0; q < wk.nslab; ++q) {
    const int sc0 = a.c0 + (wk.xgrp + q * wk.xgroups) * 32;
    const bool cok = sc0 + lr * 4 < a.c1;
    const size_t slab = (size_t)(sc0 >> 5) * (size_t)a.N * 32;
    const float* xbase = a.X + slab;
    const float* wybase = ii.WY + slab;
    float* pbase = ii.Z + slab;
    const uint32_t cb = (uint32_t)(sc0 + lr * 4) * 4u;
    const int cc = cok ? sc0 + lr * 4 : sc0;
    const float4 psi4 = cok ? ld4(ii.psi + cc) : f4(0.f);
    const float4 al1 = ld4(ts.alpha1 + cc), al2 = ld4(ts.alpha2 + cc), be1 = ld4(ts.beta1 + cc), be2 = ld4(ts.beta2 + cc);
    const bool third = ts.alpha3 != nullptr;
    const float4 al3 = third ? ld4(ts.alpha3 + cc) : f4(0.f);
    const float4 be3 = fold ? ld4(ts.beta3 + cc) : f4(0.f), al4 = fold ? ld4(ts.alpha4 + cc) : f4(0.f);
    float4 xs[2][EC], ws[2][EC], vs[2][EC], t3[2][EC];
    float bv[2][EC], ss[2][EC], s2[2][EC];
    // (no test around the loads: see init_cached_body)
    const uint32_t lrc = cok ? lr16 : 0u;
    const uint32_t cbc = cok ? cb : (uint32_t)sc0 * 4u;
    const int row_last = max(wk.rhi - 1, 0);
    auto fetch = [&](int k, float4 (&x)[EC], float4 (&w)[EC], float (&bb)[EC], float4 (&v)[EC], float (&sm)[EC], float4 (&t)[EC],
                     float (&sm2)[EC]) {
#pragma unroll
      for (int i = 0; i < EC; ++i) {
        const uint32_t row = (uint32_t)min(row_first + (k * EC + i) * wk.W8, row_last);
        x[i] = ld4_stream_at(xbase, row * 128u + lrc);
        w[i] = ld4_stream_at(wybase, row * 128u + lrc);
        bb[i] = ld1_at(a.B, row * 4u);
        v[i] = ld4_stream_at(ap.WW, row * ldb + cbc);
        sm[i] = ld1_at(ap.wsum, row * 4u);
        t[i] = ld4_stream_at(ap2.W3, row * ldb + cbc);
        sm2[i] = ld1_at(ap2.wsum2, row * 4u);
      }
    };
    auto consume = [&](int k, const float4 (&x)[EC], const float4 (&w)[EC], const float (&bb)[EC], const float4 (&v)[EC],
                       const float (&sm)[EC], const float4 (&t)[EC], const float (&sm2)[EC]) {
#pragma unroll
      for (int i = 0; i < EC; ++i) {
        const int g = k * EC + i, row = row_first + g * wk.W8;
        if (g >= ngall || row >= wk.rhi || !cok) continue;
        float4 r2, p3, x2;
        two_steps_elem(a, ii, bb[i], sm[i], sm2[i], x[i], w[i], v[i], t[i], psi4, al1, be1, al2, be2, r2, p3, x2, third, al3, fold, be3, al4);
        if (!fold) st4_stream(reinterpret_cast<float*>(reinterpret_cast<char*>(ii.R) + ((uint32_t)row * ldb + cb)), r2);
        st4_stream(reinterpret_cast<float*>(reinterpret_cast<char*>(ii.Xcopy) + ((uint32_t)row * ldb + cb)), x2);
        st4(reinterpret_cast<float*>(reinterpret_cast<char*>(pbase) + ((uint32_t)row * 128u + lr16)), p3);
      }
    };
    fetch(0, xs[0], ws[0], bv[0], vs[0], ss[0], t3[0], s2[0]);
    int k = 0;
    for (; k + 2 < nbatch; k += 2) {  // two batches per trip (the buffers keep their registers), no test around a fetch
      fetch(k + 1, xs[1], ws[1], bv[1], vs[1], ss[1], t3[1], s2[1]);
      consume(k, xs[0], ws[0], bv[0], vs[0], ss[0], t3[0], s2[0]);
      fetch(k + 2, xs[0], ws[0], bv[0], vs[0], ss[0], t3[0], s2[0]);
      consume(k + 1, xs[1], ws[1], bv[1], vs[1], ss[1], t3[1], s2[1]);
    }
    if (k + 1 < nbatch) {
      fetch(k + 1, xs[1], ws[1], bv[1], vs[1], ss[1], t3[1], s2[1]);
      consume(k, xs[0], ws[0], bv[0], vs[0], ss[0], t3[0], s2[0]);
      consume(k + 1, xs[1], ws[1], bv[1], vs[1], ss[1], t3[1], s2[1]);
    } else {
      consume(k, xs[0], ws[0], bv[0], vs[0], ss[0], t3[0], s2[0]);
    }
  }
}

// The same pass in the geometry of the update kernels (k_update_x_ring): 256 threads, the rows [row0, N) a plain grid-stride
// range, LPR lanes over a row's columns in NCH chunks of LPR float4s, RPT row groups per wave and trip.  blockIdx.y picks the
// column tile of NCH * LPR * 4 columns (windows wider than one tile; tiles start at multiples of 32).  Row-major operands
// (W W Y, W W W Y, r2, x2) sit at row * ld + col, slab-major ones (x0 = Ys, W Y, p3) at blk_off(N, row, col).  The per-column
// scalars are loaded once, before the row loop.  No test around a load (see init_cached_body): a lane without a column reads the
// window's first, a lane without a row the last row, and only the stores are guarded -- so all RPT * NCH * 4 loads of a trip are
// in flight before the first use.  No LDS, no barrier.  Same bits as k_init_two_steps (two_steps_elem).
// FOLDABLE: the instantiation that can store the folded last form's e (BlkTwoSteps::go_fold; beta3 and alpha4 per column cost eight
// registers a chunk and a wave per SIMD at two and three chunks).  The launcher picks it only where the solve may fold, so every
// other solve runs the pass with the registers it always had.
template <int LPR, int NCH, int RPT, bool FOLDABLE = false>
__global__ __launch_bounds__(256) void k_init_two_steps_stream(const BlkArgs a, const BlkInit ii, const BlkInitAp ap, const BlkInitAp2 ap2,
                                                               const BlkTwoSteps ts) {
  constexpr int RPW = 64 / LPR;
  if (*ts.go != 1u) return;
  bool fold = false;
  if constexpr (FOLDABLE) fold = *ts.go_fold == 1u;  // (wave-uniform, as in k_init_two_steps)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane / LPR, lr = lane % LPR;
  const int32_t ld = a.ld;
  const int32_t t0 = a.c0 + (int32_t)blockIdx.y * (NCH * LPR * 4);
  int coff[NCH], cld[NCH];
  bool cok[NCH];
  float4 psi4[NCH], al1[NCH], be1[NCH], al2[NCH], be2[NCH], al3[NCH];
  [[maybe_unused]] float4 be3[FOLDABLE ? NCH : 1], al4[FOLDABLE ? NCH : 1];
  const bool third = ts.alpha3 != nullptr;
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    coff[ch] = t0 + (ch * LPR + lr) * 4;
    cok[ch] = coff[ch] < a.c1;
    cld[ch] = cok[ch] ? coff[ch] : a.c0;
    psi4[ch] = ld4(ii.psi + cld[ch]);
    al1[ch] = ld4(ts.alpha1 + cld[ch]);
    be1[ch] = ld4(ts.beta1 + cld[ch]);
    al2[ch] = ld4(ts.alpha2 + cld[ch]);
    be2[ch] = ld4(ts.beta2 + cld[ch]);
    al3[ch] = third ? ld4(ts.alpha3 + cld[ch]) : f4(0.f);
    if constexpr (FOLDABLE) {
      be3[ch] = fold ? ld4(ts.beta3 + cld[ch]) : f4(0.f);
      al4[ch] = fold ? ld4(ts.alpha4 + cld[ch]) : f4(0.f);
    }
  }
  uint32_t cb[NCH], sb[NCH];  // byte offsets of the lane's columns within a row: row-major, slab-major (blk_off less the row)
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    cb[ch] = (uint32_t)cld[ch] * 4u;
    sb[ch] = ((uint32_t)(cld[ch] >> 5) * (uint32_t)a.N * 32u + (uint32_t)(cld[ch] & 31)) * 4u;
  }
  const int rend = a.N, rlast = a.N - 1;
  for (int64_t rb = ts.row0 + ((int64_t)blockIdx.x * 4 + wave) * (RPW * RPT); rb < rend; rb += (int64_t)gridDim.x * 4 * (RPW * RPT)) {
    int row[RPT], rld[RPT];
    float bv[RPT], sm[RPT], sm2[RPT];
    float4 x[RPT][NCH], w[RPT][NCH], v[RPT][NCH], t[RPT][NCH];
#pragma unroll
    for (int j = 0; j < RPT; ++j) {
      row[j] = (int)rb + j * RPW + sub;
      rld[j] = min(row[j], rlast);
      if constexpr (LPR == 64) rld[j] = __builtin_amdgcn_readfirstlane(rld[j]);  // (wave-uniform: the row's scalars by scalar loads)
      bv[j] = a.B[rld[j]];
      sm[j] = ap.wsum[rld[j]];
      sm2[j] = ap2.wsum2[rld[j]];
      // row base (wave-uniform at LPR == 64) + the lane's 32-bit column offset (the launcher checks that N * ld * 4 fits)
      const size_t rrow = (size_t)rld[j] * ld, rslab = (size_t)rld[j] * 32;
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        x[j][ch] = ld4_stream_at(a.X + rslab, sb[ch]);
        w[j][ch] = ld4_stream_at(ii.WY + rslab, sb[ch]);
        v[j][ch] = ld4_stream_at(ap.WW + rrow, cb[ch]);
        t[j][ch] = ld4_stream_at(ap2.W3 + rrow, cb[ch]);
      }
    }
#pragma unroll
    for (int j = 0; j < RPT; ++j) {
      if (row[j] >= rend) continue;
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        if (!cok[ch]) continue;
        float4 r2, p3, x2;
        two_steps_elem(a, ii, bv[j], sm[j], sm2[j], x[j][ch], w[j][ch], v[j][ch], t[j][ch], psi4[ch], al1[ch], be1[ch], al2[ch], be2[ch], r2,
                       p3, x2, third, al3[ch], fold, be3[FOLDABLE ? ch : 0], al4[FOLDABLE ? ch : 0]);
        // (a row and a column that are stored are the ones that were loaded: the same offsets; the folded last form keeps no r2)
        if (!fold) st4_stream(reinterpret_cast<float*>(reinterpret_cast<char*>(ii.R + (size_t)rld[j] * ld) + cb[ch]), r2);
        st4_stream(reinterpret_cast<float*>(reinterpret_cast<char*>(ii.Xcopy + (size_t)rld[j] * ld) + cb[ch]), x2);
        st4(reinterpret_cast<float*>(reinterpret_cast<char*>(ii.Z + (size_t)rld[j] * 32) + sb[ch]), p3);
      }
    }
  }
}

// The polynomial last form (SettlePolyArgs; anchor_gram.hpp: poly4_coeffs) in the same geometry and addressing: five row streams in,
// x4 out, nine coefficients a column loaded once before the row loop, three scalars a row.  One fixed order per element: the Y family
// from a4 W^4 Y down to a0 Y by fmaf, the psi family from q3 s3 down to q0 the same way, then one add (tests/host_logic/
// sweep_poly4.cpp evaluates it so).  Loads untested, stores guarded, as above.  No LDS, no barrier, no atomics.
template <int LPR, int NCH, int RPT>
__global__ __launch_bounds__(256) void k_settle_poly(const SettlePolyArgs a) {
  constexpr int RPW = 64 / LPR;
  if (*a.go != 1u || *a.go_fold != 1u) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane / LPR, lr = lane % LPR;
  const int32_t ld = a.ld;
  const int32_t t0 = a.c0 + (int32_t)blockIdx.y * (NCH * LPR * 4);
  bool cok[NCH];
  float4 ca[gram::kPolyY][NCH], cq[gram::kPolyS][NCH];
  uint32_t cb[NCH], sb[NCH];  // byte offsets of the lane's columns within a row: row-major, slab-major (blk_off less the row)
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    const int coff = t0 + (ch * LPR + lr) * 4;
    cok[ch] = coff < a.c1;
    const int cld = cok[ch] ? coff : a.c0;
#pragma unroll
    for (int k = 0; k < gram::kPolyY; ++k) ca[k][ch] = ld4(a.coef + (size_t)k * ld + cld);
#pragma unroll
    for (int k = 0; k < gram::kPolyS; ++k) cq[k][ch] = ld4(a.coef + (size_t)(gram::kPolyY + k) * ld + cld);
    cb[ch] = (uint32_t)cld * 4u;
    sb[ch] = ((uint32_t)(cld >> 5) * (uint32_t)a.N * 32u + (uint32_t)(cld & 31)) * 4u;
  }
  const int rend = a.N, rlast = a.N - 1;
  for (int64_t rb = ((int64_t)blockIdx.x * 4 + wave) * (RPW * RPT); rb < rend; rb += (int64_t)gridDim.x * 4 * (RPW * RPT)) {
    int row[RPT], rld[RPT];
    float s1[RPT], s2[RPT], s3[RPT];
    float4 y0[RPT][NCH], y1[RPT][NCH], y2[RPT][NCH], y3[RPT][NCH], y4[RPT][NCH];
#pragma unroll
    for (int j = 0; j < RPT; ++j) {
      row[j] = (int)rb + j * RPW + sub;
      rld[j] = min(row[j], rlast);
      if constexpr (LPR == 64) rld[j] = __builtin_amdgcn_readfirstlane(rld[j]);  // (wave-uniform: the row's scalars by scalar loads)
      s1[j] = a.wsum[rld[j]];
      s2[j] = a.wsum2[rld[j]];
      s3[j] = a.wsum3[rld[j]];
      // row base (wave-uniform at LPR == 64) + the lane's 32-bit column offset (settle_poly_supported: N * ld * 4 fits)
      const size_t rrow = (size_t)rld[j] * ld, rslab = (size_t)rld[j] * 32;
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        y0[j][ch] = ld4_stream_at(a.Ys + rslab, sb[ch]);
        y1[j][ch] = ld4_stream_at(a.WYs + rslab, sb[ch]);
        y2[j][ch] = ld4_stream_at(a.WW + rrow, cb[ch]);
        y3[j][ch] = ld4_stream_at(a.W3 + rrow, cb[ch]);
        y4[j][ch] = ld4_stream_at(a.W4 + rrow, cb[ch]);
      }
    }
#pragma unroll
    for (int j = 0; j < RPT; ++j) {
      if (row[j] >= rend) continue;
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        if (!cok[ch]) continue;
        float4 acc = make_float4(__fmul_rn(ca[4][ch].x, y4[j][ch].x), __fmul_rn(ca[4][ch].y, y4[j][ch].y), __fmul_rn(ca[4][ch].z, y4[j][ch].z),
                                 __fmul_rn(ca[4][ch].w, y4[j][ch].w));
        acc = mulacc4(ca[3][ch], y3[j][ch], acc);
        acc = mulacc4(ca[2][ch], y2[j][ch], acc);
        acc = mulacc4(ca[1][ch], y1[j][ch], acc);
        acc = mulacc4(ca[0][ch], y0[j][ch], acc);
        float4 ps = make_float4(__fmul_rn(cq[3][ch].x, s3[j]), __fmul_rn(cq[3][ch].y, s3[j]), __fmul_rn(cq[3][ch].z, s3[j]),
                                __fmul_rn(cq[3][ch].w, s3[j]));
        ps = fma4(s2[j], cq[2][ch], ps);
        ps = fma4(s1[j], cq[1][ch], ps);
        ps = make_float4(__fadd_rn(ps.x, cq[0][ch].x), __fadd_rn(ps.y, cq[0][ch].y), __fadd_rn(ps.z, cq[0][ch].z), __fadd_rn(ps.w, cq[0][ch].w));
        const float4 x4 = make_float4(__fadd_rn(acc.x, ps.x), __fadd_rn(acc.y, ps.y), __fadd_rn(acc.z, ps.z), __fadd_rn(acc.w, ps.w));
        // (a row and a column that are stored are the ones that were loaded: the same offsets)
        st4_stream(reinterpret_cast<float*>(reinterpret_cast<char*>(a.X + (size_t)rld[j] * ld) + cb[ch]), x4);
      }
    }
  }
}

// The Gram sums, first stage: workgroup (slab, chunk) sums its chunk's rows of the slab's 32 columns, a thread one column of
// every eighth row, in float64 (the product of two floats is exact there); the eight row lanes are folded through LDS in
// lane order.  Every real row of the window's columns is visited once.  The lattice's six sums ride in the slab-0 workgroups.
__global__ __launch_bounds__(256) void k_anchor_gram_part(const GramArgs a) {
  constexpr int NQ = gram::kGramPerColumn, NL = gram::kGramLattice;
  __shared__ double red[8][32];
  const int cl = threadIdx.x & 31, half = threadIdx.x >> 5;
  const int sc0 = a.c0 + (int)blockIdx.x * 32, col = sc0 + cl, chunk = (int)blockIdx.y;
  const bool cok = col < a.c1;
  const bool lat = blockIdx.x == 0 && cl == 0;
  const int r0 = (int)((int64_t)a.N * chunk / OSC_GRAM_CHUNKS), r1 = (int)((int64_t)a.N * (chunk + 1) / OSC_GRAM_CHUNKS);
  const size_t slab = (size_t)(sc0 >> 5) * (size_t)a.N * 32;
  double acc[NQ], la[NL];
#pragma unroll
  for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
#pragma unroll
  for (int q = 0; q < NL; ++q) la[q] = 0.0;
  for (int row = r0 + half; row < r1; row += 8) {
    const double s[3] = {1.0, (double)a.wsum[row], (double)a.wsum2[row]};
    if (cok) {
      const double y[4] = {(double)a.Ys[slab + (size_t)row * 32 + cl], (double)a.WYs[slab + (size_t)row * 32 + cl],
                           (double)a.WW[(size_t)row * a.ld + col], (double)a.W3[(size_t)row * a.ld + col]};
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = j; k < 4; ++k) acc[gram::yy_index(j, k)] += y[j] * y[k];
#pragma unroll
      for (int b = 0; b < 3; ++b)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[gram::ay_index(b, j)] += s[b] * y[j];
    }
    if (lat) {
#pragma unroll
      for (int b = 0; b < 3; ++b)
#pragma unroll
        for (int c = b; c < 3; ++c) la[gram::lat_index(b, c)] += s[b] * s[c];
    }
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    __syncthreads();
    red[half][cl] = acc[q];
    __syncthreads();
    if (half == 0 && cok) {
      double t = 0.0;
#pragma unroll
      for (int h = 0; h < 8; ++h) t += red[h][cl];
      a.part[((size_t)chunk * NQ + q) * a.ld + col] = t;
    }
  }
  if (blockIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < NL; ++q) {
      __syncthreads();
      if (cl == 0) red[half][0] = la[q];
      __syncthreads();
      if (threadIdx.x == 0) {
        double t = 0.0;
#pragma unroll
        for (int h = 0; h < 8; ++h) t += red[h][0];
        a.part[(size_t)OSC_GRAM_CHUNKS * NQ * a.ld + (size_t)chunk * NL + q] = t;
      }
    }
  }
}
// ... second stage: the chunks' partials in chunk order (columns outside the window: 0)
__global__ __launch_bounds__(256) void k_anchor_gram_fold(const GramArgs a) {
  constexpr int NQ = gram::kGramPerColumn, NL = gram::kGramLattice;
  const int idx = (int)(blockIdx.x * 256 + threadIdx.x);
  if (idx < NQ * a.ld) {
    const int q = idx / a.ld, col = idx % a.ld;
    double t = 0.0;
    if (col >= a.c0 && col < a.c1)
      for (int ch = 0; ch < OSC_GRAM_CHUNKS; ++ch) t += a.part[((size_t)ch * NQ + q) * a.ld + col];
    a.out[idx] = t;
  } else if (idx < NQ * a.ld + NL) {
    const int q = idx - NQ * a.ld;
    double t = 0.0;
    for (int ch = 0; ch < OSC_GRAM_CHUNKS; ++ch) t += a.part[(size_t)OSC_GRAM_CHUNKS * NQ * a.ld + (size_t)ch * NL + q];
    a.out[idx] = t;
  }
}

// The third step's sums (anchor_gram.hpp: kGram3PerColumn, kGram3Lattice), same scheme: workgroup (slab, chunk), a thread one
// column of every eighth row, float64, the eight row lanes folded through LDS in lane order, the lattice's four sums in the
// slab-0 workgroups.
__global__ __launch_bounds__(256) void k_anchor_gram3_part(const Gram3Args b) {
  constexpr int NQ = gram::kGram3PerColumn, NL = gram::kGram3Lattice;
  const GramArgs& a = b.g;
  __shared__ double red[8][32];
  const int cl = threadIdx.x & 31, half = threadIdx.x >> 5;
  const int sc0 = a.c0 + (int)blockIdx.x * 32, col = sc0 + cl, chunk = (int)blockIdx.y;
  const bool cok = col < a.c1;
  const bool lat = blockIdx.x == 0 && cl == 0;
  const int r0 = (int)((int64_t)a.N * chunk / OSC_GRAM_CHUNKS), r1 = (int)((int64_t)a.N * (chunk + 1) / OSC_GRAM_CHUNKS);
  const size_t slab = (size_t)(sc0 >> 5) * (size_t)a.N * 32;
  double acc[NQ], la[NL];
#pragma unroll
  for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
#pragma unroll
  for (int q = 0; q < NL; ++q) la[q] = 0.0;
  for (int row = r0 + half; row < r1; row += 8) {
    const double s[4] = {1.0, (double)a.wsum[row], (double)a.wsum2[row], (double)b.wsum3[row]};
    if (cok) {
      const double y[5] = {(double)a.Ys[slab + (size_t)row * 32 + cl], (double)a.WYs[slab + (size_t)row * 32 + cl],
                           (double)a.WW[(size_t)row * a.ld + col], (double)a.W3[(size_t)row * a.ld + col],
                           (double)b.W4[(size_t)row * a.ld + col]};
#pragma unroll
      for (int j = 0; j < 5; ++j) acc[gram::y4_index(j)] += y[j] * y[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[gram::a4_index(q)] += s[q] * y[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[gram::s3y_index(j)] += s[3] * y[j];
    }
    if (lat) {
#pragma unroll
      for (int q = 0; q < 4; ++q) la[gram::lat3_index(q)] += s[q] * s[3];
    }
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    __syncthreads();
    red[half][cl] = acc[q];
    __syncthreads();
    if (half == 0 && cok) {
      double t = 0.0;
#pragma unroll
      for (int h = 0; h < 8; ++h) t += red[h][cl];
      a.part[((size_t)chunk * NQ + q) * a.ld + col] = t;
    }
  }
  if (blockIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < NL; ++q) {
      __syncthreads();
      if (cl == 0) red[half][0] = la[q];
      __syncthreads();
      if (threadIdx.x == 0) {
        double t = 0.0;
#pragma unroll
        for (int h = 0; h < 8; ++h) t += red[h][0];
        a.part[(size_t)OSC_GRAM_CHUNKS * NQ * a.ld + (size_t)chunk * NL + q] = t;
      }
    }
  }
}
__global__ __launch_bounds__(256) void k_anchor_gram3_fold(const GramArgs a) {
  constexpr int NQ = gram::kGram3PerColumn, NL = gram::kGram3Lattice;
  const int idx = (int)(blockIdx.x * 256 + threadIdx.x);
  if (idx < NQ * a.ld) {
    const int q = idx / a.ld, col = idx % a.ld;
    double t = 0.0;
    if (col >= a.c0 && col < a.c1)
      for (int ch = 0; ch < OSC_GRAM_CHUNKS; ++ch) t += a.part[((size_t)ch * NQ + q) * a.ld + col];
    a.out[idx] = t;
  } else if (idx < NQ * a.ld + NL) {
    const int q = idx - NQ * a.ld;
    double t = 0.0;
    for (int ch = 0; ch < OSC_GRAM_CHUNKS; ++ch) t += a.part[(size_t)OSC_GRAM_CHUNKS * NQ * a.ld + (size_t)ch * NL + q];
    a.out[idx] = t;
  }
}

// The sums the fourth step's scalars add (anchor_gram.hpp: kGram4PerColumn, kGram4Lattice), same scheme once more: workgroup (slab,
// chunk), a thread one column of every eighth row, float64, the eight row lanes folded through LDS in lane order, the lattice's
// five sums in the slab-0 workgroups.
__global__ __launch_bounds__(256) void k_anchor_gram4_part(const Gram4Args b) {
  constexpr int NQ = gram::kGram4PerColumn, NL = gram::kGram4Lattice;
  const GramArgs& a = b.g;
  __shared__ double red[8][32];
  const int cl = threadIdx.x & 31, half = threadIdx.x >> 5;
  const int sc0 = a.c0 + (int)blockIdx.x * 32, col = sc0 + cl, chunk = (int)blockIdx.y;
  const bool cok = col < a.c1;
  const bool lat = blockIdx.x == 0 && cl == 0;
  const int r0 = (int)((int64_t)a.N * chunk / OSC_GRAM_CHUNKS), r1 = (int)((int64_t)a.N * (chunk + 1) / OSC_GRAM_CHUNKS);
  const size_t slab = (size_t)(sc0 >> 5) * (size_t)a.N * 32;
  double acc[NQ], la[NL];
#pragma unroll
  for (int q = 0; q < NQ; ++q) acc[q] = 0.0;
#pragma unroll
  for (int q = 0; q < NL; ++q) la[q] = 0.0;
  for (int row = r0 + half; row < r1; row += 8) {
    const double s[5] = {1.0, (double)a.wsum[row], (double)a.wsum2[row], (double)b.wsum3[row], (double)b.wsum4[row]};
    if (cok) {
      const double y[6] = {(double)a.Ys[slab + (size_t)row * 32 + cl], (double)a.WYs[slab + (size_t)row * 32 + cl],
                           (double)a.WW[(size_t)row * a.ld + col], (double)a.W3[(size_t)row * a.ld + col],
                           (double)b.W4[(size_t)row * a.ld + col], (double)b.W5[(size_t)row * a.ld + col]};
#pragma unroll
      for (int j = 0; j < 6; ++j) acc[gram::y5_index(j)] += y[j] * y[5];
#pragma unroll
      for (int q = 0; q < 5; ++q) acc[gram::a5_index(q)] += s[q] * y[5];
#pragma unroll
      for (int j = 0; j < 5; ++j) acc[gram::s4y_index(j)] += s[4] * y[j];
    }
    if (lat) {
#pragma unroll
      for (int q = 0; q < 5; ++q) la[gram::lat4_index(q)] += s[q] * s[4];
    }
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    __syncthreads();
    red[half][cl] = acc[q];
    __syncthreads();
    if (half == 0 && cok) {
      double t = 0.0;
#pragma unroll
      for (int h = 0; h < 8; ++h) t += red[h][cl];
      a.part[((size_t)chunk * NQ + q) * a.ld + col] = t;
    }
  }
  if (blockIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < NL; ++q) {
      __syncthreads();
      if (cl == 0) red[half][0] = la[q];
      __syncthreads();
      if (threadIdx.x == 0) {
        double t = 0.0;
#pragma unroll
        for (int h = 0; h < 8; ++h) t += red[h][0];
        a.part[(size_t)OSC_GRAM_CHUNKS * NQ * a.ld + (size_t)chunk * NL + q] = t;
      }
    }
  }
}
__global__ __launch_bounds__(256) void k_anchor_gram4_fold(const GramArgs a) {
  constexpr int NQ = gram::kGram4PerColumn, NL = gram::kGram4Lattice;
  const int idx = (int)(blockIdx.x * 256 + threadIdx.x);
  if (idx < NQ * a.ld) {
    const int q = idx / a.ld, col = idx % a.ld;
    double t = 0.0;
    if (col >= a.c0 && col < a.c1)
      for (int ch = 0; ch < OSC_GRAM_CHUNKS; ++ch) t += a.part[((size_t)ch * NQ + q) * a.ld + col];
    a.out[idx] = t;
  } else if (idx < NQ * a.ld + NL) {
    const int q = idx - NQ * a.ld;
    double t = 0.0;
    for (int ch = 0; ch < OSC_GRAM_CHUNKS; ++ch) t += a.part[(size_t)OSC_GRAM_CHUNKS * NQ * a.ld + (size_t)ch * NL + q];
    a.out[idx] = t;
  }
}

// One workgroup, a thread per column (anchor_gram.hpp: two_steps): the scalars of iterations 1 and 2, their residuals as
// k_reduce_beta publishes them (nanmax over the columns, device slot and host-mapped word), and the fused pass's gate word.
// A solve with an unusable column publishes 0 for both residuals: the host loop stops in iteration 1, nothing was written,
// and run_cg solves again on the summed route.
// With the third step planned (GramScalarArgs::gram3; three_steps on the nine vectors' matrix) also alpha3, beta3, r3 . z3 in
// rz's place, the third residual and go[1], the gate word of iteration 3's fused matvec; usable3 takes usable's place.
// With the fourth step's scalars planned as well (GramScalarArgs::gram4; four_steps on the eleven vectors' matrix: the same three
// iterations to the bit) also alpha4 and the fourth residual, the latter into its host word alone.  A column whose fourth iteration is unusable makes that residual
// NaN -- the host then keeps iteration 4 on the summed route -- and leaves the three-step route as it is.
__global__ __launch_bounds__(256) void k_anchor_gram_scalars(const GramScalarArgs a) {
  __shared__ float sh1[4], sh2[4], sh3[4], sh4[4];
  __shared__ int shu[4];
  const bool three = a.gram3 != nullptr;  // (three_steps: the same iterations 1 and 2 to the bit, and iteration 3's scalars)
  const bool four = three && a.gram4 != nullptr;
  const float b = a.B[0];
  gram::Op o;
  const float cs = fmaf(a.cs_B, b, a.cs_const);  // (blk_init_row's and init_cached_body's scalars)
  o.cs = (double)cs;
  o.cW = (double)a.cW;
  o.qb = (double)__fmul_rn(a.rbB, b);
  o.m = (double)(1.f / (fmaf(a.md_B, b, a.md_const) + 1e-12f));
  o.u = (double)__fsub_rn(__fadd_rn(a.rbU, a.rbY), cs);
  const double* lat = a.gram + (size_t)gram::kGramPerColumn * a.ld;
  float res1 = 0.f, res2 = 0.f, res3 = 0.f, res4 = 0.f;
  int usable = 1;
  for (int col = a.c0 + (int)threadIdx.x; col < a.c1; col += 256) {
    gram::Scalars s;
    if (four) {
      const double* lat3 = a.gram3 + (size_t)gram::kGram3PerColumn * a.ld;
      const double* lat4 = a.gram4 + (size_t)gram::kGram4PerColumn * a.ld;
      double G[gram::kBasis4][gram::kBasis4];
      gram::fill4(G, a.gram + col, (size_t)a.ld, lat, a.gram3 + col, (size_t)a.ld, lat3, a.gram4 + col, (size_t)a.ld, lat4, (double)a.psi[col]);
      const gram::Scalars4 f = gram::four_steps(G, o);
      s = f.three.two;
      s.usable = f.three.usable3;
      a.alpha3[col] = f.three.alpha3;
      a.beta3[col] = f.three.beta3;
      a.rz[col] = f.three.rz3;
      a.alpha4[col] = f.alpha4;
      res3 = nanmax(res3, f.three.res3);
      res4 = nanmax(res4, f.usable4 ? f.res4 : __uint_as_float(0x7FC00000u));
      if (a.poly != nullptr) {  // (for every column: go[2], under which alone they are read, is known only behind the fold below)
        const gram::Poly4 pc = gram::poly4_coeffs(o, f.alpha_d, f.beta_d, (double)a.psi[col]);
#pragma unroll
        for (int k = 0; k < gram::kPolyY; ++k) a.poly[(size_t)k * a.ld + col] = (float)pc.a[k];
#pragma unroll
        for (int k = 0; k < gram::kPolyS; ++k) a.poly[(size_t)(gram::kPolyY + k) * a.ld + col] = (float)pc.q[k];
      }
    } else if (three) {
      const double* lat3 = a.gram3 + (size_t)gram::kGram3PerColumn * a.ld;
      double G[gram::kBasis3][gram::kBasis3];
      gram::fill3(G, a.gram + col, (size_t)a.ld, lat, a.gram3 + col, (size_t)a.ld, lat3, (double)a.psi[col]);
      const gram::Scalars3 t = gram::three_steps(G, o);
      s = t.two;
      s.usable = t.usable3;
      a.alpha3[col] = t.alpha3;
      a.beta3[col] = t.beta3;
      a.rz[col] = t.rz3;
      res3 = nanmax(res3, t.res3);
    } else {
      double G[gram::kBasis][gram::kBasis];
      gram::fill(G, a.gram + col, (size_t)a.ld, lat, (double)a.psi[col]);
      s = gram::two_steps(G, o);
      a.rz[col] = s.rz2;
    }
    a.alpha1[col] = s.alpha1;
    a.alpha2[col] = s.alpha2;
    a.beta1[col] = s.beta1;
    a.beta2[col] = s.beta2;
    res1 = nanmax(res1, s.res1);
    res2 = nanmax(res2, s.res2);
    usable &= s.usable ? 1 : 0;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    res1 = nanmax(res1, __shfl_xor(res1, off, 64));
    res2 = nanmax(res2, __shfl_xor(res2, off, 64));
    res3 = nanmax(res3, __shfl_xor(res3, off, 64));
    res4 = nanmax(res4, __shfl_xor(res4, off, 64));
    usable &= __shfl_xor(usable, off, 64);
  }
  if ((threadIdx.x & 63) == 0)
    sh1[threadIdx.x >> 6] = res1, sh2[threadIdx.x >> 6] = res2, sh3[threadIdx.x >> 6] = res3, sh4[threadIdx.x >> 6] = res4,
                       shu[threadIdx.x >> 6] = usable;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w)
      res1 = nanmax(res1, sh1[w]), res2 = nanmax(res2, sh2[w]), res3 = nanmax(res3, sh3[w]), res4 = nanmax(res4, sh4[w]), usable &= shu[w];
    if (!usable) res1 = res2 = res3 = res4 = 0.f;
    a.res_slots[1] = __float_as_uint(res1);
    a.res_slots[2] = __float_as_uint(res2);
    a.go[0] = (usable && res1 > a.tol && res2 > a.tol) ? 1u : 0u;
    uint32_t go1 = 0u;
    if (three) {
      a.res_slots[3] = __float_as_uint(res3);
      go1 = (usable && res1 > a.tol && res2 > a.tol && res3 > a.tol) ? 1u : 0u;
      a.go[1] = go1;
    }
    // the solve ends in iteration 4 and in no earlier one: host::anchor_gram4_last_form on the floats published below (NaN: 0)
    a.go[2] = (four && go1 == 1u && res4 <= a.tol) ? 1u : 0u;
    // (no device slot for the fourth residual: where the host keeps iteration 4 on the summed route, k_reduce_beta forms that
    // slot by atomicMax over zero, and where it does not, nothing is launched that would read it as a gate)
    __threadfence();
    // words 4, 3 and 2 first: the host polls word 1, and once it has that it may give the solve up and reuse the words (run_cg)
    if (four) {
      reinterpret_cast<volatile uint32_t*>(a.host_words)[4] = __float_as_uint(res4);
      __threadfence_system();
    }
    if (three) {
      reinterpret_cast<volatile uint32_t*>(a.host_words)[3] = __float_as_uint(res3);
      __threadfence_system();
    }
    reinterpret_cast<volatile uint32_t*>(a.host_words)[2] = __float_as_uint(res2);
    __threadfence_system();
    reinterpret_cast<volatile uint32_t*>(a.host_words)[1] = __float_as_uint(res1);
    __threadfence_system();
  }
}

// s_i = sum_j W_ij over the ELL row, in stored order: one thread per row (BlkInitAp::wsum)
__global__ __launch_bounds__(256) void k_row_weight_sums(const float* w, const int32_t* deg, int32_t width, int32_t N, float* out) {
  const int row = (int)(blockIdx.x * 256 + threadIdx.x);
  if (row >= N) return;
  float s = 0.f;
  const int d = min(deg[row], width);
  for (int e = 0; e < d; ++e) s = __fadd_rn(s, w[(size_t)row * width + e]);
  out[row] = s;
}

// out_i = sum_j W_ij v_j over the ELL row, in stored order: one thread per row (BlkInitAp2::wsum2 = W (W 1))
__global__ __launch_bounds__(256) void k_row_weighted_sums(const int32_t* col, const float* w, const int32_t* deg, int32_t width, int32_t N,
                                                           const float* v, float* out) {
  const int row = (int)(blockIdx.x * 256 + threadIdx.x);
  if (row >= N) return;
  float s = 0.f;
  const int d = min(deg[row], width);
  for (int e = 0; e < d; ++e) {
    const int j = col[(size_t)row * width + e];
    if (j >= 0 && j < N) s = fmaf(w[(size_t)row * width + e], v[j], s);
  }
  out[row] = s;
}

// chain prior for k_apply_blocked (ChainFixArgs): one wave per (64 columns, chunk of path rows), one thread per column
__global__ __launch_bounds__(64) void k_chain_fix(const ChainFixArgs a) {
  if (a.gate != nullptr && *a.gate <= a.gate_tol) return;
  const int col = a.c0 + (int)blockIdx.x * 64 + (int)threadIdx.x;
  const int chunk = (int)blockIdx.y;
  const int per = (a.prows + a.chunks - 1) / a.chunks;
  const int s0 = chunk * per, s1 = min(a.prows, s0 + per);
  float dotc = 0.f;
  if (col < a.c1) {
    const float* xs = a.X + (size_t)(col >> 5) * (size_t)a.N * 32 + (col & 31);  // this column of the slab-major operand
    for (int s = s0; s < s1; ++s) {
      const int i = a.prow[s], d = a.pdeg[s];
      float acc = 0.f;
      for (int e = 0; e < d; ++e) acc = fmaf(a.pw[(size_t)s * a.pwidth + e], xs[(size_t)a.pcol[(size_t)s * a.pwidth + e] * 32], acc);
      const float o = -a.cP * acc;
      if (a.initR != nullptr) {  // behind the fused INIT pass: r and z of this row lack the chain term, and so does r . z
        const float invMd = 1.f / (fmaf(a.md_B, a.B[i], a.md_const) + 1e-12f);
        float* zp = a.initZ + (size_t)(col >> 5) * (size_t)a.N * 32 + (size_t)i * 32 + (col & 31);
        const float r0 = a.initR[(size_t)i * a.ld + col], z0 = *zp;
        const float r1 = r0 - o, z1 = r1 * invMd;
        a.initR[(size_t)i * a.ld + col] = r1;
        *zp = z1;
        dotc += r1 * z1 - r0 * z0;
        continue;
      }
      a.OUT[(size_t)i * a.ld + col] += o;
      dotc = fmaf(xs[(size_t)i * 32], o, dotc);
    }
    a.part[(size_t)(a.part_row0 + chunk) * a.ld + col] = dotc;
  }
}

// ---- build of the block-major graph copy ----------------------------------------------------
__device__ __forceinline__ int blk_of(int col, int rpb, int nb) { return min(nb - 1, col / rpb); }

// Placement of a row's edges in the block-major copy: an edge goes into the slot row of its own block while that has room
// (slots 0 .. c - 1 for the block's c <= SL own edges, ascending columns); an edge that finds its block full moves to
// the first later block (cyclically) whose slot row has room behind that block's own edges -- it is then gathered while
// another block is the resident one, i.e. as a miss among hits, but inside the regular rounds; only what fits nowhere
// (degree > SL * nb) goes to the `over` list of the epilogue.  Deterministic: everything follows the ELL row's order.
__device__ __forceinline__ int blk_unplaced(const int (&c)[OSC_MAX_SRC_BLOCKS]) {
  int excess = 0, room = 0;
#pragma unroll
  for (int q = 0; q < OSC_MAX_SRC_BLOCKS; ++q) {
    excess += max(0, c[q] - OSC_BLK_SLOTS);
    room += max(0, OSC_BLK_SLOTS - c[q]);  // (blocks q >= nb have c = SL: see the callers)
  }
  return max(0, excess - room);
}

// edges that fit no slot row, in total
__global__ void k_blk_count(const int32_t* col, const int32_t* deg, int32_t width, int32_t N, int32_t nb, int32_t rpb,
                            unsigned* over_count) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= N) return;
  int c[OSC_MAX_SRC_BLOCKS];
#pragma unroll
  for (int k = 0; k < OSC_MAX_SRC_BLOCKS; ++k) c[k] = k < nb ? 0 : OSC_BLK_SLOTS;
  const int d = deg[row];
  for (int e = 0; e < d; ++e) {
    const int b = blk_of(col[(size_t)row * width + e], rpb, nb);
#pragma unroll
    for (int k = 0; k < OSC_MAX_SRC_BLOCKS; ++k) c[k] += (k == b);
  }
  const int over = blk_unplaced(c);
  if (over) atomicAdd(over_count, (unsigned)over);
}

// *over_count must be zero on entry (it hands out the ranges of `over`); every slot is written
__global__ void k_blk_fill(const int32_t* col, const float* w, const int32_t* deg, int32_t width, int32_t N, int32_t nb,
                           int32_t rpb, int2* slots, int2* rest, int2* over, unsigned* over_count) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= N) return;
  int c[OSC_MAX_SRC_BLOCKS], k[OSC_MAX_SRC_BLOCKS], tail[OSC_MAX_SRC_BLOCKS];
#pragma unroll
  for (int q = 0; q < OSC_MAX_SRC_BLOCKS; ++q) c[q] = q < nb ? 0 : OSC_BLK_SLOTS, k[q] = 0;
  const int d = deg[row];
  for (int e = 0; e < d; ++e) {
    const int b = blk_of(col[(size_t)row * width + e], rpb, nb);
#pragma unroll
    for (int q = 0; q < OSC_MAX_SRC_BLOCKS; ++q) c[q] += (q == b);
  }
#pragma unroll
  for (int q = 0; q < OSC_MAX_SRC_BLOCKS; ++q) tail[q] = min(c[q], OSC_BLK_SLOTS);  // first slot behind the own edges
  const int total = blk_unplaced(c);
  unsigned at = total ? atomicAdd(over_count, (unsigned)total) : 0u;
  rest[row] = make_int2((int)at, total);
  for (int e = 0; e < d; ++e) {
    const int j = col[(size_t)row * width + e];
    const int b = blk_of(j, rpb, nb);
    int kb = 0;
#pragma unroll
    for (int q = 0; q < OSC_MAX_SRC_BLOCKS; ++q)
      if (q == b) kb = k[q]++;
    const int2 ent = make_int2(j, __float_as_int(w[(size_t)row * width + e]));
    if (kb < OSC_BLK_SLOTS) {
      slots[((size_t)b * N + row) * OSC_BLK_SLOTS + kb] = ent;
      continue;
    }
    int tb = -1, ts = 0;  // first block after b (cyclically) with room
    for (int step = 1; step < nb && tb < 0; ++step) {
      const int q = (b + step) % nb;
#pragma unroll
      for (int t = 0; t < OSC_MAX_SRC_BLOCKS; ++t)
        if (t == q && tail[t] < OSC_BLK_SLOTS) tb = q, ts = tail[t]++;
    }
    if (tb >= 0) slots[((size_t)tb * N + row) * OSC_BLK_SLOTS + ts] = ent;
    else over[at++] = ent;
  }
  // unused slots: a row every wave gathering from block q has in its caches anyway, weight zero
#pragma unroll
  for (int q = 0; q < OSC_MAX_SRC_BLOCKS; ++q)
    if (q < nb)
      for (int t = tail[q]; t < OSC_BLK_SLOTS; ++t)
        slots[((size_t)q * N + row) * OSC_BLK_SLOTS + t] = make_int2(min(N - 1, q * rpb), 0);
}

// ---- initial residual around the blocked matvec (InitFinishArgs) ---------------------------------------------------
// DIFF: dst = src - minus (the receipt's U - U*, formed on the way into the slabs: no row-major copy of the difference)
template <int LPR, int NCH, bool DIFF = false>
__global__ __launch_bounds__(256) void k_rows_to_slab(const float* src, float* dst, int64_t N, int32_t ld, int32_t c0,
                                                      int32_t c1, const float* minus = nullptr) {
  constexpr int RPW = 64 / LPR;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane / LPR, lr = lane % LPR;
  for (int64_t rb = ((int64_t)blockIdx.x * 4 + wave) * RPW; rb < N; rb += (int64_t)gridDim.x * 4 * RPW) {
    const int row = (int)rb + sub;
    if (row >= N) continue;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int col = c0 + (ch * LPR + lr) * 4;
      if (col < c1) {
        float4 v = ld4_stream(src + (size_t)row * ld + col);
        if constexpr (DIFF) {
          const float4 w = ld4_stream(minus + (size_t)row * ld + col);
          v = make_float4(v.x - w.x, v.y - w.y, v.z - w.z, v.w - w.w);
        }
        st4(dst + blk_off(N, row, col), v);
      }
    }
  }
}

template <int LPR, int NCH>
__global__ __launch_bounds__(256) void k_init_finish(const InitFinishArgs a) {
  constexpr int RPW = 64 / LPR;
  constexpr int CPW = NCH * LPR * 4;
  __shared__ __attribute__((aligned(16))) float red[4 * CPW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane / LPR, lr = lane % LPR;
  const int32_t ld = a.ld;
  int coff[NCH];
  bool cok[NCH];
  float4 psi4[NCH], rz[NCH];
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    coff[ch] = a.c0 + (ch * LPR + lr) * 4;
    cok[ch] = coff[ch] < a.c1;
    psi4[ch] = cok[ch] ? ld4(a.psi + coff[ch]) : f4(0.f);
    rz[ch] = f4(0.f);
  }
  for (int64_t rb = ((int64_t)blockIdx.x * 4 + wave) * RPW; rb < a.N; rb += (int64_t)gridDim.x * 4 * RPW) {
    const int row = (int)rb + sub;
    if (row >= a.N) continue;
    const float Bi = a.B[row];
    float invMd = 1.f;
    if (a.op.precond) invMd = 1.f / (fmaf(a.op.md_B, Bi, a.op.md_const) + 1e-12f);
    const float qb = a.op.rbB * Bi;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      if (!cok[ch]) continue;
      const size_t off = (size_t)row * ld + coff[ch];
      const float4 o = ld4_stream(a.AP + off);
      const float4 xs = ld4_stream(a.X0 + off);
      const float4 u = (a.U == a.X0) ? xs : (a.op.rbU != 0.f ? ld4_stream(a.U + off) : f4(0.f));
      const float4 y = (a.Y == a.X0) ? xs : ld4_stream(a.Y + off);
      float4 r, z;
      r.x = (a.op.rbU * u.x + a.op.rbY * y.x + qb * psi4[ch].x) - o.x;
      r.y = (a.op.rbU * u.y + a.op.rbY * y.y + qb * psi4[ch].y) - o.y;
      r.z = (a.op.rbU * u.z + a.op.rbY * y.z + qb * psi4[ch].z) - o.z;
      r.w = (a.op.rbU * u.w + a.op.rbY * y.w + qb * psi4[ch].w) - o.w;
      z = make_float4(r.x * invMd, r.y * invMd, r.z * invMd, r.w * invMd);
      if (a.X != a.X0) st4_stream(a.X + off, xs);
      st4_stream(a.R + off, r);
      st4(a.P + blk_off(a.pblk, row, coff[ch]), z);
      rz[ch] = mulacc4(r, z, rz[ch]);
    }
  }
  block_fold<LPR, NCH>(rz, red, a.part, ld, a.c0, a.c1);
}

// ---------------------------------------------------------------------------------------------
// WITHX = false: the x update of this iteration is left to the next iteration's k_update_p (or to k_update_x behind the
// last one): this kernel then moves r and Ap only (run_cg).
// STORE_R = false (with WITHX): the form for an iteration expected to be the solve's last -- x is finished here and the new
// r only feeds the two column sums; should the solve go on after all, the host has the r update redone with a store.
// WITHX = false, STORE_R = false: the expected last iteration of a solve that keeps its directions in a ring (run_cg) -- r
// and Ap are read, nothing but the two column sums is written.
template <int LPR, int NCH, bool WITHX, bool STORE_R = true>
__global__ __launch_bounds__(256) void k_update_xr(const UpdateArgs a) {
  constexpr int RPW = 64 / LPR;
  constexpr int CPW = NCH * LPR * 4;
  __shared__ __attribute__((aligned(16))) float red[4 * CPW];
  if (a.gate != nullptr && *a.gate <= a.gate_tol) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane / LPR, lr = lane % LPR;
  const int32_t ld = a.ld;
  const bool tmp = a.temporal != 0;
  [[maybe_unused]] const float* const xin = a.Xin != nullptr ? a.Xin : a.X;  // (UpdateArgs::Xin: iteration 1 of an anchor-start settle)
  int coff[NCH];
  bool cok[NCH];
  float4 al[NCH], rr[NCH], rz[NCH];
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    coff[ch] = a.c0 + (ch * LPR + lr) * 4;
    cok[ch] = coff[ch] < a.c1;
    al[ch] = cok[ch] ? ld4(a.alpha + coff[ch]) : f4(0.f);
    rr[ch] = f4(0.f);
    rz[ch] = f4(0.f);
  }
  const int64_t rend = a.N;  // streaming kernels: plain grid-stride over the row range
  for (int64_t rb = a.row0 + ((int64_t)blockIdx.x * 4 + wave) * RPW; rb < rend; rb += (int64_t)gridDim.x * 4 * RPW) {
    const int row = (int)rb + sub;
    if (row >= rend) continue;
    float invMd = 1.f;
    if (a.op.precond) invMd = 1.f / (fmaf(a.op.md_B, a.B[row], a.op.md_const) + 1e-12f);
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      if (!cok[ch]) continue;
      const size_t off = (size_t)row * ld + coff[ch];
      float4 r = ld4_sel(a.R + off, tmp);
      const float4 ap = ld4_sel(a.AP + off, tmp);
      if constexpr (WITHX) {
        float4 x = ld4_sel(xin + off, tmp);
        const float4 p = ld4_sel(a.P + p_off(a, row, coff[ch]), tmp);
        x.x = fmaf(p.x, al[ch].x, x.x); x.y = fmaf(p.y, al[ch].y, x.y);
        x.z = fmaf(p.z, al[ch].z, x.z); x.w = fmaf(p.w, al[ch].w, x.w);
        st4_sel(a.X + off, x, tmp);
      }
      r.x = fmaf(-ap.x, al[ch].x, r.x); r.y = fmaf(-ap.y, al[ch].y, r.y);
      r.z = fmaf(-ap.z, al[ch].z, r.z); r.w = fmaf(-ap.w, al[ch].w, r.w);
      if constexpr (STORE_R) st4_sel(a.R + off, r, tmp);
      rr[ch] = mulacc4(r, r, rr[ch]);
      const float4 z = make_float4(r.x * invMd, r.y * invMd, r.z * invMd, r.w * invMd);
      rz[ch] = mulacc4(r, z, rz[ch]);
    }
  }
  block_fold<LPR, NCH>(rr, red, a.part_rr, ld, a.c0, a.c1);
  block_fold<LPR, NCH>(rz, red, a.part_rz, ld, a.c0, a.c1);
}

// WITHX: also the PREVIOUS iteration's x update, x += alpha p with the p this kernel is about to replace (alpha is still
// that iteration's: the next reduce_alpha comes behind the matvec).  WITHX and UPD_P = false: only that (behind the last
// iteration of a solve).
template <int LPR, int NCH, bool WITHX, bool UPD_P = true>
__global__ __launch_bounds__(256) void k_update_p(const UpdateArgs a) {
  constexpr int RPW = 64 / LPR;
  if (a.gate != nullptr && *a.gate <= a.gate_tol) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane / LPR, lr = lane % LPR;
  const int32_t ld = a.ld;
  const bool tmp = a.temporal != 0;
  [[maybe_unused]] const float* const xin = a.Xin != nullptr ? a.Xin : a.X;  // (UpdateArgs::Xin)
  float* const pout = a.Pout != nullptr ? a.Pout : a.P;                       // (UpdateArgs::Pout)
  int coff[NCH];
  bool cok[NCH];
  float4 be[NCH], al[NCH];
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    coff[ch] = a.c0 + (ch * LPR + lr) * 4;
    cok[ch] = coff[ch] < a.c1;
    be[ch] = (cok[ch] && UPD_P) ? ld4(a.beta + coff[ch]) : f4(0.f);
    al[ch] = (cok[ch] && WITHX) ? ld4(a.alpha + coff[ch]) : f4(0.f);
  }
  const int64_t rend = a.N;  // streaming kernels: plain grid-stride over the row range
  for (int64_t rb = a.row0 + ((int64_t)blockIdx.x * 4 + wave) * RPW; rb < rend; rb += (int64_t)gridDim.x * 4 * RPW) {
    const int row = (int)rb + sub;
    if (row >= rend) continue;
    float invMd = 1.f;
    if (UPD_P && a.op.precond) invMd = 1.f / (fmaf(a.op.md_B, a.B[row], a.op.md_const) + 1e-12f);
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      if (!cok[ch]) continue;
      const size_t off = (size_t)row * ld + coff[ch];
      const size_t poff = p_off(a, row, coff[ch]);
      float4 p = ld4_sel(a.P + poff, tmp);
      if constexpr (WITHX) {
        float4 x = ld4_sel(xin + off, tmp);
        x.x = fmaf(p.x, al[ch].x, x.x); x.y = fmaf(p.y, al[ch].y, x.y);
        x.z = fmaf(p.z, al[ch].z, x.z); x.w = fmaf(p.w, al[ch].w, x.w);
        st4_sel(a.X + off, x, tmp);
      }
      if constexpr (UPD_P) {
        const float4 r = ld4_sel(a.R + off, tmp);
        p.x = fmaf(p.x, be[ch].x, r.x * invMd); p.y = fmaf(p.y, be[ch].y, r.y * invMd);
        p.z = fmaf(p.z, be[ch].z, r.z * invMd); p.w = fmaf(p.w, be[ch].w, r.w * invMd);
        st4(pout + poff, p);
      }
    }
  }
}

// Iteration 2's p update of an anchor start whose INIT pass left Q1 = A p1 (in the AP array) and T = A Q1 (UpdateArgs::T):
// p2 = z1 + beta1 p1 as k_update_p forms it (same operands, same order, and its WITHX form of iteration 1's x update), and
// with both in hand A p2 = A z1 + beta1 Q1 = (1 + beta1) Q1 - (m alpha1) T, since z1 = m (r0 - alpha1 Q1) and A r0 = Q1 / m
// under uniform gates (m the same in every row; alpha1, beta1 column scalars, which commute with A).  A p2 goes over Q1, the
// column partials of p2 . A p2 to part_rr (block_fold: deterministic), where the alpha reduction of an iteration reads them:
// the iteration launches no matvec.
template <int LPR, int NCH, bool WITHX>
__global__ __launch_bounds__(256) void k_update_p_ap2(const UpdateArgs a) {
  constexpr int RPW = 64 / LPR;
  constexpr int CPW = NCH * LPR * 4;
  __shared__ __attribute__((aligned(16))) float red[4 * CPW];
  if (a.gate != nullptr && *a.gate <= a.gate_tol) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane / LPR, lr = lane % LPR;
  const int32_t ld = a.ld;
  const bool tmp = a.temporal != 0;
  [[maybe_unused]] const float* const xin = a.Xin != nullptr ? a.Xin : a.X;
  float* const pout = a.Pout != nullptr ? a.Pout : a.P;
  int coff[NCH];
  bool cok[NCH];
  float4 be[NCH], al[NCH], pap[NCH];
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    coff[ch] = a.c0 + (ch * LPR + lr) * 4;
    cok[ch] = coff[ch] < a.c1;
    be[ch] = cok[ch] ? ld4(a.beta + coff[ch]) : f4(0.f);
    al[ch] = cok[ch] ? ld4(a.alpha + coff[ch]) : f4(0.f);
    pap[ch] = f4(0.f);
  }
  const int64_t rend = a.N;
  for (int64_t rb = a.row0 + ((int64_t)blockIdx.x * 4 + wave) * RPW; rb < rend; rb += (int64_t)gridDim.x * 4 * RPW) {
    const int row = (int)rb + sub;
    if (row >= rend) continue;
    float invMd = 1.f;
    if (a.op.precond) invMd = 1.f / (fmaf(a.op.md_B, a.B[row], a.op.md_const) + 1e-12f);
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      if (!cok[ch]) continue;
      const size_t off = (size_t)row * ld + coff[ch];
      const size_t poff = p_off(a, row, coff[ch]);
      float4 p = ld4_sel(a.P + poff, tmp);
      const float4 r = ld4_sel(a.R + off, tmp);
      const float4 q = ld4_sel(a.AP + off, tmp);
      const float4 t = ld4_stream(a.T + off);
      if constexpr (WITHX) {
        float4 x = ld4_sel(xin + off, tmp);
        x.x = fmaf(p.x, al[ch].x, x.x); x.y = fmaf(p.y, al[ch].y, x.y);
        x.z = fmaf(p.z, al[ch].z, x.z); x.w = fmaf(p.w, al[ch].w, x.w);
        st4_sel(a.X + off, x, tmp);
      }
      p.x = fmaf(p.x, be[ch].x, r.x * invMd); p.y = fmaf(p.y, be[ch].y, r.y * invMd);
      p.z = fmaf(p.z, be[ch].z, r.z * invMd); p.w = fmaf(p.w, be[ch].w, r.w * invMd);
      st4(pout + poff, p);
      auto one = [&](float qv, float tv, float bv, float av) {
        return fmaf(__fadd_rn(1.f, bv), qv, -__fmul_rn(__fmul_rn(invMd, av), tv));
      };
      const float4 o = make_float4(one(q.x, t.x, be[ch].x, al[ch].x), one(q.y, t.y, be[ch].y, al[ch].y),
                                   one(q.z, t.z, be[ch].z, al[ch].z), one(q.w, t.w, be[ch].w, al[ch].w));
      st4_sel(a.APout + off, o, tmp);
      pap[ch] = mulacc4(p, o, pap[ch]);
    }
  }
  block_fold<LPR, NCH>(pap, red, a.part_rr, ld, a.c0, a.c1);
}

// x = xin + alpha_1 p_1 + ... + alpha_M p_M from a ring of kept directions (XRingArgs), oldest first: the only kernel of such
// a solve that touches x.  All M + 1 loads of a chunk are issued before the first fmaf.  In place (xin == X): a thread reads
// and writes the same element.
template <int LPR, int NCH, int M>
__global__ __launch_bounds__(256) void k_update_x_ring(const XRingArgs a) {
  constexpr int RPW = 64 / LPR;
  if (a.gate != nullptr && *a.gate <= a.gate_tol) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane / LPR, lr = lane % LPR;
  const int32_t ld = a.ld;
  const bool tmp = a.temporal != 0;
  const float* const xin = a.Xin != nullptr ? a.Xin : a.X;
  int coff[NCH];
  bool cok[NCH];
  float4 al[M][NCH];
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    coff[ch] = a.c0 + (ch * LPR + lr) * 4;
    cok[ch] = coff[ch] < a.c1;
#pragma unroll
    for (int m = 0; m < M; ++m) al[m][ch] = cok[ch] ? ld4(a.alpha[m] + coff[ch]) : f4(0.f);
  }
  const int64_t rend = a.N;  // streaming kernels: plain grid-stride over the row range
  for (int64_t rb = a.row0 + ((int64_t)blockIdx.x * 4 + wave) * RPW; rb < rend; rb += (int64_t)gridDim.x * 4 * RPW) {
    const int row = (int)rb + sub;
    if (row >= rend) continue;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      if (!cok[ch]) continue;
      const size_t off = (size_t)row * ld + coff[ch];
      const size_t poff = a.pblk ? blk_off(a.pblk, row, coff[ch]) : off;
      float4 x = ld4_sel(xin + off, tmp);
      float4 p[M];
#pragma unroll
      for (int m = 0; m < M; ++m) p[m] = ld4_sel(a.P[m] + poff, tmp);
#pragma unroll
      for (int m = 0; m < M; ++m) {
        x.x = fmaf(p[m].x, al[m][ch].x, x.x); x.y = fmaf(p[m].y, al[m][ch].y, x.y);
        x.z = fmaf(p[m].z, al[m][ch].z, x.z); x.w = fmaf(p[m].w, al[m][ch].w, x.w);
      }
      st4_sel(a.X + off, x, tmp);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// second stage of the column reductions: 64 columns per block, 16 row-groups, fp64 accumulation
template <int NIN>
__device__ __forceinline__ bool reduce_cols(const float* p0, const float* p1, int nb, int32_t ld, int32_t c0,
                                            int32_t c1, double (&tot)[NIN], int& col) {
  __shared__ double sh[NIN][16][64];
  const int cl = threadIdx.x & 63, g = threadIdx.x >> 6;
  col = c0 + blockIdx.x * 64 + cl;
  const bool ok = col < c1;
  double s[NIN];
#pragma unroll
  for (int i = 0; i < NIN; ++i) s[i] = 0.0;
  if (ok) {
    // 8 independent loads in flight per input: the loop is latency-bound, not bandwidth-bound
    int b = g;
    for (; b + 7 * 16 < nb; b += 8 * 16) {
      float v0[8], v1[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        v0[u] = p0[(size_t)(b + 16 * u) * ld + col];
        if (NIN > 1) v1[u] = p1[(size_t)(b + 16 * u) * ld + col];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        s[0] += (double)v0[u];
        if (NIN > 1) s[NIN - 1] += (double)v1[u];
      }
    }
    for (; b < nb; b += 16) {
      s[0] += (double)p0[(size_t)b * ld + col];
      if (NIN > 1) s[NIN - 1] += (double)p1[(size_t)b * ld + col];
    }
  }
#pragma unroll
  for (int i = 0; i < NIN; ++i) sh[i][g][cl] = s[i];
  __syncthreads();
  if (g == 0) {
#pragma unroll
    for (int i = 0; i < NIN; ++i) {
      double t = 0.0;
#pragma unroll
      for (int k = 0; k < 16; ++k) t += sh[i][k][cl];
      tot[i] = t;
    }
  }
  return ok && g == 0;
}

__global__ __launch_bounds__(1024) void k_reduce_init(const float* part, int nb, int32_t ld, int32_t c0, int32_t c1,
                                                      double* rz) {
  double t[1];
  int col;
  if (reduce_cols<1>(part, nullptr, nb, ld, c0, c1, t, col)) rz[col] = t[0];
}

__global__ __launch_bounds__(1024) void k_reduce_alpha(const float* part, int nb, int32_t ld, int32_t c0, int32_t c1,
                                                       const double* rz, float* alpha, Gate gt) {
  if (gt.p != nullptr && *gt.p <= gt.tol) return;
  double t[1];
  int col;
  if (reduce_cols<1>(part, nullptr, nb, ld, c0, c1, t, col))
    alpha[col] = (float)(rz[col] / (t[0] + 1e-18));  // solver.py:25-26
}

// host_slot != nullptr: the last workgroup to finish publishes the iteration's residual straight into host-mapped
// memory (the host polls that word instead of paying a 4-byte copy + event + event wait per iteration); done_ctr is
// this iteration's arrival counter (zeroed with the residual slots).
__global__ __launch_bounds__(1024) void k_reduce_beta(const float* part_rr, const float* part_rz, int nb, int32_t ld,
                                                      int32_t c0, int32_t c1, double* rz, float* beta,
                                                      uint32_t* res_bits, Gate gt, uint32_t* done_ctr,
                                                      float* host_slot) {
  if (gt.p != nullptr && *gt.p <= gt.tol) return;
  double t[2];
  int col;
  const bool w = reduce_cols<2>(part_rr, part_rz, nb, ld, c0, c1, t, col);
  float resc = 0.f;
  if (w) {
    resc = (float)sqrt(t[0]);                            // ||r_c||_2        (solver.py:29)
    beta[col] = (float)(t[1] / (rz[col] + 1e-18));       // solver.py:33-34
    rz[col] = t[1];
  }
  if ((threadIdx.x >> 6) == 0) {  // wave 0 holds the 64 column residuals of this block
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) resc = nanmax(resc, __shfl_xor(resc, o, 64));
    if ((threadIdx.x & 63) == 0) {
      atomicMax(res_bits, __float_as_uint(resc));  // non-negative floats order as uints
      if (host_slot != nullptr) {
        __threadfence();
        if (atomicAdd(done_ctr, 1u) == gridDim.x - 1) {      // every workgroup's maximum is in
          const uint32_t bits = atomicMax(res_bits, 0u);     // read it back through the same (coherent) path
          *reinterpret_cast<volatile uint32_t*>(host_slot) = bits;
          __threadfence_system();
        }
      }
    }
  }
}

__global__ __launch_bounds__(1024) void k_reduce_sum(const float* part, int nb, int32_t ld, int32_t c0, int32_t c1,
                                                     double* out_cols, Gate gt) {
  if (gt.p != nullptr && *gt.p <= gt.tol) return;
  double t[1];
  int col;
  if (reduce_cols<1>(part, nullptr, nb, ld, c0, c1, t, col)) out_cols[col] = t[0];
}

// finish steps of the row-sharded CG (sums already complete across ranks)
__global__ void k_finish_init(const double* sums, int32_t c0, int32_t c1, double* rz) {
  const int col = c0 + blockIdx.x * blockDim.x + threadIdx.x;
  if (col < c1) rz[col] = sums[col];
}
__global__ void k_finish_alpha(const double* sums, int32_t c0, int32_t c1, const double* rz, float* alpha, Gate gt) {
  if (gt.p != nullptr && *gt.p <= gt.tol) return;
  const int col = c0 + blockIdx.x * blockDim.x + threadIdx.x;
  if (col < c1) alpha[col] = (float)(rz[col] / (sums[col] + 1e-18));
}
__global__ __launch_bounds__(256) void k_finish_beta(const double* srr, const double* srz, int32_t c0, int32_t c1,
                                                     double* rz, float* beta, uint32_t* res_bits, Gate gt) {
  if (gt.p != nullptr && *gt.p <= gt.tol) return;
  const int col = c0 + blockIdx.x * blockDim.x + threadIdx.x;
  float resc = 0.f;
  if (col < c1) {
    resc = (float)sqrt(srr[col]);
    beta[col] = (float)(srz[col] / (rz[col] + 1e-18));
    rz[col] = srz[col];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) resc = nanmax(resc, __shfl_xor(resc, o, 64));
  if ((threadIdx.x & 63) == 0) atomicMax(res_bits, __float_as_uint(resc));
}

__global__ __launch_bounds__(256) void k_axpby(float* out, const float* a, float ca, const float* b, float cb,
                                               int64_t n4) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 x = ld4(a + i * 4), y = ld4(b + i * 4);
    st4(out + i * 4, make_float4(ca * x.x + cb * y.x, ca * x.y + cb * y.y, ca * x.z + cb * y.z, ca * x.w + cb * y.w));
  }
}

// ---- dispatch -------------------------------------------------------------------------------
struct Shape {
  int lpr, nch;
};
// lanes per row x float4 chunks per lane.  Exact-fit shapes for 96 / 192 / 384 columns (the per-rank windows of D = 768
// on 8 / 4 / 2 GPUs: <8,3>, <16,3>, <32,3>) were measured and are no faster than the padded ones below (the apply is
// bound by the gathered bytes, not by idle lanes), so they are not instantiated.
inline Shape pick_shape(int ncols) {
  if (ncols <= 16) return {4, 1};  // single right-hand sides (diffusion gates: pitch 4) and very narrow lattices
  if (ncols <= 64) return {16, 1};
  if (ncols <= 128) return {32, 1};
  int nch = (ncols + 255) / 256;
  if (nch == 5) nch = 6;
  if (nch == 7) nch = 8;
  if (nch > 8) throw std::runtime_error("column window wider than 2048; split it");
  return {64, nch};
}

#define OSC_SHAPE_SWITCH(sh, CALL)                                   \
  do {                                                               \
    if ((sh).lpr == 4) { CALL(4, 1); }                               \
    else if ((sh).lpr == 16) { CALL(16, 1); }                        \
    else if ((sh).lpr == 32) { CALL(32, 1); }                        \
    else switch ((sh).nch) {                                         \
      case 1: CALL(64, 1); break;                                    \
      case 2: CALL(64, 2); break;                                    \
      case 3: CALL(64, 3); break;                                    \
      case 4: CALL(64, 4); break;                                    \
      case 6: CALL(64, 6); break;                                    \
      default: CALL(64, 8); break;                                   \
    }                                                                \
  } while (0)

// k_init_two_steps_stream: lanes per row x float4 chunks per lane x row groups per trip of one column tile; a window wider than a
// tile takes several (blockIdx.y), cut evenly.  Up to 768 columns these are the update kernels' shapes (pick_shape) on the solve's
// grid: the sweep at 100 000 x 768 over chunks, rows per trip and grid is flat (profiles/two_steps_stream_sweep.txt; RPT > 1 is
// instantiated by scripts/exp/two_steps_stream_sweep.hip alone).
struct TwoStepsShape {
  int lpr, nch, rpt;
};
inline TwoStepsShape pick_two_steps_shape(int ncols) {
  if (ncols <= 64) return {16, 1, 1};
  if (ncols <= 128) return {32, 1, 1};
  const int tiles = (ncols + 767) / 768;
  return {64, ((ncols + tiles - 1) / tiles + 255) / 256, 1};
}
#define OSC_TWO_STEPS_SHAPE_SWITCH(sh, CALL)                         \
  do {                                                               \
    if ((sh).lpr == 16) { CALL(16, 1, 1); }                          \
    else if ((sh).lpr == 32) { CALL(32, 1, 1); }                     \
    else switch ((sh).nch) {                                         \
      case 1: CALL(64, 1, 1); break;                                 \
      case 2: CALL(64, 2, 1); break;                                 \
      default: CALL(64, 3, 1); break;                                \
    }                                                                \
  } while (0)

}  // namespace

int spmm_grid(int64_t N, int32_t ncols) {
  const Shape sh = pick_shape(ncols);
  const int rpw = 64 / sh.lpr;
  const int64_t need = (N + 4 * rpw - 1) / (4 * rpw);
  return (int)std::max<int64_t>(1, std::min<int64_t>(need, 1024));
}

static void blocked_check(int32_t N, int32_t width, int32_t nb) {
  if (nb < 1 || nb > OSC_MAX_SRC_BLOCKS) throw std::runtime_error("blocked graph copy: too many source blocks");
  if ((int64_t)N * width >= ((int64_t)1 << 28) || (int64_t)N >= ((int64_t)1 << 24))  // 32-bit byte offsets in the apply
    throw std::runtime_error("blocked graph copy: lattice too large");
}
void launch_blocked_count(const int32_t* col, const int32_t* deg, int32_t width, int32_t N, int32_t nb,
                          unsigned* over_count, hipStream_t s) {
  blocked_check(N, width, nb);
  hipLaunchKernelGGL(k_blk_count, dim3((N + 255) / 256), dim3(256), 0, s, col, deg, width, N, nb, host::blocked_rows_per_block(N, nb),
                     over_count);
  HIP_CHECK(hipGetLastError());
}
void launch_blocked_fill(const int32_t* col, const float* w, const int32_t* deg, int32_t width, int32_t N, int32_t nb,
                         int2* slots, int2* rest, int2* over, unsigned* over_count, hipStream_t s) {
  blocked_check(N, width, nb);
  hipLaunchKernelGGL(k_blk_fill, dim3((N + 255) / 256), dim3(256), 0, s, col, w, deg, width, N, nb, host::blocked_rows_per_block(N, nb),
                     slots, rest, over, over_count);
  HIP_CHECK(hipGetLastError());
}
// one instantiation of k_apply_blocked per entry of kBlkShapes (host_logic.hpp)
#define OSC_BLK_SHAPE_CASE(v, CALL) \
  case v: CALL(kBlkShapes[v].gm, kBlkShapes[v].cw, kBlkShapes[v].pd, kBlkShapes[v].wpe); break;
#define OSC_BLK_SHAPE_SWITCH(v, CALL)                                         \
  switch (v) {                                                               \
    OSC_BLK_SHAPE_CASE(0, CALL) OSC_BLK_SHAPE_CASE(1, CALL) OSC_BLK_SHAPE_CASE(2, CALL) OSC_BLK_SHAPE_CASE(3, CALL) \
    OSC_BLK_SHAPE_CASE(4, CALL) OSC_BLK_SHAPE_CASE(5, CALL) OSC_BLK_SHAPE_CASE(6, CALL)                             \
    default: throw std::runtime_error("blocked apply: unknown kernel shape");    \
  }
static_assert(kBlkShapeCount == 7, "OSC_BLK_SHAPE_SWITCH needs one case per entry of kBlkShapes");
void launch_rows_to_slab(const float* src, float* dst, int64_t N, int32_t ld, int32_t c0, int32_t c1, int grid, hipStream_t s,
                         const float* sub) {
  for (int32_t s0 = c0; s0 < c1; s0 += 2048) {  // at most 2048 columns per launch, like the other elementwise kernels
    const int32_t s1 = std::min(c1, s0 + 2048);
    const Shape sh = pick_shape(s1 - s0);
    if (sub != nullptr) {
#define CALL(L, C) hipLaunchKernelGGL((k_rows_to_slab<L, C, true>), dim3(grid), dim3(256), 0, s, src, dst, N, ld, s0, s1, sub)
      OSC_SHAPE_SWITCH(sh, CALL);
#undef CALL
      continue;
    }
#define CALL(L, C) hipLaunchKernelGGL((k_rows_to_slab<L, C, false>), dim3(grid), dim3(256), 0, s, src, dst, N, ld, s0, s1, nullptr)
    OSC_SHAPE_SWITCH(sh, CALL);
#undef CALL
  }
  HIP_CHECK(hipGetLastError());
}
void launch_init_finish(const InitFinishArgs& a, int grid, hipStream_t s) {
  if (a.c1 - a.c0 > 2048) throw std::runtime_error("init_finish: column window wider than 2048");
  const Shape sh = pick_shape(a.c1 - a.c0);
#define CALL(L, C) hipLaunchKernelGGL((k_init_finish<L, C>), dim3(grid), dim3(256), 0, s, a)
  OSC_SHAPE_SWITCH(sh, CALL);
#undef CALL
  HIP_CHECK(hipGetLastError());
}
int chain_fix_chunks(int32_t prows) { return std::max(1, std::min(OSC_CHAIN_FIX_MAX_CHUNKS, (prows + 7) / 8)); }
void launch_chain_fix(const ChainFixArgs& a, hipStream_t s) {
  if (a.prows < 1 || a.prows > OSC_CHAIN_FIX_MAX_ROWS || a.chunks < 1 || a.chunks > OSC_CHAIN_FIX_MAX_CHUNKS || a.c1 <= a.c0)
    throw std::runtime_error("chain fix-up: unsupported arguments");
  hipLaunchKernelGGL(k_chain_fix, dim3((a.c1 - a.c0 + 63) / 64, a.chunks), dim3(64), 0, s, a);
  HIP_CHECK(hipGetLastError());
}
int blocked_resident_per_cu(int variant) {
  int n = 0;
#define CALL(G, W, P, E) HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_apply_blocked<G, W, false, P, E>, (W + 1) * 64, 0))
  OSC_BLK_SHAPE_SWITCH(variant, CALL);
#undef CALL
  return n;
}

static void blocked_args_check(const BlkArgs& a, int grid, int variant) {
  if (variant < 0 || variant >= kBlkShapeCount) throw std::runtime_error("blocked apply: unknown kernel shape");
  const BlkShape& sh = kBlkShapes[variant];
  if (grid < 8 || (grid & 7) != 0 || a.xs < 1 || a.xs > grid / 8 || a.xs_groups < 1 || 8 % a.xs_groups != 0 || a.groups < 1 ||
      a.groups > sh.gm || a.slices < 1 || a.nb < 1 || a.nb > OSC_MAX_SRC_BLOCKS || !a.slots || !a.rest ||
      (int64_t)a.N * a.ld * 4 >= ((int64_t)1 << 32) || (a.c0 & 31) != 0)
    throw std::runtime_error("blocked apply: unsupported arguments");
}

// the cached INIT pass in the geometry of kernel shape `variant` (the shape fixes the gathering waves per workgroup)
void launch_init_cached(const BlkArgs& a, int grid, hipStream_t s, const BlkInit& init, int variant, const BlkInitAp* ap,
                        const BlkInitAp2* ap2) {
  blocked_args_check(a, grid, variant);
  if (!init.R || !init.Z || !init.psi || !init.WY || init.Y != nullptr || init.Z == a.X || init.Z == init.WY)
    throw std::runtime_error("cached INIT pass: bad arguments");
  if (ap2 != nullptr && ap == nullptr) throw std::runtime_error("cached INIT pass: the second apply needs the first");
  if (ap != nullptr) {
    if (!ap->WW || !ap->wsum || !ap->AP || !ap->part || ap->part == a.part || ap->AP == init.R || ap->AP == init.Z || ap->AP == init.Xcopy ||
        ap->AP == ap->WW)
      throw std::runtime_error("cached INIT pass: bad first-apply arguments");
    if (ap2 != nullptr) {
      if (!ap2->W3 || !ap2->wsum2 || !ap2->T || ap2->T == ap->AP || ap2->T == init.R || ap2->T == init.Z || ap2->T == init.Xcopy ||
          ap2->T == ap2->W3 || ap2->T == ap->WW || ap2->T == init.WY || ap2->T == a.X)
        throw std::runtime_error("cached INIT pass: bad second-apply arguments");
#define CALL(G, W, P, E) hipLaunchKernelGGL((k_init_cached_ap2<W>), dim3(grid), dim3((W + 1) * 64), 0, s, a, init, *ap, *ap2)
      OSC_BLK_SHAPE_SWITCH(variant, CALL);
#undef CALL
      HIP_CHECK(hipGetLastError());
      return;
    }
#define CALL(G, W, P, E) hipLaunchKernelGGL((k_init_cached_ap<W>), dim3(grid), dim3((W + 1) * 64), 0, s, a, init, *ap)
    OSC_BLK_SHAPE_SWITCH(variant, CALL);
#undef CALL
    HIP_CHECK(hipGetLastError());
    return;
  }
#define CALL(G, W, P, E) hipLaunchKernelGGL((k_init_cached<W>), dim3(grid), dim3((W + 1) * 64), 0, s, a, init)
  OSC_BLK_SHAPE_SWITCH(variant, CALL);
#undef CALL
  HIP_CHECK(hipGetLastError());
}
void launch_init_two_steps(const BlkArgs& a, int grid, hipStream_t s, const BlkInit& init, int variant, const BlkInitAp& ap,
                           const BlkInitAp2& ap2, const BlkTwoSteps& ts, bool stream) {
  if (stream) {
    if (grid < 1 || a.N < 1 || ts.row0 < 0 || ts.row0 > a.N || (a.c0 & 31) != 0 || a.c1 <= a.c0 || a.c1 > a.ld || (a.c1 & 3) != 0 ||
        (a.ld & 31) != 0 || (int64_t)a.N * a.ld * 4 >= ((int64_t)1 << 32) || !a.X || !a.B)
      throw std::runtime_error("two-step INIT pass: unsupported arguments");
  } else {
    blocked_args_check(a, grid, variant);
    if (ts.row0 != 0) throw std::runtime_error("two-step INIT pass: the blocked form covers every row");
  }
  if (!init.R || !init.Z || !init.Xcopy || !init.psi || !init.WY || init.Y != nullptr || !ap.WW || !ap.wsum || !ap2.W3 || !ap2.wsum2 ||
      !ts.alpha1 || !ts.alpha2 || !ts.beta1 || !ts.beta2 || !ts.go ||
      (ts.go_fold != nullptr && (!ts.alpha3 || !ts.beta3 || !ts.alpha4)))
    throw std::runtime_error("two-step INIT pass: bad arguments");
  for (const float* out : {init.R, init.Z, init.Xcopy})  // no output is an input ...
    if (out == a.X || out == init.WY || out == ap.WW || out == ap2.W3) throw std::runtime_error("two-step INIT pass: aliased arrays");
  if (init.R == init.Z || init.R == init.Xcopy || init.Z == init.Xcopy)  // ... or another output
    throw std::runtime_error("two-step INIT pass: aliased arrays");
  if (stream) {
    const TwoStepsShape sh = pick_two_steps_shape(a.c1 - a.c0);
    const int tile = sh.lpr * 4 * sh.nch, tiles = (a.c1 - a.c0 + tile - 1) / tile;
    const int rows_per_wg = 4 * (64 / sh.lpr) * sh.rpt;
    const int64_t need = ((int64_t)(a.N - ts.row0) + rows_per_wg - 1) / rows_per_wg;
    const dim3 g((unsigned)std::max<int64_t>(1, std::min<int64_t>(need, grid / tiles)), (unsigned)tiles);  // (the solve's grid over the tiles)
    if (ts.go_fold != nullptr) {
#define CALLS(L, C, R) hipLaunchKernelGGL((k_init_two_steps_stream<L, C, R, true>), g, dim3(256), 0, s, a, init, ap, ap2, ts)
      OSC_TWO_STEPS_SHAPE_SWITCH(sh, CALLS);
#undef CALLS
    } else {
#define CALLS(L, C, R) hipLaunchKernelGGL((k_init_two_steps_stream<L, C, R>), g, dim3(256), 0, s, a, init, ap, ap2, ts)
      OSC_TWO_STEPS_SHAPE_SWITCH(sh, CALLS);
#undef CALLS
    }
    HIP_CHECK(hipGetLastError());
    return;
  }
#define CALL(G, W, P, E) hipLaunchKernelGGL((k_init_two_steps<W>), dim3(grid), dim3((W + 1) * 64), 0, s, a, init, ap, ap2, ts)
  OSC_BLK_SHAPE_SWITCH(variant, CALL);
#undef CALL
  HIP_CHECK(hipGetLastError());
}
bool settle_poly_supported(const SettlePolyArgs& a) {
  return a.N >= 1 && (a.c0 & 31) == 0 && a.c1 > a.c0 && a.c1 <= a.ld && (a.c1 & 3) == 0 && (a.ld & 31) == 0 &&
         (int64_t)a.N * a.ld * 4 < ((int64_t)1 << 32);
}
void launch_settle_poly(const SettlePolyArgs& a, int grid, hipStream_t s) {
  if (grid < 1 || !settle_poly_supported(a)) throw std::runtime_error("polynomial settle pass: unsupported arguments");
  if (!a.Ys || !a.WYs || !a.WW || !a.W3 || !a.W4 || !a.wsum || !a.wsum2 || !a.wsum3 || !a.coef || !a.X || !a.go || !a.go_fold)
    throw std::runtime_error("polynomial settle pass: bad arguments");
  for (const float* in : {a.Ys, a.WYs, a.WW, a.W3, a.W4})
    if (in == a.X) throw std::runtime_error("polynomial settle pass: aliased arrays");
  const TwoStepsShape sh = pick_two_steps_shape(a.c1 - a.c0);
  const int tile = sh.lpr * 4 * sh.nch, tiles = (a.c1 - a.c0 + tile - 1) / tile;
  const int rows_per_wg = 4 * (64 / sh.lpr) * sh.rpt;
  const int64_t need = ((int64_t)a.N + rows_per_wg - 1) / rows_per_wg;
  const dim3 g((unsigned)std::max<int64_t>(1, std::min<int64_t>(need, grid / tiles)), (unsigned)tiles);  // (the solve's grid over the tiles)
#define CALLS(L, C, R) hipLaunchKernelGGL((k_settle_poly<L, C, R>), g, dim3(256), 0, s, a)
  OSC_TWO_STEPS_SHAPE_SWITCH(sh, CALLS);
#undef CALLS
  HIP_CHECK(hipGetLastError());
}
void launch_anchor_gram(const GramArgs& a, hipStream_t s) {
  if (!a.Ys || !a.WYs || !a.WW || !a.W3 || !a.wsum || !a.wsum2 || !a.part || !a.out || a.N < 1 || (a.c0 & 31) != 0 || a.c1 <= a.c0 ||
      a.c1 > a.ld)
    throw std::runtime_error("anchor Gram sums: bad arguments");
  hipLaunchKernelGGL(k_anchor_gram_part, dim3((a.c1 - a.c0 + 31) / 32, OSC_GRAM_CHUNKS), dim3(256), 0, s, a);
  HIP_CHECK(hipGetLastError());
  const int n = gram::kGramPerColumn * a.ld + gram::kGramLattice;
  hipLaunchKernelGGL(k_anchor_gram_fold, dim3((n + 255) / 256), dim3(256), 0, s, a);
  HIP_CHECK(hipGetLastError());
}
void launch_anchor_gram3(const Gram3Args& b, hipStream_t s) {
  const GramArgs& a = b.g;
  if (!a.Ys || !a.WYs || !a.WW || !a.W3 || !b.W4 || !a.wsum || !a.wsum2 || !b.wsum3 || !a.part || !a.out || a.N < 1 || (a.c0 & 31) != 0 ||
      a.c1 <= a.c0 || a.c1 > a.ld)
    throw std::runtime_error("anchor Gram sums, third step: bad arguments");
  hipLaunchKernelGGL(k_anchor_gram3_part, dim3((a.c1 - a.c0 + 31) / 32, OSC_GRAM_CHUNKS), dim3(256), 0, s, b);
  HIP_CHECK(hipGetLastError());
  const int n = gram::kGram3PerColumn * a.ld + gram::kGram3Lattice;
  hipLaunchKernelGGL(k_anchor_gram3_fold, dim3((n + 255) / 256), dim3(256), 0, s, a);
  HIP_CHECK(hipGetLastError());
}
void launch_anchor_gram4(const Gram4Args& b, hipStream_t s) {
  const GramArgs& a = b.g;
  if (!a.Ys || !a.WYs || !a.WW || !a.W3 || !b.W4 || !b.W5 || b.W4 == b.W5 || !a.wsum || !a.wsum2 || !b.wsum3 || !b.wsum4 || !a.part ||
      !a.out || a.N < 1 || (a.c0 & 31) != 0 || a.c1 <= a.c0 || a.c1 > a.ld)
    throw std::runtime_error("anchor Gram sums, fourth step: bad arguments");
  hipLaunchKernelGGL(k_anchor_gram4_part, dim3((a.c1 - a.c0 + 31) / 32, OSC_GRAM_CHUNKS), dim3(256), 0, s, b);
  HIP_CHECK(hipGetLastError());
  const int n = gram::kGram4PerColumn * a.ld + gram::kGram4Lattice;
  hipLaunchKernelGGL(k_anchor_gram4_fold, dim3((n + 255) / 256), dim3(256), 0, s, a);
  HIP_CHECK(hipGetLastError());
}
void launch_anchor_gram_scalars(const GramScalarArgs& a, hipStream_t s) {
  if (a.gram3 != nullptr && (!a.alpha3 || !a.beta3 || a.beta3 == a.beta2 || a.alpha3 == a.alpha1 || a.alpha3 == a.alpha2))
    throw std::runtime_error("anchor Gram scalars: bad arguments of the third step");
  if (a.gram4 != nullptr && (a.gram3 == nullptr || !a.alpha4 || a.alpha4 == a.alpha1 || a.alpha4 == a.alpha2 || a.alpha4 == a.alpha3))
    throw std::runtime_error("anchor Gram scalars: bad arguments of the fourth step");
  if (a.poly != nullptr && a.gram4 == nullptr) throw std::runtime_error("anchor Gram scalars: the polynomial form needs the fourth step");
  hipLaunchKernelGGL(k_anchor_gram_scalars, dim3(1), dim3(256), 0, s, a);
  HIP_CHECK(hipGetLastError());
}
void launch_row_weight_sums(const float* w, const int32_t* deg, int32_t width, int32_t N, float* out, hipStream_t s) {
  hipLaunchKernelGGL(k_row_weight_sums, dim3((N + 255) / 256), dim3(256), 0, s, w, deg, width, N, out);
  HIP_CHECK(hipGetLastError());
}

void launch_row_weighted_sums(const int32_t* col, const float* w, const int32_t* deg, int32_t width, int32_t N, const float* v,
                              float* out, hipStream_t s) {
  hipLaunchKernelGGL(k_row_weighted_sums, dim3((N + 255) / 256), dim3(256), 0, s, col, w, deg, width, N, v, out);
  HIP_CHECK(hipGetLastError());
}

void launch_apply_blocked(const BlkArgs& a, int grid, hipStream_t s, const BlkInit* init, int variant, bool store_wy) {
  blocked_args_check(a, grid, variant);
  if (store_wy) {
    if (init == nullptr || !init->R || !init->Z || !init->psi || !init->WY || init->Y != nullptr || init->Z == a.X || init->WY == a.X || init->WY == init->Z)
      throw std::runtime_error("blocked apply: bad INIT arguments");
#define CALL(G, W, P, E) hipLaunchKernelGGL((k_apply_blocked<G, W, true, P, E, true>), dim3(grid), dim3((W + 1) * 64), 0, s, a, *init)
    OSC_BLK_SHAPE_SWITCH(variant, CALL);
#undef CALL
  } else if (init != nullptr) {
    if (!init->R || !init->Z || !init->psi || init->Z == a.X) throw std::runtime_error("blocked apply: bad INIT arguments");
#define CALL(G, W, P, E) hipLaunchKernelGGL((k_apply_blocked<G, W, true, P, E>), dim3(grid), dim3((W + 1) * 64), 0, s, a, *init)
    OSC_BLK_SHAPE_SWITCH(variant, CALL);
#undef CALL
  } else {
#define CALL(G, W, P, E) hipLaunchKernelGGL((k_apply_blocked<G, W, false, P, E>), dim3(grid), dim3((W + 1) * 64), 0, s, a, BlkInit{})
    OSC_BLK_SHAPE_SWITCH(variant, CALL);
#undef CALL
  }
  HIP_CHECK(hipGetLastError());
}

// iteration 3 of an anchor start in one launch (BlkFused); with BlkFused::X the last form, which leaves x4 and nothing else
void launch_apply_blocked_fused(const BlkArgs& a, int grid, hipStream_t s, const BlkFused& f, int variant) {
  blocked_args_check(a, grid, variant);
  if (f.go_fold != nullptr) {
    if (!f.X || !f.alpha || !f.alpha_last || !f.go || f.X == a.X || (a.c1 & 3) != 0 || a.c1 > a.ld)
      throw std::runtime_error("blocked apply: bad arguments of the folded last form");
#define CALL(G, W, P, E) hipLaunchKernelGGL((k_apply_blocked<G, W, false, P, E, false, 3>), dim3(grid), dim3((W + 1) * 64), 0, s, a, f)
    OSC_BLK_SHAPE_SWITCH(variant, CALL);
#undef CALL
    HIP_CHECK(hipGetLastError());
    return;
  }
  if (f.X != nullptr) {
    if (!f.R || !f.alpha || !f.beta || !f.alpha_last || !f.go || f.R == a.X || f.X == a.X || f.X == f.R || (a.c1 & 3) != 0 || a.c1 > a.ld)
      throw std::runtime_error("blocked apply: bad arguments of the last fused form");
#define CALL(G, W, P, E) hipLaunchKernelGGL((k_apply_blocked<G, W, false, P, E, false, 2>), dim3(grid), dim3((W + 1) * 64), 0, s, a, f)
    OSC_BLK_SHAPE_SWITCH(variant, CALL);
#undef CALL
    HIP_CHECK(hipGetLastError());
    return;
  }
  if (!f.R || !f.Pout || !f.alpha || !f.beta || !f.go || f.Pout == a.X || f.R == a.X || f.R == f.Pout || (a.c1 & 3) != 0 || a.c1 > a.ld)
    throw std::runtime_error("blocked apply: bad arguments of the fused form");
#define CALL(G, W, P, E) hipLaunchKernelGGL((k_apply_blocked<G, W, false, P, E, false, 1>), dim3(grid), dim3((W + 1) * 64), 0, s, a, f)
  OSC_BLK_SHAPE_SWITCH(variant, CALL);
#undef CALL
  HIP_CHECK(hipGetLastError());
}

void launch_spmm(int mode, const SpmmArgs& a, int grid, hipStream_t s) {
  if (a.xs != 0) {  // XCD-affine 32-column slabs: 8 lanes per row
    if (grid < 8 || (grid & 7) != 0 || a.xs > grid / 8 || a.xs_groups < 1 || 8 % a.xs_groups != 0)
      throw std::runtime_error("xs mode needs a grid that is a multiple of 8 and 1, 2, 4 or 8 slab groups");
    if (mode == SPMM_AP) hipLaunchKernelGGL((k_spmm<8, 1, SPMM_AP>), dim3(grid), dim3(256), 0, s, a);
    else if (mode == SPMM_INIT) hipLaunchKernelGGL((k_spmm<8, 1, SPMM_INIT>), dim3(grid), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_spmm<8, 1, SPMM_DOT>), dim3(grid), dim3(256), 0, s, a);
    HIP_CHECK(hipGetLastError());
    return;
  }
  const Shape sh = pick_shape(a.c1 - a.c0);
  if (a.deep != 0 && sh.nch == 1 && (sh.lpr == 32 || sh.lpr == 64) && mode != SPMM_DOT) {  // local row order: more hits in flight
    if (sh.lpr == 32) {
      if (mode == SPMM_AP) hipLaunchKernelGGL((k_spmm<32, 1, SPMM_AP, OSC_SPMM_UDEEP>), dim3(grid), dim3(256), 0, s, a);
      else hipLaunchKernelGGL((k_spmm<32, 1, SPMM_INIT, OSC_SPMM_UDEEP>), dim3(grid), dim3(256), 0, s, a);
    } else {
      if (mode == SPMM_AP) hipLaunchKernelGGL((k_spmm<64, 1, SPMM_AP, OSC_SPMM_UDEEP>), dim3(grid), dim3(256), 0, s, a);
      else hipLaunchKernelGGL((k_spmm<64, 1, SPMM_INIT, OSC_SPMM_UDEEP>), dim3(grid), dim3(256), 0, s, a);
    }
    HIP_CHECK(hipGetLastError());
    return;
  }
#define CALL(L, C)                                                                                   \
  do {                                                                                               \
    if (mode == SPMM_AP) hipLaunchKernelGGL((k_spmm<L, C, SPMM_AP>), dim3(grid), dim3(256), 0, s, a); \
    else if (mode == SPMM_INIT) hipLaunchKernelGGL((k_spmm<L, C, SPMM_INIT>), dim3(grid), dim3(256), 0, s, a); \
    else hipLaunchKernelGGL((k_spmm<L, C, SPMM_DOT>), dim3(grid), dim3(256), 0, s, a);               \
  } while (0)
  OSC_SHAPE_SWITCH(sh, CALL);
#undef CALL
  HIP_CHECK(hipGetLastError());
}

void launch_update_xr(const UpdateArgs& a, int grid, hipStream_t s) {
  const Shape sh = pick_shape(a.c1 - a.c0);
#define CALL(L, C) hipLaunchKernelGGL((k_update_xr<L, C, true>), dim3(grid), dim3(256), 0, s, a)
#define CALL_NOX(L, C) hipLaunchKernelGGL((k_update_xr<L, C, false>), dim3(grid), dim3(256), 0, s, a)
#define CALL_LAST(L, C) hipLaunchKernelGGL((k_update_xr<L, C, true, false>), dim3(grid), dim3(256), 0, s, a)
#define CALL_BARE(L, C) hipLaunchKernelGGL((k_update_xr<L, C, false, false>), dim3(grid), dim3(256), 0, s, a)
  if (a.xmode & OSC_XMODE_XR_LAST) {
    OSC_SHAPE_SWITCH(sh, CALL_LAST);
  } else if (a.xmode & OSC_XMODE_XR_BARE) {
    OSC_SHAPE_SWITCH(sh, CALL_BARE);
  } else if (a.xmode & OSC_XMODE_XR_SKIPS_X) {
    OSC_SHAPE_SWITCH(sh, CALL_NOX);
  } else {
    OSC_SHAPE_SWITCH(sh, CALL);
  }
#undef CALL
#undef CALL_NOX
#undef CALL_LAST
#undef CALL_BARE
  HIP_CHECK(hipGetLastError());
}

void launch_update_p(const UpdateArgs& a, int grid, hipStream_t s) {
  const Shape sh = pick_shape(a.c1 - a.c0);
#define CALL(L, C) hipLaunchKernelGGL((k_update_p<L, C, false>), dim3(grid), dim3(256), 0, s, a)
#define CALL_X(L, C) hipLaunchKernelGGL((k_update_p<L, C, true>), dim3(grid), dim3(256), 0, s, a)
  if (a.xmode & OSC_XMODE_P_APPLIES_X) {
    OSC_SHAPE_SWITCH(sh, CALL_X);
  } else {
    OSC_SHAPE_SWITCH(sh, CALL);
  }
#undef CALL
#undef CALL_X
  HIP_CHECK(hipGetLastError());
}

void launch_update_p_ap2(const UpdateArgs& a, int grid, hipStream_t s) {
  if (!a.T || !a.APout || a.APout != a.AP || !a.part_rr || !a.alpha || !a.beta || a.T == a.AP || a.T == a.R || a.T == a.P || a.T == a.Pout)
    throw std::runtime_error("p update with streamed A p: bad arguments");
  const Shape sh = pick_shape(a.c1 - a.c0);
#define CALL(L, C) hipLaunchKernelGGL((k_update_p_ap2<L, C, false>), dim3(grid), dim3(256), 0, s, a)
#define CALL_X(L, C) hipLaunchKernelGGL((k_update_p_ap2<L, C, true>), dim3(grid), dim3(256), 0, s, a)
  if (a.xmode & OSC_XMODE_P_APPLIES_X) {
    OSC_SHAPE_SWITCH(sh, CALL_X);
  } else {
    OSC_SHAPE_SWITCH(sh, CALL);
  }
#undef CALL
#undef CALL_X
  HIP_CHECK(hipGetLastError());
}

void launch_update_x(const UpdateArgs& a, int grid, hipStream_t s) {  // x += alpha p
  const Shape sh = pick_shape(a.c1 - a.c0);
#define CALL(L, C) hipLaunchKernelGGL((k_update_p<L, C, true, false>), dim3(grid), dim3(256), 0, s, a)
  OSC_SHAPE_SWITCH(sh, CALL);
#undef CALL
  HIP_CHECK(hipGetLastError());
}

void launch_update_x_ring(const XRingArgs& a, int grid, hipStream_t s) {
  const Shape sh = pick_shape(a.c1 - a.c0);
#define CALL1(L, C) hipLaunchKernelGGL((k_update_x_ring<L, C, 1>), dim3(grid), dim3(256), 0, s, a)
#define CALL2(L, C) hipLaunchKernelGGL((k_update_x_ring<L, C, 2>), dim3(grid), dim3(256), 0, s, a)
#define CALL3(L, C) hipLaunchKernelGGL((k_update_x_ring<L, C, 3>), dim3(grid), dim3(256), 0, s, a)
#define CALL4(L, C) hipLaunchKernelGGL((k_update_x_ring<L, C, 4>), dim3(grid), dim3(256), 0, s, a)
  switch (a.M) {
    case 1: OSC_SHAPE_SWITCH(sh, CALL1); break;
    case 2: OSC_SHAPE_SWITCH(sh, CALL2); break;
    case 3: OSC_SHAPE_SWITCH(sh, CALL3); break;
    case 4: OSC_SHAPE_SWITCH(sh, CALL4); break;
    default: throw std::runtime_error("x ring pass: 1 to 4 directions");
  }
#undef CALL1
#undef CALL2
#undef CALL3
#undef CALL4
  HIP_CHECK(hipGetLastError());
}

static inline int red_grid(int32_t c0, int32_t c1) { return (c1 - c0 + 63) / 64; }

void launch_reduce_init(const float* part, int nb, int32_t ld, int32_t c0, int32_t c1, double* rz, hipStream_t s) {
  hipLaunchKernelGGL(k_reduce_init, dim3(red_grid(c0, c1)), dim3(1024), 0, s, part, nb, ld, c0, c1, rz);
  HIP_CHECK(hipGetLastError());
}
void launch_reduce_alpha(const float* part, int nb, int32_t ld, int32_t c0, int32_t c1, const double* rz, float* alpha,
                         Gate g, hipStream_t s) {
  hipLaunchKernelGGL(k_reduce_alpha, dim3(red_grid(c0, c1)), dim3(1024), 0, s, part, nb, ld, c0, c1, rz, alpha, g);
  HIP_CHECK(hipGetLastError());
}
void launch_reduce_beta(const float* part_rr, const float* part_rz, int nb, int32_t ld, int32_t c0, int32_t c1,
                        double* rz, float* beta, uint32_t* res_bits_slot, Gate g, hipStream_t s, uint32_t* done_ctr,
                        float* host_slot) {
  hipLaunchKernelGGL(k_reduce_beta, dim3(red_grid(c0, c1)), dim3(1024), 0, s, part_rr, part_rz, nb, ld, c0, c1, rz,
                     beta, res_bits_slot, g, done_ctr, host_slot);
  HIP_CHECK(hipGetLastError());
}
namespace {
// one word device -> host-mapped memory (the globally reduced residual of a sharded solve, behind its all-reduce)
__global__ void k_publish_word(const uint32_t* src, uint32_t* host_slot) {
  *reinterpret_cast<volatile uint32_t*>(host_slot) = *reinterpret_cast<const volatile uint32_t*>(src);
  __threadfence_system();
}
}  // namespace
void launch_publish_word(const uint32_t* src, uint32_t* host_slot, hipStream_t s) {
  hipLaunchKernelGGL(k_publish_word, dim3(1), dim3(1), 0, s, src, host_slot);
  HIP_CHECK(hipGetLastError());
}
void launch_reduce_sum(const float* part, int nb, int32_t ld, int32_t c0, int32_t c1, double* out_cols, hipStream_t s) {
  hipLaunchKernelGGL(k_reduce_sum, dim3(red_grid(c0, c1)), dim3(1024), 0, s, part, nb, ld, c0, c1, out_cols,
                     Gate{nullptr, 0.f});
  HIP_CHECK(hipGetLastError());
}
void launch_reduce_sum_gated(const float* part, int nb, int32_t ld, int32_t c0, int32_t c1, double* out_cols, Gate g,
                             hipStream_t s) {
  hipLaunchKernelGGL(k_reduce_sum, dim3(red_grid(c0, c1)), dim3(1024), 0, s, part, nb, ld, c0, c1, out_cols, g);
  HIP_CHECK(hipGetLastError());
}
void launch_finish_init(const double* sums, int32_t c0, int32_t c1, double* rz, hipStream_t s) {
  hipLaunchKernelGGL(k_finish_init, dim3((c1 - c0 + 255) / 256), dim3(256), 0, s, sums, c0, c1, rz);
  HIP_CHECK(hipGetLastError());
}
void launch_finish_alpha(const double* sums, int32_t c0, int32_t c1, const double* rz, float* alpha, Gate g,
                         hipStream_t s) {
  hipLaunchKernelGGL(k_finish_alpha, dim3((c1 - c0 + 255) / 256), dim3(256), 0, s, sums, c0, c1, rz, alpha, g);
  HIP_CHECK(hipGetLastError());
}
void launch_finish_beta(const double* sums_rr, const double* sums_rz, int32_t c0, int32_t c1, double* rz, float* beta,
                        uint32_t* res_bits_slot, Gate g, hipStream_t s) {
  hipLaunchKernelGGL(k_finish_beta, dim3((c1 - c0 + 255) / 256), dim3(256), 0, s, sums_rr, sums_rz, c0, c1, rz, beta,
                     res_bits_slot, g);
  HIP_CHECK(hipGetLastError());
}
void launch_axpby(float* out, const float* a, float ca, const float* b, float cb, int64_t n, hipStream_t s) {
  const int64_t n4 = n / 4;
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((n4 + 255) / 256, 2048));
  hipLaunchKernelGGL(k_axpby, dim3(grid), dim3(256), 0, s, out, a, ca, b, cb, n4);
  HIP_CHECK(hipGetLastError());
}

}  // namespace osc

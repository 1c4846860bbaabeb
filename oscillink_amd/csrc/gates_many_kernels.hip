// Screened-diffusion gates for many queries: (L_sym + gamma I) h_q = s_q for a panel of queries as
// ONE Jacobi-PCG over the lattice graph, every column with its own alpha, beta and stop.
//
// Layout and partition (gates_many_plan.hpp): a panel is cut into 32-column slabs, each a contiguous N x 32 array whose rows
// are 128-byte lines; the rows are cut into `parts` runs of part_rows rows by a rule of N alone.  Every N-sized kernel runs
// one workgroup per (part, slab): 4 waves, each wave 8 rows x 8 lanes x float4 (a lane's access is 16 bytes, a row's is one
// whole line), 32 rows per step.  A thread accumulates its row class (thread / 8) in row order; the workgroup adds its 32
// classes in class order in fp64; the per-column kernels add the parts in a fixed order.  Nothing of that depends on how
// many slabs the panel has or on which queries fill them, so a query's gates are the same to the bit in any batch.  No
// float atomics anywhere; the only atomic is the integer count of live columns.
#include "gates_many.hpp"
#include "gates_many_dev.hpp"

namespace osc {
namespace {

__global__ __launch_bounds__(256) void k_gm_source(const GmPanel p, const float* __restrict__ C, float beta, float inv_md) {
  __shared__ double sh[1024];
  const int t = threadIdx.x, lr = t & 7;
  const int slab = blockIdx.y, qc = p.slabs * 32, c0 = slab * 32 + lr * 4;
  const size_t so = (size_t)slab * p.N * 32;
  const GmRows rr = gm_rows(p);
  float4 rz = f4(0.f), ss = f4(0.f);
  for (int64_t rb = rr.r0; rb < rr.r1; rb += 32) {
    const int64_t row = rb + (t >> 3);
    if (row >= rr.r1) continue;
    const float4 c = ld4(C + (size_t)row * qc + c0);
    // beta * np.maximum(0, cos): a NaN stays; the panel's pad columns are zero
    float4 s;
    s.x = c0 + 0 < p.nq ? beta * (c.x <= 0.f ? 0.f : c.x) : 0.f;
    s.y = c0 + 1 < p.nq ? beta * (c.y <= 0.f ? 0.f : c.y) : 0.f;
    s.z = c0 + 2 < p.nq ? beta * (c.z <= 0.f ? 0.f : c.z) : 0.f;
    s.w = c0 + 3 < p.nq ? beta * (c.w <= 0.f ? 0.f : c.w) : 0.f;
    const float4 z = make_float4(s.x * inv_md, s.y * inv_md, s.z * inv_md, s.w * inv_md);
    const size_t o = so + (size_t)row * 32 + lr * 4;
    st4(p.X + o, f4(0.f));
    st4(p.R + o, s);
    st4(p.P + o, z);
    rz = mulacc4(s, z, rz);
    ss = mulacc4(s, s, ss);
  }
  gm_fold(rz, sh, p.part_a + gm_part_at(p));
  gm_fold(ss, sh, p.part_b + gm_part_at(p));
}

// The Green's columns' start: column c's right-hand side is the unit vector of row node[c] (node[c] < 0: a pad column, all
// zero); x = 0, r = e, p = z = r / d.  part_a / part_b: r . z and e . e like k_gm_source.
__global__ __launch_bounds__(256) void k_gm_unit_source(const GmPanel p, const int32_t* __restrict__ node, const GmRowOp op) {
  __shared__ double sh[1024];
  const int t = threadIdx.x, lr = t & 7;
  const int slab = blockIdx.y, c0 = slab * 32 + lr * 4;
  const size_t so = (size_t)slab * p.N * 32;
  const int4 nd = *reinterpret_cast<const int4*>(node + c0);
  const GmRows rr = gm_rows(p);
  float4 rz = f4(0.f), ss = f4(0.f);
  for (int64_t rb = rr.r0; rb < rr.r1; rb += 32) {
    const int64_t row = rb + (t >> 3);
    if (row >= rr.r1) continue;
    const float4 s = make_float4(nd.x == row ? 1.f : 0.f, nd.y == row ? 1.f : 0.f, nd.z == row ? 1.f : 0.f, nd.w == row ? 1.f : 0.f);
    const float inv_md = 1.0f / op.d[row];
    const float4 z = make_float4(s.x * inv_md, s.y * inv_md, s.z * inv_md, s.w * inv_md);
    const size_t o = so + (size_t)row * 32 + lr * 4;
    st4(p.X + o, f4(0.f));
    st4(p.R + o, s);
    st4(p.P + o, z);
    rz = mulacc4(s, z, rz);
    ss = mulacc4(s, s, ss);
  }
  gm_fold(rz, sh, p.part_a + gm_part_at(p));
  gm_fold(ss, sh, p.part_b + gm_part_at(p));
}

// d_i = c + lamQ B_i
__global__ __launch_bounds__(256) void k_gm_row_diag(const float* __restrict__ B, float c, float lamQ, int32_t N, float* __restrict__ d) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < N) d[i] = fmaf(lamQ, B[i], c);
}

__global__ __launch_bounds__(kGmSumThreads) void k_gm_init(const GmPanel p, int direct, float tol) {
  __shared__ double sh[kGmSumThreads];
  const int slab = blockIdx.x, t = threadIdx.x;
  const size_t at = (size_t)slab * p.parts * 32;
  const double rz = gm_part_sum(p.part_a + at, p.parts, sh);
  const double ss = gm_part_sum(p.part_b + at, p.parts, sh);
  if (t < 32) {
    const int c = slab * 32 + t;
    const int live = c < p.nq ? 1 : 0;
    p.rz[c] = rz;
    // diffusion.py's "direct": CG to 1e-7 max(1, |s|), |s| a float32 norm
    p.tol[c] = direct ? (float)(1e-7 * fmax(1.0, (double)(float)sqrt(ss))) : tol;
    p.alpha[c] = 0.f;
    p.beta[c] = 0.f;
    p.res[c] = 0.f;
    p.iters[c] = 0;
    p.live[c] = live;
    const int cnt = __popcll(__ballot(live != 0));
    if (t == 0) {
      p.slab_live[slab] = cnt;
      if (slab == 0) {
        p.n_live[0] = 0;
        p.n_live[1] = 0;
      }
    }
  }
}

// One wave: 8 rows, 8 lanes a row.  A row's ELL entries are read 8 at a time (one per lane of the row's group) and handed
// round by shuffles; the 8 neighbour lines of that step are all requested before the first is used, so a wave keeps up to
// 64 gathered lines in flight.  The sum runs in slot order with one fmaf per entry.
// ROWD (the Green's columns of osc_chain_prior_many): AP = d_i p_i - lamC (W p)_i with the per-row
// diagonal op.d, where the gates' operator has the one scalar cs and the factor 1.
template <bool ROWD>
__global__ __launch_bounds__(256) void k_gm_apply(const GmPanel p, const GmGraph g, float cs, const GmRowOp op) {
  __shared__ double sh[1024];
  const int slab = blockIdx.y;
  if (p.slab_live[slab] == 0) return;
  const int t = threadIdx.x, lane = t & 63, lr = lane & 7, g0 = lane & ~7;
  const size_t so = (size_t)slab * p.N * 32;
  const float* __restrict__ P = p.P + so;
  float* __restrict__ AP = p.AP + so;
  const GmRows rr = gm_rows(p);
  float4 pap = f4(0.f);
  for (int64_t rb = rr.r0; rb < rr.r1; rb += 32) {
    const int64_t row = rb + (t >> 3);
    const bool ok = row < rr.r1;
    const int deg = ok ? min(g.deg[row], g.width) : 0;
    int dmax = deg;
    dmax = max(dmax, __shfl_xor(dmax, 8, 64));
    dmax = max(dmax, __shfl_xor(dmax, 16, 64));
    dmax = max(dmax, __shfl_xor(dmax, 32, 64));
    float4 sum = f4(0.f);
    for (int e0 = 0; e0 < dmax; e0 += 8) {
      const int e = e0 + lr;
      int j = 0;
      float wv = 0.f;
      if (e < deg) {
        j = g.col[(size_t)row * g.width + e];
        wv = g.w[(size_t)row * g.width + e];
      }
      float4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int ju = __shfl(j, g0 + u, 64);
        v[u] = e0 + u < deg ? ld4(P + (size_t)ju * 32 + lr * 4) : f4(0.f);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const float wu = __shfl(wv, g0 + u, 64);  // 0 past the row's end, where v[u] is 0 as well
        sum = mulacc4(f4(wu), v[u], sum);
      }
    }
    if (ok) {
      const size_t o = (size_t)row * 32 + lr * 4;
      const float4 x = ld4(P + o);
      float4 a;
      if constexpr (ROWD) {
        const float d = op.d[row], nc = -op.lamC;
        a = make_float4(fmaf(d, x.x, nc * sum.x), fmaf(d, x.y, nc * sum.y), fmaf(d, x.z, nc * sum.z), fmaf(d, x.w, nc * sum.w));
      } else {
        a = make_float4(fmaf(cs, x.x, -sum.x), fmaf(cs, x.y, -sum.y), fmaf(cs, x.z, -sum.z), fmaf(cs, x.w, -sum.w));
      }
      st4(AP + o, a);
      pap = mulacc4(x, a, pap);
    }
  }
  gm_fold(pap, sh, p.part_a + gm_part_at(p));
}

__global__ __launch_bounds__(kGmSumThreads) void k_gm_alpha(const GmPanel p) {
  __shared__ double sh[kGmSumThreads];
  const int slab = blockIdx.x, t = threadIdx.x;
  if (p.slab_live[slab] == 0) return;
  const double pap = gm_part_sum(p.part_a + (size_t)slab * p.parts * 32, p.parts, sh);
  if (t < 32) {
    const int c = slab * 32 + t;
    p.alpha[c] = p.live[c] ? (float)(p.rz[c] / (pap + 1e-18)) : 0.f;  // solver.py:25-26
  }
}

template <bool ROWD>
__global__ __launch_bounds__(256) void k_gm_update(const GmPanel p, float inv_md_all, const GmRowOp op) {
  __shared__ double sh[1024];
  const int slab = blockIdx.y;
  if (p.slab_live[slab] == 0) return;
  const int t = threadIdx.x, lr = t & 7, c0 = slab * 32 + lr * 4;
  const size_t so = (size_t)slab * p.N * 32;
  const float4 al = ld4(p.alpha + c0);
  const int4 lv = *reinterpret_cast<const int4*>(p.live + c0);
  const GmRows rr = gm_rows(p);
  float4 rr2 = f4(0.f), rz = f4(0.f);
  for (int64_t rb = rr.r0; rb < rr.r1; rb += 32) {
    const int64_t row = rb + (t >> 3);
    if (row >= rr.r1) continue;
    const size_t o = so + (size_t)row * 32 + lr * 4;
    const float inv_md = ROWD ? 1.0f / op.d[row] : inv_md_all;
    float4 x = ld4(p.X + o), r = ld4(p.R + o);
    const float4 d = ld4(p.P + o), a = ld4(p.AP + o);
    // a frozen column keeps its x and r bit for bit
    if (lv.x) { x.x = fmaf(d.x, al.x, x.x); r.x = fmaf(-a.x, al.x, r.x); }
    if (lv.y) { x.y = fmaf(d.y, al.y, x.y); r.y = fmaf(-a.y, al.y, r.y); }
    if (lv.z) { x.z = fmaf(d.z, al.z, x.z); r.z = fmaf(-a.z, al.z, r.z); }
    if (lv.w) { x.w = fmaf(d.w, al.w, x.w); r.w = fmaf(-a.w, al.w, r.w); }
    st4(p.X + o, x);
    st4(p.R + o, r);
    rr2 = mulacc4(r, r, rr2);
    rz = mulacc4(r, make_float4(r.x * inv_md, r.y * inv_md, r.z * inv_md, r.w * inv_md), rz);
  }
  gm_fold(rr2, sh, p.part_a + gm_part_at(p));
  gm_fold(rz, sh, p.part_b + gm_part_at(p));
}

__global__ __launch_bounds__(kGmSumThreads) void k_gm_beta(const GmPanel p, int it) {
  __shared__ double sh[kGmSumThreads];
  const int slab = blockIdx.x, t = threadIdx.x;
  if (slab == 0 && t == 0) p.n_live[(it + 1) & 1] = 0;
  if (p.slab_live[slab] == 0) return;
  const size_t at = (size_t)slab * p.parts * 32;
  const double rr = gm_part_sum(p.part_a + at, p.parts, sh);
  const double rz = gm_part_sum(p.part_b + at, p.parts, sh);
  if (t < 32) {
    const int c = slab * 32 + t;
    int live = p.live[c];
    float be = 0.f;
    if (live) {
      const float res = (float)sqrt(rr);  // |r_q| (solver.py:29)
      p.iters[c] = it;
      p.res[c] = res;
      if (res <= p.tol[c]) {  // (a NaN never freezes: it runs to max_iters like cg_solve)
        live = 0;
        p.live[c] = 0;
      } else {
        be = (float)(rz / (p.rz[c] + 1e-18));  // solver.py:33-34
        p.rz[c] = rz;
      }
    }
    p.beta[c] = be;
    const int cnt = __popcll(__ballot(live != 0));
    if (t == 0) {
      p.slab_live[slab] = cnt;
      if (cnt > 0) atomicAdd(p.n_live + (it & 1), cnt);
    }
  }
}

template <bool ROWD>
__global__ __launch_bounds__(256) void k_gm_direction(const GmPanel p, float inv_md_all, const GmRowOp op) {
  const int slab = blockIdx.y;
  if (p.slab_live[slab] == 0) return;
  const int t = threadIdx.x, lr = t & 7;
  const size_t so = (size_t)slab * p.N * 32;
  const float4 be = ld4(p.beta + slab * 32 + lr * 4);
  const GmRows rr = gm_rows(p);
  for (int64_t rb = rr.r0; rb < rr.r1; rb += 32) {
    const int64_t row = rb + (t >> 3);
    if (row >= rr.r1) continue;
    const size_t o = so + (size_t)row * 32 + lr * 4;
    const float inv_md = ROWD ? 1.0f / op.d[row] : inv_md_all;
    const float4 r = ld4(p.R + o);
    float4 d = ld4(p.P + o);
    d.x = fmaf(d.x, be.x, r.x * inv_md);
    d.y = fmaf(d.y, be.y, r.y * inv_md);
    d.z = fmaf(d.z, be.z, r.z * inv_md);
    d.w = fmaf(d.w, be.w, r.w * inv_md);
    st4(p.P + o, d);
  }
}

// minima and maxima of x per part and column (floats in the part arrays)
__global__ __launch_bounds__(256) void k_gm_minmax(const GmPanel p) {
  __shared__ float sh[2][1024];
  const int t = threadIdx.x, lr = t & 7, slab = blockIdx.y;
  const size_t so = (size_t)slab * p.N * 32;
  const GmRows rr = gm_rows(p);
  float4 lo = f4(INFINITY), hi = f4(-INFINITY);
  for (int64_t rb = rr.r0; rb < rr.r1; rb += 32) {
    const int64_t row = rb + (t >> 3);
    if (row >= rr.r1) continue;
    const float4 x = ld4(p.X + so + (size_t)row * 32 + lr * 4);
    lo = make_float4(nan_min(lo.x, x.x), nan_min(lo.y, x.y), nan_min(lo.z, x.z), nan_min(lo.w, x.w));
    hi = make_float4(nan_max(hi.x, x.x), nan_max(hi.y, x.y), nan_max(hi.z, x.z), nan_max(hi.w, x.w));
  }
  const int at = (t >> 3) * 32 + lr * 4;
  sh[0][at] = lo.x; sh[0][at + 1] = lo.y; sh[0][at + 2] = lo.z; sh[0][at + 3] = lo.w;
  sh[1][at] = hi.x; sh[1][at + 1] = hi.y; sh[1][at + 2] = hi.z; sh[1][at + 3] = hi.w;
  __syncthreads();
  if (t < 32) {
    float a = INFINITY, b = -INFINITY;
    for (int c = 0; c < 32; ++c) {
      a = nan_min(a, sh[0][c * 32 + t]);
      b = nan_max(b, sh[1][c * 32 + t]);
    }
    reinterpret_cast<float*>(p.part_a)[gm_part_at(p) + t] = a;
    reinterpret_cast<float*>(p.part_b)[gm_part_at(p) + t] = b;
  }
}

__global__ __launch_bounds__(256) void k_gm_range(const GmPanel p) {
  __shared__ float sh[2][256];
  const int slab = blockIdx.x, t = threadIdx.x, c = t & 31, g = t >> 5;
  const float* pa = reinterpret_cast<const float*>(p.part_a) + (size_t)slab * p.parts * 32;
  const float* pb = reinterpret_cast<const float*>(p.part_b) + (size_t)slab * p.parts * 32;
  float a = INFINITY, b = -INFINITY;
  for (int k = g; k < p.parts; k += 8) {
    a = nan_min(a, pa[(size_t)k * 32 + c]);
    b = nan_max(b, pb[(size_t)k * 32 + c]);
  }
  sh[0][t] = a;
  sh[1][t] = b;
  __syncthreads();
  if (t >= 32) return;
  for (int k = 1; k < 8; ++k) {
    a = nan_min(a, sh[0][k * 32 + c]);
    b = nan_max(b, sh[1][k * 32 + c]);
  }
  p.lo[slab * 32 + t] = a;
  p.hi[slab * 32 + t] = b;
}

// diffusion.py:119-123 in float32 (h - lo, then the division by the float32 of hi - lo), ones when hi - lo < 1e-12
__device__ __forceinline__ float gm_gate(float h, float lo, float hi, int clamp) {
  float g = h;
  if (clamp) {
    const double span = (double)hi - (double)lo;
    g = span < 1e-12 ? 1.0f : __fdiv_rn(__fsub_rn(h, lo), (float)span);
  }
  return g < 0.f ? 0.f : (g > 1.f ? 1.f : g);  // np.clip: a NaN stays
}

// 32 API rows x one slab per workgroup: whole lines in (a row of the slab), whole lines out (32 rows of a query)
__global__ __launch_bounds__(256) void k_gm_finish(const GmPanel p, int clamp, const int32_t* __restrict__ inv,
                                                   float* __restrict__ out) {
  __shared__ float tile[32][33];
  const int t = threadIdx.x, lr = t & 7, slab = blockIdx.y;
  const int64_t a0 = (int64_t)blockIdx.x * 32;
  {
    const int64_t a = a0 + (t >> 3);
    if (a < p.N) {
      const int64_t row = inv ? (int64_t)inv[a] : a;
      const float4 x = ld4(p.X + (size_t)slab * p.N * 32 + (size_t)row * 32 + lr * 4);
      const float4 lo = ld4(p.lo + slab * 32 + lr * 4), hi = ld4(p.hi + slab * 32 + lr * 4);
      tile[lr * 4 + 0][t >> 3] = gm_gate(x.x, lo.x, hi.x, clamp);
      tile[lr * 4 + 1][t >> 3] = gm_gate(x.y, lo.y, hi.y, clamp);
      tile[lr * 4 + 2][t >> 3] = gm_gate(x.z, lo.z, hi.z, clamp);
      tile[lr * 4 + 3][t >> 3] = gm_gate(x.w, lo.w, hi.w, clamp);
    }
  }
  __syncthreads();
  const int c = t >> 3, q = slab * 32 + c;
  if (q >= p.nq) return;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int r = lr * 4 + k;
    if (a0 + r < p.N) out[(size_t)q * p.N + a0 + r] = tile[c][r];
  }
}

dim3 gm_grid(const GmPanel& p) { return dim3((unsigned)p.parts, (unsigned)p.slabs); }

}  // namespace

void launch_gm_source(const GmPanel& p, const float* C, float beta, float inv_md, hipStream_t s) {
  hipLaunchKernelGGL(k_gm_source, gm_grid(p), dim3(256), 0, s, p, C, beta, inv_md);
  HIP_CHECK(hipGetLastError());
}

void launch_gm_init(const GmPanel& p, int direct, float tol, hipStream_t s) {
  hipLaunchKernelGGL(k_gm_init, dim3((unsigned)p.slabs), dim3(kGmSumThreads), 0, s, p, direct, tol);
  HIP_CHECK(hipGetLastError());
}

void launch_gm_apply(const GmPanel& p, const GmGraph& g, float cs, hipStream_t s) {
  hipLaunchKernelGGL(k_gm_apply<false>, gm_grid(p), dim3(256), 0, s, p, g, cs, GmRowOp{});
  HIP_CHECK(hipGetLastError());
}

void launch_gm_alpha(const GmPanel& p, hipStream_t s) {
  hipLaunchKernelGGL(k_gm_alpha, dim3((unsigned)p.slabs), dim3(kGmSumThreads), 0, s, p);
  HIP_CHECK(hipGetLastError());
}

void launch_gm_update(const GmPanel& p, float inv_md, hipStream_t s) {
  hipLaunchKernelGGL(k_gm_update<false>, gm_grid(p), dim3(256), 0, s, p, inv_md, GmRowOp{});
  HIP_CHECK(hipGetLastError());
}

void launch_gm_beta(const GmPanel& p, int it, hipStream_t s) {
  hipLaunchKernelGGL(k_gm_beta, dim3((unsigned)p.slabs), dim3(kGmSumThreads), 0, s, p, it);
  HIP_CHECK(hipGetLastError());
}

void launch_gm_direction(const GmPanel& p, float inv_md, hipStream_t s) {
  hipLaunchKernelGGL(k_gm_direction<false>, gm_grid(p), dim3(256), 0, s, p, inv_md, GmRowOp{});
  HIP_CHECK(hipGetLastError());
}

void launch_gm_finish(const GmPanel& p, int clamp, const int32_t* inv, float* out, hipStream_t s) {
  if (clamp) {
    hipLaunchKernelGGL(k_gm_minmax, gm_grid(p), dim3(256), 0, s, p);
    hipLaunchKernelGGL(k_gm_range, dim3((unsigned)p.slabs), dim3(256), 0, s, p);
  }
  hipLaunchKernelGGL(k_gm_finish, dim3((unsigned)((p.N + 31) / 32), (unsigned)p.slabs), dim3(256), 0, s, p, clamp, inv, out);
  HIP_CHECK(hipGetLastError());
}

// ---- the Green's columns of osc_chain_prior_many: the same solve over M' = diag(d) - lamC W -----------------------------------
void launch_gm_row_diag(const float* B, float c, float lamQ, int32_t N, float* d, hipStream_t s) {
  hipLaunchKernelGGL(k_gm_row_diag, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, B, c, lamQ, N, d);
  HIP_CHECK(hipGetLastError());
}

void launch_gm_unit_source(const GmPanel& p, const int32_t* node, const GmRowOp& op, hipStream_t s) {
  hipLaunchKernelGGL(k_gm_unit_source, gm_grid(p), dim3(256), 0, s, p, node, op);
  HIP_CHECK(hipGetLastError());
}

void launch_gm_apply_rows(const GmPanel& p, const GmGraph& g, const GmRowOp& op, hipStream_t s) {
  hipLaunchKernelGGL(k_gm_apply<true>, gm_grid(p), dim3(256), 0, s, p, g, 0.f, op);
  HIP_CHECK(hipGetLastError());
}

void launch_gm_update_rows(const GmPanel& p, const GmRowOp& op, hipStream_t s) {
  hipLaunchKernelGGL(k_gm_update<true>, gm_grid(p), dim3(256), 0, s, p, 0.f, op);
  HIP_CHECK(hipGetLastError());
}

void launch_gm_direction_rows(const GmPanel& p, const GmRowOp& op, hipStream_t s) {
  hipLaunchKernelGGL(k_gm_direction<true>, gm_grid(p), dim3(256), 0, s, p, 0.f, op);
  HIP_CHECK(hipGetLastError());
}

}  // namespace osc

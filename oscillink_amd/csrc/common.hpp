// Shared declarations for liboscillink_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>

#include "host_logic.hpp"  // (OSC_MAX_SRC_BLOCKS, OSC_CHAIN_FIX_MAX_ROWS, kBlkShapes)

namespace osc {

struct HipError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

inline void hip_check(hipError_t e, const char* what, const char* file, int line) {
  if (e != hipSuccess) {
    char buf[512];
    snprintf(buf, sizeof buf, "%s failed: %s (%s:%d)", what, hipGetErrorString(e), file, line);
    throw HipError(buf);
  }
}
#define HIP_CHECK(x) ::osc::hip_check((x), #x, __FILE__, __LINE__)

// Device memory comes from a per-process caching allocator (osc_api.hip): hipMalloc / hipFree cost 0.1-1 ms each and
// hipFree synchronises the device, which dominated the create + destroy time of small lattices (one lattice per request
// in the reference's service).  Freed blocks are parked per device in size classes and handed out again; a block is
// parked only after the freeing handle's stream has drained (alloc_ctx.stream), so no other handle can receive memory
// that still has work in flight.  Contents are NOT zeroed -- exactly like hipMalloc.  OSC_POOL_MB caps the parked bytes
// per device (default 16384, 0 = no caching).
struct AllocCtx {
  int device = 0;
  hipStream_t stream = nullptr;  // the stream the calling handle enqueues on (nullptr: nothing can be in flight)
};
AllocCtx& alloc_ctx();  // thread-local, set by every API entry point
void* pool_alloc(size_t bytes, size_t* cap_bytes);
void pool_free(void* p, size_t cap_bytes);

template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  size_t cap = 0;  // bytes of the underlying block (size class)
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void release() {
    if (p) pool_free(p, cap);
    p = nullptr;
    n = 0;
    cap = 0;
  }
  void alloc(size_t count) {
    if (count == n && p) return;
    release();
    if (count) p = reinterpret_cast<T*>(pool_alloc(count * sizeof(T), &cap));
    n = count;
  }
  void swap(DevBuf& o) {
    std::swap(p, o.p);
    std::swap(n, o.n);
    std::swap(cap, o.cap);
  }
};

// ---- operator description ------------------------------------------------------------------
// out_i = (cs_const + cs_B * B_i) x_i - cW * sum_j W_ij x_j - cP * sum_j Wp_ij x_j
// Jacobi diagonal  Md_i = md_const + md_B * B_i   (lattice.py:187-192, 257-259: lamC is NOT in it)
// rhs              b_i  = rbU U_i + rbY Y_i + rbB B_i psi
struct OpParams {
  float cs_const, cs_B, cW, cP;
  float md_const, md_B;
  int precond;
  float rbU, rbY, rbB;
};

// ELL view of the lattice graph (degree <= width; columns ascending within a row)
struct GraphView {
  const int32_t* col;   // [N][width]
  const float* w;       // [N][width]   normalised weights W_ij
  const int32_t* deg;   // [N]
  int32_t width;
  // chain prior: path_slot[i] = -1 or row index into the (tiny) path ELL
  const int32_t* path_slot;  // nullptr when no chain / lamP == 0
  const int32_t* pcol;       // [P][pwidth]
  const float* pw;           // [P][pwidth]  normalised path weights
  const int32_t* pdeg;       // [P]
  int32_t pwidth;
};

// The lattice graph a second time, split by SOURCE-row block (k_spmm_blocked): block b holds the edges whose neighbour row
// lies in [b * rows_per_block, (b + 1) * rows_per_block), rows_per_block = ceil(N / nb).  Fixed-width: every (block, row)
// owns OSC_BLK_SLOTS slots {neighbour row, bits of W_ij}, filled in the order of the ELL row, unused slots {first row of
// the block, 0.0f} (gathered and multiplied by zero: no tests in the gather loop); an
// edge that finds the slot row of its block full sits in a later block's free slots instead (k_blk_fill), and what fits
// nowhere is in over[rest[row].x .. + rest[row].y), added after the blocks (so such rows' sums are formed in a different
// order than k_spmm's: same terms, last-bit differences).
constexpr int OSC_BLK_SLOTS = 4;
struct BlockedView {
  const int2* slots;    // [nb][N][OSC_BLK_SLOTS]
  const int2* rest;     // [N] {first, count} into over
  const int2* over;
  int32_t nb;           // source blocks; 0 = no blocked copy
};

// arguments of the source-blocked CG matvec (k_apply_blocked): out = (cs_const + cs_B B_i) x_i - cW sum_j W_ij x_j
struct BlkArgs {
  const float* X;   // operand, slab-major [ld / 32][N][32]
  float* OUT;       // result, row-major with pitch ld
  const float* B;   // [N]
  float* part;      // [grid][ld] column partial sums of x . out
  const int2* slots;
  const int2* rest;
  const int2* over;
  const float* gate;  // see SpmmArgs
  float gate_tol;
  float cs_const, cs_B, cW;
  int32_t N, ld, c0, c1;
  int32_t xs, xs_groups;  // workgroups per XCD that take part, slab groups (as in SpmmArgs)
  int32_t nb, groups, slices;  // source blocks; row groups (of 8 rows) per gathering wave and slice; dest-row slices
};

// k_apply_blocked as the solve's INIT pass (r = rhs - A x0, z, r . z in the matvec's epilogue): see the kernel
struct BlkInit {
  const float* Y;    // rhs term, row-major; nullptr: it is x0 (BlkArgs::X)
  float* Xcopy;      // nullptr, or the solution array x0 is copied to (row-major)
  float* R;          // residual out, row-major
  float* Z;          // z = M^-1 r out, SLAB-major like BlkArgs::X (must not be that array)
  const float* psi;  // [ld]
  float rbU, rbY, rbB, md_B, md_const;  // no preconditioner: md_B = 0, md_const = 1
  // the row sums sum_j W_ij x0_j, slab-major like BlkArgs::X (the anchors' cached W.Y, L::WYs): written by the gathering pass
  // in its storing form (launch_apply_blocked, store_wy), read in place of the gather by k_init_cached; nullptr otherwise
  float* WY;
};

// k_init_cached in the form that also emits iteration 1's operator output A p1 (p1 = z0) of an anchor start under uniform
// gates, from the anchors' cached second row sums (L::WWs, L::Wsum): see the kernel
struct BlkInitAp {
  const float* WW;    // W (W Y), row-major with pitch ld
  const float* wsum;  // [N] s = W 1
  float* AP;          // A p1 out, row-major
  float* part;        // [grid][ld] column partial sums of p1 . A p1
};

// ... and, one level further, T = A (A p1) from the anchors' third row sums (L::W3s, L::Wsum2): iteration 2's p update then
// forms A p2 = (1 + beta1) A p1 - m alpha1 T without a gather (k_update_p_ap2)
struct BlkInitAp2 {
  const float* W3;     // W (W (W Y)), row-major with pitch ld
  const float* wsum2;  // [N] s2 = W (W 1)
  float* T;            // A (A p1) out, row-major
};

// The Gram sums of an anchor start's seven basis vectors (anchor_gram.hpp has the layout): one streaming pass over the cached
// row sums, per-chunk partials in float64, folded in chunk order (k_anchor_gram_part, k_anchor_gram_fold)
constexpr int OSC_GRAM_CHUNKS = 64;
struct GramArgs {
  const float* Ys;     // the anchors, slab-major (BlkArgs::X)
  const float* WYs;    // W Y, slab-major (BlkInit::WY)
  const float* WW;     // W W Y, row-major
  const float* W3;     // W W W Y, row-major
  const float* wsum;   // [N] s = W 1
  const float* wsum2;  // [N] s2 = W s
  double* part;        // [OSC_GRAM_CHUNKS][22][ld], then [OSC_GRAM_CHUNKS][6]
  double* out;         // [22][ld], then [6]
  int32_t N, ld, c0, c1;
};
void launch_anchor_gram(const GramArgs& a, hipStream_t s);
// ... and of the two vectors the third step adds (anchor_gram.hpp: kGram3PerColumn, kGram3Lattice): the same two kernels' scheme
// (k_anchor_gram3_part, k_anchor_gram3_fold) with W W W W Y (row-major, scratch: read here and never again) and s3 = W s2 beside
// the six arrays above
struct Gram3Args {
  GramArgs g;          // part: [OSC_GRAM_CHUNKS][13][ld], then [OSC_GRAM_CHUNKS][4]; out: [13][ld], then [4]
  const float* W4;     // W W W W Y, row-major
  const float* wsum3;  // [N] s3 = W s2
};
void launch_anchor_gram3(const Gram3Args& a, hipStream_t s);
// ... and of the two the fourth step's scalars add (anchor_gram.hpp: kGram4PerColumn, kGram4Lattice): the same scheme again
// (k_anchor_gram4_part, k_anchor_gram4_fold) with W^4 Y and W^5 Y (row-major, scratch) and s3, s4 = W s3
struct Gram4Args {
  GramArgs g;          // part: [OSC_GRAM_CHUNKS][16][ld], then [OSC_GRAM_CHUNKS][5]; out: [16][ld], then [5]
  const float* W4;     // W^4 Y, row-major
  const float* W5;     // W^5 Y, row-major
  const float* wsum3;  // [N] s3 = W s2
  const float* wsum4;  // [N] s4 = W s3
};
void launch_anchor_gram4(const Gram4Args& a, hipStream_t s);

// k_anchor_gram_scalars: iterations 1 and 2's alpha, beta, residuals and r2 . z2 per column from the Gram sums, the two
// residuals (max over the columns) into the solve's residual slots and host-mapped words, and the word that lets
// k_init_two_steps run: 1 only if every column is usable and both residuals are above tol
struct GramScalarArgs {
  const double* gram;
  const float* psi;  // [ld]
  const float* B;    // [N], one value
  float cs_const, cs_B, cW, rbU, rbY, rbB, md_B, md_const;  // BlkArgs' / BlkInit's
  float tol;
  int32_t ld, c0, c1;
  float* alpha1;
  float* alpha2;
  float* beta1;
  float* beta2;
  double* rz;
  uint32_t* res_slots;   // the solve's residual slots: [1] and [2] are written
  uint32_t* host_words;  // the same two, host-mapped
  uint32_t* go;          // three words: [0] lets k_init_two_steps run, [1] (third step only) iteration 3's fused matvec, [2] see gram4
  // The third step (anchor_gram.hpp: three_steps), planned iff gram3 != nullptr: alpha3, beta3 and r3 . z3 per column (rz then
  // holds r3 . z3, not r2 . z2), |r3| into residual slot and host word 3, and go[1], the word that lets the FUSED matvec of
  // iteration 3 run: 1 only if every column is usable and all three residuals are above tol.
  const double* gram3;
  float* alpha3;
  float* beta3;
  // The fourth step's scalars (anchor_gram.hpp: four_steps), planned iff gram4 != nullptr (only with gram3): alpha4 per column and
  // |r4| into host word 4 (the device's residual slot 4 stays zero for k_reduce_beta's atomicMax: only the host acts on |r4|).  rz and beta3 keep iteration 3's values: a solve that goes on past iteration 4 sums
  // that iteration's scalars as ever.  The host words go out in the order 4, 3, 2, 1.
  // go[2] (always written): 1 exactly if the fourth step is planned, go[1] == 1 and |r4| <= tol -- host::anchor_gram4_last_form on
  // the very floats that are published, as a device word: the INIT pass and the matvec's folded last form act on it.
  const double* gram4;
  float* alpha4;
  // The polynomial last form's coefficients (anchor_gram.hpp: poly4_coeffs; only with gram4; nullptr: not planned): nine rows of ld
  // floats, a0 .. a4 then q0 .. q3, from alpha1 .. alpha4 and beta1 .. beta3 before they are rounded to float.  Written for every
  // column of the window; k_settle_poly, their one reader, runs only where go[2] == 1.
  float* poly;
};
void launch_anchor_gram_scalars(const GramScalarArgs& a, hipStream_t s);

// k_settle_poly: an anchor start that ends in iteration 4 as one elementwise pass over the lattice's five row-sum arrays,
//   x4 = a0 Y + a1 W Y + a2 W W Y + a3 W^3 Y + a4 W^4 Y + (q0 + q1 s + q2 s2 + q3 s3)
// with GramScalarArgs::poly's coefficients per column.  Writes X alone; a no-op unless *go == 1 and *go_fold == 1 (go[0] and go[2]
// of the scalars kernel).  The launch geometry and addressing are k_init_two_steps_stream's.
struct SettlePolyArgs {
  const float* Ys;     // the anchors, slab-major
  const float* WYs;    // W Y, slab-major
  const float* WW;     // W W Y, row-major with pitch ld
  const float* W3;     // W^3 Y, row-major
  const float* W4;     // W^4 Y, row-major
  const float* wsum;   // [N] s = W 1
  const float* wsum2;  // [N] s2 = W s
  const float* wsum3;  // [N] s3 = W s2
  const float* coef;   // [9][ld]
  float* X;            // x4 out, row-major
  const uint32_t* go;
  const uint32_t* go_fold;
  int32_t N, ld, c0, c1;
};
// false (nothing launched): the arguments are outside what the kernel's 32-bit offsets and float4 columns cover
bool settle_poly_supported(const SettlePolyArgs& a);
void launch_settle_poly(const SettlePolyArgs& a, int grid, hipStream_t s);

// k_init_two_steps: the cached INIT pass of BlkInitAp2 run through iterations 1 and 2 with the scalars above.  Of BlkInit it
// writes R (r2, row-major), Z (p3, slab-major) and Xcopy (x2 = x0 + alpha1 p1 + alpha2 p2, or with BlkTwoSteps::alpha3 x3 = x2 +
// alpha3 p3, row-major; required); of BlkInitAp
// and BlkInitAp2 it reads WW, wsum, W3, wsum2 and writes nothing.  A no-op unless *go == 1.
// Two forms with the same bits (launch_init_two_steps): the streaming one (k_init_two_steps_stream, the update kernels' launch
// geometry; of BlkArgs it reads X, B, N, ld, c0, c1 and the operator's scalars only) and the blocked one, the reference form.
struct BlkTwoSteps {
  const float* alpha1;
  const float* alpha2;
  const float* beta1;
  const float* beta2;
  const uint32_t* go;
  int32_t row0;  // first row (streaming form; the blocked form's geometry covers every row: 0 there)
  // The three-step route: alpha3 is out before the pass runs, and Xcopy takes x3 = x2 + alpha3 p3 (k_update_x_ring's fmaf on
  // the same floats) instead of x2.  nullptr: x2.
  const float* alpha3;
  // The folded last form (only with alpha3; go_fold == nullptr: never): where *go_fold == 1 the solve ends in iteration 4, beta3 and
  // alpha4 are out, and Xcopy takes e = x4 with a zero row sum in A p3's place -- r3 = r2 - alpha3 (cs p3), p4 = beta3 p3 + M^-1 r3,
  // e = x3 + alpha4 p4, the FUSED_LAST epilogue's operations in its operand order -- instead of x3.  R is not written then; Z takes
  // p3 as ever.  With *go_fold == 0 every stored bit is the pass's without it.
  const float* beta3;
  const float* alpha4;
  const uint32_t* go_fold;
};

// k_apply_blocked as iteration 3 of an anchor start whose alpha3 and beta3 are known beforehand (GramScalarArgs::gram3): the
// epilogue forms r3 = r2 - alpha3 A p3 (k_update_xr's expression) in place in R and p4 = z3 + beta3 p3 (k_update_p's) slab-major
// into Pout; BlkArgs::OUT and BlkArgs::part are not written.  A no-op unless *go == 1.
struct BlkFused {
  float* R;            // r2 in, r3 out, row-major
  float* Pout;         // p4 out, slab-major like BlkArgs::X (must not be that array)
  const float* alpha;  // [ld] alpha3
  const float* beta;   // [ld] beta3
  const uint32_t* go;
  float md_B, md_const;  // no preconditioner: 0, 1
  // The last form (FUSED_LAST: the solve ends in iteration 4 and alpha4 is known, GramScalarArgs::gram4): r3 and p4 are formed in
  // registers with the same expressions and x4 = x3 + alpha4 p4 is written in place over X; R and Pout are not written (Pout may
  // be nullptr).
  float* X;                  // x3 in, x4 out, row-major
  const float* alpha_last;   // [ld] alpha4
  // The folded last form (go_fold != nullptr; needs X and alpha_last): the INIT pass left e in X (BlkTwoSteps::go_fold), x4 is affine
  // in the gathered row sum, x4 = e + (alpha4 alpha3) (M^-1 cW) acc, and the epilogue is one fmaf per element on the row of e: no own
  // row of p3, no R, no beta.  A no-op unless *go_fold == 1 (the word the INIT pass acted on).
  const uint32_t* go_fold;
};

enum SpmmMode { SPMM_AP = 0, SPMM_INIT = 1, SPMM_DOT = 2 };

struct SpmmArgs {
  GraphView g;
  OpParams op;
  const float* X;     // operand (gathered)
  float* OUT;         // AP: A x ; INIT: x copy (x0)     (may alias nothing else)
  float* R;           // INIT: residual out
  float* P;           // INIT: search direction out
  const float* U;     // INIT rhs
  const float* Y;     // INIT rhs
  const float* B;     // [N]
  const float* psi;   // [ld]
  float* part;        // [grid][ld] column partial sums of the mode's dot product
  int64_t N;          // end of the row range this launch works on (rows [row0, N))
  int64_t row0;       // first row (0 except in row-sharded multi-GPU runs)
  int32_t ld;         // row pitch in floats (multiple of 4)
  int32_t c0, c1;     // column window [c0, c1), multiples of 4
  // speculative-launch gate: the kernel is a no-op when *gate <= gate_tol (the CG already converged; the host
  // enqueues one iteration ahead of its residual read-back).  nullptr = always run.
  const float* gate;
  float gate_tol;
  // xs > 0: XCD-affine narrow slabs.  The window [c0, c1) is cut into 32-column slabs (one 128-byte line per row).
  // The eight XCDs (x = blockIdx % 8) form xs_groups slab groups of 8 / xs_groups XCDs each: group g = x % xs_groups
  // owns slabs g, g + xs_groups, ... and its XCDs split the rows among themselves (part x / xs_groups); the first xs
  // workgroups of each XCD do the work.  The slab an XCD gathers from (N x 128 B) then competes for that XCD's 4 MB
  // L2 alone instead of with the other slabs of the window.  xs_groups = gcd(8, number of slabs): always balanced.
  int32_t xs;
  int32_t xs_groups;
  // Slab-major ("blocked") layout of the CG search direction, xs mode only: element (row, col) of an array stored
  // that way sits at ((col / 32) * rows + row) * 32 + col % 32, so the 32-column slab an XCD gathers from is one
  // contiguous N x 128 B range (even spread over the L2 channels; no 3 KB row stride).  xblk != 0: the operand X is
  // stored that way (value = rows per slab = N); pblk != 0: INIT writes its P output that way.
  int64_t xblk, pblk;
  // != 0: the rows are stored in a local order (maybe_reorder): launch the variant with more gathers in flight per row
  int32_t deep;
};

struct UpdateArgs {
  float* X;
  float* R;
  float* P;
  const float* AP;
  const float* B;
  const float* alpha;  // [ld]
  const float* beta;   // [ld]
  float* part_rr;      // [grid][ld]
  float* part_rz;      // [grid][ld]
  OpParams op;
  int64_t N;      // rows [row0, N)
  int64_t row0;
  int32_t ld, c0, c1;
  const float* gate;  // see SpmmArgs
  float gate_tol;
  int64_t pblk;  // != 0: P is stored slab-major with this many rows per slab (see SpmmArgs)
  // != 0: the solve's five N x window arrays fit the Infinity Cache together (a per-rank window of a sharded solve, a
  // mid-size lattice): X, R, AP are then read and written with ordinary loads / stores so that the next kernel finds them
  // there; 0: streamed nontemporally (they would only push the gathered operand out).
  int32_t temporal;
  // where the x update happens (run_cg): 0 = in k_update_xr, next to the r update (x, r, p, Ap read; x, r written);
  // OSC_XMODE_XR_SKIPS_X: not there; OSC_XMODE_P_APPLIES_X: k_update_p applies the PREVIOUS iteration's while it has p in
  // hand (launch_update_x behind the last iteration) -- one array pass less per iteration; OSC_XMODE_XR_LAST: k_update_xr
  // in the form for the expected last iteration (x finished there, the new r not stored)
  int32_t xmode;
  // the x an x update READS (nullptr: X itself).  The settle that starts from the anchors without copying them: the one
  // launch that applies iteration 1's update reads x0 from the anchors and writes x into X (run_cg)
  const float* Xin;
  // where k_update_p writes the new direction (nullptr: over P).  A solve that keeps its directions in a ring (run_cg) reads
  // the previous one from P and writes the next slot; no kernel of such a solve touches x but k_update_x_ring
  float* Pout;
  // k_update_p_ap2 only (iteration 2 of an anchor start whose INIT pass left Q1 = A p1 in the AP array and T = A Q1): the
  // launch also writes A p2 = (1 + beta) Q1 - (m alpha) T over Q1 (APout, the array AP names) and the column partials of
  // p2 . A p2 into part_rr; alpha is iteration 1's.  nullptr in every other launch.
  const float* T;
  float* APout;
};
// OSC_XMODE_XR_BARE (with XR_SKIPS_X): the x-r kernel of the expected last iteration of a ring solve -- x left alone, the new
// r not stored
constexpr int32_t OSC_XMODE_XR_SKIPS_X = 1, OSC_XMODE_P_APPLIES_X = 2, OSC_XMODE_XR_LAST = 4, OSC_XMODE_XR_BARE = 8;

// k_update_x_ring: x = Xin (nullptr: X) + sum over m < M of alpha[m] * P[m], applied in ascending m with one fmaf each --
// the roundings the per-iteration x updates perform through memory
constexpr int OSC_X_RING_MAX = 4;
struct XRingArgs {
  float* X;
  const float* Xin;
  const float* P[OSC_X_RING_MAX];      // kept directions, oldest first (layout: pblk)
  const float* alpha[OSC_X_RING_MAX];  // [ld] each
  int32_t M;
  int64_t N, row0;
  int32_t ld, c0, c1;
  const float* gate;
  float gate_tol;
  int64_t pblk;
  int32_t temporal;
};

struct Gate {
  const float* p;
  float tol;
};

// launchers implemented in cg_kernels.hip
int spmm_grid(int64_t N, int32_t ncols);
// source-blocked copy of an ELL graph (BlockedView): count the overflow entries (-> *over_count, device), then fill
void launch_blocked_count(const int32_t* col, const int32_t* deg, int32_t width, int32_t N, int32_t nb,
                          unsigned* over_count, hipStream_t s);
void launch_blocked_fill(const int32_t* col, const float* w, const int32_t* deg, int32_t width, int32_t N, int32_t nb,
                         int2* slots, int2* rest, int2* over, unsigned* over_count, hipStream_t s);
// Chain prior beside the blocked matvec: out_i -= cP sum_j Wp_ij x_j for the (few) rows of the chain's path graph, and
// the matching terms of the p . Ap column sums into the rows [part_row0, part_row0 + chunks) of `part`.
constexpr int OSC_CHAIN_FIX_MAX_CHUNKS = 64;
struct ChainFixArgs {
  const float* X;        // operand, slab-major
  float* OUT;            // row-major, pitch ld: already holds the result without the chain term
  float* part;
  const int32_t* prow;   // [prows] lattice row of path row s
  const int32_t* pcol;   // [prows][pwidth]
  const float* pw;
  const int32_t* pdeg;
  const float* gate;
  float gate_tol, cP;
  int32_t prows, pwidth, N, ld, c0, c1, part_row0, chunks;
  // behind k_apply_blocked's INIT pass (BlkInit): patch r (row-major), z (slab-major) and the r . z partials of the path
  // rows instead of OUT / x . out; nullptr otherwise
  float* initR;
  float* initZ;
  const float* B;
  float md_B, md_const;  // no preconditioner: 0, 1
};
// initial residual of a solve around the blocked matvec: rows_to_slab copies the columns [c0, c1) of a row-major array into
// the slab-major layout the blocked matvec gathers from; init_finish turns AP = A x0 into r = b - A x0, z = r / (Md + eps),
// p = z (slab-major), the x0 copy (when the solve is not in place) and the r . z column partials -- the tail of
// k_spmm<.., INIT>, same expressions (solver.py:19-22)
struct InitFinishArgs {
  const float* AP;   // A x0, row-major
  const float* X0;   // x0
  float* X;          // solution array (== X0: in place, nothing to copy)
  float* R;
  float* P;          // slab-major, `pblk` rows per slab
  const float* U;    // rhs terms (either may alias X0)
  const float* Y;
  const float* B;
  const float* psi;
  float* part;       // [grid][ld] r . z partials
  OpParams op;
  int64_t N, pblk;
  int32_t ld, c0, c1;
};
void launch_rows_to_slab(const float* src, float* dst, int64_t N, int32_t ld, int32_t c0, int32_t c1, int grid, hipStream_t s,
                         const float* sub = nullptr);  // sub: dst = src - sub
void launch_init_finish(const InitFinishArgs& a, int grid, hipStream_t s);
int chain_fix_chunks(int32_t prows);
void launch_chain_fix(const ChainFixArgs& a, hipStream_t s);
// store_wy: the INIT pass (init != nullptr) also writes its row sums to init->WY
void launch_apply_blocked(const BlkArgs& a, int grid, hipStream_t s, const BlkInit* init = nullptr, int variant = 0,
                          bool store_wy = false);
void launch_apply_blocked_fused(const BlkArgs& a, int grid, hipStream_t s, const BlkFused& f, int variant);
// the same INIT pass with the row sums read from init.WY instead of gathered (k_init_cached): same results to the bit
// ap: the form that also streams iteration 1's A p1 and its p . Ap sums (BlkInitAp)
// ap2 (with ap): ... and T = A (A p1) (BlkInitAp2)
void launch_init_cached(const BlkArgs& a, int grid, hipStream_t s, const BlkInit& init, int variant, const BlkInitAp* ap = nullptr,
                        const BlkInitAp2* ap2 = nullptr);
// stream: the streaming form (its shape by the window alone, as launch_update_x_ring's; `variant` is the blocked form's)
void launch_init_two_steps(const BlkArgs& a, int grid, hipStream_t s, const BlkInit& init, int variant, const BlkInitAp& ap,
                           const BlkInitAp2& ap2, const BlkTwoSteps& ts, bool stream);
void launch_row_weight_sums(const float* w, const int32_t* deg, int32_t width, int32_t N, float* out, hipStream_t s);
// out_i = sum_j W_ij v_j over the ELL row, in stored order (BlkInitAp2::wsum2 from BlkInitAp::wsum)
void launch_row_weighted_sums(const int32_t* col, const float* w, const int32_t* deg, int32_t width, int32_t N, const float* v,
                              float* out, hipStream_t s);
int blocked_resident_per_cu(int variant);  // workgroups per CU a kernel shape (kBlkShapes) gets resident
void launch_spmm(int mode, const SpmmArgs& a, int grid, hipStream_t s);
void launch_update_xr(const UpdateArgs& a, int grid, hipStream_t s);
void launch_update_p(const UpdateArgs& a, int grid, hipStream_t s);
void launch_update_p_ap2(const UpdateArgs& a, int grid, hipStream_t s);  // (UpdateArgs::T, APout)
void launch_update_x(const UpdateArgs& a, int grid, hipStream_t s);  // x += alpha p (UpdateArgs::xmode)
void launch_update_x_ring(const XRingArgs& a, int grid, hipStream_t s);
// column reductions over `nb` partial rows
void launch_reduce_init(const float* part, int nb, int32_t ld, int32_t c0, int32_t c1, double* rz, hipStream_t s);
void launch_reduce_alpha(const float* part, int nb, int32_t ld, int32_t c0, int32_t c1, const double* rz,
                         float* alpha, Gate g, hipStream_t s);
void launch_reduce_beta(const float* part_rr, const float* part_rz, int nb, int32_t ld, int32_t c0, int32_t c1,
                        double* rz, float* beta, uint32_t* res_bits_slot, Gate g, hipStream_t s,
                        uint32_t* done_ctr = nullptr, float* host_slot = nullptr);
void launch_publish_word(const uint32_t* src, uint32_t* host_slot, hipStream_t s);
void launch_reduce_sum(const float* part, int nb, int32_t ld, int32_t c0, int32_t c1, double* out_cols,
                       hipStream_t s);
void launch_axpby(float* out, const float* a, float ca, const float* b, float cb, int64_t n, hipStream_t s);
// row-sharded CG: the column sums are completed across ranks (all-reduce of fp64 sums) before these finish steps
void launch_finish_init(const double* sums, int32_t c0, int32_t c1, double* rz, hipStream_t s);
void launch_finish_alpha(const double* sums, int32_t c0, int32_t c1, const double* rz, float* alpha, Gate g,
                         hipStream_t s);
void launch_finish_beta(const double* sums_rr, const double* sums_rz, int32_t c0, int32_t c1, double* rz, float* beta,
                        uint32_t* res_bits_slot, Gate g, hipStream_t s);
void launch_reduce_sum_gated(const float* part, int nb, int32_t ld, int32_t c0, int32_t c1, double* out_cols, Gate g,
                             hipStream_t s);

}  // namespace osc

// Multi-query bundles: the kernels behind osc_bundle_many / osc_mmr_many (query_kernels.hip).
// Everything is in device row order; queries are contiguous per row (an N x qs array holds query q of row i at i * qs + q).
#pragma once
#include "../../include/oscillink_hip.h"
#include "common.hpp"

namespace osc {

constexpr int kQueryChunk = OSC_QUERY_CHUNK;  // queries per pass (include/oscillink_hip.h)
constexpr int kQueryTileQ = 128;              // query columns of one k_query_gemm workgroup
constexpr int kQueryTileK = 32;               // K step of the GEMM (the B operand is padded to a multiple of it)

inline int32_t query_kpad(int32_t D) { return (D + kQueryTileK - 1) / kQueryTileK * kQueryTileK; }
inline int32_t query_qpad(int32_t Q) { return (Q + kQueryTileQ - 1) / kQueryTileQ * kQueryTileQ; }
inline int32_t query_qs(int32_t Q) { return (Q + 3) & ~3; }  // row pitch of the N x Q arrays

// per-row constants of a query basis (X, x): s_i = x_i / (sd_i + 1e-12), |X_i|^2 and the two per-edge sums
//   c0_i = sum_j 1/2 lamC A_ij (|Yn_i - Yn_j|^2 - |P_i - P_j|^2),  c2_i = sum_j 1/2 lamC A_ij (s_i - s_j)^2
struct QueryBasisArgs {
  const float* Y;
  const float* X;       // N x ld
  const float* x4;      // N x 4, column 0 = x
  const float* sqrt_deg;
  const int32_t* col;
  const float* adj;     // capped adjacency A_ij (ELL)
  const int32_t* deg;
  int32_t width, N, D, ld;
  float lamC;
  double* s;            // [N] (fp64: (s_i - s_j)^2 |psi|^2 carries its rounding through every column)
  double* xn2;          // [N]
  double* c0;           // [N]
  double* c2;           // [N]
};
void launch_query_basis_stats(const QueryBasisArgs& a, hipStream_t s);

// C[N x qs] = A[N x D] (row pitch ld) . Bt[qpad x kpad]^T on v_mfma_f32_32x32x2_f32, K in one fixed order for every output.
// mode 0 (dots): C = g = X psi^T; the epilogue writes align (cos(U*_i, psi_q)) and p = g / (sd_i + 1e-12)
// mode 1 (mmr):  C = <Yn_i, Yn_pick(q)>; the epilogue folds it into the running maximum (first: replaces it; +inf = taken)
// mode 2 (rows): C = A Bt^T for any rows of Bt (the nq rows of a pass's T_q V_q blocks); the epilogue
//                writes p = C / (sd_i + 1e-12) and nothing else (sqrt_deg and p of mode 0's fields)
struct QueryGemmArgs {
  const float* A;
  const float* Bt;
  int32_t N, D, ld, kpad, qs, nq;  // nq: real query columns (< qs are stored, >= nq stored as 0 / untouched)
  int mode, first;
  // mode 0
  const float* x4;
  const double* xn2;
  const float* sqrt_deg;
  const double* pn2;   // [nq] |psi_q|^2
  const double* pinv;  // [nq] 1 / (|psi_q| + 1e-12)
  float* align;
  float* p;
  // mode 1
  float* maxsim;
};
void launch_query_gemm(const QueryGemmArgs& a, hipStream_t s);

// coh_iq = c0_i - |psi_q|^2 c2_i - sum_j lamC A_ij (s_i - s_j)(p_iq - p_jq) in fp64, stored fp32
void launch_query_coh(const int32_t* col, const float* adj, const int32_t* deg, int32_t width, int32_t N, float lamC,
                      const double* s, const double* c0, const double* c2, const double* pn2, const float* p, int32_t qs,
                      int32_t nq, float* coh, hipStream_t st);
// score = alpha (coh - mu_q) / sigma_q + (1 - alpha) align, in place over coh; mu / sigma per query from a deterministic
// two-stage fp64 column reduction (part: [nb x nq] double2 partials, stats: [nq] double2)
int query_stat_parts(int32_t N);
void launch_query_score(float* coh_score, const float* align, int32_t N, int32_t qs, int32_t nq, double alpha, double2* part,
                        double2* stats, hipStream_t st);

// row-normalised anchors Yn_i = Y_i / (|Y_i| + 1e-12) (the MMR's representers; pad columns 0)
void launch_rows_normalise(const float* Y, float* Yn, int32_t N, int32_t D, int32_t ld, hipStream_t st);

// batched greedy MMR: one step for every query at once.  maxsim: N x qs running maxima (+inf = already chosen);
// per query the best (1 - lambda) score - lambda maxsim under the total order of osc_mmr (value, then the smaller API id)
struct MmrManyArgs {
  const float* score;   // N x qs
  float* maxsim;        // N x qs
  const int32_t* api_id;  // nullptr = identity
  const float* Yn;      // N x ld
  float* Bt;            // [qpad x kpad] normalised anchor rows of this step's picks (the next GEMM's operand)
  double* pval;         // [nb x nq]
  int32_t* pid;
  int32_t* prow;
  int32_t* chosen_api;  // [nq x k]
  int32_t* chosen_row;  // [nq x k]
  int32_t N, D, ld, kpad, qs, nq, k;
  double lambda;
};
int mmr_many_parts(int32_t N);
void launch_mmr_many_argmax(const MmrManyArgs& a, int step, hipStream_t st);

// out[q * k + t] = score / align of query q at its t-th pick (0 past the end)
void launch_query_pack(const float* score, const float* align, const int32_t* chosen_row, int32_t qs, int32_t nq, int32_t k,
                       float* out_score, float* out_align, hipStream_t st);

}  // namespace osc

// ---- bundles under per-query chain priors: bundle_prior_kernels.hip ---------------------------
namespace osc {

constexpr int kBpNodes = 64;  // nodes of a chain system at most (chain_prior_plan.hpp: kChainPriorMaxNodes): one per lane

// Bt[r][0 .. kpad) = TV[r][0 .. D) then zeros for r < rows, zeros for rows <= r < rows_pad (TV at pitch ld)
void launch_bp_pack(const float* TV, int64_t rows, int64_t rows_pad, int32_t D, int32_t ld, int32_t kpad, float* Bt,
                    hipStream_t s);

// Per (row, query) of a pass on U*_q,i = X'_i + x'_i psi_q + sum_b G_ib C_b (C = T_q V_q, the query's m rows of TV), in the
// units of section 11: di = sd_i + 1e-12, s = x' / di, p = X'_i . psi / di, gamma_ib = G_ib / di, kappa_ib = X'_i . C_b / di.
struct BpArgs {
  const int32_t* col;     // ELL, device rows
  const float* adj;       // capped adjacency
  const int32_t* deg;
  int32_t width, N;
  float lamC;
  const float* sqrt_deg;
  const double* s;        // [N] of the shifted basis, with xn2 / c0 / c2 (k_query_basis_stats on (X', x'))
  const double* xn2;
  const double* c0;
  const double* c2;
  const float* p;         // N x qs (k_query_gemm<0> on the shifted basis)
  const float* G;         // the pass's Green's columns, slab-major
  const float* kappa;     // N x ks (k_query_gemm<2>); query q's columns start at tv_at[q] / ld
  const float* TV;        // the pass's T_q V_q blocks, m x ld each at tv_at[q]
  const float* psi;       // nq x ld
  const int32_t* q_sys;   // [nq] the query's chain system
  const int32_t* sys_m;
  const int32_t* sys_col_at;
  const int32_t* sys_cols;
  const int64_t* tv_at;   // [nq]
  const double* pn2;      // [nq] |psi_q|^2
  const double* pinv;     // [nq] 1 / (|psi_q| + 1e-12)
  int32_t D, ld, ks, qs, nq;
  int32_t gs;             // lanes of a (row, query) pair in the row kernels: a power of two in [max m of the pass, 64]
  double* e;              // [nq][64]      e_b = C_b . psi (0 past m)
  double* H;              // [nq][64][64]  H_bb' = C_b . C_b' (0 past m)
  double* nu;             // N x qs  gamma_i^T H gamma_i
  float* align;           // N x qs
  float* coh;             // N x qs
};
// e and H per query: fp64 sums over the columns in column order
void launch_bp_scalars(const BpArgs& a, hipStream_t s);
// nu and align per (row, query): gs lanes each, lane b of the group owns node b
void launch_bp_rows_self(const BpArgs& a, hipStream_t s);
// coh per (row, query): section 11's three terms on the shifted basis and, per graph edge in slot order,
//   1/2 lamC A_ij [2 sum_b dgamma_b (dkappa_b + ds e_b) + nu_i + nu_j - 2 gamma_j . (H gamma_i)]
void launch_bp_rows_coh(const BpArgs& a, hipStream_t s);

}  // namespace osc

// ---- multi-query receipts: receipt_many_kernels.hip ------------------------------------------
namespace osc {

constexpr int kRmSelectMax = 1024;  // largest null-point cap the device selection keeps (larger caps: host sort)

// per basis, one wave per row: Mx_i = (M x)_i in fp64 (the U* operator with the lattice's gates / chain / lambdas), and
// with dslot != nullptr d_ij = |P_i - P_j|^2 per ELL slot (k_query_basis_stats' dp, 0 where A_ij <= 0)
struct RmBasisArgs {
  const float* X;
  const float* x4;
  const float* B;
  const float* sqrt_deg;
  GraphView g;       // normalised weights + chain prior (the operator's)
  const float* adj;  // capped adjacency (the receipt's weights)
  OpParams op;
  int32_t N, D, ld;
  double* Mx;     // [N]
  float* dslot;   // [N * width] or nullptr
};
void launch_rm_basis_rows(const RmBasisArgs& a, hipStream_t s);

// deterministic fp64 column sums over the rows (row r goes to partial r % nb, summed in row order; the partials in block
// order).  mode 0 (per basis): part[b][4][ld] = x_i (X - Y), B_i (x_i - 1) X, (X - Y)^2, B_i X^2 and spart[b][3] =
// x_i^2, B_i (x_i - 1)^2, x_i Mx_i.  mode 1 (per call): part[b][1][ld] = (U - X - x psi0)_i Mx_i, and U0 = X + x psi0^T.
struct RmColArgs {
  const float* X;
  const float* x4;
  const float* Y;   // mode 0
  const float* B;   // mode 0
  const double* Mx;
  const float* U;     // mode 1
  const float* psi0;  // mode 1, [ld]
  float* U0;          // mode 1, N x ld
  int32_t N, D, ld, nb;
  double* part;
  double* spart;
};
int rm_col_parts(int64_t N);
void launch_rm_cols(const RmColArgs& a, int mode, hipStream_t s);
// out[w] = sum_b part[b * W + w] in block order: directly up to kRmFinishRows partials, else by groups of that many
// (scratch: rm_finish_groups(nb) * W doubles), then the groups in order
constexpr int kRmFinishRows = 64;
inline int rm_finish_groups(int nb) { return (nb + kRmFinishRows - 1) / kRmFinishRows; }
void launch_rm_colfinish(const double* part, int nb, int64_t W, double* out, double* scratch, hipStream_t s);

// fused per-(row, query) pass over the graph: the coherence drop's per-wave sums and each row's null-point candidate
// R_ij = lamC A_ij (d_ij + 2 (s_i - s_j)(p_i - p_j) + (s_i - s_j)^2 |psi|^2), fp64 S1 / S2 / first argmax.
// Rows are dealt to nw waves round-robin (fixed for a lattice): cohpart[w * nq + q].  z / j / r are N x qs (device rows;
// j an API id, z = -inf where the row has no null point).
struct RmRowsArgs {
  const int32_t* col;
  const float* adj;
  const int32_t* deg;
  const float* dslot;
  const double* s;
  const double* c0;
  const double* c2;
  const double* pn2;
  const float* p;
  const int32_t* api_id;  // nullptr = identity
  int32_t width, N, qs, nq, nw;
  float lamC, z_th;
  double* cohpart;
  float* z;
  int32_t* j;
  float* r;
};
int rm_row_waves(int64_t N);
void launch_rm_rows(const RmRowsArgs& a, hipStream_t s);

// zt[q * N + a] = z[dev(a) * qs + q]: per query, API row order (inv = API row -> device row, nullptr = identity)
void launch_rm_transpose(const float* z, const int32_t* inv, int32_t N, int32_t qs, int32_t nq, float* zt, hipStream_t s);
// total[q] = number of null points of query q
void launch_rm_null_count(const float* zt, int32_t N, int32_t nq, int32_t* total, hipStream_t s);
// per query the kept records at out + off[q]: the cap highest z (ties in API row order) in that order when sel[q] != 0
// (total > cap, cap <= kRmSelectMax), else every null point in API row order
struct RmSelectArgs {
  const float* zt;
  const int32_t* j;     // N x qs
  const float* r;       // N x qs
  const int32_t* inv;   // nullptr = identity
  const int64_t* off;   // [nq]
  const int32_t* sel;   // [nq]
  int32_t N, qs, nq, cap;
  int32_t* oi;
  int32_t* oj;
  float* oz;
  float* orr;
};
void launch_rm_null_select(const RmSelectArgs& a, hipStream_t s);

}  // namespace osc

// ---- receipts under per-query chain priors: receipt_prior_kernels.hip -----------------------
namespace osc {

// The moments of the Green's columns: per 32-column slab of the slab-major panel and per row part (gates_many_plan.hpp),
//   part[(sl * parts + p) * 32 + c][w] = sum over the part's rows of G[i, 32 (slab0 + sl) + c] V[i, w],
//   V_i = [X'_i - Y_i | B_i X'_i | x'_i | B_i (x'_i - 1)]  (wout = 2 ld + 2 columns; zeros at and past D in both blocks)
// on v_mfma_f32_32x32x2_f32, the rows of a part in order.  launch_rp_moments_finish adds the parts in fp64 in part order into
// mom[32 (slab0 + sl) + c][w].  A column's moments depend on its own column and N alone.
struct RpMomArgs {
  const float* G;   // slab-major panel
  const float* X;   // the shifted basis, N x ld
  const float* x4;
  const float* Y;
  const float* B;
  int32_t N, D, ld, parts, part_rows, slab0, nslab, wout;
  float* part;
};
void launch_rp_moments(const RpMomArgs& a, hipStream_t s);
void launch_rp_moments_finish(const float* part, int32_t parts, int32_t slab0, int32_t nslab, int32_t wout, double* mom,
                              hipStream_t s);

// Gamma_A = G^T G and Gamma_B = G^T diag(B) G on the m columns of every chain system of a pass: per run of `per` consecutive
// parts, part[(grp * 2 + k) * msq + g_at[sys] + b * m + c] in fp64 (a part's rows in order, then the parts in order)
struct RpGramArgs {
  const float* G;
  const float* B;
  const int32_t* sys_m;
  const int32_t* sys_col_at;
  const int32_t* sys_cols;
  const int64_t* g_at;   // [n_sys]
  int32_t N, n_sys, parts, part_rows, groups, per;
  int64_t msq;
  double* part;
};
void launch_rp_gram(const RpGramArgs& a, hipStream_t s);

// One workgroup per query: deltaH under M_q = M' - S K S^T by the identity of section 12.3 and, in full detail, the anchor
// and query sums.  base = [h0', h2', a0, a2, b0, b2, lamG, lamQ | h1' (D) | a1 (D) | b1 (D)] of the shifted slot and the call.
struct RpScalArgs {
  BpArgs b;              // TV, psi, q_sys, sys_*, tv_at, e, H (launch_bp_scalars has run), G, N, D, ld, nq
  const float* U;        // the state, N x ld
  const float* X;        // X'
  const float* x4;
  const float* psi0;     // [ld]
  const int32_t* sys_rows;  // device row per (system, local node), at sys_col_at
  const int32_t* k_at;   // [n_sys + 1] the systems' K entries
  const int32_t* kr;
  const int32_t* kc;
  const float* kw;
  float lamP;
  const double* base;
  int32_t full;
  const double* mom;     // [qc][wout]
  int32_t wout;
  const double* gram_part;
  const int64_t* g_at;
  int32_t groups;
  int64_t msq;
  const float* res_in;   // [nq] k_cp_tv's bound and iterations
  const int32_t* iters_in;
  double* J;             // [nq][64][64]
  double* Z;
  double* scal;          // [nq][4]: deltaH, anchor sum, query sum
  float* res_out;
  int32_t* iters_out;
};
void launch_rp_scalars(const RpScalArgs& a, hipStream_t s);

// The fused row pass: k_bp_rows_coh's arithmetic per (row, query) and, per graph edge in slot order,
//   R_ij = lamC A_ij [d_ij + 2 ds dp + ds^2 n2 + 2 sum_b dgamma_b (dkappa_b + ds e_b) + nu_i + nu_j - 2 gamma_j . (H gamma_i)]
// with fp64 S1 / S2 / first argmax and k_rm_rows' dense-row rule.  coh is N x qs doubles; z / j / r as RmRowsArgs'.
struct RpRowsArgs {
  BpArgs b;              // nu written (launch_bp_rows_self has run)
  const float* dslot;    // the shifted basis's |P'_i - P'_j|^2 per ELL slot
  const int32_t* api_id;
  float z_th;
  double* cohd;
  float* z;
  int32_t* j;
  float* r;
};
void launch_rp_rows(const RpRowsArgs& a, hipStream_t s);
// part[b * nq + q] = sum of coh[r * qs + q] over the rows r = b, b + nb, ... in row order
void launch_rp_colsum(const double* coh, int32_t N, int32_t qs, int32_t nq, int32_t nb, double* part, hipStream_t s);

}  // namespace osc

// ---- multi-query chain receipts: chain_many_kernels.hip -------------------------------------
#include "chain_many.hpp"

namespace osc {

constexpr int kCmMaxBlocks = 4096;  // k_cm_edges' grid: 4 waves a workgroup, grid-stride over the units beyond it

// per (query, chain edge) unit u = (q, i, j) of a chunk, on U*(psi_q) = X + x psi_q^T with Un = U* / (sd + 1e-12):
//   R_s = lamC a_ic |Un_i - Un_c|^2 over row i's ELL slots with a_ic > 0, R_p = max(lamC, 1e-6) A_path[i][c] |Un_i - Un_c|^2
//   over its path entries [pb, pe); per row mu = sum R / N, sigma = sqrt(sum R^2 / N - mu^2) + 1e-12 in fp64, slot order;
//   z = (R_ij - mu) / sigma with R_ij = 0 when j is not an entry; term = 0.5 lamC a_ij (|Yn_i - Yn_j|^2 - |Un_i - Un_j|^2)
struct CmEdgesArgs {
  const float* X;        // N x ld
  const float* x4;       // N x 4, column 0 = x
  const float* Y;        // N x ld
  const float* sqrt_deg;
  const int32_t* col;    // ELL, device rows
  const float* adj;      // capped adjacency
  const int32_t* deg;
  const float* psi;      // nq x ld, pad columns zero
  const host::ChainManyUnit* units;
  const int32_t* pcol;   // the chunk's path entries, device rows
  const float* pa;       // A_path
  int32_t width, N, D, ld;
  int64_t n_units;
  float lamC;
  float* z_struct;       // [n_units] each
  float* z_path;
  float* r_struct;
  float* r_path;
  double* term;
  double* zmax;          // max(z_struct, z_path) in fp64
  // per-query chain priors (launch_cm_edges_prior): every gathered row r of query q becomes
  // X'_r + x'_r psi_q + sum_b G[r, col_b] TV_q[b, :] over the m nodes of the query's chain system
  const float* G;            // the pass's Green's columns, slab-major (gates_many_plan.hpp)
  const int32_t* q_sys;      // [nq] the query's system
  const int32_t* sys_m;      // per system: its nodes,
  const int32_t* sys_col_at; // where their panel columns start in sys_cols
  const int32_t* sys_cols;
  const float* TV;           // query q's T_q V_q: m x ld floats at tv_at[q], pad columns zero
  const int64_t* tv_at;
};
int cm_edge_blocks(int64_t n_units);
void launch_cm_edges(const CmEdgesArgs& a, hipStream_t s);
void launch_cm_edges_prior(const CmEdgesArgs& a, hipStream_t s);

// T = (I - K Ghat)^-1 K per chain system of a pass, one 64-thread workgroup each: Ghat gathered from the panel, K = lamP W_path
// scattered from the system's entries, Gauss-Jordan with partial pivoting in fp64 in LDS (two 64 x 64 arrays)
struct CpSystemsArgs {
  const float* G;
  const int32_t* m;       // [n_sys]
  const int32_t* col_at;  // [n_sys]
  const int32_t* k_at;    // [n_sys + 1]
  const int64_t* t_at;    // [n_sys]
  const int32_t* cols;    // panel column per (system, local node)
  const int32_t* rows;    // device row per (system, local node)
  const int32_t* kr;
  const int32_t* kc;
  const float* kw;
  int32_t N, n_sys;
  float lamP;
  double* T;
};
void launch_cp_systems(const CpSystemsArgs& a, hipStream_t s);

// per query of the pass: TV_q = T_q V_q with V_q the chain rows of X' + x' psi_q^T (fp64 sums, stored fp32), the bound
// base[q] + max_c sum_e res_e |TV_q[e, c]| and the most iterations of its columns
struct CpTvArgs {
  const float* X;      // the shifted basis, N x ld
  const float* x4;
  const float* psi;    // nq x ld
  const double* T;
  const int32_t* q_sys;
  const int32_t* m;
  const int32_t* col_at;
  const int64_t* t_at;
  const int32_t* cols;
  const int32_t* rows;
  const float* col_res;     // [qc] |r_e| of the panel's columns
  const int32_t* col_iters;
  const float* base;        // [nq] the basis's own residual for the query
  const int64_t* tv_at;
  int32_t nq, D, ld;
  float* TV;
  float* prior_res;         // [nq]
  int32_t* prior_iters;     // [nq]
};
void launch_cp_tv(const CpTvArgs& a, hipStream_t s);

// X *= f in place (the shifted basis's X' = lamG / (lamG + lamP) X''); part[b] = the block's max |X f| over the real columns
int cp_scale_blocks(int64_t N);
void launch_cp_scale_max(float* X, int32_t N, int32_t D, int32_t ld, float f, float* part, hipStream_t s);

// per query of the chunk over its units [eoff[q], eoff[q + 1]): the gain, the verdict, the weakest link
struct CmFinishArgs {
  const int32_t* eoff;   // [nq + 1]
  const double* term;
  const double* zmax;
  int32_t nq;
  float z_th;
  double* gain;
  int32_t* verdict;
  int32_t* weak_k;       // -1: no edge's max(z) exceeds -1
  float* weak_z;
};
void launch_cm_finish(const CmFinishArgs& a, hipStream_t s);

}  // namespace osc

// The CG scalars of iterations 1 and 2 of an anchor start under uniform gates, from the lattice's cached Gram sums: plain
// C++, free of every HIP type (the style of host_logic.hpp), used by k_anchor_gram_scalars (cg_kernels.hip) and by the host
// sweep tests/host_logic/sweep_anchor_gram.cpp.
//
// On that route (no chain prior, x0 = Y, one gate value b) every vector of the first two iterations is, per column c, a
// combination with column-independent coefficients of the seven N-vectors
//     psi_c 1, psi_c s, psi_c s2, Y_c, (W Y)_c, (W W Y)_c, (W W W Y)_c          (s = W 1, s2 = W s)
// so r0.z0, p1.Ap1, |r1|^2, p2.Ap2 and |r2|^2 are quadratic forms in their 7 x 7 Gram matrix.  That matrix depends on the
// anchors and the graph alone (the lifetime of L::W3s); psi, the gate value, the lams and dt enter through the coefficients.
// |r2|^2 is about 1e6 times smaller than the terms it is formed from: sums and forms are float64 throughout, and alpha /
// beta / the residuals are rounded to float exactly where k_reduce_alpha / k_reduce_beta round them.
// At the end of the file: poly4_coeffs, the coefficients of x4 itself in the two families W^k Y and psi W^k 1, for the solve that
// ends in iteration 4 (k_settle_poly; swept by tests/host_logic/sweep_poly4.cpp).
//
// Storage of the sums (L::gram, read back by osc_anchor_gram_read): kGramPerColumn arrays of ld doubles, then kGramLattice
// doubles.  Array q < 10: <W^j Y, W^k Y> for j <= k in the order (0,0) (0,1) (0,2) (0,3) (1,1) (1,2) (1,3) (2,2) (2,3) (3,3);
// array 10 + 4 a + j: <a, W^j Y> for a in (1, s, s2); the lattice's six: <a, b> in the order (1,1) (1,s) (1,s2) (s,s) (s,s2)
// (s2,s2).
#pragma once
#include <cmath>
#include <cstddef>

#if defined(__HIPCC__)
#define OSC_GRAM_HD __host__ __device__ inline
#else
#define OSC_GRAM_HD inline
#endif

namespace osc {
namespace gram {

constexpr int kGramPerColumn = 22;  // 10 <W^j Y, W^k Y> + 12 <a, W^j Y>
constexpr int kGramLattice = 6;     // <a, b>
constexpr int kBasis = 7;           // psi 1, psi s, psi s2, Y, W Y, W W Y, W W W Y

// index of <W^j Y, W^k Y>, j <= k <= 3, among the per-column arrays
OSC_GRAM_HD int yy_index(int j, int k) { return j * 4 - j * (j - 1) / 2 + (k - j); }
// index of <a, W^j Y>, a in 0..2
OSC_GRAM_HD int ay_index(int a, int j) { return 10 + 4 * a + j; }
// index of <a, b>, a <= b <= 2, among the lattice's sums
OSC_GRAM_HD int lat_index(int a, int b) { return a * 3 - a * (a - 1) / 2 + (b - a); }

// One column's 7 x 7 Gram matrix from the stored sums: col[q * stride] is array q's entry of this column.
OSC_GRAM_HD void fill(double (&G)[kBasis][kBasis], const double* col, size_t stride, const double* lat, double psi) {
  for (int a = 0; a < 3; ++a)
    for (int b = a; b < 3; ++b) G[a][b] = G[b][a] = psi * psi * lat[lat_index(a, b)];
  for (int a = 0; a < 3; ++a)
    for (int j = 0; j < 4; ++j) G[a][3 + j] = G[3 + j][a] = psi * col[(size_t)ay_index(a, j) * stride];
  for (int j = 0; j < 4; ++j)
    for (int k = j; k < 4; ++k) G[3 + j][3 + k] = G[3 + k][3 + j] = col[(size_t)yy_index(j, k) * stride];
}

// the solve's scalars as the kernels form them in float (blk_init_row), converted to double
struct Op {
  double m;   // 1 / (Md + 1e-12)
  double cs;  // the operator's diagonal
  double cW;
  double qb;  // rbB b
  double u;   // rbU + rbY - cs
};

struct Scalars {
  float alpha1 = 0.f, alpha2 = 0.f, beta1 = 0.f, beta2 = 0.f;
  float res1 = 0.f, res2 = 0.f;  // |r1|, |r2| of this column
  double rz2 = 0.0;              // r2 . z2: what iteration 3's alpha and beta divide
  bool usable = false;
};

OSC_GRAM_HD double form(const double (&G)[kBasis][kBasis], const double (&v)[kBasis], const double (&w)[kBasis]) {
  double t = 0.0;
  for (int a = 0; a < kBasis; ++a) {
    double row = 0.0;
    for (int b = 0; b < kBasis; ++b) row += G[a][b] * w[b];
    t += v[a] * row;
  }
  return t;
}
// out = A v = cs v - cW W v; W shifts psi 1 -> psi s -> psi s2 and Y -> W Y -> W W Y -> W W W Y (no vector of the two
// iterations has a component W would shift out of the basis)
OSC_GRAM_HD void apply(const Op& o, const double (&v)[kBasis], double (&out)[kBasis]) {
  double wv[kBasis] = {0.0, v[0], v[1], 0.0, v[3], v[4], v[5]};
  for (int a = 0; a < kBasis; ++a) out[a] = o.cs * v[a] - o.cW * wv[a];
}
OSC_GRAM_HD bool finite(double x) { return x - x == 0.0; }

// Iterations 1 and 2 (solver.py:19-36 as the reduce kernels spell it, + 1e-18 and float roundings included).
// usable: every value is finite, no form that must be non-negative came out negative, and the column has a residual at all
// (a zero column has no scale its |r2|^2 could be judged against: it takes the summed route).
OSC_GRAM_HD Scalars two_steps(const double (&G)[kBasis][kBasis], const Op& o) {
  Scalars s;
  double r0[kBasis] = {o.qb, 0.0, 0.0, o.u, o.cW, 0.0, 0.0};
  double p1[kBasis], q1[kBasis], r1[kBasis], p2[kBasis], ap2[kBasis], r2[kBasis];
  for (int a = 0; a < kBasis; ++a) p1[a] = o.m * r0[a];
  apply(o, p1, q1);
  const double rr0 = form(G, r0, r0), rz0 = o.m * rr0;
  const double pq1 = form(G, p1, q1);
  s.alpha1 = (float)(rz0 / (pq1 + 1e-18));
  for (int a = 0; a < kBasis; ++a) r1[a] = r0[a] - (double)s.alpha1 * q1[a];
  const double rr1 = form(G, r1, r1), rz1 = o.m * rr1;
  s.res1 = (float)sqrt(rr1);
  s.beta1 = (float)(rz1 / (rz0 + 1e-18));
  for (int a = 0; a < kBasis; ++a) p2[a] = o.m * r1[a] + (double)s.beta1 * p1[a];
  apply(o, p2, ap2);
  const double pq2 = form(G, p2, ap2);
  s.alpha2 = (float)(rz1 / (pq2 + 1e-18));
  for (int a = 0; a < kBasis; ++a) r2[a] = r1[a] - (double)s.alpha2 * ap2[a];
  const double rr2 = form(G, r2, r2);
  s.res2 = (float)sqrt(rr2);
  s.rz2 = o.m * rr2;
  s.beta2 = (float)(s.rz2 / (rz1 + 1e-18));
  s.usable = finite(rr0) && finite(pq1) && finite(rr1) && finite(pq2) && finite(rr2) && finite((double)s.alpha1) &&
             finite((double)s.alpha2) && finite((double)s.beta1) && finite((double)s.beta2) && rr0 > 0.0 && pq1 >= 0.0 &&
             rr1 >= 0.0 && pq2 >= 0.0 && rr2 >= 0.0;
  return s;
}

// ---- the third step ------------------------------------------------------------------------------------------------------
// A p3 adds two vectors to the seven: psi_c s3 (s3 = W s2) and (W W W W Y)_c.  p3 . A p3 and |r3|^2 are then quadratic forms in
// the 9 x 9 Gram matrix of
//     psi 1, psi s, psi s2, psi s3, Y, W Y, W W Y, W W W Y, W W W W Y
// (the a-vectors first, as above, so that the seven-vector forms are sums of the same terms in the same order).  The sums that
// matrix needs beyond the seven vectors' are a second block (L::gram3, read back by osc_anchor_gram3_read): kGram3PerColumn
// arrays of ld doubles, then kGram3Lattice doubles.  Array j < 5: <W^j Y, W^4 Y>; array 5 + a: <a, W^4 Y> for a in (1, s, s2,
// s3); array 9 + j: <s3, W^j Y>, j < 4; the lattice's four: <a, s3> for a in (1, s, s2, s3).  Every one is summed directly from
// the stored float arrays (no <W^j Y, W^4 Y> = <W^(j+1) Y, W^3 Y>).
constexpr int kGram3PerColumn = 13;  // 5 <W^j Y, W^4 Y> + 4 <a, W^4 Y> + 4 <s3, W^j Y>
constexpr int kGram3Lattice = 4;     // <a, s3>
constexpr int kBasis3 = 9;

OSC_GRAM_HD int y4_index(int j) { return j; }        // <W^j Y, W^4 Y>, j <= 4
OSC_GRAM_HD int a4_index(int a) { return 5 + a; }    // <a, W^4 Y>, a in 0..3
OSC_GRAM_HD int s3y_index(int j) { return 9 + j; }   // <s3, W^j Y>, j <= 3
OSC_GRAM_HD int lat3_index(int a) { return a; }      // <a, s3>, a in 0..3

// One column's 9 x 9 Gram matrix: the seven vectors' part from the first block (fill's entries, moved to the new order), the
// rest from the second (col3[q * stride3], lat3).
OSC_GRAM_HD void fill3(double (&G)[kBasis3][kBasis3], const double* col, size_t stride, const double* lat, const double* col3,
                       size_t stride3, const double* lat3, double psi) {
  for (int a = 0; a < 3; ++a)
    for (int b = a; b < 3; ++b) G[a][b] = G[b][a] = psi * psi * lat[lat_index(a, b)];
  for (int a = 0; a < 4; ++a) G[a][3] = G[3][a] = psi * psi * lat3[lat3_index(a)];
  for (int a = 0; a < 3; ++a)
    for (int j = 0; j < 4; ++j) G[a][4 + j] = G[4 + j][a] = psi * col[(size_t)ay_index(a, j) * stride];
  for (int j = 0; j < 4; ++j) G[3][4 + j] = G[4 + j][3] = psi * col3[(size_t)s3y_index(j) * stride3];
  for (int a = 0; a < 4; ++a) G[a][8] = G[8][a] = psi * col3[(size_t)a4_index(a) * stride3];
  for (int j = 0; j < 4; ++j)
    for (int k = j; k < 4; ++k) G[4 + j][4 + k] = G[4 + k][4 + j] = col[(size_t)yy_index(j, k) * stride];
  for (int j = 0; j < 5; ++j) G[4 + j][8] = G[8][4 + j] = col3[(size_t)y4_index(j) * stride3];
}

struct Scalars3 {
  Scalars two;       // iterations 1 and 2: two_steps()' values to the bit (the same terms in the same order, the rest zeros)
  float alpha3 = 0.f, beta3 = 0.f;
  float res3 = 0.f;  // |r3| of this column
  double rz3 = 0.0;  // r3 . z3: what iteration 4's alpha and beta divide
  bool usable3 = false;
};

OSC_GRAM_HD double form3(const double (&G)[kBasis3][kBasis3], const double (&v)[kBasis3], const double (&w)[kBasis3]) {
  double t = 0.0;
  for (int a = 0; a < kBasis3; ++a) {
    double row = 0.0;
    for (int b = 0; b < kBasis3; ++b) row += G[a][b] * w[b];
    t += v[a] * row;
  }
  return t;
}
// out = A v; W shifts psi 1 -> psi s -> psi s2 -> psi s3 and Y -> ... -> W W W W Y (p1, p2 and p3 have no psi s3 and no
// W W W W Y component)
OSC_GRAM_HD void apply3(const Op& o, const double (&v)[kBasis3], double (&out)[kBasis3]) {
  double wv[kBasis3] = {0.0, v[0], v[1], v[2], 0.0, v[4], v[5], v[6], v[7]};
  for (int a = 0; a < kBasis3; ++a) out[a] = o.cs * v[a] - o.cW * wv[a];
}

// two_steps()' recurrence one iteration further: p3 = z2 + beta2 p2 (k_update_p), alpha3 = r2 . z2 / (p3 . A p3 + 1e-18)
// (k_reduce_alpha), r3 = r2 - alpha3 A p3 (k_update_xr), res3, beta3 and r3 . z3 as k_reduce_beta rounds them.  usable3: two's
// rules, and the same for the third iteration's values.
OSC_GRAM_HD Scalars3 three_steps(const double (&G)[kBasis3][kBasis3], const Op& o) {
  Scalars3 t;
  Scalars& s = t.two;
  double r0[kBasis3] = {o.qb, 0.0, 0.0, 0.0, o.u, o.cW, 0.0, 0.0, 0.0};
  double p1[kBasis3], q1[kBasis3], r1[kBasis3], p2[kBasis3], ap2[kBasis3], r2[kBasis3], p3[kBasis3], ap3[kBasis3], r3[kBasis3];
  for (int a = 0; a < kBasis3; ++a) p1[a] = o.m * r0[a];
  apply3(o, p1, q1);
  const double rr0 = form3(G, r0, r0), rz0 = o.m * rr0;
  const double pq1 = form3(G, p1, q1);
  s.alpha1 = (float)(rz0 / (pq1 + 1e-18));
  for (int a = 0; a < kBasis3; ++a) r1[a] = r0[a] - (double)s.alpha1 * q1[a];
  const double rr1 = form3(G, r1, r1), rz1 = o.m * rr1;
  s.res1 = (float)sqrt(rr1);
  s.beta1 = (float)(rz1 / (rz0 + 1e-18));
  for (int a = 0; a < kBasis3; ++a) p2[a] = o.m * r1[a] + (double)s.beta1 * p1[a];
  apply3(o, p2, ap2);
  const double pq2 = form3(G, p2, ap2);
  s.alpha2 = (float)(rz1 / (pq2 + 1e-18));
  for (int a = 0; a < kBasis3; ++a) r2[a] = r1[a] - (double)s.alpha2 * ap2[a];
  const double rr2 = form3(G, r2, r2);
  s.res2 = (float)sqrt(rr2);
  s.rz2 = o.m * rr2;
  s.beta2 = (float)(s.rz2 / (rz1 + 1e-18));
  s.usable = finite(rr0) && finite(pq1) && finite(rr1) && finite(pq2) && finite(rr2) && finite((double)s.alpha1) &&
             finite((double)s.alpha2) && finite((double)s.beta1) && finite((double)s.beta2) && rr0 > 0.0 && pq1 >= 0.0 &&
             rr1 >= 0.0 && pq2 >= 0.0 && rr2 >= 0.0;
  for (int a = 0; a < kBasis3; ++a) p3[a] = o.m * r2[a] + (double)s.beta2 * p2[a];
  apply3(o, p3, ap3);
  const double pq3 = form3(G, p3, ap3);
  t.alpha3 = (float)(s.rz2 / (pq3 + 1e-18));
  for (int a = 0; a < kBasis3; ++a) r3[a] = r2[a] - (double)t.alpha3 * ap3[a];
  const double rr3 = form3(G, r3, r3);
  t.res3 = (float)sqrt(rr3);
  t.rz3 = o.m * rr3;
  t.beta3 = (float)(t.rz3 / (s.rz2 + 1e-18));
  t.usable3 = s.usable && finite(pq3) && finite(rr3) && finite((double)t.alpha3) && finite((double)t.beta3) && pq3 >= 0.0 && rr3 >= 0.0;
  return t;
}

// ---- the fourth step's scalars ---------------------------------------------------------------------------------------------
// A p4 adds psi_c s4 (s4 = W s3) and (W^5 Y)_c: p4 . A p4 and |r4|^2 are quadratic forms in the 11 x 11 Gram matrix of
//     psi 1, psi s, psi s2, psi s3, psi s4, Y, W Y, W W Y, W W W Y, W^4 Y, W^5 Y
// (the a-vectors first again: with finite sums the nine-vector forms are sums of the same terms in the same order, the rest
// zeros).  Only scalars
// are taken from this level -- alpha4 and |r4| of a solve that ends in iteration 4 (host_logic.hpp: anchor_gram4_route); no
// vector of iteration 4 is formed from them but x4 = x3 + alpha4 p4.  The sums beyond the nine vectors' are a third block
// (L::gram4, read back by osc_anchor_gram4_read): kGram4PerColumn arrays of ld doubles, then kGram4Lattice doubles.  Array j < 6:
// <W^j Y, W^5 Y>; array 6 + a: <a, W^5 Y> for a in (1, s, s2, s3, s4); array 11 + j: <s4, W^j Y>, j < 5; the lattice's five: <a, s4>
// for a in (1, s, s2, s3, s4).  Every one is summed directly from the stored float arrays.
constexpr int kGram4PerColumn = 16;  // 6 <W^j Y, W^5 Y> + 5 <a, W^5 Y> + 5 <s4, W^j Y>
constexpr int kGram4Lattice = 5;     // <a, s4>
constexpr int kBasis4 = 11;

OSC_GRAM_HD int y5_index(int j) { return j; }        // <W^j Y, W^5 Y>, j <= 5
OSC_GRAM_HD int a5_index(int a) { return 6 + a; }    // <a, W^5 Y>, a in 0..4
OSC_GRAM_HD int s4y_index(int j) { return 11 + j; }  // <s4, W^j Y>, j <= 4
OSC_GRAM_HD int lat4_index(int a) { return a; }      // <a, s4>, a in 0..4

// One column's 11 x 11 Gram matrix: the nine vectors' part from the first two blocks (fill3's entries, moved to the new order),
// the rest from the third (col4[q * stride4], lat4).
OSC_GRAM_HD void fill4(double (&G)[kBasis4][kBasis4], const double* col, size_t stride, const double* lat, const double* col3,
                       size_t stride3, const double* lat3, const double* col4, size_t stride4, const double* lat4, double psi) {
  for (int a = 0; a < 3; ++a)
    for (int b = a; b < 3; ++b) G[a][b] = G[b][a] = psi * psi * lat[lat_index(a, b)];
  for (int a = 0; a < 4; ++a) G[a][3] = G[3][a] = psi * psi * lat3[lat3_index(a)];
  for (int a = 0; a < 5; ++a) G[a][4] = G[4][a] = psi * psi * lat4[lat4_index(a)];
  for (int a = 0; a < 3; ++a)
    for (int j = 0; j < 4; ++j) G[a][5 + j] = G[5 + j][a] = psi * col[(size_t)ay_index(a, j) * stride];
  for (int j = 0; j < 4; ++j) G[3][5 + j] = G[5 + j][3] = psi * col3[(size_t)s3y_index(j) * stride3];
  for (int a = 0; a < 4; ++a) G[a][9] = G[9][a] = psi * col3[(size_t)a4_index(a) * stride3];
  for (int j = 0; j < 5; ++j) G[4][5 + j] = G[5 + j][4] = psi * col4[(size_t)s4y_index(j) * stride4];
  for (int a = 0; a < 5; ++a) G[a][10] = G[10][a] = psi * col4[(size_t)a5_index(a) * stride4];
  for (int j = 0; j < 4; ++j)
    for (int k = j; k < 4; ++k) G[5 + j][5 + k] = G[5 + k][5 + j] = col[(size_t)yy_index(j, k) * stride];
  for (int j = 0; j < 5; ++j) G[5 + j][9] = G[9][5 + j] = col3[(size_t)y4_index(j) * stride3];
  for (int j = 0; j < 6; ++j) G[5 + j][10] = G[10][5 + j] = col4[(size_t)y5_index(j) * stride4];
}

struct Scalars4 {
  Scalars3 three;    // iterations 1 to 3: three_steps()' values to the bit
  float alpha4 = 0.f, beta4 = 0.f;
  float res4 = 0.f;  // |r4| of this column
  double rz4 = 0.0;  // r4 . z4
  bool usable4 = false;
  double alpha_d[4] = {0.0, 0.0, 0.0, 0.0};  // alpha1 .. alpha4 and beta1 .. beta3 before they are rounded to float (poly4_coeffs)
  double beta_d[3] = {0.0, 0.0, 0.0};
};

OSC_GRAM_HD double form4(const double (&G)[kBasis4][kBasis4], const double (&v)[kBasis4], const double (&w)[kBasis4]) {
  double t = 0.0;
  for (int a = 0; a < kBasis4; ++a) {
    double row = 0.0;
    for (int b = 0; b < kBasis4; ++b) row += G[a][b] * w[b];
    t += v[a] * row;
  }
  return t;
}
// out = A v; W shifts psi 1 -> ... -> psi s4 and Y -> ... -> W^5 Y (p1 .. p4 have no psi s4 and no W^5 Y component)
OSC_GRAM_HD void apply4(const Op& o, const double (&v)[kBasis4], double (&out)[kBasis4]) {
  double wv[kBasis4] = {0.0, v[0], v[1], v[2], v[3], 0.0, v[5], v[6], v[7], v[8], v[9]};
  for (int a = 0; a < kBasis4; ++a) out[a] = o.cs * v[a] - o.cW * wv[a];
}

// three_steps()' recurrence one iteration further: p4 = z3 + beta3 p3, alpha4 = r3 . z3 / (p4 . A p4 + 1e-18), r4 = r3 - alpha4 A
// p4, res4, beta4 and r4 . z4 as k_reduce_alpha / k_reduce_beta round them.  usable4: three's rules, and the same for the fourth
// iteration's values.
OSC_GRAM_HD Scalars4 four_steps(const double (&G)[kBasis4][kBasis4], const Op& o) {
  Scalars4 f;
  Scalars3& t = f.three;
  Scalars& s = t.two;
  double r0[kBasis4] = {o.qb, 0.0, 0.0, 0.0, 0.0, o.u, o.cW, 0.0, 0.0, 0.0, 0.0};
  double p1[kBasis4], q1[kBasis4], r1[kBasis4], p2[kBasis4], ap2[kBasis4], r2[kBasis4], p3[kBasis4], ap3[kBasis4], r3[kBasis4];
  double p4[kBasis4], ap4[kBasis4], r4[kBasis4];
  for (int a = 0; a < kBasis4; ++a) p1[a] = o.m * r0[a];
  apply4(o, p1, q1);
  const double rr0 = form4(G, r0, r0), rz0 = o.m * rr0;
  const double pq1 = form4(G, p1, q1);
  f.alpha_d[0] = rz0 / (pq1 + 1e-18);
  s.alpha1 = (float)f.alpha_d[0];
  for (int a = 0; a < kBasis4; ++a) r1[a] = r0[a] - (double)s.alpha1 * q1[a];
  const double rr1 = form4(G, r1, r1), rz1 = o.m * rr1;
  s.res1 = (float)sqrt(rr1);
  f.beta_d[0] = rz1 / (rz0 + 1e-18);
  s.beta1 = (float)f.beta_d[0];
  for (int a = 0; a < kBasis4; ++a) p2[a] = o.m * r1[a] + (double)s.beta1 * p1[a];
  apply4(o, p2, ap2);
  const double pq2 = form4(G, p2, ap2);
  f.alpha_d[1] = rz1 / (pq2 + 1e-18);
  s.alpha2 = (float)f.alpha_d[1];
  for (int a = 0; a < kBasis4; ++a) r2[a] = r1[a] - (double)s.alpha2 * ap2[a];
  const double rr2 = form4(G, r2, r2);
  s.res2 = (float)sqrt(rr2);
  s.rz2 = o.m * rr2;
  f.beta_d[1] = s.rz2 / (rz1 + 1e-18);
  s.beta2 = (float)f.beta_d[1];
  s.usable = finite(rr0) && finite(pq1) && finite(rr1) && finite(pq2) && finite(rr2) && finite((double)s.alpha1) &&
             finite((double)s.alpha2) && finite((double)s.beta1) && finite((double)s.beta2) && rr0 > 0.0 && pq1 >= 0.0 &&
             rr1 >= 0.0 && pq2 >= 0.0 && rr2 >= 0.0;
  for (int a = 0; a < kBasis4; ++a) p3[a] = o.m * r2[a] + (double)s.beta2 * p2[a];
  apply4(o, p3, ap3);
  const double pq3 = form4(G, p3, ap3);
  f.alpha_d[2] = s.rz2 / (pq3 + 1e-18);
  t.alpha3 = (float)f.alpha_d[2];
  for (int a = 0; a < kBasis4; ++a) r3[a] = r2[a] - (double)t.alpha3 * ap3[a];
  const double rr3 = form4(G, r3, r3);
  t.res3 = (float)sqrt(rr3);
  t.rz3 = o.m * rr3;
  f.beta_d[2] = t.rz3 / (s.rz2 + 1e-18);
  t.beta3 = (float)f.beta_d[2];
  t.usable3 = s.usable && finite(pq3) && finite(rr3) && finite((double)t.alpha3) && finite((double)t.beta3) && pq3 >= 0.0 && rr3 >= 0.0;
  for (int a = 0; a < kBasis4; ++a) p4[a] = o.m * r3[a] + (double)t.beta3 * p3[a];
  apply4(o, p4, ap4);
  const double pq4 = form4(G, p4, ap4);
  f.alpha_d[3] = t.rz3 / (pq4 + 1e-18);
  f.alpha4 = (float)f.alpha_d[3];
  for (int a = 0; a < kBasis4; ++a) r4[a] = r3[a] - (double)f.alpha4 * ap4[a];
  const double rr4 = form4(G, r4, r4);
  f.res4 = (float)sqrt(rr4);
  f.rz4 = o.m * rr4;
  f.beta4 = (float)(f.rz4 / (t.rz3 + 1e-18));
  f.usable4 = t.usable3 && finite(pq4) && finite(rr4) && finite((double)f.alpha4) && finite((double)f.beta4) && pq4 >= 0.0 && rr4 >= 0.0;
  return f;
}

// ---- the polynomial last form ------------------------------------------------------------------------------------------------
// Every vector of the solve lies, per column, in the span of W^k Y and psi s_k (s_0 = 1, s_k = W s_{k-1}), and A shifts either
// family by one: A v_k = cs v_k - cW v_{k+1}.  So a solve that ends in iteration 4 has
//     x4[i] = sum_{k <= 4} a[k] (W^k Y)[i] + sum_{k <= 3} q[k] s_k[i]
// with nine coefficients a column, which follow from the CG recurrences run on coefficient vectors (x0 = Y, r0 = qb psi 1 + u Y
// + cW W Y, z = m r) with the solve's alpha1 .. alpha4 and beta1 .. beta3.  Only x is formed from them, and at A = cs (I - (cW /
// cs) W) with cW / cs well below 1 they are all of one sign and fall from power to power: nothing cancels (unlike the small
// vectors A p3, r3, p4, which do -- see DESIGN.md section 10 (f)).  psi is multiplied into q.
constexpr int kPolyY = 5;  // a[0..4]
constexpr int kPolyS = 4;  // q[0..3]
constexpr int kPolyCoeffs = kPolyY + kPolyS;
struct Poly4 {
  double a[kPolyY];
  double q[kPolyS];
};
OSC_GRAM_HD Poly4 poly4_coeffs(const Op& o, const double (&alpha)[4], const double (&beta)[3], double psi) {
  // (one slot more than x4 needs in either family: A p3's shift lands there and nothing reads it)
  double xy[kPolyY + 1] = {1.0, 0.0, 0.0, 0.0, 0.0, 0.0}, xs[kPolyS + 1] = {0.0, 0.0, 0.0, 0.0, 0.0};
  double ry[kPolyY + 1] = {o.u, o.cW, 0.0, 0.0, 0.0, 0.0}, rs[kPolyS + 1] = {o.qb, 0.0, 0.0, 0.0, 0.0};
  double py[kPolyY + 1], ps[kPolyS + 1];
  for (int k = 0; k <= kPolyY; ++k) py[k] = o.m * ry[k];
  for (int k = 0; k <= kPolyS; ++k) ps[k] = o.m * rs[k];
  for (int it = 1; it <= 4; ++it) {
    const double al = alpha[it - 1];
    for (int k = 0; k <= kPolyY; ++k) xy[k] += al * py[k];
    for (int k = 0; k <= kPolyS; ++k) xs[k] += al * ps[k];
    if (it == 4) break;
    const double be = beta[it - 1];
    for (int k = kPolyY; k >= 0; --k) {  // r -= alpha A p; p = m r + beta p (descending: p[k - 1] is still the old one)
      ry[k] -= al * (o.cs * py[k] - (k > 0 ? o.cW * py[k - 1] : 0.0));
      py[k] = o.m * ry[k] + be * py[k];
    }
    for (int k = kPolyS; k >= 0; --k) {
      rs[k] -= al * (o.cs * ps[k] - (k > 0 ? o.cW * ps[k - 1] : 0.0));
      ps[k] = o.m * rs[k] + be * ps[k];
    }
  }
  Poly4 c;
  for (int k = 0; k < kPolyY; ++k) c.a[k] = xy[k];
  for (int k = 0; k < kPolyS; ++k) c.q[k] = psi * xs[k];
  return c;
}

}  // namespace gram
}  // namespace osc

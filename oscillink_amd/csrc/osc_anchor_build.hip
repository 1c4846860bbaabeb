// The builders of the anchor-start chain (derived_state.hpp: Level): each forms one level's arrays from the levels below it where
// they are not held, once per lattice and graph copy, for the solve that first takes the level's route (osc_solve.hip: CgSolve).
// Host code only; every launch is an INIT-time one and is not counted in blk_applies.  The builders stand over five pieces:
//   apply_w / apply_w_rows : W applied to a slab-major array / to a row-major one through its slab image in T
//   reserve                : a list of the handle's arrays under the memory rule of the direction ring, a denial remembered
//   gram_scratch           : a level's sums array and the scratch of the pass that forms it
//   gram_args              : the arguments the three summing passes share
#include <initializer_list>

#include "anchor_gram.hpp"
#include "osc_internal.hpp"

namespace {

using host::Level;

// W x for a slab-major x, row-major into `out`: the loop-form matvec itself with cs = 0, cW = -1 (its cs x - cW acc stores acc)
void apply_w(const AnchorBuild& c, const float* x_slab, float* out) {
  BlkArgs wa = c.ba;
  wa.X = x_slab;
  wa.OUT = out;
  wa.cs_const = wa.cs_B = 0.f;
  wa.cW = -1.f;
  wa.gate = nullptr;
  wa.gate_tol = 0.f;
  launch_apply_blocked(wa, c.grid, c.h.stream, nullptr, c.shape);
}

// ... for a row-major x, over the slab image k_rows_to_slab writes into T (free until the INIT pass fills it)
void apply_w_rows(const AnchorBuild& c, const float* x_rows, float* out) {
  rows_to_slab(c.h, x_rows, c.h.Tap.p, c.h.ld, c.c0, c.c1, c.grid);
  apply_w(c, c.h.Tap.p, out);
}

struct Want {
  DevBuf<float>& buf;
  size_t n;
};

// Every array at its size, or none: they are only taken from a quarter of the free device memory (what they hold now counts as
// free; cap_bytes >= 0: nor from more than a quarter of that), and where they do not fit or the allocation fails all of them are
// released and the denial is remembered.
bool reserve(std::initializer_list<Want> wants, bool& denied, int64_t cap_bytes = -1) {
  bool sized = true;
  for (const Want& w : wants) sized = sized && w.buf.n == w.n;
  if (sized) return true;
  int64_t need = 0, avail = device_free_bytes();
  for (const Want& w : wants) {
    need += (int64_t)w.n * 4;
    avail += (int64_t)w.buf.n * 4;
  }
  if (cap_bytes >= 0) avail = std::min(avail, cap_bytes);
  bool ok = host::anchor_ap_fits(need, avail);
  if (ok) {
    try {
      for (const Want& w : wants) w.buf.alloc(w.n);
    } catch (const HipError&) {
      (void)hipGetLastError();
      ok = false;
    }
  }
  if (!ok) {
    for (const Want& w : wants) w.buf.release();
    denied = true;
  }
  return ok;
}

// A level's sums array of n doubles, the row sums the pass leaves beside it (nullptr: none) and the pass's partials.  No memory
// rule (135 KB of sums at 768 columns); a failed allocation releases what the level would have kept and is not remembered.
bool gram_scratch(DevBuf<double>& sums, size_t n, DevBuf<float>* row_sums, size_t rows, DevBuf<double>& part) {
  try {
    if (sums.n != n) sums.alloc(n);
    if (row_sums != nullptr && row_sums->n != rows) row_sums->alloc(rows);
    part.alloc(n * OSC_GRAM_CHUNKS);
  } catch (const HipError&) {
    (void)hipGetLastError();
    sums.release();
    if (row_sums != nullptr) row_sums->release();
    return false;
  }
  return true;
}

GramArgs gram_args(const L& h, double* part, double* out) {
  GramArgs g{};
  g.Ys = h.Ys.p;
  g.WYs = h.WYs.p;
  g.WW = h.WWs.p;
  g.W3 = h.W3s.p;
  g.wsum = h.Wsum.p;
  g.wsum2 = h.Wsum2.p;
  g.part = part;
  g.out = out;
  g.N = (int32_t)h.N;
  g.ld = h.ld;
  g.c0 = h.c0;
  g.c1 = h.c1;
  return g;
}

void row_weighted_sums(L& h, const float* v, float* out) {
  launch_row_weighted_sums(h.ell_col.p, h.ell_w.p, h.deg.p, h.width, (int32_t)h.N, v, out, h.stream);
}

// wwy: the anchors' second row sums for the streamed first apply (L::WWs, L::Wsum), from WYs: W (W Y), and W 1 over the ELL rows.
// False where the arrays do not fit: the solve keeps its gathered first apply.
bool build_wwy(const AnchorBuild& c) {
  L& h = c.h;
  if (h.at(Level::wwy).denied) return false;
  host::begin_build(h.derived, Level::wwy);
  if (!reserve({{h.WWs, (size_t)h.N * h.ld}, {h.Wsum, (size_t)h.N}}, h.at(Level::wwy).denied)) return false;
  apply_w(c, h.WYs.p, h.WWs.p);
  launch_row_weight_sums(h.ell_w.p, h.deg.p, h.width, (int32_t)h.N, h.Wsum.p, h.stream);
  return true;
}

// w3: the third row sums for the streamed second apply (L::W3s, L::Wsum2) and the T array, from WWs / Wsum: W (W W Y), and W (W 1)
// over the ELL rows.  W3s and T together under the memory rule, or the solve keeps depth 1.
bool build_w3(const AnchorBuild& c) {
  L& h = c.h;
  if (h.at(Level::w3).denied) return false;
  host::begin_build(h.derived, Level::w3);
  const size_t n = (size_t)h.N * h.ld;
  if (!reserve({{h.W3s, n}, {h.Tap, n}, {h.Wsum2, (size_t)h.N}}, h.at(Level::w3).denied)) return false;
  apply_w_rows(c, h.WWs.p, h.W3s.p);
  row_weighted_sums(h, h.Wsum.p, h.Wsum2.p);
  return true;
}

// gram: the Gram sums of the seven vectors (L::gram; anchor_gram.hpp): one streaming pass over the arrays of the levels below.
bool build_gram(const AnchorBuild& c) {
  L& h = c.h;
  host::begin_build(h.derived, Level::gram);
  DevBuf<double> part;
  if (!gram_scratch(h.gram, (size_t)gram::kGramPerColumn * h.ld + gram::kGramLattice, nullptr, 0, part)) return false;
  launch_anchor_gram(gram_args(h, part.p, h.gram.p), h.stream);
  sync(h);  // part goes out of scope
  return true;
}

// gram3: the third step's sums (L::gram3; anchor_gram.hpp): s3 = W s2 over the ELL rows, W (W3s) into the solve's first scratch
// array, where nothing lives before the INIT pass, then one streaming pass.  Only the sums and s3 are kept.
bool build_gram3(const AnchorBuild& c) {
  L& h = c.h;
  host::begin_build(h.derived, Level::gram3);
  if (c.ld != h.ld || h.part1.n < 3 * (size_t)c.ld) return false;
  DevBuf<double> part;
  if (!gram_scratch(h.gram3, (size_t)gram::kGram3PerColumn * h.ld + gram::kGram3Lattice, &h.Wsum3, (size_t)h.N, part)) return false;
  row_weighted_sums(h, h.Wsum2.p, h.Wsum3.p);
  apply_w_rows(c, h.W3s.p, c.scratch0);
  Gram3Args g{};
  g.g = gram_args(h, part.p, h.gram3.p);
  g.W4 = c.scratch0;
  g.wsum3 = h.Wsum3.p;
  launch_anchor_gram3(g, h.stream);
  sync(h);  // part goes out of scope
  return true;
}

// gram4 (and w4): the fourth step's sums (L::gram4; anchor_gram.hpp): s4 = W s3 over the ELL rows, W^4 Y as build_gram3 forms it,
// W^5 Y = W (W^4 Y) the same way into the solve's second scratch array -- both are free until the INIT pass, and both must be live
// for <W^4 Y, W^5 Y> --, then one streaming pass.  The sums are kept, and W^4 Y where the polynomial last form may read it later:
// then it goes to an array of its own (the memory rule, and OSC_ANCHOR_POLY_MAX_MB: no larger than that either -- anchor_ap_fits
// takes a quarter of what it is given), which is level w4; otherwise to the first scratch array, to be dropped.
bool build_gram4(const AnchorBuild& c) {
  L& h = c.h;
  host::begin_build(h.derived, Level::gram4);
  if (c.ld != h.ld || h.part1.n < 4 * (size_t)c.ld || c.scratch1 == nullptr || c.scratch1 == c.scratch0) return false;
  DevBuf<double> part;
  DevBuf<float> wsum4;
  if (!gram_scratch(h.gram4, (size_t)gram::kGram4PerColumn * h.ld + gram::kGram4Lattice, &wsum4, (size_t)h.N, part)) return false;
  L::AnchorLevel& poly = h.at(Level::w4);
  float* w4 = c.scratch0;
  if (host::anchor_auto_rows(poly.mode, h.N) && !poly.denied) {
    const int64_t cap = h.anchor_poly_max_mb >= 0 ? (int64_t)h.anchor_poly_max_mb * 4 * 1048576 : -1;
    if (reserve({{h.W4s, (size_t)h.N * h.ld}}, poly.denied, cap)) w4 = h.W4s.p;
  }
  row_weighted_sums(h, h.Wsum3.p, wsum4.p);
  apply_w_rows(c, h.W3s.p, w4);
  apply_w_rows(c, w4, c.scratch1);
  Gram4Args g{};
  g.g = gram_args(h, part.p, h.gram4.p);
  g.W4 = w4;
  g.W5 = c.scratch1;
  g.wsum3 = h.Wsum3.p;
  g.wsum4 = wsum4.p;
  launch_anchor_gram4(g, h.stream);
  sync(h);  // part and s4 go out of scope
  if (w4 == h.W4s.p) {
    host::built(h.derived, Level::w4, c.ba.nb);
    poly.builds += 1;
  }
  return true;
}

}  // namespace

bool ensure_anchor(const AnchorBuild& c, Level level) {
  L& h = c.h;
  if (host::held(h.derived, level, c.ba.nb)) return true;
  bool ok = false;
  switch (level) {
    case Level::wwy: ok = build_wwy(c); break;
    case Level::w3: ok = build_w3(c); break;
    case Level::gram: ok = build_gram(c); break;
    case Level::gram3: ok = build_gram3(c); break;
    case Level::gram4: ok = build_gram4(c); break;
    default: throw std::logic_error("ensure_anchor: the level has no builder of its own");
  }
  if (!ok) return false;
  host::built(h.derived, level, c.ba.nb);
  h.at(level).builds += 1;
  return true;
}

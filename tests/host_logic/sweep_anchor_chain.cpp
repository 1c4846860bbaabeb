// Sweep of the anchor-start chain's validity (derived_state.hpp: Level, held, begin_build, built) against the transitions the
// builders used to spell out one by one.  The chain rule is stricter than those were -- a builder dropped a hand-picked subset of
// the levels above it and checked a hand-picked subset of those below --, so the two agree only if the states in which they differ
// cannot be reached.  Part A holds the three functions to their definitions over every combination of block counts.  Part B keeps
// the old per-level ints as a model, runs the chain beside it through every solve an anchor start can make (two block counts; each
// builder succeeding, failing or not being called, in the order a solve calls them; the W.Y re-gather) and through changed() for
// every Input, from the empty state to every reachable one, and asserts at every step that each builder gets the same "must build"
// answer and that every reader (the builders' checks, the polynomial form's, the byte counts) sees the same validity.
// Run under -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#include "../../oscillink_amd/csrc/derived_state.hpp"

using namespace osc::host;

static int fail(const char* what, long long a, long long b) {
  std::printf("ERROR %s (%lld, %lld)\n", what, a, b);
  return 1;
}

enum { WY, WWY, W3, GRAM, GRAM3, GRAM4, W4, NL };
static const Level kLevel[NL] = {Level::wy, Level::wwy, Level::w3, Level::gram, Level::gram3, Level::gram4, Level::w4};
static const int kNb[2] = {2, 5};

// ---- the model: seven ints and the assignments each site made ------------------------------------------------------------
struct Model {
  int nb[NL] = {0, 0, 0, 0, 0, 0, 0};
  void zero(std::initializer_list<int> ls) {
    for (int l : ls) nb[l] = 0;
  }
  // each builder's own test of "held" ...
  bool check(int l, int n) const {
    switch (l) {
      case WY: return nb[WY] == n;
      case WWY: return nb[WWY] == n;
      case W3: return nb[W3] == n && nb[WWY] == n;
      case GRAM: return nb[GRAM] == n && nb[W3] == n;
      case GRAM3: return nb[GRAM3] == n && nb[GRAM] == n;
      case GRAM4: return nb[GRAM4] == n && nb[GRAM3] == n && nb[GRAM] == n;
      default: return nb[W4] == n && nb[GRAM4] == n;  // the polynomial form's
    }
  }
  // ... and what it dropped before it built
  void begin(int l) {
    switch (l) {
      case WY: zero({WY, WWY, W3, GRAM, GRAM3, GRAM4, W4}); break;
      case WWY: zero({WWY}); break;
      case W3: zero({W3, GRAM, GRAM3, GRAM4}); break;
      case GRAM: zero({GRAM, GRAM3, GRAM4}); break;
      case GRAM3: zero({GRAM3, GRAM4}); break;
      case GRAM4: zero({GRAM4, W4}); break;
      default: break;
    }
  }
  bool bytes(int l) const { return nb[l] > 0; }  // the byte counts and the readers: "some block count"
};

struct State {
  Model m;
  Derived d;
  bool denied[NL] = {false, false, false, false, false, false, false};  // wwy, w3 and w4 have one
  uint64_t key() const {
    uint64_t k = 0;
    for (int l = 0; l < NL; ++l) k = k * 3 + (m.nb[l] == 0 ? 0 : m.nb[l] == kNb[0] ? 1 : 2);
    for (int l = 0; l < NL; ++l) k = k * 3 + (d.level_nb[l] == 0 ? 0 : d.level_nb[l] == kNb[0] ? 1 : 2);
    for (int l = 0; l < NL; ++l) k = k * 2 + (denied[l] ? 1 : 0);
    return k;
  }
};

// every reader sees the same
static int same(const State& s, const char* where) {
  for (int l = 0; l < NL; ++l) {
    for (int n : kNb)
      if (s.m.check(l, n) != held(s.d, kLevel[l], n)) {
        std::printf("ERROR %s: level %d differs at %d blocks\n", where, l, n);
        return 1;
      }
    if (s.m.bytes(l) != held(s.d, kLevel[l])) {
      std::printf("ERROR %s: level %d held for the readers differs\n", where, l);
      return 1;
    }
  }
  return 0;
}

enum Outcome { SKIP, OK, FAIL };
// One builder call (wwy .. gram4) on both sides: the check, the denial, the drop, the outcome, the mark.  w4: what gram4's build
// does about W^4 Y (SKIP: not kept, OK: kept, FAIL: denied now).  Returns < 0 on a mismatch, else whether the level is held now.
static int build(State& s, int l, int n, Outcome how, Outcome w4) {
  const bool have = s.m.check(l, n);
  if (have != held(s.d, kLevel[l], n)) return -fail("must build", l, n);
  if (have) return 1;
  if (s.denied[l]) return 0;
  s.m.begin(l);
  begin_build(s.d, kLevel[l]);
  if (same(s, "after the drop")) return -1;
  if (how == FAIL) {
    if (l == WWY || l == W3) s.denied[l] = true;  // (the sums' allocations are not remembered)
    return 0;
  }
  if (l == GRAM4 && !s.denied[W4]) {
    if (w4 == FAIL) s.denied[W4] = true;
    if (w4 == OK) {
      s.m.nb[W4] = n;
      built(s.d, Level::w4, n);
    }
  }
  s.m.nb[l] = n;
  built(s.d, kLevel[l], n);
  if (same(s, "after the mark")) return -1;
  return 1;
}

// One anchor start at n blocks: init_fused's W.Y branch, then the builders in the solve's order, each called only behind the
// success of the one before it.
static int solve(State& s, int n, const Outcome how[NL], Outcome w4) {
  const bool wy = s.m.check(WY, n);
  if (wy != held(s.d, Level::wy, n)) return fail("W.Y held", n, wy);
  if (!wy) {  // the gathering pass rewrites W.Y: everything goes, every denial is forgotten
    s.m.begin(WY);
    begin_build(s.d, Level::wy);
    for (bool& b : s.denied) b = false;
    if (same(s, "while W.Y is rewritten")) return 1;
    s.m.nb[WY] = n;
    built(s.d, Level::wy, n);
    return same(s, "after the re-gather");
  }
  for (int l = WWY; l <= GRAM4; ++l) {
    if (how[l] == SKIP) break;
    const int r = build(s, l, n, how[l], w4);
    if (r < 0) return 1;
    if (r == 0) break;
  }
  return same(s, "after the solve");
}

int main() {
  if ((unsigned)Level::count != NL) return fail("levels", (long long)Level::count, NL);
  for (int l = 0; l < NL; ++l)
    if ((int)kLevel[l] != l) return fail("level order", l, (int)kLevel[l]);

  // ---- A. the three functions are what they say, from every combination of block counts ------------------------------------
  const int vals[3] = {0, 2, 5};
  long long combos = 0;
  for (int code = 0; code < 2187; ++code) {
    int v[NL];
    Derived d;
    for (int l = 0, c = code; l < NL; ++l, c /= 3) {
      v[l] = vals[c % 3];
      built(d, kLevel[l], v[l]);
    }
    for (int l = 0; l < NL; ++l) {
      for (int n : {0, 2, 5, 7}) {
        bool want = n > 0;
        for (int j = 0; j <= l; ++j) want = want && v[j] == n;
        if (held(d, kLevel[l], n) != want) return fail("held", code, l);
      }
      bool any = v[0] > 0;
      for (int j = 0; j <= l; ++j) any = any && v[j] == v[0];
      if (held(d, kLevel[l]) != any) return fail("held for the readers", code, l);
      Derived e = d;
      begin_build(e, kLevel[l]);
      for (int j = 0; j < NL; ++j)  // nothing below l moved, everything from l on is gone
        if (e.level_nb[j] != (j < l ? v[j] : 0)) return fail("begin_build", code, l);
    }
    Derived e = d;
    drop(e, Cache::anchor_wy);
    for (int j = 0; j < NL; ++j)
      if (e.level_nb[j] != 0) return fail("drop(anchor_wy)", code, j);
    ++combos;
  }

  // ---- B. every reachable state, the model beside the chain ------------------------------------------------------------------
  std::set<uint64_t> seen;
  std::vector<State> todo;
  todo.push_back(State{});
  seen.insert(todo.back().key());
  long long steps = 0;
  auto visit = [&](const State& s) {
    if (seen.insert(s.key()).second) todo.push_back(s);
  };
  while (!todo.empty()) {
    const State s0 = todo.back();
    todo.pop_back();
    if (same(s0, "on arrival")) return 1;
    // changed(): parent drop() cleared all seven ints exactly where the table names anchor_wy
    for (unsigned i = 0; i < (unsigned)Input::count; ++i) {
      State s = s0;
      if (depends_on(Cache::anchor_wy, (Input)i)) s.m.begin(WY);
      changed(s.d, (Input)i);
      if (same(s, "after changed()")) return 1;
      ++steps;
      visit(s);
    }
    // a solve: either block count, every outcome of every builder, every fate of W^4 Y
    for (int n : kNb)
      for (int code = 0; code < 243; ++code)
        for (int w = 0; w < 3; ++w) {
          Outcome how[NL] = {SKIP, SKIP, SKIP, SKIP, SKIP, SKIP, SKIP};
          for (int l = WWY, c = code; l <= GRAM4; ++l, c /= 3) how[l] = (Outcome)(c % 3);
          State s = s0;
          if (solve(s, n, how, (Outcome)w)) return 1;
          ++steps;
          visit(s);
        }
  }
  std::printf("anchor chain sweep ok (%lld combinations, %zu reachable states, %lld steps)\n", combos, seen.size(), steps);
  return 0;
}

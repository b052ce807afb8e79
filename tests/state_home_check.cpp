// Stand-alone host program for tests/test_host_cpu.py: csrc/state_home.h against the flag statements it replaced in api.hip, which are
// transcribed here as reference models.  Built with -fsanitize=address,undefined; exits 0 when every check holds.
#include <cstdio>
#include <cstdlib>

#include "state_home.h"

#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      std::exit(1);                                                      \
    }                                                                    \
  } while (0)

using kmpc::Progress;
using kmpc::StateHome;
using kmpc::Term;
using Home = kmpc::StateHome::Home;

// ---- where the state is valid.  The six operations, as the entry points perform them:
enum Op { DenseRead, DenseWrite, TakeFast, DenseOverwritten, DropFast, Steps0Prepare, kOps };

// the two booleans of the old Impl and its statements: ensure_dense, ensure_image, and what the entry points wrote directly
struct FlagModel {
  bool has_fast, dense_valid = true, img_valid = false;
  int to_dense = 0, to_fast = 0;  // conversions launched so far
  void ensure_dense(bool will_modify) {
    if (has_fast && !dense_valid) { ++to_dense; dense_valid = true; }
    if (will_modify) img_valid = false;
  }
  void ensure_image() {  // (its callers asked has_fast first: without an image it would have converted into a null buffer)
    if (!img_valid) { ++to_fast; img_valid = true; }
    dense_valid = false;
  }
  void apply(Op op) {
    switch (op) {
      case DenseRead: ensure_dense(false); break;                  // get_model, condense, the head of export and pack
      case DenseWrite: ensure_dense(true); break;                  // set_model, reset, step, rls_update, the head of unpack
      case TakeFast: if (has_fast) ensure_image(); else ensure_dense(true); break;  // rollout_fused
      case DenseOverwritten: dense_valid = true; img_valid = false; break;          // import, the tail of unpack
      case DropFast: if (has_fast) img_valid = false; break;       // export and pack: `if (core) img_valid = false`
      case Steps0Prepare: if (has_fast) ensure_image(); break;     // rollout_impl with steps == 0
      default: CHECK(false);
    }
  }
};

// the same operations through StateHome, as Impl::ensure_dense / ensure_image and the entry points go through it now
struct HomeModel {
  StateHome h;
  int to_dense = 0, to_fast = 0;
  void ensure_dense(bool will_modify) {
    if (h.dense_stale()) ++to_dense;
    h.dense_ready(will_modify);
  }
  void ensure_image() {
    if (h.fast_stale()) ++to_fast;
    h.fast_taken();
  }
  void apply(Op op) {
    switch (op) {
      case DenseRead: ensure_dense(false); break;
      case DenseWrite: ensure_dense(true); break;
      case TakeFast: if (h.has_fast) ensure_image(); else ensure_dense(true); break;
      case DenseOverwritten: h.dense_overwritten(); break;
      case DropFast: h.drop_fast(); break;
      case Steps0Prepare: ensure_image(); break;  // (unguarded now: nothing to do without a fast form)
      default: CHECK(false);
    }
  }
};

static long g_sequences = 0, g_cut = 0;

// every sequence of up to `left` more operations from the pair of states (f, m), which agree so far
static void walk(const FlagModel& f, const HomeModel& m, int left) {
  if (left == 0) return;
  for (int op = 0; op < kOps; ++op) {
    FlagModel f2 = f;
    HomeModel m2 = m;
    f2.apply((Op)op);
    m2.apply((Op)op);
    ++g_sequences;
    // the same conversions at the same points
    CHECK(f2.to_dense == m2.to_dense && f2.to_fast == m2.to_fast);
    if (!f.has_fast) CHECK(m2.to_dense == 0 && m2.to_fast == 0 && m2.h.home == Home::Dense);
    if (!f2.dense_valid && !f2.img_valid) {
      // The flags can name no valid form at all: drop-fast while only the fast form is valid.  No entry point did that (export and
      // pack make the dense form ready first), and nothing but the order of their statements ruled it out.  A StateHome has no such
      // state: it stays Fast, and the state is not lost.  The two models no longer correspond, so the sequence ends here.
      CHECK(op == DropFast && m.h.home == Home::Fast && m2.h.home == Home::Fast);
      ++g_cut;
      continue;
    }
    // Dense = (true, false), Both = (true, true), Fast = (false, true)
    const Home want = f2.dense_valid ? (f2.img_valid ? Home::Both : Home::Dense) : Home::Fast;
    CHECK(m2.h.home == want);
    walk(f2, m2, left - 1);
  }
}

// ---- the estimator's progress: the rule of one step, as step_impl had it
static void one_step(Progress& p, bool update_on) {
  if (p.have_prev && update_on) p.rls_fresh = false;
  p.have_prev = true;
  p.cur ^= 1;
}

int main() {
  for (int has_fast = 0; has_fast <= 1; ++has_fast) {
    FlagModel f;
    f.has_fast = has_fast != 0;
    HomeModel m;
    m.h.has_fast = has_fast != 0;
    CHECK(m.h.home == Home::Dense);
    g_sequences = g_cut = 0;
    walk(f, m, 6);
    std::printf("has_fast = %d: %ld sequences, %ld ended at a flag pair without a valid form\n", has_fast, g_sequences, g_cut);
    CHECK(has_fast ? g_cut > 0 : (g_cut == 0 && g_sequences == 6 + 36 + 216 + 1296 + 7776 + 46656));
  }

  for (int steps = 0; steps <= 5; ++steps)
    for (int on = 0; on <= 1; ++on)
      for (int start = 0; start < 8; ++start) {
        Progress a;
        a.have_prev = (start & 1) != 0; a.rls_fresh = (start & 2) != 0; a.cur = (start >> 2) & 1;
        Progress b = a;
        const Progress a0 = a;
        a.advance(steps, on != 0);
        for (int i = 0; i < steps; ++i) one_step(b, on != 0);
        CHECK(a.cur == b.cur && a.have_prev == b.have_prev && a.rls_fresh == b.rls_fresh);
        if (steps >= 1) {  // the closed form rollout_fused had beside it
          Progress c = a0;
          if (on && (steps >= 2 || (steps == 1 && c.have_prev))) c.rls_fresh = false;
          c.have_prev = true;
          c.cur ^= (steps & 1);
          CHECK(a.cur == c.cur && a.have_prev == c.have_prev && a.rls_fresh == c.rls_fresh);
        }
      }

  // the header's three flags: exactly the four triples a handle can write, and back
  int legal = 0;
  for (int t = 0; t < 8; ++t) {
    const int have = t & 1, from_dare = (t >> 1) & 1, per_traj = (t >> 2) & 1;
    bool ok = false;
    const Term term = kmpc::term_from_flags(have, from_dare, per_traj, &ok);
    const bool want_ok = (!have && !from_dare && !per_traj) || (have && !from_dare && !per_traj) || (have && from_dare);
    CHECK(ok == want_ok);
    if (!ok) continue;
    ++legal;
    int h2 = -1, d2 = -1, p2 = -1;
    kmpc::term_to_flags(term, &h2, &d2, &p2);
    CHECK(h2 == have && d2 == from_dare && p2 == per_traj);
  }
  CHECK(legal == 4);
  const Term kinds[4] = {Term::None, Term::Given, Term::DareOne, Term::DarePerTraj};
  for (const Term k : kinds) {
    int h = -1, d = -1, p = -1;
    bool ok = false;
    kmpc::term_to_flags(k, &h, &d, &p);
    CHECK(kmpc::term_from_flags(h, d, p, &ok) == k && ok);
    CHECK(kmpc::term_from_dare(k) == (d == 1));
  }
  std::puts("state_home ok");
  return 0;
}

// state_home.h -- the three small state machines of a handle (Impl in api.hip) as types: where the per-trajectory state is valid
// (StateHome), how far the estimator has come (Progress) and what kind of terminal block the handle holds (Term).  Plain host code
// without HIP: api.hip goes through these calls, tests/state_home_check.cpp holds them to the flag statements they replaced.
#pragma once

namespace kmpc {

// Where the per-trajectory state (P, [A B], bar_Q, C; on a float32 handle also psi_{k-1}, u_{k-1}, the warm start) is valid.
// The state has a DENSE form, which every entry point but the fused roll-out works on, and on some handles a FAST form that the
// fused roll-out advances: on a float64 handle the wave image (Impl::dImg, has_fast = use_img), on a float32 handle the float64 core
// (Impl::core, has_fast = core != nullptr).
//
//   Dense  only the dense form is valid        Both  both hold the same state        Fast  the roll-out has advanced the fast form
//
//                  take fast (converts)
//        +--------------------------------------+
//        |                  take fast           v
//      Dense <----------- Both -------------> Fast
//        ^   dense write,   ^    dense read     |
//        |   drop fast      +--- (converts) ----+
//        +------- dense write (converts) -------+
//
//   dense read in Dense or Both and dense write in Dense change nothing; dense overwritten (import, unpack): any -> Dense, no conversion
//
// Two-phase, so that a conversion which fails leaves the home as it was: ask (dense_stale / fast_stale), convert, then commit
// (dense_ready / fast_taken).  Without a fast form every query answers "nothing to do" and the home stays Dense.
struct StateHome {
  enum class Home { Dense, Both, Fast };
  Home home = Home::Dense;
  bool has_fast = false;

  // the dense form is about to be read or modified: must the fast form be converted into it first?
  bool dense_stale() const { return has_fast && home == Home::Fast; }
  // ... it is valid now (converted, or it was); a caller that will modify it leaves the fast form behind
  void dense_ready(bool will_modify) {
    if (!has_fast) return;
    if (will_modify) home = Home::Dense;
    else if (home == Home::Fast) home = Home::Both;
  }
  // the roll-out is about to advance the fast form: must the dense form be converted into it first?
  bool fast_stale() const { return has_fast && home == Home::Dense; }
  // ... it is valid now and about to be written
  void fast_taken() {
    if (has_fast) home = Home::Fast;
  }
  // every dense block has been written from outside (checkpoint import, unpacked rows behind an ensure_dense): no conversion
  void dense_overwritten() { home = Home::Dense; }
  // continue from the dense form although the fast one holds the same state (a float32 handle after export / pack: from its rounded
  // blocks, as the receiver will).  For a caller that has just made the dense form ready; a home of Fast, whose dense form is not
  // valid, stays as it is.
  void drop_fast() {
    if (home == Home::Both) home = Home::Dense;
  }
};

// The estimator's progress: which of the two psi buffers is psi_k's, whether a previous (psi, u) exists (the next step runs the RLS
// update) and whether that update would be the first after a restart (it starts from K_A = 0, bar_X = 0).
struct Progress {
  int cur = 0;
  bool have_prev = false, rls_fresh = true;
  // `steps` control steps have run (per-step launch: 1; the fused roll-out: the kernel's own bookkeeping, followed here): the first
  // of them updated only if a previous transition existed, every later one did
  void advance(int steps, bool update_on) {
    if (steps <= 0) return;
    if (update_on && (have_prev || steps >= 2)) rls_fresh = false;
    have_prev = true;
    cur ^= steps & 1;
  }
};

// The terminal block P_N - Qw I of the handle: none; one block given by the caller (Impl::dWt, in the handle's dtype); one block or
// one per trajectory from the Riccati iteration (Impl::dWtB, float64).
enum class Term { None, Given, DareOne, DarePerTraj };
inline bool term_from_dare(Term t) { return t == Term::DareOne || t == Term::DarePerTraj; }
// The three 0 / 1 flags of the blob header (have_wterm, wterm_from_dare, wterm_per_traj) exist here alone.  *ok: the triple is one of
// the four a handle can write.
inline Term term_from_flags(int have, int from_dare, int per_traj, bool* ok) {
  *ok = true;
  if (!have && !from_dare && !per_traj) return Term::None;
  if (have == 1 && !from_dare && !per_traj) return Term::Given;
  if (have == 1 && from_dare == 1 && !per_traj) return Term::DareOne;
  if (have == 1 && from_dare == 1 && per_traj == 1) return Term::DarePerTraj;
  *ok = false;
  return Term::None;
}
inline void term_to_flags(Term t, int* have, int* from_dare, int* per_traj) {
  *have = t != Term::None;
  *from_dare = term_from_dare(t);
  *per_traj = t == Term::DarePerTraj;
}

}  // namespace kmpc

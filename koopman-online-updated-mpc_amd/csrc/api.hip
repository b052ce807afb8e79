// api.hip -- the C ABI of libkoopmpc.so (include/koopmpc.h): handle, parameter upload,
// persistent state and stream-ordered launches.  No compute happens on the host.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/koopmpc.h"
#include "devbuf.h"
#include "kernels.h"
#include "state_home.h"
#include "state_rows.h"
#include <dlfcn.h>
#include <rccl/rccl.h>  // types and enumerators only (ncclDouble, ncclSum): the library resolves ncclAllReduce at run time

using namespace kmpc;

static thread_local std::string g_create_error;

struct kmpc_handle {
  kmpc_config cfg{};
  mutable std::string err;
  virtual ~kmpc_handle() {
    for (auto& mk : marks) (void)hipEventDestroy(mk.e);
  }
  virtual int set_encoder_layer(int layer, const double* W, const double* b, int rows, int cols) = 0;
  virtual int set_centres(const double* cx, int L, int n) = 0;
  virtual int set_rbf_order(int k) = 0;
  virtual int set_model(const double* A, const double* B, const double* C) = 0;
  virtual int set_terminal_weight(const double* PN) = 0;
  virtual int terminal_from_dare(const double* Qh, double R, int maxiter, double eps, int per_traj, double* PN_out,
                                 int32_t* iters_out, hipStream_t s) = 0;
  virtual int set_terminal_refresh(int every, const double* Qh, double R, int maxiter, double eps) = 0;
  virtual int rollout_is_fused() const = 0;
  // the route the last kmpc_rollout with steps > 0 took: 0 per-step launches (or no roll-out yet), 1 the fused generic kernel, 2 the
  // fused default-option kernel (csrc/step_body.h RoOpt)
  int last_rollout_variant = 0;
  int last_rollout_resident = 0, last_rollout_lds = 0;  // kmpc_rollout_resident
  virtual int rollout_plugin_status(std::string* text) const = 0;
  virtual int reset(hipStream_t s) = 0;
  virtual int state_init(double P0, double barQ0, hipStream_t s) = 0;
  virtual int state_init_from(const double* KA0, const double* P0m, const double* barX0, const double* barQ0m, hipStream_t s) = 0;
  virtual int lift(const void* X, void* Psi, int B, hipStream_t s) = 0;
  virtual int rls_update(const void* psi, const void* u, const void* psin, const void* xn, int B, hipStream_t s) = 0;
  virtual int get_model(void* A, void* B, void* C, hipStream_t s) = 0;
  virtual int condense(const void* psi, const void* ref, int rpt, void* H, void* f, void* c, int B, hipStream_t s) = 0;
  virtual int mpc_solve(const void* A, const void* Bv, const void* C, int shared, const void* psi, const void* ref, int rpt,
                        double lb, double ub, double Qw, double Rw, const double* PN, void* U, void* U0, void* fun,
                        int32_t* st, int32_t* it, int B, hipStream_t s) = 0;
  virtual int generate_and_fit(int plant, const void* X0, const void* U, int n_traj, int n_steps, double hs, double ridge,
                               int init_rls, void* A, void* B, void* C, void* Xo, void* Yo, hipStream_t s) = 0;
  int device = 0;
  // The few entry points that work on the null stream (kmpc_set_model, checkpoints, the first shared-model call) wait for the handle's OWN
  // outstanding work instead of the whole device (a device-wide synchronisation stalls the caller's unrelated streams).
  // What that work is: every stream-ordered entry point ends by recording a handle-owned event on its stream (one event per distinct
  // stream the caller has used with this handle); sync_own() waits for those events.  An event stays valid after the caller has
  // destroyed the stream, and a roll-out on stream A followed by a call on stream B leaves both recorded (the raw handle of
  // "the last stream" dangled and covered one stream only).  Calls made while their stream is being captured into a graph leave no mark.
  struct StreamMark { hipStream_t s; hipEvent_t e; unsigned long long age; };
  std::vector<StreamMark> marks;
  unsigned long long mark_clock = 0;
  void mark_stream(hipStream_t s) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cap) != hipSuccess) { (void)hipGetLastError(); return; }
    if (cap != hipStreamCaptureStatusNone) return;
    StreamMark* m = nullptr;
    for (auto& mk : marks)
      if (mk.s == s) { m = &mk; break; }
    if (!m) {
      if (marks.size() >= 16) {  // (a caller that keeps making streams: the least recently used mark is waited for and reused)
        m = &marks[0];
        for (auto& mk : marks)
          if (mk.age < m->age) m = &mk;
        (void)hipEventSynchronize(m->e);
        m->s = s;
      } else {
        hipEvent_t e = nullptr;
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); return; }
        marks.push_back(StreamMark{s, e, 0});
        m = &marks.back();
      }
    }
    m->age = ++mark_clock;
    if (hipEventRecord(m->e, s) != hipSuccess) (void)hipGetLastError();
  }
  hipError_t sync_marks() {
    for (auto& mk : marks) {
      const hipError_t e = hipEventSynchronize(mk.e);
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  }
  virtual int qp_solve(const void* H, const void* f, void* U, int32_t* st, int32_t* it, int B, hipStream_t s) = 0;
  virtual int step(const void* X, const void* ref, int rpt, void* U0, void* Useq, int32_t* st, int32_t* it,
                   hipStream_t s) = 0;
  virtual int plant_step(int plant, void* X, const void* U, double h, int sw, int B, hipStream_t s) = 0;
  virtual int set_applied_input(const void* U, int B, hipStream_t s) = 0;
  virtual int set_online_update(int on) = 0;
  virtual int rollout(int plant, void* X, const void* ref, int rpt, int steps, int step0, int switch_step, double hs,
                      void* Ulog, void* Xlog, int32_t* st, int32_t* it, hipStream_t s) = 0;
  virtual int set_rollout_diagnostics(int on) = 0;
  virtual int estimator_status(double* P0, double* barQ0) const = 0;
  virtual int get_prev_transition(void* psi_prev, void* u_prev, hipStream_t s) = 0;
  virtual int rollout_diag(int plant, void* X, const void* ref, int rpt, int steps, int step0, int switch_step, double hs, void* Ulog,
                           void* Xlog, void* Psilog, void* dAlog, void* dBlog, void* dClog, int32_t* st, int32_t* it, hipStream_t s) = 0;
  virtual int offline_fit(const void* X, const void* Y, const void* U, int M, double ridge, int init_rls, void* A,
                          void* B, void* C, hipStream_t s) = 0;
  virtual int64_t gram_elems() const = 0;
  virtual int shared_local_gram(const void* X, double* delta, hipStream_t s) = 0;
  virtual int shared_solve_plant(const double* delta, const void* ref, void* U0, void* Useq, int32_t* st, int32_t* it, int plant, void* X,
                                 int switched, double hstep, hipStream_t s) = 0;
  virtual int shared_solve(const double* delta, const void* ref, void* U0, void* Useq, int32_t* st, int32_t* it,
                           hipStream_t s) = 0;
  virtual int shared_get_model(void* A, void* B, void* C, hipStream_t s) = 0;
  virtual int shared_rollout(int plant, void* X, const void* ref, int steps, int step0, int switch_step, double hstep, void* comm,
                             void* Ulog, void* Xlog, void* U0out, void* Useq, int32_t* st, int32_t* it, hipStream_t s) = 0;
  virtual int64_t state_bytes() const = 0;
  virtual int state_export(void* blob, int64_t bytes) = 0;
  virtual int state_import(const void* blob, int64_t bytes) = 0;
  virtual int64_t state_row_elems() const = 0;
  virtual int state_pack(const int32_t* idx, int count, void* rows, hipStream_t s) = 0;
  virtual int state_unpack(const int32_t* idx, int count, const void* rows, hipStream_t s) = 0;
  virtual int state_transfer(const int32_t* dst_idx, kmpc_handle* src, const int32_t* src_idx, int count, hipStream_t s) = 0;
  virtual int profile_enable(int on) = 0;
  virtual int profile_read(double* ms2, int64_t* count, int reset) = 0;
  virtual int64_t algorithmic_bytes() const = 0;
};

// ncclAllReduce of the RCCL that lives in this process (under PyTorch: torch's own copy), else of the system library; null: none.
// The library itself does not link against RCCL.
static void* resolve_nccl_allreduce() {
  static void* fn = nullptr;
  if (!fn) {
    fn = dlsym(RTLD_DEFAULT, "ncclAllReduce");
    if (!fn) {
      void* lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
      if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
      if (lib) fn = dlsym(lib, "ncclAllReduce");
    }
  }
  return fn;
}

#define HIPCHK(expr)                                                                  \
  do {                                                                                \
    hipError_t e_ = (expr);                                                           \
    if (e_ != hipSuccess) {                                                           \
      err = std::string(#expr) + ": " + hipGetErrorString(e_);                        \
      return -(int)(1000 + (int)e_);                                                  \
    }                                                                                 \
  } while (0)

#define FAIL(code, msg) \
  do {                  \
    err = (msg);        \
    return (code);      \
  } while (0)

static inline long even_up(long v) { return (v + 1) & ~1L; }
// what kmpc_rollout_plugin_status says (code 2) of a handle that Impl::fused_kind_ok refuses.  (kmpc_rollout_plugin_prebuild has no
// output kind: by its contract out_rows == L, or out_rows = 0 with n == L, asks for the y = psi object, which is what it makes.)
static const char* const kFusedKindReason =
    "no fused roll-out: y = C x with as many output rows as lifted states (q == L), which the fused kernels read as y = psi (per-step launches)";
// KMPC_PLANT_* with the optional KMPC_PLANT_RK4_MATLAB bit (not for the tank map, which has no Runge-Kutta step)
static inline bool plant_id_ok(int plant) {
  const int base = plant & ~KMPC_PLANT_RK4_MATLAB;
  return base >= KMPC_PLANT_DUFFING && base <= KMPC_PLANT_TANK && !(base == KMPC_PLANT_TANK && (plant & KMPC_PLANT_RK4_MATLAB));
}

// What a caller hands down to the step / solve / roll-out bodies of a handle (nothing of it is kept in the handle).  The default is a plain
// call: kmpc_step, kmpc_shared_solve, kmpc_rollout.
struct DiagLogs { void *Psi, *dA, *dB, *dC; };  // the logs of a kmpc_rollout_diag call (RolloutArgs::Psi_log ...), any may be null
struct StepCtx {
  bool accumulate = false;         // a step of a roll-out: status / iterations are worst / total over the steps
  int plant = -1, switched = 0;    // >= 0: the step kernel advances the plant itself, with step h, on X_rw
  double h = 0.05;
  void* X_rw = nullptr;
  const DiagLogs* diag = nullptr;  // the call is a kmpc_rollout_diag
};

// ---- The state blob of kmpc_state_export / kmpc_state_import, version 2.  This comment is the format; Impl::sections() is its one
// implementation and tests/test_gpu_state_blob_layout.py holds the bytes to it.  Everything is native-endian and packed back to back,
// without alignment between sections.  T is the handle's dtype (float or double), p = L + 1, q the number of output rows,
// even_up(v) = v rounded up to an even number.
//
//   header    BlobHeader, 80 bytes: 16 int32 in the order of the struct, then the float64 scales P0, barQ0 of the estimator's restart.
//             dtype is KMPC_F32 / KMPC_F64; the flags are 0 or 1; wterm_blocks is 0 without a terminal section, B with
//             wterm_from_dare and wterm_per_traj, else 1; reserved is 0.
//   P         [B][sP] T   inv_K_G of every trajectory: p x p row-major at the head of a stride of sP = even_up(p p) elements
//   K         [B][sK] T   [A B]: L x p row-major, sK = even_up(L p)
//   Q         [B][sQ] T   bar_Q: L x L row-major, sQ = even_up(L L)
//   C         [B][sC] T   n x L row-major, sC = even_up(n L)   (unused for y = psi)
//   psi_prev  [B][L]  T   psi(x_{k-1})
//   warm      [N][B]  T   the last minimiser, the start of the next solve
//   u_prev    [B]     T   u_{k-1}
//   -- with has_shared:
//   Gram      [(p + L + n) p] float64   the Gram sums of the shared model
//   shared K  [L p] T, shared C [n L] T
//   -- with have_wterm:
//   terminal  [wterm_blocks][q q]   PN - Qw I, as T; as float64 with wterm_from_dare (the blocks of the Riccati iteration)
//
// The content of the stride padding (the odd element of sP .. sC) is no part of the format.
static constexpr int32_t kBlobMagic = 0x4b4d5043;
struct BlobHeader {
  int32_t magic, version, dtype, n, L, N, B, have_prev, rls_fresh;
  int32_t has_shared, shared_has_samples, have_wterm, wterm_from_dare, wterm_per_traj, wterm_blocks, reserved;
  double P0, barQ0;
};
static_assert(sizeof(BlobHeader) == 80, "BlobHeader is the first 80 bytes of a state blob");
// (Section / Sections, one section of a blob as a handle holds it and the ordered list of them: csrc/state_rows.h)
static inline int64_t blob_bytes(const Sections& t) { return (int64_t)sizeof(BlobHeader) + t.payload_bytes(); }
//
// ---- The packed row of kmpc_state_pack / kmpc_state_unpack / kmpc_state_transfer: ONE trajectory's share of the leading n_traj
// sections above, in the blob's order and the handle's dtype T.  This comment is the format; build_row_plan (csrc/state_rows.h) derives
// it from Impl::sections() and tests/test_gpu_state_rows.py holds the bytes to the blob's.
//
//   P[sP] K[sK] Q[sQ] C[sC]   the trajectory's full strides, padding element included
//   psi_prev[L]
//   warm[N]                   the trajectory's column of the [N][B] panel
//   u_prev[1]
//   have_prev, rls_fresh      the handle's two flags, 0 or 1 as T
//   zero padding              up to row_elems = the next multiple of 16 bytes
//
// rows_dev of the three calls is [count][row_elems], trajectory-major.  The bytes of a row's segments equal the bytes of the blob's
// sections for that trajectory.

template <typename T>
struct Impl : kmpc_handle {
  int n, m, L, p, q, N, B, threads;
  long sP, sK, sQ, sC;
  // ---- persistent state
  // (every device block of the handle is a DevBuf, csrc/devbuf.h: freed with the handle, no list to keep)
  DevBuf<T> dP, dK, dQ, dC;
  DevBuf<T> dPsi[2];  // [B][L] trajectory-major: [cur], [prev]
  DevBuf<T> dUprev;
  DevBuf<T> dWarm;  // [N][B] last minimiser = start of the next solve (the reference restarts at zeros, duffing.py:634-635)
  DevBuf<T> dQpScr;  // [batch][N*N] fall-back tableau of the register QP solvers (global scratch, rarely touched); grown by kmpc_qp_solve
  // four-wave solver (threads = 256, float64): every trajectory's last tableau and its variable set, kept from step to step
  // (StepArgs::qp_carry); any change of the model from outside forgets them (the next solve starts from 2H)
  DevBuf<T> dQpCarry;
  DevBuf<int32_t> dQpCarrySet;
  // Register-state step (step_v2.h): the fused roll-out of the small y = C x dimension sets streams the state as a "wave image"
  // ([B][sImg] doubles).  The dense blocks above stay the form every other entry point works on; the image is the fast form of
  // `home` (csrc/state_home.h: which of the two is valid, and when the other is rebuilt by state_to_image / image_to_state, one
  // pass over the state).
  DevBuf<double> dImg;
  long sImg = 0;
  bool use_img = false;
  // KMPC_F32 handle of a register-state dimension set (row g2: BASELINE configs[1] names fp32; SURVEY G6: fp32 panels, float64
  // covariance): kmpc_rollout runs the float64 fused roll-out behind float32 panels.  `core` is a float64 handle of the same
  // configuration that owns the state while roll-outs run (its wave image; psi_{k-1}, u_{k-1}, the warm start in float64); the
  // float32 blocks of this handle are the form every other entry point works on.  The core is the fast form of this handle's
  // `home` (csrc/state_home.h); the other side is rebuilt on demand by a cast over the blocks (core_push / core_pull).
  Impl<double>* core = nullptr;
  bool is_core = false;  // this handle IS the float64 core of a float32 handle
  StateHome home;        // where the per-trajectory state is valid: ensure_dense / ensure_image
  Progress prog;         // psi_k's buffer; a previous (psi, u) exists -> next step runs the RLS update; that update starts from K_A = 0, bar_X = 0
  // the loop WITHOUT the online update (duffing.py:738-805, vanderpol.py:645-722): kmpc_step / kmpc_rollout skip the RLS phase and
  // solve with the model as it is; the lift / input history keeps running, so that switching the update back on continues
  bool update_on = true;
  DevBuf<T> dMsK, dMsC, dMsH, dMsf, dMsc, dMsW;  // kmpc_mpc_solve: scratch model blocks, H, f, c, terminal block
  // ---- parameters
  EncoderShape enc{};  // the encoder as the kernels see it (effective hidden width, padding, k-steps)
  int Lenc = 0;        // the encoder's own output dimension (lift_offset)
  std::vector<std::vector<double>> hostW, hostb;  // the layers as given (row-major), kept for finalize_encoder
  DevBuf<T> dW1, db1, dWh[2], dbh[2], dWo, dbo, dcx, dTmp;
  DevBuf<T> dWhp[2], dWop;  // hidden / output weights as MFMA A-fragments
  bool packed_ok = false;
  std::vector<bool> layer_set;
  bool centres_set = false;
  int rbf_k = 1;  // polyharmonic coefficient (rbf.m:15-17), kmpc_set_rbf_order
  // ---- fused roll-out (one launch for all the steps; rollout_kernel in step_kernel.hip)
  DevBuf<T> dU0;  // rollout scratch [B]
  DevBuf<int32_t> dWork;  // [B] solver work of every trajectory in the last fused launch (RolloutArgs::work)
  DevBuf<int32_t> dPerm;  // [B] slot -> trajectory for the next fused launch (RolloutArgs::perm); valid after a launch that wrote dWork
  bool place_valid = false;
  hipEvent_t evPlace = nullptr;      // recorded behind the launch (and the rank pass) that wrote dWork / dPerm
  hipStream_t place_stream = nullptr;
  // kmpc_set_rollout_diagnostics / kmpc_rollout_diag: the reference's logXLOClift and A_error, B_error, C_error (duffing.py:850, 985-990,
  // 1015) from inside the roll-out.  Fused route: rollout_kernel<.., DIAG> (a plug-in made by the setter, also for the built-in sets;
  // with a terminal refresh armed the variant that has both); every other route: rls_diag_kernel in front of each step's update.
  bool diag_on = false;
  // ---- shared-model mode
  DevBuf<double> dGram, dPartial;  // (dGram set: the handle has its shared-model blocks, all seven -- shared_alloc)
  DevBuf<T> dKs, dCs, dHs, dFs, df0s, dTs;
  DevBuf<double> dFastPack;      // F, T0, H of the shared model as shared_fast_kernel's operand fragments (SharedModel2Args::pack)
  bool fast_pack_valid = false;  // ... written by the last model launch
  DevBuf<int32_t> dNeed;  // [B] flags of shared_fast_kernel
  DevBuf<int32_t> dQpList;  // two alternating counters, then the list of the trajectories shared_fast_kernel left to the solve-only kernel
  int qp_list_parity = 0;
  DevBuf<double> dDelta;  // kmpc_shared_rollout: this rank's Gram sums of a step (all-reduced in place)
  bool shared_has_samples = false;
  static constexpr int GRAM_BLOCKS = 256;  // partial blocks of the Gram kernels (512 measured slower: lift + Gram 21.8 vs 17.2 us, reduce 7.6 vs 4.8 us)
  // ---- terminal block (PN - Qw I of Q_bar; the kinds: Term, csrc/state_home.h)
  Term wterm = Term::None;
  DevBuf<T> dWt;  // the block given to kmpc_set_terminal_weight
  std::vector<double> hostPN;  // P_N as given to kmpc_set_terminal_weight
  // kmpc_terminal_from_dare: Riccati workspace and the block(s) it produced ([1] or [B][q*q], PN - Qw I)
  DevBuf<double> dDareP, dWtB;
  DevBuf<int32_t> dDareIt;
  int dare_cap = 0;  // models the three hold room for (dare_buffers alone changes it)
  DevBuf<double> dEyeL;  // L x L identity: the output map of y = psi
  // kmpc_set_terminal_refresh: the MATLAB controller recomputes its terminal ingredients with the updated model at EVERY iteration
  // (Koopman_update.m:215 dlqr, :381 Q_bar(end) = C P C').  every > 0: kmpc_step / kmpc_rollout run the reference's Riccati iteration
  // (duffing.py:583-598) on every trajectory's freshly updated [A B] each `every`-th step and rebuild its block Co P Co' before the
  // condensed QP is formed -- INSIDE the launch for the fused roll-out (rollout_kernel<.., TERM>, a plug-in made here), as RLS launch /
  // dare_kernel / QP launch on the per-step route.  0: off (the blocks stay what the last refresh left).
  int term_every = 0, term_maxiter = 500;
  long term_count = 0;
  double term_R = 0.01, term_eps = 0.01;
  DevBuf<double> dTermQ, dTermScr;
  // ---- packed rows
  DevBuf<int32_t> dRowChk;  // [B] marks of the duplicate check, then the status word of state_rows_check_kernel
  DevBuf<T> dRowStage;      // kmpc_state_transfer into this handle: the packed rows between gather and scatter, grown on demand
  // ---- profiling
  bool prof = false;
  std::vector<hipEvent_t> ev;  // triples
  size_t ev_used = 0;
  static constexpr size_t EV_CAP = 3 * 4096;
  int64_t prof_steps = 0;  // control steps covered by the recorded events

  // The fused roll-out objects of this handle's dimension set (rollout_plugin.hip), variant[term][diag]: [0][0] the plain kernel (loaded by
  // init unless the set is built-in), [1][0] with the terminal refresh inside (kmpc_set_terminal_refresh), [.][1] with the diagnostics logs
  // (kmpc_set_rollout_diagnostics).  state: 0 not asked for / built-in set / no fused roll-out at all, 1 loaded, -1 could not be made or no
  // such variant.  A launch runs the one variant_of() names: it never looks up or compiles a plug-in.
  struct RolloutVariant { int state = 0; RolloutPlugin plugin{}; std::string msg; };
  RolloutVariant variant[2][2];
  std::string& diag_msg() { return variant[0][1].msg; }  // (the two DIAG variants share one message: whichever load spoke last)
  const std::string& diag_msg() const { return variant[0][1].msg; }
  // the variant a call runs now: with the refresh armed the TERM objects, a kmpc_rollout_diag call the DIAG ones
  const RolloutVariant& variant_of(bool diag_call) const { return variant[term_every > 0][diag_call]; }
  // asks for the object of variant[term][diag] (process table, kernel cache, else hipcc); false: this configuration has no such object
  bool load_variant(bool term, bool diag) {
    RolloutVariant& v = variant[term][diag];
    if (!rollout_plugin_key(n, L, N, q, cfg.lift_kind != KMPC_LIFT_MLP, enc.Lp, enc.KS, enc.Hp, B, sizeof(T) == 4, &v.plugin.key, term, diag,
                            cfg.lift_kind >= KMPC_LIFT_RBF_GAUSS))
      return false;
    v.plugin.fn = rollout_plugin_get(v.plugin.key, diag ? &diag_msg() : &v.msg);
    v.state = v.plugin.fn ? 1 : -1;
    return true;
  }
  // this handle's dimension set can run fused at all (single-wave trajectories, two states, an instantiation or a plug-in that was not refused)
  bool fused_dims_ok() const {
    return threads == 64 && n == 2 && fused_kind_ok() && variant[0][0].state >= 0 &&
           rollout_fused_available<double>(n, L, N, q, threads, cfg.lift_kind != KMPC_LIFT_MLP);
  }
  // (the fused kernels are static instantiations, which take the output kind from q -- Q_ == L_ means y = psi, step_body.h --: a handle
  //  with y = C x and as many output rows as lifted states (n = 2, L = 2, both rows of C) would track psi(x).  It keeps the per-step
  //  launches, whose launcher hands such a handle to the generic kernel: step_kernel.hip launch_step)
  bool fused_kind_ok() const { return (q == L) == (cfg.output_kind == KMPC_OUT_LIFT); }
  // what the lift kernels get in LiftArgs / RolloutArgs::rbf_matlab: 0 / 1 the thin plates, else the kind with k in bits 8-15 (plant_device.h)
  int rbf_code() const {
    if (cfg.lift_kind <= KMPC_LIFT_RBF_MATLAB) return cfg.lift_kind == KMPC_LIFT_RBF_MATLAB ? 1 : 0;
    return cfg.lift_kind | (rbf_k << 8);
  }

  int init(const kmpc_config& c) {
    cfg = c;
    n = c.n; m = c.m; L = c.L; N = c.N; B = c.batch; p = L + 1;
    q = (c.output_kind == KMPC_OUT_LIFT) ? L : (c.out_rows > 0 ? c.out_rows : n);
    if (c.output_kind != KMPC_OUT_LIFT && (c.out_row0 < 0 || c.out_row0 + q > n)) FAIL(-2, "out_row0/out_rows outside C");
    if (c.delta_u && !(c.umax > c.umin)) FAIL(-2, "delta_u needs umin < umax");
    if (c.lift_kind < KMPC_LIFT_MLP || c.lift_kind > KMPC_LIFT_RBF_POLYHARMONIC) FAIL(-2, "lift_kind must be one of KMPC_LIFT_* (0..6)");
    if (c.lift_kind >= KMPC_LIFT_RBF_GAUSS && c.lift_kind <= KMPC_LIFT_RBF_INVMULTQUAD && !std::isfinite(c.rbf_eps))
      FAIL(-2, "rbf_eps (the kernel width of rbf.m) must be finite for the gauss, invquad and invmultquad lifts");
    if (m != 1) FAIL(-2, "m must be 1 (the reference takes B_hat = K[:, Nlift], duffing.py:170-171)");
    if (n < 1 || n > 4) FAIL(-2, "n must be in 1..4");
    if (L < 1 || L > 64) FAIL(-2, "L must be in 1..64");
    if (N < 1 || N > 64) FAIL(-2, "N must be in 1..64");
    if (B < 1) FAIL(-2, "batch must be >= 1");
    if (!(c.lambda > 0.0 && c.lambda <= 1.0)) FAIL(-2, "lambda must be in (0, 1]");
    if (!(c.ub > c.lb)) FAIL(-2, "need lb < ub");
    threads = c.threads;
    if (threads == 0) threads = (p * p > 2048 || N * N > 2048) ? 256 : 64;
    if (threads != 64 && threads != 256) FAIL(-2, "threads must be 0, 64 or 256");
    int r1, r2;
    if (step_lds_bytes(n, L, q, N, sizeof(T), &r1, &r2) > 160 * 1024) FAIL(-2, "configuration exceeds 160 KB of LDS");
    sP = even_up((long)p * p); sK = even_up((long)L * p); sQ = even_up((long)L * L); sC = even_up((long)n * L);
    HIPCHK(dP.alloc((size_t)sP * B));
    HIPCHK(dK.alloc((size_t)sK * B));
    HIPCHK(dQ.alloc((size_t)sQ * B));
    HIPCHK(dC.alloc((size_t)sC * B));
    HIPCHK(dPsi[0].alloc((size_t)L * B));
    HIPCHK(dPsi[1].alloc((size_t)L * B));
    HIPCHK(dUprev.alloc((size_t)B));
    HIPCHK(dQpScr.alloc((size_t)B * N * N));
    HIPCHK(dWarm.alloc((size_t)N * B));
    HIPCHK(dTmp.alloc((size_t)(L * p + n * L + 64)));
    // every block a checkpoint carries starts as zeros, the padding of the strides included (reset() below fills P and bar_Q)
    const Sections blocks = sections(blob_header());
    for (int i = 0; i < blocks.n_traj; ++i) HIPCHK(hipMemset(blocks.s[i].ptr, 0, blocks.s[i].bytes()));
    HIPCHK(hipMemset(dPsi[prog.cur], 0, sizeof(T) * (size_t)L * B));
    if (sizeof(T) == 8 && threads == 256 && !dbg_env("KMPC_QP_NO_CARRY")) {  // (the variable is a measurement aid)
      HIPCHK(dQpCarry.alloc((size_t)B * N * N));
      HIPCHK(dQpCarrySet.alloc((size_t)B * 4));
      HIPCHK(hipMemset(dQpCarrySet, 0, sizeof(int32_t) * (size_t)B * 4));
    }
    // a dimension set without a built-in fused roll-out gets its kernel now (rollout_plugin.hip: kernel cache, else hipcc, 4-8 s);
    // a set that cannot be served stays on per-step launches and kmpc_rollout_plugin_status says why
    enc = encoder_shape(c.hidden, c.lift_offset, n, L);
    // a float32 handle runs the float64 fused roll-out behind float32 panels (its core, below)
    // (KMPC_NO_IO32_ROLLOUT is a measurement / test aid: float32 handles as per-step launches)
    const bool io32_ok = sizeof(T) == 4 && c.output_kind != KMPC_OUT_LIFT && !c.delta_u && rollout_io32_available(n, L, N, q, c.lift_kind != KMPC_LIFT_MLP) &&
                         !dbg_env("KMPC_NO_IO32_ROLLOUT");
    if (fused_dims_ok() && !is_core && (c.lift_kind != KMPC_LIFT_MLP || (enc.hid >= 1 && enc.hid <= 128)) && (sizeof(T) == 8 || io32_ok)) load_variant(false, false);
    if constexpr (sizeof(T) == 8) {
      use_img = fused_dims_ok() && (c.output_kind != KMPC_OUT_LIFT || q == L) && rollout_uses_image(n, L, N, q);
      if (use_img) {
        sImg = state_image_elems(L, n);
        HIPCHK(dImg.alloc((size_t)sImg * B));
      }
      home.has_fast = use_img;
    }
    if constexpr (sizeof(T) == 4) {
      if (fused_dims_ok() && io32_ok) {
        kmpc_config c64 = c;
        c64.dtype = KMPC_F64;
        core = new Impl<double>();
        core->is_core = true;  // (its launches carry float32 panels: this handle's plug-in, loaded above, serves them)
        const int rc = core->init(c64);
        if (rc) { err = "float64 core of the float32 handle: " + core->err; delete core; core = nullptr; return rc; }
        core->variant[0][0].plugin = variant[0][0].plugin;
        home.has_fast = true;
      }
    }
    if (c.lift_kind == KMPC_LIFT_MLP) {
      if (c.layers != 2 && c.layers != 3) FAIL(-2, "layers (hidden layers) must be 2 or 3");
      if (c.hidden < 1 || c.hidden > 128) FAIL(-2, "hidden must be in 1..128");
      // lift_offset (the MATLAB scripts' lifts): 1: psi(x) - psi(0) (Koopman_update_Tracking_Lift.m:65) -- an output bias;
      // 2: [x; psi(x)] - [0; psi(0)] (Koopman_update.m:67, L = n + the encoder's outputs) -- 2n more hidden units carry
      // relu(x), relu(-x) through the layers with identity weights and the first n output rows read x = relu(x) - relu(-x)
      // back (exact: one of the two is zero).  Either way the kernels see an ordinary encoder (finalize_encoder).
      if (c.lift_offset < 0 || c.lift_offset > 2) FAIL(-2, "lift_offset must be 0, 1 or 2");
      Lenc = L - (c.lift_offset == 2 ? n : 0);
      if (Lenc < 1) FAIL(-2, "lift_offset = 2 needs L > n (L = n + the encoder's output dimension)");
      if (enc.hid > 128) FAIL(-2, "hidden + 2 n must not exceed 128 with lift_offset = 2");
      const int Hp = enc.Hp, Lp = enc.Lp;
      HIPCHK(dW1.alloc((size_t)Hp * 4));
      HIPCHK(db1.alloc((size_t)Hp));
      for (int k = 0; k < c.layers - 1; ++k) {
        HIPCHK(dWh[k].alloc((size_t)Hp * Hp));
        HIPCHK(dbh[k].alloc((size_t)Hp));
      }
      HIPCHK(dWo.alloc((size_t)Lp * Hp));
      HIPCHK(dbo.alloc((size_t)Lp));
      layer_set.assign(c.layers + 1, false);
      hostW.assign(c.layers + 1, std::vector<double>());
      hostb.assign(c.layers + 1, std::vector<double>());
    } else {
      if (c.lift_offset != 0) FAIL(-2, "lift_offset applies to the MLP encoder only");
      HIPCHK(dcx.alloc((size_t)L * n));
    }
    return reset(nullptr);
  }

  ~Impl() override {
    delete core;
    for (auto e : ev) (void)hipEventDestroy(e);
    if (evPlace) (void)hipEventDestroy(evPlace);
  }

  // the handle's own outstanding work has finished (the events behind its stream-ordered calls, then the null stream the caller is
  // about to use)
  int sync_own() {
    HIPCHK(sync_marks());
    HIPCHK(hipStreamSynchronize(nullptr));
    return 0;
  }
  // upload a (rows x cols) host double matrix into a zero-padded (prow x pcol) device matrix of T
  int upload_padded(T* dst, const double* src, int rows, int cols, int prow, int pcol) {
    std::vector<T> tmp((size_t)prow * pcol, T(0));
    for (int r = 0; r < rows; ++r)
      for (int c2 = 0; c2 < cols; ++c2) tmp[(size_t)r * pcol + c2] = (T)src[(size_t)r * cols + c2];
    HIPCHK(hipMemcpy(dst, tmp.data(), tmp.size() * sizeof(T), hipMemcpyHostToDevice));
    return 0;
  }

  // the dense blocks are about to be read or modified / the wave image is about to be used by the roll-out
  int ensure_dense(hipStream_t s, bool will_modify) {
    if (home.dense_stale()) {
      if constexpr (sizeof(T) == 8) {
        HIPCHK(launch_image_to_state(dImg, sImg, n, L, B, (double*)dP, sP, (double*)dK, sK, (double*)dQ, sQ, (double*)dC, sC, s));
      } else {
        const int rc = core_pull(s);
        if (rc) return rc;
      }
    }
    home.dense_ready(will_modify);
    return 0;
  }
  // a call that the float64 core of a float32 handle takes too: its return code, with its message; 0 without a core
  template <typename F>
  int on_core(F&& f) {
    if (!core) return 0;
    const int rc = f(*core);
    if (rc) err = core->err;
    return rc;
  }
  // float32 handle <-> its float64 core: the state blocks (same strides on both sides), psi_{k-1}, u_{k-1}, the warm start, the progress
  int core_push(hipStream_t s) {
    if constexpr (sizeof(T) == 4) {
      const int rc = on_core([&](Impl<double>& c) { return c.ensure_dense(s, true); });
      if (rc) return rc;
      core->prog = prog;  // (both sides' tables name the same psi_{k-1} buffer)
      const Sections mine = sections(blob_header()), cores = core->sections(core->blob_header());
      for (int i = 0; i < mine.n_traj; ++i)
        HIPCHK((launch_cast<float, double>((const float*)mine.s[i].ptr, (double*)cores.s[i].ptr, mine.s[i].count, s)));
      // (psi_k's buffer is no part of a checkpoint, but it has always travelled with the rest)
      HIPCHK((launch_cast<float, double>((const float*)dPsi[prog.cur], core->dPsi[prog.cur], (size_t)L * B, s)));
      core->update_on = update_on; core->cfg.P0 = cfg.P0; core->cfg.barQ0 = cfg.barQ0;
      core->home.dense_overwritten();
    }
    return 0;
  }
  int core_pull(hipStream_t s) {
    if constexpr (sizeof(T) == 4) {
      const int rc = on_core([&](Impl<double>& c) { return c.ensure_dense(s, false); });
      if (rc) return rc;
      prog = core->prog;
      const Sections mine = sections(blob_header()), cores = core->sections(core->blob_header());
      for (int i = 0; i < mine.n_traj; ++i)
        HIPCHK((launch_cast<double, float>((const double*)cores.s[i].ptr, (float*)mine.s[i].ptr, mine.s[i].count, s)));
      HIPCHK((launch_cast<double, float>(core->dPsi[prog.cur], (float*)dPsi[prog.cur], (size_t)L * B, s)));
    }
    return 0;
  }
  // the fast form (wave image / float64 core) is about to be advanced by the roll-out; nothing to do on a handle without one
  int ensure_image(hipStream_t s) {
    if (home.fast_stale()) {
      if constexpr (sizeof(T) == 8) {
        HIPCHK(launch_state_to_image((const double*)dP, sP, (const double*)dK, sK, (const double*)dQ, sQ, (const double*)dC, sC, n, L, B, dImg, sImg, s));
      } else {
        const int rc = core_push(s);
        if (rc) return rc;
      }
    }
    home.fast_taken();
    return 0;
  }

  // (called where the model or the state is replaced from outside: set_model, reset, offline fit, checkpoint import)
  int forget_tableaux(hipStream_t s) {
    if (dQpCarrySet) HIPCHK(hipMemsetAsync(dQpCarrySet, 0, sizeof(int32_t) * (size_t)B * 4, s));
    return 0;
  }

  int set_encoder_layer(int layer, const double* W, const double* b, int rows, int cols) override {
    if (cfg.lift_kind != KMPC_LIFT_MLP) FAIL(-3, "handle was not created with KMPC_LIFT_MLP");
    const int nl = cfg.layers + 1;  // linear layers
    if (layer < 0 || layer >= nl) FAIL(-3, "layer index out of range");
    const int in_dim = layer == 0 ? n : cfg.hidden;
    const int out_dim = layer == nl - 1 ? Lenc : cfg.hidden;
    if (rows != out_dim || cols != in_dim) FAIL(-3, "encoder layer shape does not match the configuration");
    hostW[layer].assign(W, W + (size_t)rows * cols);
    hostb[layer].assign(b, b + rows);
    layer_set[layer] = true;
    packed_ok = false;
    if (const int rc = on_core([&](Impl<double>& c) { return c.set_encoder_layer(layer, W, b, rows, cols); })) return rc;
    for (int k = 0; k < nl; ++k)
      if (!layer_set[k]) return 0;
    return finalize_encoder();
  }
  // every layer is known: upload the network the kernels evaluate (the given one, or the one that realises lift_offset)
  int finalize_encoder() {
    const int nl = cfg.layers + 1, H = cfg.hidden, off = cfg.lift_offset, ex = off == 2 ? 2 * n : 0;
    std::vector<double> psi0((size_t)Lenc, 0.0);
    if (off) {  // psi(0) = W_o relu(... relu(b_1)) + b_o, float64 on the host
      std::vector<double> h(hostb[0]), hn;
      for (double& v : h) v = v > 0.0 ? v : 0.0;
      for (int k = 1; k < nl; ++k) {
        const int rows = k == nl - 1 ? Lenc : H;
        hn.assign((size_t)rows, 0.0);
        for (int r = 0; r < rows; ++r) {
          double acc = hostb[k][r];
          for (int c2 = 0; c2 < H; ++c2) acc += hostW[k][(size_t)r * H + c2] * h[c2];
          hn[r] = (k == nl - 1) ? acc : (acc > 0.0 ? acc : 0.0);
        }
        h.swap(hn);
      }
      psi0 = h;
    }
    int rc;
    for (int k = 0; k < nl; ++k) {
      const bool first = k == 0, last = k == nl - 1;
      const int rin = first ? n : H, rout = last ? Lenc : H;          // the given layer
      const int ein = first ? n : enc.hid, eout = last ? L : enc.hid; // the effective one
      std::vector<double> We((size_t)eout * ein, 0.0), be((size_t)eout, 0.0);
      const int r0 = (last && off == 2) ? n : 0;                       // (the first n output rows are x)
      for (int r = 0; r < rout; ++r) {
        for (int c2 = 0; c2 < rin; ++c2) We[(size_t)(r0 + r) * ein + c2] = hostW[k][(size_t)r * rin + c2];
        be[r0 + r] = hostb[k][r] - (last ? psi0[r] : 0.0);
      }
      if (ex) {
        if (first) {
          for (int i = 0; i < n; ++i) { We[(size_t)(H + i) * ein + i] = 1.0; We[(size_t)(H + n + i) * ein + i] = -1.0; }
        } else if (!last) {
          for (int i = 0; i < ex; ++i) We[(size_t)(H + i) * ein + (H + i)] = 1.0;
        } else {
          for (int i = 0; i < n; ++i) { We[(size_t)i * ein + (H + i)] = 1.0; We[(size_t)i * ein + (H + n + i)] = -1.0; }
        }
      }
      if (first) {
        if ((rc = upload_padded(dW1, We.data(), eout, ein, enc.Hp, 4))) return rc;
        if ((rc = upload_padded(db1, be.data(), 1, eout, 1, enc.Hp))) return rc;
      } else if (last) {
        if ((rc = upload_padded(dWo, We.data(), eout, ein, enc.Lp, enc.Hp))) return rc;
        if ((rc = upload_padded(dbo, be.data(), 1, eout, 1, enc.Lp))) return rc;
      } else {
        if ((rc = upload_padded(dWh[k - 1], We.data(), eout, ein, enc.Hp, enc.Hp))) return rc;
        if ((rc = upload_padded(dbh[k - 1], be.data(), 1, eout, 1, enc.Hp))) return rc;
      }
    }
    packed_ok = false;
    return 0;
  }

  int set_centres(const double* cx, int L_, int n_) override {
    if (cfg.lift_kind == KMPC_LIFT_MLP) FAIL(-3, "handle was created with KMPC_LIFT_MLP");
    if (L_ != L || n_ != n) FAIL(-3, "centre shape does not match the configuration");
    int rc = upload_padded(dcx, cx, L, n, L, n);
    if (rc) return rc;
    if ((rc = on_core([&](Impl<double>& c) { return c.set_centres(cx, L_, n_); }))) return rc;
    centres_set = true;
    return 0;
  }
  // the polyharmonic coefficient k of rbf.m:38, for every later call of every route (it travels with the launch arguments)
  int set_rbf_order(int k) override {
    if (cfg.lift_kind != KMPC_LIFT_RBF_POLYHARMONIC) FAIL(-3, "handle was not created with KMPC_LIFT_RBF_POLYHARMONIC");
    if (k < 1 || k > 8) FAIL(-3, "the polyharmonic coefficient k must be an integer in 1..8");
    if (const int rc = on_core([&](Impl<double>& c) { return c.set_rbf_order(k); })) return rc;
    rbf_k = k;
    return 0;
  }

  int set_model(const double* A, const double* Bm, const double* C) override {
    std::vector<T> k((size_t)L * p);
    for (int r = 0; r < L; ++r) {
      for (int c2 = 0; c2 < L; ++c2) k[(size_t)r * p + c2] = (T)A[(size_t)r * L + c2];
      k[(size_t)r * p + L] = (T)Bm[r];
    }
    // (a roll-out enqueued on a non-blocking stream may still be writing the wave image: the null-stream conversion below does
    //  not wait for such a stream by itself)
    { int rc = sync_own(); if (rc) return rc; }
    { int rc = ensure_dense(nullptr, true); if (rc) return rc; }
    { int rc = forget_tableaux(nullptr); if (rc) return rc; }
    HIPCHK(hipMemcpy(dTmp, k.data(), k.size() * sizeof(T), hipMemcpyHostToDevice));
    HIPCHK(launch_broadcast<T>(dK, sK, dTmp, L * p, B, nullptr));
    if (cfg.output_kind == KMPC_OUT_CX) {
      if (!C) FAIL(-3, "C is required for KMPC_OUT_CX");
      std::vector<T> c((size_t)n * L);
      for (size_t i = 0; i < c.size(); ++i) c[i] = (T)C[i];
      HIPCHK(hipMemcpy(dTmp + L * p, c.data(), c.size() * sizeof(T), hipMemcpyHostToDevice));
      HIPCHK(launch_broadcast<T>(dC, sC, dTmp + L * p, n * L, B, nullptr));
    }
    if (dKs) {
      HIPCHK(hipMemcpy(dKs, dK, sizeof(T) * (size_t)L * p, hipMemcpyDeviceToDevice));
      HIPCHK(hipMemcpy(dCs, dC, sizeof(T) * (size_t)n * L, hipMemcpyDeviceToDevice));
    }
    HIPCHK(hipStreamSynchronize(nullptr));
    return 0;
  }

  // (a float32 handle's float64 core gets the block this handle itself works with -- PN - Qw I rounded to float32 -- so that the
  //  fused roll-outs, the per-step entry points and a checkpoint loaded into another handle all use the same weight: core_weight)
  int core_weight(const std::vector<T>* w) {
    std::vector<double> pn;
    if (w) pn = pn_from_block(*w, cfg.Qw);
    return on_core([&](Impl<double>& c) { return c.set_terminal_weight(w ? pn.data() : nullptr); });
  }
  // the block the kernels add to Q_bar's last diagonal block, P_N - Qw I in the handle's dtype, and P_N back from it
  std::vector<T> block_from_pn(const double* PN, double Qw) const {
    std::vector<T> w((size_t)q * q);
    for (int r = 0; r < q; ++r)
      for (int c2 = 0; c2 < q; ++c2) w[(size_t)r * q + c2] = (T)(PN[(size_t)r * q + c2] - (r == c2 ? Qw : 0.0));
    return w;
  }
  std::vector<double> pn_from_block(const std::vector<T>& w, double Qw) const {
    std::vector<double> pn(w.size());
    for (int r = 0; r < q; ++r)
      for (int c2 = 0; c2 < q; ++c2) pn[(size_t)r * q + c2] = (double)w[(size_t)r * q + c2] + (r == c2 ? Qw : 0.0);
    return pn;
  }
  // the handle's terminal block(s) as the kernels read them; null: none
  T* wterm_ptr() const { return wterm == Term::None ? nullptr : (term_from_dare(wterm) ? (T*)dWtB.get() : dWt.get()); }
  int32_t wterm_block_count(Term t) const { return t == Term::None ? 0 : (t == Term::DarePerTraj ? B : 1); }
  // every trajectory gets the one block w0 ([q q]) as its own Riccati block: dWtB becomes [B][q q]
  int spread_block(const std::vector<double>& w0) {
    { int rc = dare_buffers(B); if (rc) return rc; }
    std::vector<double> wb((size_t)B * q * q);
    for (int b = 0; b < B; ++b) std::copy(w0.begin(), w0.end(), wb.begin() + (size_t)b * q * q);
    HIPCHK(hipMemcpy(dWtB, wb.data(), sizeof(double) * wb.size(), hipMemcpyHostToDevice));
    return 0;
  }
  int set_terminal_weight(const double* PN) override {
    if (!PN) { wterm = Term::None; hostPN.clear(); return core_weight(nullptr); }
    const std::vector<T> w = block_from_pn(PN, cfg.Qw);
    { const int rc = core_weight(&w); if (rc) return rc; }
    HIPCHK(dWt.ensure((size_t)q * q));
    HIPCHK(hipMemcpy(dWt, w.data(), w.size() * sizeof(T), hipMemcpyHostToDevice));
    hostPN.assign(PN, PN + (size_t)q * q);
    wterm = Term::Given;
    return 0;
  }

  // Terminal block from the Riccati iteration of the reference (solve_DARE, duffing.py:583-598) on this handle's
  // model(s): P = DARE(A, B, Q_lift, R), Q_bar(end) = Co P Co' (Koopman_update.m:381).  per_traj = 0: the model of
  // trajectory 0 (after kmpc_set_model / kmpc_offline_fit every trajectory holds that one) gives ONE block for the
  // batch; per_traj = 1: every trajectory's current [A B], C gives its own block (the MATLAB controller recomputes
  // its terminal ingredients with the updated model, Koopman_update.m:215, 276-281).
  int terminal_from_dare(const double* Qh, double R, int maxiter, double eps, int per_traj, double* PN_out,
                         int32_t* iters_out, hipStream_t s) override {
    if constexpr (sizeof(T) != 8) {
      FAIL(-2, "kmpc_terminal_from_dare: float64 handles only (the reference's Riccati iteration is float64)");
    } else {
      if (!Qh || maxiter < 1) FAIL(-3, "kmpc_terminal_from_dare: bad arguments");
      const int nb = per_traj ? B : 1;
      if (nb == 0) return 0;
      { int rc = ensure_dense(s, false); if (rc) return rc; }
      DevBuf<double> dQl;
      HIPCHK(dQl.alloc((size_t)L * L));
      HIPCHK(hipMemcpyAsync(dQl, Qh, sizeof(double) * (size_t)L * L, hipMemcpyHostToDevice, s));
      { int rc = dare_buffers(nb); if (rc) return rc; }
      { int rc = dare_blocks(nb, dQl, R, maxiter, eps, s); if (rc) return rc; }
      if (PN_out || iters_out) {
        HIPCHK(hipStreamSynchronize(s));
        if (PN_out) {
          HIPCHK(hipMemcpy(PN_out, dWtB, sizeof(double) * (size_t)nb * q * q, hipMemcpyDeviceToHost));
          for (int m = 0; m < nb; ++m)
            for (int r = 0; r < q; ++r) PN_out[((size_t)m * q + r) * q + r] += cfg.Qw;  // hand back P_N, not P_N - Qw I
        }
        if (iters_out) HIPCHK(hipMemcpy(iters_out, dDareIt, sizeof(int32_t) * (size_t)nb, hipMemcpyDeviceToHost));
      }
      HIPCHK(hipStreamSynchronize(s));
      wterm = per_traj ? Term::DarePerTraj : Term::DareOne;
      return 0;
    }
  }

  // Riccati workspace and the terminal block(s) for nb models (kmpc_terminal_from_dare, kmpc_set_terminal_refresh, kmpc_state_import):
  // all three blocks grow or none does; their contents are not kept
  int dare_buffers(int nb) {
    if (dare_cap >= nb) return 0;
    HIPCHK(replace_together(dDareP, (size_t)nb * L * L, dDareIt, (size_t)nb, dWtB, (size_t)nb * q * q));
    dare_cap = nb;
    return 0;
  }
  // P = DARE(A, B, Qdev, R) of the first nb trajectories' current [A B] and their blocks Co P Co' - Qw I -> dWtB   (dare_kernel)
  int dare_blocks(int nb, const double* Qdev, double R, int maxiter, double eps, hipStream_t s) {
    if constexpr (sizeof(T) == 8) {
      // y = psi (lifted output): Co = I, the block is P itself; y = C x: rows cy0 .. cy0+q-1 of C
      const bool lift_out = cfg.output_kind == KMPC_OUT_LIFT;
      if (lift_out && !dEyeL) {
        std::vector<double> eye((size_t)L * L, 0.0);
        for (int i = 0; i < L; ++i) eye[(size_t)i * L + i] = 1.0;
        HIPCHK(dEyeL.alloc((size_t)L * L));
        HIPCHK(hipMemcpy(dEyeL, eye.data(), sizeof(double) * (size_t)L * L, hipMemcpyHostToDevice));
      }
      DareArgs d{};
      d.nb = nb; d.L = L; d.q = q; d.maxiter = maxiter; d.shared_model = 0;
      d.A = (const double*)dK; d.strideA = sK; d.ldA = p;
      d.B = (const double*)dK + L; d.strideB = sK; d.incB = p;
      d.Q = Qdev; d.R = R; d.eps = eps;
      d.Co = lift_out ? dEyeL.get() : (const double*)dC + (size_t)cfg.out_row0 * L;
      d.strideC = lift_out ? 0 : sC;
      d.P = dDareP; d.K = nullptr; d.PN = dWtB; d.pn_sub_diag = cfg.Qw; d.iters = dDareIt;
      HIPCHK(launch_dare(d, s));
    }
    return 0;
  }

  // kmpc_set_terminal_refresh (what it does: the comment at term_every)
  int set_terminal_refresh(int every, const double* Qh, double R, int maxiter, double eps) override {
    if constexpr (sizeof(T) != 8) {
      FAIL(-2, "kmpc_set_terminal_refresh: float64 handles only (the reference's Riccati iteration is float64)");
    } else {
      if (every < 0 || (every > 0 && (!Qh || maxiter < 1))) FAIL(-3, "kmpc_set_terminal_refresh: bad arguments");
      if (every == 0) {
        term_every = 0;
        if (diag_on) (void)load_diag_plugins();  // (diagnostics armed while the refresh was on: now the variant without it)
        return 0;
      }
      { int rc = sync_own(); if (rc) return rc; }
      std::vector<double> w0((size_t)q * q, 0.0);  // the block every trajectory holds until its first refresh: the current one, else Qw I
      if (wterm == Term::Given || wterm == Term::DareOne)
        HIPCHK(hipMemcpy(w0.data(), wterm_ptr(), sizeof(double) * w0.size(), hipMemcpyDeviceToHost));
      if (!(wterm == Term::DarePerTraj && dare_cap >= B)) { int rc = spread_block(w0); if (rc) return rc; }
      HIPCHK(dTermQ.ensure((size_t)L * L));
      HIPCHK(hipMemcpy(dTermQ, Qh, sizeof(double) * (size_t)L * L, hipMemcpyHostToDevice));
      wterm = Term::DarePerTraj;
      term_R = R; term_maxiter = maxiter; term_eps = eps; term_count = 0;
      // the fused roll-out of this configuration with the refresh inside: a plug-in of its own (also for the built-in dimension sets)
      variant[1][0].state = 0;
      if (fused_dims_ok()) load_variant(true, false);
      if (variant[1][0].state > 0) HIPCHK(dTermScr.ensure((size_t)B * term_scratch_elems(L)));
      term_every = every;
      if (diag_on) (void)load_diag_plugins();  // (diagnostics armed before the refresh: the variant that has both)
      return 0;
    }
  }

  // the DIAG variant this handle needs now (asked for once); 0: the fused route is ready, 1: per-step launches
  int load_diag_plugins() {
    if constexpr (sizeof(T) == 8) {
      if (!(fused_dims_ok() && use_img)) return 1;
      const bool term = term_every > 0 && variant[1][0].state > 0;
      if (variant[term][1].state == 0 && !load_variant(term, true)) {
        variant[term][1].state = -1;
        diag_msg() = "no diagnostics variant of the fused roll-out for this configuration";
      }
      return diag_fused_ready() ? 0 : 1;
    }
    return 1;
  }
  // kmpc_estimator_status: bit 0 a previous transition exists (the next step runs an update), bit 1 that update would be the FIRST one
  // after a restart (K_A = 0, bar_X = 0, inv_K_G = P0 I, bar_Q = barQ0 I); nothing is touched, nothing is waited for
  int estimator_status(double* P0o, double* barQ0o) const override {
    if (P0o) *P0o = cfg.P0;
    if (barQ0o) *barQ0o = cfg.barQ0;
    return (prog.have_prev ? 1 : 0) | ((prog.rls_fresh && update_on) ? 2 : 0);
  }
  // kmpc_get_prev_transition: copies of psi(x_{k-1}) ([B][L]) and u_{k-1} ([B]) the next update will regress on (stream-ordered, read-only)
  int get_prev_transition(void* psi_prev, void* u_prev, hipStream_t s) override {
    if (core) FAIL(-2, "kmpc_get_prev_transition: float64 handles only");
    if (psi_prev) HIPCHK(hipMemcpyAsync(psi_prev, dPsi[prog.cur ^ 1], sizeof(T) * (size_t)L * B, hipMemcpyDeviceToDevice, s));
    if (u_prev) HIPCHK(hipMemcpyAsync(u_prev, dUprev, sizeof(T) * (size_t)B, hipMemcpyDeviceToDevice, s));
    return 0;
  }
  bool diag_fused_ready() const { return diag_on && use_img && variant_of(true).state > 0; }
  int set_rollout_diagnostics(int on) override {
    if constexpr (sizeof(T) != 8) {
      FAIL(-2, "kmpc_set_rollout_diagnostics: float64 handles only (the norms come out of the float64 update)");
    } else {
      if (on == 0) { diag_on = false; return 0; }
      if (cfg.lambda != 1.0) FAIL(-2, "kmpc_set_rollout_diagnostics: needs lambda = 1 -- with a forgetting factor the change of the model is not rank one (Koopman_update.m:270-274)");
      if (shared_has_samples) FAIL(-2, "kmpc_set_rollout_diagnostics: this handle runs the shared-model loop -- one Gram-solved model is not a rank-one update");
      diag_on = true;
      const int route = load_diag_plugins();
      if (route == 0 && fused_rollout_ok()) return 0;
      if (route != 0) err = "diagnostics through per-step launches: " + (diag_msg().empty() ? std::string("this configuration has no register-state fused roll-out") : diag_msg());
      else err = "diagnostics through per-step launches: the handle's roll-out is not fused";
      return 1;
    }
  }
  int rollout_diag(int plant, void* X, const void* ref, int rpt, int steps, int step0, int switch_step, double hs, void* Ulog, void* Xlog,
                   void* Psilog, void* dAlog, void* dBlog, void* dClog, int32_t* st, int32_t* it, hipStream_t s) override {
    if (!diag_on) FAIL(-3, "kmpc_rollout_diag: kmpc_set_rollout_diagnostics(h, 1) has not succeeded on this handle");
    const DiagLogs logs{Psilog, dAlog, dBlog, dClog};
    StepCtx ctx;
    ctx.diag = &logs;
    return rollout_impl(ctx, plant, X, ref, rpt, steps, step0, switch_step, hs, Ulog, Xlog, st, it, s);
  }
  // per-step route: psi(x_k) into the handle's buffer (the step computes the same values again), then the diagnostics of the update the
  // step is about to make, from the dense blocks as they are before it
  int diag_before_step(const DiagLogs& lg, const void* X, int i, hipStream_t s) {
    if constexpr (sizeof(T) == 8) {
      int rc = ensure_dense(s, true);
      if (rc) return rc;
      if ((rc = lift_to((const T*)X, dPsi[prog.cur], 1, L, B, s))) return rc;
      RlsDiagArgs d{};
      d.B = B; d.n = n; d.L = L;
      d.has_update = (prog.have_prev && update_on) ? 1 : 0; d.first_update = prog.rls_fresh ? 1 : 0; d.use_C = cfg.output_kind == KMPC_OUT_CX ? 1 : 0;
      d.P = (const double*)dP; d.strideP = sP; d.K = (const double*)dK; d.strideK = sK; d.Qb = (const double*)dQ; d.strideQ = sQ;
      d.C = (const double*)dC; d.strideC = sC;
      d.psi_prev = (const double*)dPsi[prog.cur ^ 1]; d.psi_now = (const double*)dPsi[prog.cur]; d.u_prev = (const double*)dUprev; d.x_now = (const double*)X;
      d.Psi_row = lg.Psi ? (double*)lg.Psi + (size_t)i * L * B : nullptr;
      d.dA_row = lg.dA ? (double*)lg.dA + (size_t)i * B : nullptr;
      d.dB_row = lg.dB ? (double*)lg.dB + (size_t)i * B : nullptr;
      d.dC_row = lg.dC ? (double*)lg.dC + (size_t)i * B : nullptr;
      HIPCHK(launch_rls_diag(d, s));
    }
    return 0;
  }

  int reset(hipStream_t s) override {
    if (dGram) HIPCHK(hipMemsetAsync(dGram, 0, sizeof(double) * (size_t)gram_elems(), s));
    shared_has_samples = false;
    { int rc = ensure_dense(s, true); if (rc) return rc; }
    { int rc = forget_tableaux(s); if (rc) return rc; }
    HIPCHK(launch_fill_state<T>(dP, sP, p, (T)cfg.P0, dQ, sQ, L, (T)cfg.barQ0, nullptr, sK, nullptr, sC, n, B, s));
    HIPCHK(hipMemsetAsync(dWarm, 0, sizeof(T) * (size_t)N * B, s));  // first solve starts at clip(0) like the reference's (duffing.py:634-635)
    prog = Progress{};
    return 0;
  }

  // kmpc_state_init: the reference's start of the online update (duffing.py:927-930, 944-946) with the given scales
  int state_init(double P0, double barQ0, hipStream_t s) override {
    if (!(P0 > 0.0) || !(barQ0 > 0.0)) FAIL(-3, "kmpc_state_init: the scales must be positive");
    cfg.P0 = P0; cfg.barQ0 = barQ0;
    return reset(s);
  }
  // kmpc_state_init_from: every trajectory continues from given reference-form accumulators (the MATLAB start from the
  // offline Gram, Koopman_update.m:264-265): K_A0 (L x p), inv_K_G = P0 (p x p), bar_X0 (n x L), bar_Q0 (L x L), host,
  // row-major.  The handle keeps the gain form: K = K_A0 P0 (duffing.py:938), C = bar_X0 bar_Q0 (duffing.py:953).
  int state_init_from(const double* KA0, const double* P0m, const double* barX0, const double* barQ0m, hipStream_t s) override {
    if (!KA0 || !P0m || !barQ0m || (cfg.output_kind == KMPC_OUT_CX && !barX0)) FAIL(-3, "kmpc_state_init_from: bad arguments");
    int rc = reset(s);
    if (rc) return rc;
    std::vector<T> hP((size_t)p * p), hQ((size_t)L * L), hK((size_t)L * p), hC((size_t)n * L, T(0));
    for (size_t i = 0; i < hP.size(); ++i) hP[i] = (T)P0m[i];
    for (size_t i = 0; i < hQ.size(); ++i) hQ[i] = (T)barQ0m[i];
    for (int r = 0; r < L; ++r)
      for (int c2 = 0; c2 < p; ++c2) {
        double acc = 0.0;
        for (int k = 0; k < p; ++k) acc += KA0[(size_t)r * p + k] * P0m[(size_t)k * p + c2];
        hK[(size_t)r * p + c2] = (T)acc;
      }
    if (cfg.output_kind == KMPC_OUT_CX)
      for (int r = 0; r < n; ++r)
        for (int c2 = 0; c2 < L; ++c2) {
          double acc = 0.0;
          for (int k = 0; k < L; ++k) acc += barX0[(size_t)r * L + k] * barQ0m[(size_t)k * L + c2];
          hC[(size_t)r * L + c2] = (T)acc;
        }
    DevBuf<T> tmp;
    HIPCHK(tmp.alloc(hP.size() + hQ.size() + hK.size() + hC.size()));
    T* tP = tmp; T* tQ = tP + hP.size(); T* tK = tQ + hQ.size(); T* tC = tK + hK.size();
    HIPCHK(hipMemcpyAsync(tP, hP.data(), sizeof(T) * hP.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(tQ, hQ.data(), sizeof(T) * hQ.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(tK, hK.data(), sizeof(T) * hK.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(tC, hC.data(), sizeof(T) * hC.size(), hipMemcpyHostToDevice, s));
    HIPCHK(launch_broadcast<T>(dP, sP, tP, p * p, B, s));
    HIPCHK(launch_broadcast<T>(dQ, sQ, tQ, L * L, B, s));
    HIPCHK(launch_broadcast<T>(dK, sK, tK, L * p, B, s));
    if (cfg.output_kind == KMPC_OUT_CX) HIPCHK(launch_broadcast<T>(dC, sC, tC, n * L, B, s));
    if (dKs) HIPCHK(hipMemcpyAsync(dKs, tK, sizeof(T) * (size_t)L * p, hipMemcpyDeviceToDevice, s));
    if (dCs) HIPCHK(hipMemcpyAsync(dCs, tC, sizeof(T) * (size_t)n * L, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    prog.rls_fresh = false;  // the first online update continues from these accumulators
    return 0;
  }

  int check_lift_ready() {
    if (cfg.lift_kind == KMPC_LIFT_MLP) {
      for (size_t i = 0; i < layer_set.size(); ++i)
        if (!layer_set[i]) FAIL(-4, "encoder layer " + std::to_string(i) + " has not been set");
    } else if (!centres_set) {
      FAIL(-4, "RBF centres have not been set");
    }
    return 0;
  }

  // the MLP encoder's fields of a lift launch: the layers and (packed now if need be) their MFMA fragments
  int encoder_args(LiftArgs<T>& a, hipStream_t s) {
    a.W1 = dW1; a.b1 = db1; a.Wh[0] = dWh[0]; a.Wh[1] = dWh[1]; a.bh[0] = dbh[0]; a.bh[1] = dbh[1];
    a.Wo = dWo; a.bo = dbo; a.Hp = enc.Hp; a.Lp = enc.Lp;
    const int rc = pack_encoder(s);
    if (rc) return rc;
    a.Whp[0] = dWhp[0]; a.Whp[1] = dWhp[1] ? dWhp[1] : dWhp[0]; a.Wop = dWop; a.KSp = enc.KS;
    return 0;
  }
  int lift_to(const T* X, T* Psi, long ps_l, long ps_b, int Bc, hipStream_t s) {
    int rc = check_lift_ready();
    if (rc) return rc;
    LiftArgs<T> a{};
    a.B = Bc; a.n = n; a.L = L; a.hidden = enc.hid; a.nlayers = cfg.layers;
    a.X = X; a.Psi = Psi; a.ps_l = ps_l; a.ps_b = ps_b;
    if (cfg.lift_kind == KMPC_LIFT_MLP) {
      if ((rc = encoder_args(a, s))) return rc;
      HIPCHK(launch_lift_mlp<T>(a, s));
    } else {
      a.cx = dcx; a.eps = (T)cfg.rbf_eps; a.rbf_matlab = rbf_code();
      HIPCHK(launch_lift_rbf<T>(a, s));
    }
    return 0;
  }

  int lift(const void* X, void* Psi, int Bc, hipStream_t s) override {
    if (Bc == 0) return 0;  // empty batch: nothing to do
    if (Bc < 0 || !X || !Psi) FAIL(-3, "kmpc_lift: bad arguments");
    return lift_to((const T*)X, (T*)Psi, Bc, 1, Bc, s);
  }

  StepArgs<T> base_args(int Bc) {
    StepArgs<T> a{};
    a.B = Bc; a.n = n; a.L = L; a.q = q; a.N = N;
    a.out_kind = cfg.output_kind == KMPC_OUT_LIFT ? OUT_LIFT : OUT_CX;
    a.max_iter = cfg.qp_max_iter > 0 ? cfg.qp_max_iter : 8 * N + 40;
    a.P = dP; a.strideP = sP; a.K = dK; a.strideK = sK; a.Qb = dQ; a.strideQ = sQ; a.C = dC; a.strideC = sC;
    a.Wterm = wterm_ptr();
    a.wterm_per_traj = wterm == Term::DarePerTraj ? 1 : 0;
    a.lam = (T)cfg.lambda; a.Qw = (T)cfg.Qw; a.Rw = (T)cfg.Rw; a.lb = (T)cfg.lb; a.ub = (T)cfg.ub;
    a.du_mode = cfg.delta_u ? 1 : 0;
    a.cy0 = cfg.output_kind == KMPC_OUT_LIFT ? 0 : cfg.out_row0;
    a.c_skip_first = cfg.c_skip_first ? 1 : 0;
    a.umin = (T)cfg.umin; a.umax = (T)cfg.umax;
    a.u_prev = dUprev;  // delta-u reads the absolute previous input in every phase
    a.qp_scratch = dQpScr;
    static const int predict = dbg_env("KMPC_QP_PREDICT") ? atoi(dbg_env("KMPC_QP_PREDICT")) : 1;  // measurement aid: 0 = plain projected Newton
    a.qp_predict = predict;
    a.plant = -1;
    return a;
  }
  // a step that also advances every trajectory's plant with its u_k (the roll-outs, kmpc_shared_solve_plant)
  void plant_args(StepArgs<T>& a, const StepCtx& ctx) {
    if (ctx.plant >= 0) { a.plant = ctx.plant; a.plant_switched = ctx.switched; a.plant_h = (T)ctx.h; a.X_rw = (T*)ctx.X_rw; }
  }

  int rls_update(const void* psi, const void* u, const void* psin, const void* xn, int Bc, hipStream_t s) override {
    if (Bc != B) FAIL(-3, "kmpc_rls_update: B must equal the handle's batch (the state is per trajectory)");
    if (!psi || !u || !psin || !xn) FAIL(-3, "kmpc_rls_update: null pointer");
    { int rc = ensure_dense(s, true); if (rc) return rc; }
    StepArgs<T> a = base_args(Bc);
    a.phases = PH_RLS;
    a.first_update = prog.rls_fresh ? 1 : 0;
    a.psi_prev = (const T*)psi; a.pp_sl = Bc; a.pp_sb = 1;
    a.psi_now = (const T*)psin; a.pn_sl = Bc; a.pn_sb = 1;
    a.u_prev = (const T*)u; a.x_now = (const T*)xn;
    HIPCHK(launch_step<T>(a, threads, s));
    prog.rls_fresh = false;
    return 0;
  }

  int get_model(void* A, void* Bm, void* C, hipStream_t s) override {
    { int rc = ensure_dense(s, false); if (rc) return rc; }
    HIPCHK(launch_export_model<T>(dK, sK, cfg.output_kind == KMPC_OUT_CX ? dC : nullptr, sC, n, L, B, (T*)A, (T*)Bm,
                                  (T*)C, s));
    return 0;
  }

  int condense(const void* psi, const void* ref, int rpt, void* H, void* f, void* c, int Bc, hipStream_t s) override {
    if (Bc != B) FAIL(-3, "kmpc_condense: B must equal the handle's batch");
    if (!psi || !ref || !H || !f) FAIL(-3, "kmpc_condense: null pointer");
    { int rc = ensure_dense(s, false); if (rc) return rc; }
    StepArgs<T> a = base_args(Bc);
    a.phases = PH_CONDENSE;
    a.psi_now = (const T*)psi; a.pn_sl = Bc; a.pn_sb = 1;
    a.ref = (const T*)ref; a.ref_per_traj = rpt;
    a.H_out = (T*)H; a.f_out = (T*)f; a.c_out = (T*)c;
    HIPCHK(launch_step<T>(a, threads, s));
    return 0;
  }

  // kmpc_mpc_solve: the solve wrapper with the model as an argument; scratch model blocks, H, f, c are the handle's
  int mpc_solve(const void* A, const void* Bv, const void* C, int shared, const void* psi, const void* ref, int rpt,
                double lb_, double ub_, double Qw_, double Rw_, const double* PN, void* U, void* U0, void* fun,
                int32_t* st, int32_t* it, int Bc, hipStream_t s) override {
    if (Bc != B) FAIL(-3, "kmpc_mpc_solve: B must equal the handle's batch");
    if (!A || !Bv || !psi || !ref || !U) FAIL(-3, "kmpc_mpc_solve: null pointer");
    if (cfg.output_kind == KMPC_OUT_CX && !C) FAIL(-3, "kmpc_mpc_solve: C is required for KMPC_OUT_CX");
    if (cfg.delta_u) FAIL(-3, "kmpc_mpc_solve: not available in the delta-u form (its state includes the handle's u_prev)");
    if (!(ub_ > lb_)) FAIL(-3, "kmpc_mpc_solve: need lb < ub");
    HIPCHK(dMsK.ensure((size_t)sK * B));  // (each on its own: a call that failed half-way leaves nothing the next one trips over)
    HIPCHK(dMsC.ensure((size_t)sC * B));
    HIPCHK(dMsH.ensure((size_t)B * N * N));
    HIPCHK(dMsf.ensure((size_t)B * N));
    HIPCHK(dMsc.ensure((size_t)B));
    HIPCHK(dMsW.ensure((size_t)q * q));
    HIPCHK(launch_import_model<T>((const T*)A, (const T*)Bv, (const T*)C, shared, n, L, B, dMsK, sK,
                                  cfg.output_kind == KMPC_OUT_CX ? dMsC : nullptr, sC, s));
    if (PN) {
      const std::vector<T> w = block_from_pn(PN, Qw_);
      HIPCHK(hipMemcpyAsync(dMsW, w.data(), w.size() * sizeof(T), hipMemcpyHostToDevice, s));
      HIPCHK(hipStreamSynchronize(s));  // (the host vector goes out of scope)
    }
    StepArgs<T> a = base_args(B);
    a.K = dMsK; a.C = dMsC;
    a.lb = (T)lb_; a.ub = (T)ub_; a.Qw = (T)Qw_; a.Rw = (T)Rw_;
    // the terminal block: P_N of this call, else the handle's (kmpc_set_terminal_weight / kmpc_terminal_from_dare), as
    // kmpc_condense and kmpc_step use it -- the same cost on every route through the handle
    if (PN) { a.Wterm = dMsW; a.wterm_per_traj = 0; }
    else if (wterm != Term::None && Qw_ != cfg.Qw) {
      if (term_from_dare(wterm) || hostPN.empty()) FAIL(-3, "kmpc_mpc_solve: the handle's terminal block was formed with the handle's Q; pass P_N with another Q");
      const std::vector<T> w = block_from_pn(hostPN.data(), Qw_);
      HIPCHK(hipMemcpyAsync(dMsW, w.data(), w.size() * sizeof(T), hipMemcpyHostToDevice, s));
      HIPCHK(hipStreamSynchronize(s));
      a.Wterm = dMsW; a.wterm_per_traj = 0;
    }
    a.phases = PH_CONDENSE | PH_QP;
    a.psi_now = (const T*)psi; a.pn_sl = B; a.pn_sb = 1;
    a.ref = (const T*)ref; a.ref_per_traj = rpt;
    a.H_out = fun ? dMsH : nullptr; a.f_out = fun ? dMsf : nullptr; a.c_out = fun ? dMsc : nullptr;
    a.Useq = (T*)U; a.U0 = (T*)U0; a.status = st; a.iters = it;
    HIPCHK(launch_step<T>(a, threads, s));
    if (fun) HIPCHK(launch_qp_value<T>(dMsH, dMsf, dMsc, (const T*)U, N, B, (T*)fun, s));
    return 0;
  }

  int generate_and_fit(int plant, const void* X0, const void* U, int n_traj, int n_steps, double hs, double ridge,
                       int init_rls, void* A, void* Bm, void* C, void* Xo, void* Yo, hipStream_t s) override {
    if (!X0 || !U || n_traj < 1 || n_steps < 1) FAIL(-3, "kmpc_generate_and_fit: bad arguments");
    if (n != 2) FAIL(-3, "plants are two-state systems");
    if (!plant_id_ok(plant)) FAIL(-3, "unknown plant");
    const size_t M = (size_t)n_traj * n_steps;
    DevBuf<T> gx, gy;  // the panels the caller did not ask for
    if (!Xo) HIPCHK(gx.alloc(2 * M));
    if (!Yo) HIPCHK(gy.alloc(2 * M));
    T* Xp = Xo ? (T*)Xo : gx.get(); T* Yp = Yo ? (T*)Yo : gy.get();
    int rc = 0;
    hipError_t e = launch_datagen<T>(plant, (T)hs, (const T*)X0, (const T*)U, n_traj, n_steps, Xp, Yp, s);
    if (e != hipSuccess) { err = std::string("kmpc_generate_and_fit: ") + hipGetErrorString(e); rc = -(int)(1000 + (int)e); }
    if (!rc) rc = offline_fit(Xp, Yp, U, (int)M, ridge, init_rls, A, Bm, C, s);  // (synchronises the stream before it returns)
    return rc;
  }

  int qp_solve(const void* H, const void* f, void* U, int32_t* st, int32_t* it, int Bc, hipStream_t s) override {
    if (Bc == 0) return 0;  // empty batch: nothing to do
    if (Bc < 0 || !H || !f || !U) FAIL(-3, "kmpc_qp_solve: bad arguments");
    if (cfg.delta_u && Bc != B) FAIL(-3, "kmpc_qp_solve: with delta_u the batch must equal the handle's (per-trajectory u_prev)");
    if ((size_t)Bc * N * N > dQpScr.capacity()) {  // (a stateless solve may bring a larger batch than the handle's)
      HIPCHK(hipStreamSynchronize(s));
      HIPCHK(dQpScr.grow((size_t)Bc * N * N));
    }
    StepArgs<T> a = base_args(Bc);
    a.phases = PH_QP;
    a.H_in = (const T*)H; a.f_in = (const T*)f;
    a.Useq = (T*)U; a.status = st; a.iters = it;
    HIPCHK(launch_step<T>(a, threads, s));
    return 0;
  }

  // profiling: one event triple per recorded launch sequence -- its begin, behind its lift (at once where the kernel lifts itself), its end
  int prof_begin(hipStream_t s, bool* rec) {
    *rec = prof && ev_used + 3 <= EV_CAP;
    if (!*rec) return 0;
    while (ev.size() < ev_used + 3) {
      hipEvent_t e;
      HIPCHK(hipEventCreate(&e));
      ev.push_back(e);
    }
    HIPCHK(hipEventRecord(ev[ev_used], s));
    return 0;
  }
  int prof_mid(hipStream_t s) {
    HIPCHK(hipEventRecord(ev[ev_used + 1], s));
    return 0;
  }
  int prof_end(hipStream_t s, int steps) {
    HIPCHK(hipEventRecord(ev[ev_used + 2], s));
    ev_used += 3;
    prof_steps += steps;
    return 0;
  }

  int step(const void* X, const void* ref, int rpt, void* U0, void* Useq, int32_t* st, int32_t* it, hipStream_t s) override {
    return step_impl(StepCtx{}, X, ref, rpt, U0, Useq, st, it, s);
  }
  int step_impl(const StepCtx& ctx, const void* X, const void* ref, int rpt, void* U0, void* Useq, int32_t* st, int32_t* it, hipStream_t s) {
    if (!X || !ref || !U0) FAIL(-3, "kmpc_step: null pointer");
    // Configurations with a fused roll-out instantiation and the MLP lift take ONE launch for the step as well: the
    // roll-out kernel with a single step and no plant (encoder inside on MFMA, no separate lift kernel, psi handed
    // over in registers).  Same results up to the summation order of the encoder.
    if (sizeof(T) == 8 && ctx.plant < 0 && !ctx.accumulate && cfg.lift_kind == KMPC_LIFT_MLP && fused_rollout_ok()) {
      static const bool two = dbg_env("KMPC_STEP_TWO_KERNELS") != nullptr;  // measurement aid
      if (!two)
        return rollout_fused(ctx, -1, const_cast<void*>(X), ref, rpt, 1, 0, -1, 0.05, nullptr, nullptr, st, it, s, U0, Useq);
    }
    bool rec;
    int rc = prof_begin(s, &rec);
    if (rc) return rc;
    if ((rc = ensure_dense(s, true))) return rc;  // (first: on a float32 handle the ping-pong index follows the core's)
    T* psi_now = dPsi[prog.cur];
    T* psi_prev = dPsi[prog.cur ^ 1];
    if ((rc = lift_to((const T*)X, psi_now, 1, L, B, s))) return rc;
    if (rec && (rc = prof_mid(s))) return rc;
    StepArgs<T> a = base_args(B);
    a.phases = PH_CONDENSE | PH_QP | ((prog.have_prev && update_on) ? PH_RLS : 0);
    a.first_update = prog.rls_fresh ? 1 : 0;
    a.psi_prev = psi_prev; a.pp_sl = 1; a.pp_sb = L;
    a.psi_now = psi_now; a.pn_sl = 1; a.pn_sb = L;
    a.u_prev = dUprev; a.x_now = (const T*)X;
    a.ref = (const T*)ref; a.ref_per_traj = rpt;
    a.U0 = (T*)U0; a.Useq = (T*)Useq; a.u_store = dUprev; a.status = st; a.iters = it;
    a.x_warm = cfg.cold_start ? nullptr : dWarm;
    a.qp_carry = dQpCarry; a.qp_carry_set = dQpCarrySet;
    a.accumulate = ctx.accumulate ? 1 : 0;
    plant_args(a, ctx);
    if (term_every > 0) {
      // per-step terminal refresh on the per-step route: the RLS update as a launch of its own, the Riccati iteration on the updated
      // models (dare_kernel, every term_every-th step), then condensed QP and solve with the refreshed blocks
      const int ph = a.phases;
      if (ph & PH_RLS) {
        StepArgs<T> a1 = a;
        a1.phases = PH_RLS; a1.plant = -1; a1.U0 = nullptr; a1.Useq = nullptr; a1.u_store = nullptr; a1.status = nullptr; a1.iters = nullptr;
        HIPCHK(launch_step<T>(a1, threads, s));
      }
      if (term_count % term_every == 0) { const int rc2 = dare_blocks(B, dTermQ, term_R, term_maxiter, term_eps, s); if (rc2) return rc2; }
      a.phases = ph & ~PH_RLS;
      a.Wterm = (T*)dWtB.get(); a.wterm_per_traj = 1;
      term_count += 1;
    }
    HIPCHK(launch_step<T>(a, threads, s));
    if (rec && (rc = prof_end(s, 1))) return rc;
    prog.advance(1, update_on);
    return 0;
  }

  int set_online_update(int on) override { update_on = on != 0; if (core) core->update_on = update_on; return 0; }
  // the input that was actually applied at the last step, when it is not the one kmpc_step returned (actuator limits, a
  // logged trajectory that is being followed): the next RLS update regresses on it (z = [psi; u], duffing.py:900)
  int set_applied_input(const void* U, int Bc, hipStream_t s) override {
    if (!U || Bc != B) FAIL(-3, "kmpc_set_applied_input: U must hold one input per trajectory of the handle");
    if (core) { const int rc = ensure_dense(s, true); if (rc) return rc; }  // (u_{k-1} is part of what the core owns during roll-outs)
    HIPCHK(hipMemcpyAsync(dUprev, U, sizeof(T) * (size_t)B, hipMemcpyDeviceToDevice, s));
    return 0;
  }

  int plant_step(int plant, void* X, const void* U, double h, int sw, int Bc, hipStream_t s) override {
    if (n != 2) FAIL(-3, "plants are two-state systems");
    if (!plant_id_ok(plant)) FAIL(-3, "unknown plant");
    PlantArgs<T> a{};
    a.B = Bc; a.plant = plant; a.switched = sw; a.h = (T)h; a.X = (T*)X; a.U = (const T*)U;
    HIPCHK(launch_plant<T>(a, s));
    return 0;
  }

  // ---- fused roll-out (one launch for all the steps; rollout_kernel in step_kernel.hip) ----------------
  int pack_encoder(hipStream_t s) {
    if (packed_ok) return 0;
    const int KS = enc.KS;
    const int nhh = cfg.layers - 1;
    for (int k = 0; k < nhh; ++k) {
      HIPCHK(dWhp[k].ensure((size_t)(enc.Hp / 16) * KS * 64));
      HIPCHK(launch_pack_afrag<T>(dWh[k], enc.Hp, enc.Hp, KS, dWhp[k], s));
    }
    HIPCHK(dWop.ensure((size_t)(enc.Lp / 16) * KS * 64));
    HIPCHK(launch_pack_afrag<T>(dWo, enc.Lp, enc.Hp, KS, dWop, s));
    packed_ok = true;
    return 0;
  }
  int rollout_is_fused() const override { return fused_rollout_ok() ? 1 : 0; }
  bool fused_rollout_ok() const {
    static const bool off = dbg_env("KMPC_NO_FUSED_ROLLOUT") != nullptr;  // measurement aid: per-step launches
    if (core) return !off && core->fused_rollout_ok();  // (float32 panels around the float64 roll-out)
    if (term_every > 0 && variant_of(false).state <= 0) return false;  // (the refresh needs the TERM plug-in; else the per-step route)
    return !off && sizeof(T) == 8 && fused_dims_ok();
  }
  // 0: the library's own instantiation, 1: a plug-in (text: its file and whether it was compiled now or found in the kernel cache),
  // -1: the plug-in could not be made (text: why; the handle works with per-step launches), 2: this configuration has no fused roll-out
  int rollout_plugin_status(std::string* text) const override {
    const int code = rollout_plugin_status_plain(text);
    // (diagnostics armed: kmpc_rollout_diag launches the DIAG object, kmpc_rollout the one above)
    if (text && diag_on) {
      if (diag_fused_ready() && fused_rollout_ok()) *text += "; kmpc_rollout_diag: " + rollout_plugin_describe(variant_of(true).plugin.key);
      else *text += "; kmpc_rollout_diag: per-step launches" + (diag_msg().empty() ? std::string() : " (" + diag_msg() + ")");
    }
    return code;
  }
  int rollout_plugin_status_plain(std::string* text) const {
    for (const RolloutVariant* v : {&variant_of(false), &variant[0][0]}) {  // (the refreshing object where one was asked for, else the plain one)
      if (v->state > 0) { if (text) *text = rollout_plugin_describe(v->plugin.key); return 1; }
      if (v->state < 0) { if (text) *text = v->msg; return -1; }
    }
    if (!fused_kind_ok()) { if (text) *text = kFusedKindReason; return 2; }
    if (!fused_rollout_ok()) {
      if (text) *text = "no fused roll-out for this configuration (per-step launches): the fused kernels serve float64, n = 2, (L + 1)^2 <= 2048, "
                        "horizons N <= 40 and q = 1, 2 or L output rows";
      return 2;
    }
    if (text) *text = "built-in instantiation of libkoopmpc.so";
    return 0;
  }
  // io32: the caller-owned panels (X, ref, Ulog, Xlog, U0out, Useqout) are float32 -- the call comes from a KMPC_F32 handle's core
  int rollout_fused(const StepCtx& ctx, int plant, void* X, const void* ref, int rpt, int steps, int step0, int switch_step, double hs,
                    void* Ulog, void* Xlog, int32_t* st, int32_t* it, hipStream_t s, void* U0out = nullptr,
                    void* Useqout = nullptr, bool io32 = false) {
    int rc = check_lift_ready();
    if (rc) return rc;
    if constexpr (sizeof(T) == 4) {
      if (core) {
        if ((rc = ensure_image(s))) return rc;
        core->prof = prof;
        rc = on_core([&](Impl<double>& c) { return c.rollout_fused(ctx, plant, X, ref, rpt, steps, step0, switch_step, hs, Ulog, Xlog, st, it, s, U0out, Useqout, true); });
        if (!rc) prog = core->prog;
        return rc;
      }
    }
    RolloutArgs<T> r{};
    r.s = base_args(B);
    r.s.u_prev = dUprev; r.s.x_now = (const T*)X;
    r.s.ref = (const T*)ref; r.s.ref_per_traj = rpt;
    r.s.U0 = U0out ? (T*)U0out : dU0; r.s.Useq = (T*)Useqout; r.s.u_store = dUprev; r.s.status = st; r.s.iters = it;
    r.s.x_warm = cfg.cold_start ? nullptr : dWarm;
    r.s.plant = plant; r.s.plant_h = (T)hs; r.s.X_rw = (T*)X;
    r.s.pp_sl = 1; r.s.pp_sb = L; r.s.pn_sl = 1; r.s.pn_sb = L;
    r.s.accumulate = 1;
    if (cfg.lift_kind == KMPC_LIFT_MLP) {
      if ((rc = pack_encoder(s))) return rc;
      r.lift_rbf = 0;
      r.W1 = dW1; r.b1 = db1; r.Whp[0] = dWhp[0]; r.Whp[1] = dWhp[1]; r.bh[0] = dbh[0]; r.bh[1] = dbh[1];
      r.Wop = dWop; r.bo = dbo; r.Hp = enc.Hp; r.Lp = enc.Lp; r.KS = enc.KS; r.nhh = cfg.layers - 1;
    } else {
      r.lift_rbf = 1;
      r.cx = dcx; r.eps = (T)cfg.rbf_eps; r.rbf_matlab = rbf_code();
    }
    r.psi[0] = dPsi[0]; r.psi[1] = dPsi[1]; r.cur = prog.cur;
    r.steps = steps; r.step0 = step0; r.switch_step = switch_step;
    r.have_prev = prog.have_prev ? 1 : 0; r.rls_fresh = prog.rls_fresh ? 1 : 0;
    r.no_update = update_on ? 0 : 1;
    r.U_log = (T*)Ulog; r.X_log = (T*)Xlog;
    r.io_f32 = io32 ? 1 : 0;
    if (io32 && !r.s.U0) r.s.U0 = dU0;
    if (ctx.diag) { r.diag = 1; r.Psi_log = (T*)ctx.diag->Psi; r.dA_log = (T*)ctx.diag->dA; r.dB_log = (T*)ctx.diag->dB; r.dC_log = (T*)ctx.diag->dC; }
    if constexpr (sizeof(T) == 8) {
      if (term_every > 0) {
        if (io32) FAIL(-3, "the per-step terminal refresh is a float64 feature");
        r.term_every = term_every; r.term_count0 = (int)(term_count % term_every); r.term_maxiter = term_maxiter;
        r.term_R = term_R; r.term_eps = term_eps; r.term_Q = dTermQ; r.term_W = dWtB;
        r.term_scratch = dTermScr; r.term_scratch_stride = term_scratch_elems(L); r.term_iters = dDareIt;
        r.s.Wterm = dWtB; r.s.wterm_per_traj = 1;
      }
    }
    // (the card deal across the workgroups where the batch allows it: whole workgroups; the rank kernel is O(B^2 / lanes))
    const bool global_place = cfg.lift_kind == KMPC_LIFT_MLP && (B & 15) == 0 && B <= (1 << 20);
    if (!dbg_env("KMPC_ROLLOUT_NO_PLACE")) {  // (the trajectories' solver work of the previous launch: RolloutArgs::work)
      if (!dWork) {
        HIPCHK(dWork.alloc((size_t)B));
        HIPCHK(hipMemsetAsync(dWork, 0, sizeof(int32_t) * (size_t)B, s));
      }
      r.work = dWork;
      static const int tail = dbg_env("KMPC_PLACE_TAIL") ? atoi(dbg_env("KMPC_PLACE_TAIL")) : 5;  // (measurement aid; 0 = the whole launch)
      r.work_tail = tail;
      if (place_valid && global_place && !dbg_env("KMPC_ROLLOUT_NO_GLOBAL_PLACE")) r.perm = dPerm;
      // (work and perm were written on the stream of the previous call: a call on another stream waits for them -- a torn perm would
      //  hand one trajectory to two waves and skip another: ADVICE r4)
      if (evPlace && place_stream != s) HIPCHK(hipStreamWaitEvent(s, evPlace, 0));
    }
    if constexpr (sizeof(T) == 8) {
      if (use_img) {
        if ((rc = ensure_image(s))) return rc;
        r.img = dImg; r.img_stride = sImg;
      } else if ((rc = ensure_dense(s, true))) return rc;
    }
    bool rec;
    if ((rc = prof_begin(s, &rec)) || (rec && (rc = prof_mid(s)))) return rc;  // (no separate lift kernel)
    HIPCHK(launch_rollout_fused<T>(r, s, &variant_of(ctx.diag != nullptr).plugin));
    // (profiling: the closing event sits right behind the roll-out kernel -- until round 5 it sat behind the rank pass below, whose
    //  9 us at B = 4096 were counted into "the dominant kernel's duration": rocprofv3 0.630 ms against 0.647 ms from these events)
    if (rec && (rc = prof_end(s, steps))) return rc;
    if (r.work && steps >= 4 && global_place) {
      HIPCHK(dPerm.ensure((size_t)B * 3));  // (perm, then the sort's two ping-pong buffers)
      HIPCHK(launch_place(dWork, B, dPerm, reinterpret_cast<uint32_t*>(dPerm + B), s));  // (the next launch's deal: RolloutArgs::perm)
      place_valid = true;
    } else {
      place_valid = false;
    }
    if (r.work) {
      if (!evPlace) HIPCHK(hipEventCreateWithFlags(&evPlace, hipEventDisableTiming));
      HIPCHK(hipEventRecord(evPlace, s));
      place_stream = s;
    }
    if (term_every > 0) term_count += steps;
    prog.advance(steps, update_on);  // (the host side follows the kernel's own bookkeeping)
    return 0;
  }

  int rollout(int plant, void* X, const void* ref, int rpt, int steps, int step0, int switch_step, double hs,
              void* Ulog, void* Xlog, int32_t* st, int32_t* it, hipStream_t s) override {
    return rollout_impl(StepCtx{}, plant, X, ref, rpt, steps, step0, switch_step, hs, Ulog, Xlog, st, it, s);
  }
  int rollout_impl(const StepCtx& ctx, int plant, void* X, const void* ref, int rpt, int steps, int step0, int switch_step, double hs,
                   void* Ulog, void* Xlog, int32_t* st, int32_t* it, hipStream_t s) {
    if (!X || !ref || steps < 0) FAIL(-3, "kmpc_rollout: bad arguments");
    HIPCHK(dU0.ensure((size_t)B));
    if (n != 2) FAIL(-3, "plants are two-state systems");
    if (!plant_id_ok(plant)) FAIL(-3, "unknown plant");
    // (the fused roll-out with the MLP lift accumulates status / iterations in LDS and WRITES them when it ends: no zeroing
    //  launches in front of it -- two of the ~70 us a 20-step call spends outside its kernel)
    const bool fused = fused_rollout_ok() && (!ctx.diag || diag_fused_ready());  // (kmpc_rollout_diag: its fused route needs the DIAG plug-in)
    const bool kernel_writes_totals = steps > 0 && fused && cfg.lift_kind == KMPC_LIFT_MLP;
    if (!kernel_writes_totals) {
      if (st) HIPCHK(hipMemsetAsync(st, 0, sizeof(int32_t) * (size_t)B, s));
      if (it) HIPCHK(hipMemsetAsync(it, 0, sizeof(int32_t) * (size_t)B, s));
    }
    if (steps > 0 && fused) {
      const int rcf = rollout_fused(ctx, plant, X, ref, rpt, steps, step0, switch_step, hs, Ulog, Xlog, st, it, s);
      if (!rcf) {
        last_rollout_variant = rollout_last_variant();
        last_rollout_resident = rollout_last_resident(&last_rollout_lds);
      }
      return rcf;
    }
    if (steps > 0) last_rollout_variant = last_rollout_resident = last_rollout_lds = 0;
    if (steps == 0 && fused) {
      // a call without steps brings the handle into the form the fused roll-out works on (the wave image of a state that was
      // set, restored or stepped through the dense blocks): set-up that the next kmpc_rollout would otherwise pay -- a float32 handle's
      // core, then the core's own image
      int rc = ensure_image(s);
      if (!rc) rc = on_core([&](Impl<double>& c) { return c.ensure_image(s); });
      return rc;
    }
    for (int i = 0; i < steps; ++i) {
      const int gi = step0 + i;
      T* u = Ulog ? (T*)Ulog + (size_t)i * B : dU0;
      if (ctx.diag) { const int rcd = diag_before_step(*ctx.diag, X, i, s); if (rcd) return rcd; }
      // lift kernel + fused RLS/condense/QP/plant kernel
      int rc = step_impl(StepCtx{true, plant, (switch_step >= 0 && gi >= switch_step) ? 1 : 0, hs, X, nullptr}, X, ref, rpt, u, nullptr, st, it, s);
      if (rc) return rc;
      if (Xlog) HIPCHK(hipMemcpyAsync((T*)Xlog + (size_t)i * n * B, X, sizeof(T) * (size_t)n * B,
                                      hipMemcpyDeviceToDevice, s));
    }
    return 0;
  }

  // ---- shared-model mode -----------------------------------------------------------------------------
  int64_t gram_elems() const override { return (int64_t)(p + L + n) * p; }
  // the seven blocks of the shared-model mode, made and filled in locals and handed to the handle together: a call that fails leaves the
  // handle without any of them, and the next one starts over
  int shared_alloc() {
    if (dGram) return 0;
    const int R = p + L + n, MT = (R + 15) / 16, NT = (p + 15) / 16;
    DevBuf<double> gram, partial;
    DevBuf<T> ks, cs, hs, fs, f0s;
    HIPCHK(gram.alloc((size_t)R * p));
    HIPCHK(hipMemset(gram, 0, sizeof(double) * (size_t)R * p));
    HIPCHK(partial.alloc((size_t)GRAM_BLOCKS * MT * 16 * NT * 16));
    HIPCHK(ks.alloc((size_t)L * p));
    HIPCHK(cs.alloc((size_t)n * L));
    HIPCHK(hs.alloc((size_t)N * N));
    HIPCHK(fs.alloc((size_t)N * (L + 1)));  // (one more column in the delta-u form)
    HIPCHK(f0s.alloc((size_t)N));
    // until samples exist the shared model is the offline one (trajectory 0's copy, duffing.py:811-813)
    { int rc = sync_own(); if (rc) return rc; }  // (before the conversion: non-blocking streams do not order with the null stream)
    { int rc = ensure_dense(nullptr, false); if (rc) return rc; HIPCHK(hipStreamSynchronize(nullptr)); }
    HIPCHK(hipMemcpy(ks, dK, sizeof(T) * (size_t)L * p, hipMemcpyDeviceToDevice));
    HIPCHK(hipMemcpy(cs, dC, sizeof(T) * (size_t)n * L, hipMemcpyDeviceToDevice));
    dGram = std::move(gram); dPartial = std::move(partial);
    dKs = std::move(ks); dCs = std::move(cs); dHs = std::move(hs); dFs = std::move(fs); df0s = std::move(f0s);
    return 0;
  }
  // the route of the model stage: one launch (shared_model_kernel / shared_model2_kernel), or the round-1 pair shared_solve_kernel +
  // shared_condense_kernel (every y = psi handle, y = C x with L + 1 > 64)
  bool shared_one_launch() const {
    static const bool two_kernels = dbg_env("KMPC_SHARED_TWO_KERNELS") != nullptr;  // measurement aid: the round-1 launches
    return !two_kernels && cfg.output_kind == KMPC_OUT_CX && shared_model_available(L, n, q, N, cfg.delta_u ? 1 : 0);
  }
  // Every entry of the shared-model mode asks this before it allocates or launches anything: a shape the pair cannot take (the condensed
  // QP keeps Gamma_0 .. Gamma_N, (N + 1) q L values, in the LDS of one workgroup) used to surface as the launcher's hipErrorInvalidValue
  // after G <- lambda G + delta and the model solve had already changed the handle.
  int shared_route_check(const char* who) {
    const int du = cfg.delta_u ? 1 : 0;
    if (shared_one_launch() || shared_condense_fits(L, n, q, N, du)) return 0;
    FAIL(-3, std::string(who) + ": the condensed QP of the shared model does not fit this shape: with " +
                 (cfg.output_kind == KMPC_OUT_LIFT ? "y = psi (q = L = " : "y = C x (q = ") + std::to_string(q) + " output rows), L = " + std::to_string(L) +
                 ", N = " + std::to_string(N) + " shared_condense_kernel needs " + std::to_string(shared_condense_lds_bytes(L, q, N, du)) +
                 " bytes of LDS and a workgroup has " + std::to_string(SHARED_LDS_MAX) + "; the handle is unchanged (kmpc_step takes this shape)");
  }
  int shared_local_gram(const void* X, double* delta, hipStream_t s) override {
    if (!X || !delta) FAIL(-3, "kmpc_shared_local_gram: null pointer");
    int rc = shared_route_check("kmpc_shared_local_gram");
    if (rc) return rc;
    if ((rc = shared_alloc())) return rc;
    // (only `if (core)`: psi, u_{k-1} and the ping-pong index are this side's from here on; the wave image of a float64 handle holds none of them)
    if (core && (rc = ensure_dense(s, true))) return rc;
    T* psi_now = dPsi[prog.cur];
    T* psi_prev = dPsi[prog.cur ^ 1];
    GramArgs<T> g{};
    g.B = B; g.n = n; g.L = L; g.max_blocks = GRAM_BLOCKS;
    g.psi_prev = psi_prev; g.pp_sl = 1; g.pp_sb = L;
    g.psi_now = psi_now; g.pn_sl = 1; g.pn_sb = L;
    g.u_prev = dUprev; g.x_now = (const T*)X; g.partial = dPartial;
    if constexpr (sizeof(T) == 8) {
      // float64 MLP lift: the lift and the Gram sums of the transitions in ONE launch (lift_coop_kernel<.., GRAM>), then the reduce
      const bool two = dbg_env("KMPC_SHARED_LIFT_GRAM_2") != nullptr;  // measurement / test aid (read per call): the two round-3 launches
      if (prog.have_prev && !two && cfg.lift_kind == KMPC_LIFT_MLP) {
        if ((rc = check_lift_ready())) return rc;
        LiftArgs<T> a{};
        a.B = B; a.n = n; a.L = L; a.hidden = enc.hid; a.nlayers = cfg.layers;
        a.X = (const T*)X; a.Psi = psi_now; a.ps_l = 1; a.ps_b = L;
        if ((rc = encoder_args(a, s))) return rc;
        if (lift_gram_available(a)) {
          int nb = 0;
          HIPCHK(launch_lift_gram(a, g, &nb, s));
          HIPCHK(launch_gram_reduce(dPartial, nb, L, n, 0.0, delta, s));  // (forget = 0 overwrites delta)
          return 0;
        }
      }
    }
    rc = lift_to((const T*)X, psi_now, 1, L, B, s);
    if (rc) return rc;
    if (!prog.have_prev) {
      HIPCHK(hipMemsetAsync(delta, 0, sizeof(double) * (size_t)gram_elems(), s));
      return 0;
    }
    HIPCHK(launch_gram<T>(g, 0.0, delta, s));  // (forget = 0 overwrites delta)
    return 0;
  }
  int shared_solve_plant(const double* delta, const void* ref, void* U0, void* Useq, int32_t* st, int32_t* it, int plant, void* X,
                         int switched, double hstep, hipStream_t s) override {
    if (!X) FAIL(-3, "kmpc_shared_solve_plant: null pointer");
    if (n != 2) FAIL(-3, "plants are two-state systems");
    if (!plant_id_ok(plant)) FAIL(-3, "unknown plant");
    return shared_solve_impl(StepCtx{false, plant, switched ? 1 : 0, hstep, X, nullptr}, delta, ref, U0, Useq, st, it, s);
  }
  // kmpc_shared_rollout: the stages of the shared-model step, `steps` times, on one stream, the collective between them
  int shared_rollout(int plant, void* X, const void* ref, int steps, int step0, int switch_step, double hstep, void* comm, void* Ulog,
                     void* Xlog, void* U0out, void* Useq, int32_t* st, int32_t* it, hipStream_t s) override {
    if (!X || !ref || steps < 0) FAIL(-3, "kmpc_shared_rollout: bad arguments");
    if (n != 2) FAIL(-3, "plants are two-state systems");
    if (!plant_id_ok(plant)) FAIL(-3, "unknown plant");
    int rc = shared_route_check("kmpc_shared_rollout");
    if (rc) return rc;
    if ((rc = shared_alloc())) return rc;
    HIPCHK(dDelta.ensure((size_t)gram_elems()));
    HIPCHK(dU0.ensure((size_t)B));
    typedef ncclResult_t (*allreduce_fn)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t);
    allreduce_fn ar = nullptr;
    if (comm) {
      ar = (allreduce_fn)resolve_nccl_allreduce();
      if (!ar) FAIL(-4, "kmpc_shared_rollout: no RCCL in this process (ncclAllReduce not found)");
    }
    if (st) HIPCHK(hipMemsetAsync(st, 0, sizeof(int32_t) * (size_t)B, s));
    if (it) HIPCHK(hipMemsetAsync(it, 0, sizeof(int32_t) * (size_t)B, s));
    for (int i = 0; i < steps; ++i) {
      const int gi = step0 + i;
      if ((rc = shared_local_gram(X, dDelta, s))) return rc;
      if (ar && prog.have_prev) {  // (before the first transition every rank's block is zero: nothing to sum)
        const ncclResult_t nr = ar(dDelta, dDelta, (size_t)gram_elems(), ncclDouble, ncclSum, (ncclComm_t)comm, s);
        if (nr != ncclSuccess) FAIL(-(2000 + (int)nr), "kmpc_shared_rollout: ncclAllReduce failed");
      }
      T* const u = Ulog ? (T*)Ulog + (size_t)i * B : (U0out ? (T*)U0out : dU0);
      rc = shared_solve_impl(StepCtx{true, plant, (switch_step >= 0 && gi >= switch_step) ? 1 : 0, hstep, X, nullptr}, dDelta, ref, u, Useq, st, it, s);
      if (rc) return rc;
      if (Xlog) HIPCHK(hipMemcpyAsync((T*)Xlog + (size_t)i * n * B, X, sizeof(T) * (size_t)n * B, hipMemcpyDeviceToDevice, s));
    }
    if (Ulog && U0out && steps > 0)
      HIPCHK(hipMemcpyAsync(U0out, (T*)Ulog + (size_t)(steps - 1) * B, sizeof(T) * (size_t)B, hipMemcpyDeviceToDevice, s));
    return 0;
  }
  int shared_solve(const double* delta, const void* ref, void* U0, void* Useq, int32_t* st, int32_t* it, hipStream_t s) override {
    return shared_solve_impl(StepCtx{}, delta, ref, U0, Useq, st, it, s);
  }
  int shared_solve_impl(const StepCtx& ctx, const double* delta, const void* ref, void* U0, void* Useq, int32_t* st, int32_t* it, hipStream_t s) {
    if (!delta || !ref || !U0) FAIL(-3, "kmpc_shared_solve: null pointer");
    if (wterm == Term::DarePerTraj)
      FAIL(-3, "kmpc_shared_solve: per-trajectory terminal blocks do not apply to the shared model (kmpc_terminal_from_dare with per_trajectory = 0)");
    int rc = shared_route_check("kmpc_shared_solve");
    if (rc) return rc;
    if ((rc = shared_alloc())) return rc;
    if (core && (rc = ensure_dense(s, true))) return rc;  // (only `if (core)`, as in shared_local_gram: u_{k-1} and the warm start are written here)
    const T* wt = wterm_ptr();
    const int okind = cfg.output_kind == KMPC_OUT_LIFT ? OUT_LIFT : OUT_CX;
    const int cy0 = cfg.output_kind == KMPC_OUT_LIFT ? 0 : cfg.out_row0;
    const bool one_launch = shared_one_launch();
    if (prog.have_prev && !one_launch) HIPCHK(launch_axpby(dGram, delta, cfg.lambda, (int)gram_elems(), s));
    if (one_launch) {
      // model solve + condensed QP + the tableau the box QPs start from, one launch (shared_model_kernel)
      HIPCHK(dTs.ensure((size_t)N * N));
      const bool old_kernel = dbg_env("KMPC_SHARED_MODEL_R3") != nullptr;  // measurement / test aid (read per call): the round-3 model kernel
      bool on16 = false;
      if constexpr (sizeof(T) == 8) {
        if (!old_kernel && shared_model2_available(L, n, q, N, cfg.delta_u ? 1 : 0)) {
          SharedModel2Args m{};
          m.gram = dGram; m.delta = prog.have_prev ? delta : nullptr; m.forget = cfg.lambda; m.ref = (const double*)ref;
          m.Lm = L; m.n = n; m.q = q; m.N = N; m.dP = 1.0 / cfg.P0; m.dQ = 1.0 / cfg.barQ0; m.have_samples = prog.have_prev ? 1 : 0;
          m.Qw = cfg.Qw; m.Rw = cfg.Rw;
          m.Kio = (double*)dKs; m.Cio = (double*)dCs; m.Hout = (double*)dHs; m.Fout = (double*)dFs; m.f0out = (double*)df0s; m.Tout = (double*)dTs;
          m.Wt = (const double*)wt; m.du_mode = cfg.delta_u ? 1 : 0; m.cy0 = cy0;
          // (F, T0, H once more as the operand fragments of shared_fast_kernel: written by the model kernel beside the dense blocks)
          int fmt = 0, fk1 = 0, fk2 = 0;
          if (N <= 64 && shared_fast_shape(N, L + (cfg.delta_u ? 1 : 0), &fmt, &fk1, &fk2)) {
            if (!dFastPack) {
              const size_t elems = shared_fast_pack_elems(fmt, fk1, fk2);
              HIPCHK(dFastPack.alloc(elems));
              HIPCHK(hipMemsetAsync(dFastPack, 0, sizeof(double) * elems, s));  // (the padding of the fragments stays zero: only elements of the matrices are written)
            }
            m.pack = dFastPack; m.pack_mt = fmt; m.pack_ks1 = fk1; m.pack_ks2 = fk2;
          }
          HIPCHK(launch_shared_model2(m, s));
          on16 = true;
          fast_pack_valid = m.pack != nullptr;
        }
      }
      if (!on16) {
        fast_pack_valid = false;
        HIPCHK(launch_shared_model<T>(dGram, prog.have_prev ? delta : nullptr, cfg.lambda, (const T*)ref, L, n, q, N, 1.0 / cfg.P0, 1.0 / cfg.barQ0, 1, prog.have_prev ? 1 : 0, cfg.Qw,
                                      cfg.Rw, dKs, dCs, dHs, dFs, df0s, dTs, wt, cfg.delta_u ? 1 : 0, cy0, s));
      }
      if (prog.have_prev) shared_has_samples = true;
    } else {
      if (prog.have_prev) {
        HIPCHK(launch_shared_solve<T>(dGram, L, n, 1.0 / cfg.P0, 1.0 / cfg.barQ0,
                                      cfg.output_kind == KMPC_OUT_CX ? 1 : 0, dKs, dCs, s, nullptr, nullptr, 1));
        shared_has_samples = true;
      }
      HIPCHK(launch_shared_condense<T>(dKs, dCs, (const T*)ref, L, n, q, N, okind, cfg.Qw, cfg.Rw, dHs, dFs, df0s, s, wt,
                                       cfg.delta_u ? 1 : 0, cy0));
    }
    StepArgs<T> a = base_args(B);
    a.phases = PH_QP;
    a.H_in = dHs; a.h_shared = 1; a.F_in = dFs; a.f0_in = df0s;
    a.T_in = one_launch ? dTs : nullptr;
    a.fast_pack = (one_launch && fast_pack_valid) ? dFastPack : nullptr;
    a.psi_now = dPsi[prog.cur]; a.pn_sl = 1; a.pn_sb = L;
    a.U0 = (T*)U0; a.Useq = (T*)Useq; a.u_store = dUprev; a.status = st; a.iters = it;
    a.x_warm = cfg.cold_start ? nullptr : dWarm;
    a.accumulate = ctx.accumulate ? 1 : 0;  // (kmpc_shared_rollout: worst status / total Newton solves over the steps)
    plant_args(a, ctx);  // (kmpc_shared_solve_plant: the solve also advances every trajectory's plant with its u_k, as the roll-outs do)
    bool rec;  // (profiling: the QP launch of the shared-model step)
    if ((rc = prof_begin(s, &rec)) || (rec && (rc = prof_mid(s)))) return rc;
    // the trajectories whose unconstrained minimiser lies inside the box are finished 16 per wave on the matrix cores
    // (shared_fast_kernel); the solve-only kernel then only runs for the flagged rest
    const bool no_fast = dbg_env("KMPC_SHARED_NO_FAST") != nullptr;  // measurement / test aid (read per call): every trajectory through the QP kernel
    if (one_launch && sizeof(T) == 8 && N <= 64 && !no_fast) {
      HIPCHK(dNeed.ensure((size_t)B));
      // (the flagged trajectories also go into a list that a fixed grid of the solve-only kernel walks; two counters alternate)
      if (!dQpList) {
        HIPCHK(dQpList.alloc((size_t)(B + 2)));
        HIPCHK(hipMemsetAsync(dQpList, 0, sizeof(int32_t) * (size_t)(B + 2), s));
      }
      if (!dbg_env("KMPC_SHARED_NO_LIST")) {  // (measurement / test aid, read per call: one workgroup per trajectory, flags only)
        a.qp_list = dQpList + 2;
        a.qp_count = dQpList + qp_list_parity;
        a.qp_count_next = dQpList + (qp_list_parity ^ 1);
        qp_list_parity ^= 1;
      }
      HIPCHK(launch_shared_fast<T>(a, dNeed, s));
      a.qp_need = dNeed;
    }
    HIPCHK(launch_step<T>(a, threads, s));
    if (rec && (rc = prof_end(s, 1))) return rc;
    // (not Progress::advance: the shared-model step runs no RLS update and never clears rls_fresh)
    prog.have_prev = true;
    prog.cur ^= 1;
    return 0;
  }
  int offline_fit(const void* X, const void* Y, const void* U, int M, double ridge, int init_rls, void* A, void* Bm,
                  void* C, hipStream_t s) override {
    if (!X || !Y || !U || M < 1) FAIL(-3, "kmpc_offline_fit: bad arguments");
    int rc = shared_alloc();
    if (rc) return rc;
    if ((rc = ensure_dense(s, true))) return rc;
    if ((rc = forget_tableaux(s))) return rc;
    DevBuf<T> px, py, pinv;  // (pinv stays empty without init_rls)
    DevBuf<double> g;
    if (init_rls) HIPCHK(pinv.alloc((size_t)(p * p + L * L)));
    HIPCHK(px.alloc((size_t)L * M));
    HIPCHK(py.alloc((size_t)L * M));
    HIPCHK(g.alloc((size_t)gram_elems()));
    rc = lift_to((const T*)X, px, M, 1, M, s);           // panels (L x M)
    if (!rc) rc = lift_to((const T*)Y, py, M, 1, M, s);
    if (!rc) {
      GramArgs<T> ga{};
      ga.B = M; ga.n = n; ga.L = L; ga.max_blocks = GRAM_BLOCKS;
      ga.psi_prev = px; ga.pp_sl = M; ga.pp_sb = 1;
      ga.psi_now = py; ga.pn_sl = M; ga.pn_sb = 1;
      ga.u_prev = (const T*)U; ga.x_now = (const T*)X;  // C pairs X with PHIX (duffing.py:177)
      ga.partial = dPartial;
      hipError_t e = hipMemsetAsync(g, 0, sizeof(double) * (size_t)gram_elems(), s);
      if (e == hipSuccess) e = launch_gram<T>(ga, 0.0, g, s);
      if (e == hipSuccess)
        e = launch_shared_solve<T>(g, L, n, ridge, ridge, 1, dTmp, dTmp + L * p, s, pinv, pinv ? pinv + p * p : nullptr);
      if (e == hipSuccess && init_rls) {
        // the online RLS continues from the offline data: K_A = Ylift V', inv_K_G = pinv(V V')
        // (Koopman_update.m:258-278) -- in gain form: K = offline [A B], P = (V V')^-1
        e = launch_broadcast<T>(dP, sP, pinv, p * p, B, s);
        if (e == hipSuccess) e = launch_broadcast<T>(dQ, sQ, pinv + p * p, L * L, B, s);
      }
      if (e == hipSuccess) e = launch_broadcast<T>(dK, sK, dTmp, L * p, B, s);
      if (e == hipSuccess && cfg.output_kind == KMPC_OUT_CX) e = launch_broadcast<T>(dC, sC, dTmp + L * p, n * L, B, s);
      if (e == hipSuccess) e = hipMemcpyAsync(dKs, dTmp, sizeof(T) * (size_t)L * p, hipMemcpyDeviceToDevice, s);
      if (e == hipSuccess) e = hipMemcpyAsync(dCs, dTmp + L * p, sizeof(T) * (size_t)n * L, hipMemcpyDeviceToDevice, s);
      if (e == hipSuccess && (A || Bm || C))
        e = launch_export_model<T>(dTmp, (long)L * p, dTmp + L * p, (long)n * L, n, L, 1, (T*)A, (T*)Bm, (T*)C, s);
      if (e == hipSuccess) e = hipStreamSynchronize(s);
      if (e != hipSuccess) { err = std::string("kmpc_offline_fit: ") + hipGetErrorString(e); rc = -(int)(1000 + (int)e); }
    }
    if (!rc && init_rls) prog.rls_fresh = false;  // the first online update refines this model instead of restarting from K_A = 0
    return rc;
  }

  int shared_get_model(void* A, void* Bm, void* C, hipStream_t s) override {
    int rc = shared_alloc();
    if (rc) return rc;
    HIPCHK(launch_export_model<T>(dKs, (long)L * p, cfg.output_kind == KMPC_OUT_CX ? dCs : nullptr, (long)n * L, n, L,
                                  1, (T*)A, (T*)Bm, (T*)C, s));
    return 0;
  }

  // ---- state blob (the layout: the comment at BlobHeader, above Impl)
  // the header of a blob written now: which optional sections the handle has, and the flags that travel with the state
  BlobHeader blob_header() const {
    BlobHeader hd{};
    hd.magic = kBlobMagic; hd.version = 2; hd.dtype = cfg.dtype; hd.n = n; hd.L = L; hd.N = N; hd.B = B;
    hd.have_prev = prog.have_prev ? 1 : 0; hd.rls_fresh = prog.rls_fresh ? 1 : 0;
    hd.has_shared = dGram ? 1 : 0; hd.shared_has_samples = shared_has_samples ? 1 : 0;
    term_to_flags(wterm, &hd.have_wterm, &hd.wterm_from_dare, &hd.wterm_per_traj);
    hd.wterm_blocks = wterm_block_count(wterm);
    hd.P0 = cfg.P0; hd.barQ0 = cfg.barQ0;
    return hd;
  }
  // THE list of the state blocks: what a blob with header hd holds behind it, in its order, as this handle's buffers.  Checkpoints
  // (size, export, import), the float32 <-> float64 hand-over (core_push / core_pull: the first n_traj entries) and the zero-fill of
  // init all walk this list.  (Pointers of sections the handle has not allocated are null: sizes are valid before, copies after.)
  Sections sections(const BlobHeader& hd) const {
    Sections t;
    t.add(dP, sizeof(T), (size_t)sP * B); t.add(dK, sizeof(T), (size_t)sK * B);
    t.add(dQ, sizeof(T), (size_t)sQ * B); t.add(dC, sizeof(T), (size_t)sC * B);
    t.add(dPsi[prog.cur ^ 1], sizeof(T), (size_t)L * B); t.add(dWarm, sizeof(T), (size_t)N * B, (size_t)N); t.add(dUprev, sizeof(T), (size_t)B);
    t.n_traj = t.n;
    if (hd.has_shared) { t.add(dGram, sizeof(double), (size_t)gram_elems()); t.add(dKs, sizeof(T), (size_t)L * p); t.add(dCs, sizeof(T), (size_t)n * L); }
    if (hd.have_wterm && hd.wterm_from_dare) t.add(dWtB, sizeof(double), (size_t)hd.wterm_blocks * q * q);
    else if (hd.have_wterm) t.add(dWt, sizeof(T), (size_t)hd.wterm_blocks * q * q);
    return t;
  }
  int64_t state_bytes() const override { return blob_bytes(sections(blob_header())); }
  int state_export(void* blob, int64_t bytes) override {
    if (bytes < state_bytes() || !blob) FAIL(-3, "kmpc_state_export: buffer too small");
    { int rc = sync_own(); if (rc) return rc; }  // (a roll-out on a non-blocking stream may still be writing the wave image)
    { int rc = ensure_dense(nullptr, false); if (rc) return rc; }
    { int rc = forget_tableaux(nullptr); if (rc) return rc; }  // (a checkpoint is a synchronisation point: exporter and importer continue alike)
    if (core) home.drop_fast();  // (... a float32 handle from its float32 blocks, as the importer will, not from its core's unrounded state)
    HIPCHK(hipStreamSynchronize(nullptr));
    const BlobHeader hd = blob_header();
    const Sections t = sections(hd);
    char* o = (char*)blob;  // host or device memory (unified addressing)
    HIPCHK(hipMemcpy(o, &hd, sizeof(hd), hipMemcpyDefault)); o += sizeof(hd);
    for (int i = 0; i < t.n; ++i) {
      HIPCHK(hipMemcpy(o, t.s[i].ptr, t.s[i].bytes(), hipMemcpyDefault));
      o += t.s[i].bytes();
    }
    return 0;
  }
  int state_import(const void* blob, int64_t bytes) override {
    if (bytes < (int64_t)sizeof(BlobHeader) || !blob) FAIL(-3, "kmpc_state_import: buffer too small");
    BlobHeader hd;
    const char* o = (const char*)blob;
    HIPCHK(hipMemcpy(&hd, o, sizeof(hd), hipMemcpyDefault)); o += sizeof(hd);
    if (hd.magic != kBlobMagic || hd.version != 2 || hd.dtype != cfg.dtype || hd.n != n || hd.L != L || hd.N != N || hd.B != B)
      FAIL(-3, "kmpc_state_import: blob does not match this handle");
    // a consistent header: flags are 0 / 1, the number of terminal blocks is what the flags imply, Riccati blocks only where
    // kmpc_terminal_from_dare would have produced them (float64)  (round-1 blobs, version 1, are not accepted: they carry no
    // shared-model / terminal sections and were written with another state order)
    auto flag01 = [](int32_t v) { return v == 0 || v == 1; };
    if (!flag01(hd.have_prev) || !flag01(hd.rls_fresh) || !flag01(hd.has_shared) || !flag01(hd.shared_has_samples) || !flag01(hd.have_wterm) ||
        !flag01(hd.wterm_from_dare) || !flag01(hd.wterm_per_traj))
      FAIL(-3, "kmpc_state_import: inconsistent header (flags)");
    bool term_ok;
    const Term blob_term = term_from_flags(hd.have_wterm, hd.wterm_from_dare, hd.wterm_per_traj, &term_ok);
    if (!term_ok || hd.wterm_blocks != wterm_block_count(blob_term)) FAIL(-3, "kmpc_state_import: inconsistent header (terminal blocks)");
    if (term_from_dare(blob_term) && sizeof(T) != 8) FAIL(-3, "kmpc_state_import: Riccati terminal blocks need a float64 handle");
    if (bytes < blob_bytes(sections(hd))) FAIL(-3, "kmpc_state_import: buffer too small");
    { int rc = sync_own(); if (rc) return rc; }
    home.dense_overwritten();  // (the blob overwrites every dense block)
    { int rc = forget_tableaux(nullptr); if (rc) return rc; }
    if (hd.has_shared) { int rc = shared_alloc(); if (rc) return rc; }
    if (term_from_dare(blob_term)) { int rc = dare_buffers(hd.wterm_blocks); if (rc) return rc; }
    else if (blob_term == Term::Given) HIPCHK(dWt.ensure((size_t)q * q));
    const Sections t = sections(hd);  // (now that every section of the blob has its buffer)
    for (int i = 0; i < t.n; ++i) {
      HIPCHK(hipMemcpy(t.s[i].ptr, o, t.s[i].bytes(), hipMemcpyDefault));
      o += t.s[i].bytes();
    }
    prog.have_prev = hd.have_prev != 0;
    prog.rls_fresh = hd.rls_fresh != 0;
    if (hd.has_shared) shared_has_samples = hd.shared_has_samples != 0;
    else if (dGram) {  // the blob comes from a handle that never ran a shared-model step
      HIPCHK(hipMemset(dGram, 0, sizeof(double) * (size_t)gram_elems()));
      shared_has_samples = false;
    }
    wterm = blob_term;
    cfg.P0 = hd.P0; cfg.barQ0 = hd.barQ0;
    if constexpr (sizeof(T) == 8) {
      // terminal refresh armed: its launches read one block per trajectory (dWtB[B]) whatever the blob held.  A blob with one block
      // for the batch (or none) gives that block (or Qw I) to every trajectory until its next refresh -- the copy above filled
      // trajectory 0 alone and left the other B - 1 what they were before the import.
      if (term_every > 0 && wterm != Term::DarePerTraj) {
        std::vector<double> w0((size_t)q * q, 0.0);
        if (wterm != Term::None) HIPCHK(hipMemcpy(w0.data(), wterm_ptr(), sizeof(double) * w0.size(), hipMemcpyDeviceToHost));
        { int rc = spread_block(w0); if (rc) return rc; }
        wterm = Term::DarePerTraj;
      }
    }
    // the host copy of a given P_N (kmpc_mpc_solve with another Q re-forms the block from it) and -- float32 handle with a float64
    // core -- the core's terminal weight follow the blob: the core only learns about a weight through set_terminal_weight, so a
    // checkpoint loaded into a fresh handle would otherwise run its fused roll-outs WITHOUT the terminal block, and one without a block
    // loaded over a handle that had one would keep using it
    hostPN.clear();
    if (wterm == Term::Given) {
      std::vector<T> w((size_t)q * q);
      HIPCHK(hipMemcpy(w.data(), dWt, sizeof(T) * w.size(), hipMemcpyDeviceToHost));
      hostPN = pn_from_block(w, cfg.Qw);
      return core_weight(&w);
    }
    return core_weight(nullptr);
  }

  // ---- packed rows: trajectories in and out of the handle on the device (the row format: the comment behind BlobHeader)
  // a trajectory of this handle has state of its own that a row carries whole
  bool rows_supported(const char* who) const {
    if (dGram) { err = std::string(who) + ": the handle has its shared-model blocks -- the model is pooled over the batch, a trajectory has no state of its own"; return false; }
    if (wterm == Term::DarePerTraj || term_every > 0) {
      err = std::string(who) + ": per-trajectory terminal blocks (kmpc_terminal_from_dare per trajectory, kmpc_set_terminal_refresh) are no part of a packed row";
      return false;
    }
    return true;
  }
  // the one layout of a row: derived from the list of state blocks
  bool row_plan(RowPlan* pl) const { return build_row_plan(sections(blob_header()), B, pl); }
  int64_t state_row_elems() const override {
    RowPlan pl;
    if (!rows_supported("kmpc_state_row_elems")) return -3;
    if (!row_plan(&pl)) { err = "kmpc_state_row_elems: no row layout for this handle"; return -3; }
    return pl.row_elems;
  }
  // runs the check kernel on s and reads its word back: 0, or -3 with the message; *word: the status (the flags of row 0)
  int rows_check(const char* who, const RowPlan& pl, const int32_t* idx, int count, bool dup, const void* rows, int want_hp, int want_rf, int* word,
                 hipStream_t s) {
    HIPCHK(dRowChk.ensure((size_t)B + 1));
    int32_t* const status = dRowChk.get() + B;
    HIPCHK(launch_state_rows_check(idx, count, B, dup ? dRowChk.get() : nullptr, rows, pl, want_hp, want_rf, status, s));
    int32_t w = 0;
    HIPCHK(hipMemcpyAsync(&w, status, sizeof(w), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (word) *word = w;
    if (w & ROWS_BAD_RANGE) FAIL(-3, std::string(who) + ": a trajectory index lies outside [0, batch)");
    if (w & ROWS_BAD_DUP) FAIL(-3, std::string(who) + ": a destination trajectory is named twice");
    if (w & ROWS_BAD_FLAG_VALUE) FAIL(-3, std::string(who) + ": a row's have_prev / rls_fresh elements are not 0 or 1");
    if (w & ROWS_BAD_FLAG_MIXED)
      FAIL(-3, std::string(who) + (want_hp < 0 ? ": the rows carry different have_prev / rls_fresh flags" : ": the rows' have_prev / rls_fresh flags are not the handle's (only a call that fills the whole handle adopts them)"));
    return 0;
  }
  int state_pack(const int32_t* idx, int count, void* rows, hipStream_t s) override {
    if (count < 0 || (count > 0 && !rows)) FAIL(-3, "kmpc_state_pack: bad arguments");
    if (!rows_supported("kmpc_state_pack")) return -3;
    if (count == 0) return 0;
    { int rc = sync_own(); if (rc) return rc; }
    RowPlan pl;
    if (!row_plan(&pl)) FAIL(-3, "kmpc_state_pack: no row layout for this handle");
    if (idx) { int rc = rows_check("kmpc_state_pack", pl, idx, count, false, nullptr, 0, 0, nullptr, s); if (rc) return rc; }
    else if (count > B) FAIL(-3, "kmpc_state_pack: count exceeds the batch (no index list)");
    // a synchronisation point for the source, as kmpc_state_export is
    { int rc = ensure_dense(s, false); if (rc) return rc; }
    { int rc = forget_tableaux(s); if (rc) return rc; }
    if (core) home.drop_fast();  // (a float32 handle continues from its rounded float32 blocks, as the receiver of the rows will)
    HIPCHK(launch_state_rows_gather<T>(pl, idx, count, B, (T*)rows, prog.have_prev ? 1 : 0, prog.rls_fresh ? 1 : 0, s));
    return 0;
  }
  int state_unpack(const int32_t* idx, int count, const void* rows, hipStream_t s) override {
    if (count < 0 || (count > 0 && !rows)) FAIL(-3, "kmpc_state_unpack: bad arguments");
    if (count > B) FAIL(-3, "kmpc_state_unpack: more rows than the handle has trajectories");
    if (!rows_supported("kmpc_state_unpack")) return -3;
    if (count == 0) return 0;
    { int rc = sync_own(); if (rc) return rc; }
    RowPlan pl;
    if (!row_plan(&pl)) FAIL(-3, "kmpc_state_unpack: no row layout for this handle");
    // the flags belong to the handle: every row must carry its pair, except that a call which fills the whole handle brings its own
    const bool whole = !idx && count == B;
    int word = 0;
    { int rc = rows_check("kmpc_state_unpack", pl, idx, count, idx != nullptr, rows, whole ? -1 : (prog.have_prev ? 1 : 0), whole ? -1 : (prog.rls_fresh ? 1 : 0), &word, s);
      if (rc) return rc; }
    { int rc = ensure_dense(s, true); if (rc) return rc; }  // (first: the trajectories the call leaves alone must be valid in the dense blocks)
    HIPCHK(launch_state_rows_scatter<T>(pl, idx, count, B, (const T*)rows, s));
    home.dense_overwritten();
    { int rc = forget_tableaux(s); if (rc) return rc; }
    if (whole) { prog.have_prev = (word & ROWS_ROW0_HAVE_PREV) != 0; prog.rls_fresh = (word & ROWS_ROW0_RLS_FRESH) != 0; }
    return 0;
  }
  int state_transfer(const int32_t* dst_idx, kmpc_handle* src_h, const int32_t* src_idx, int count, hipStream_t s) override {
    if (!src_h || count < 0) FAIL(-3, "kmpc_state_transfer: bad arguments");
    const kmpc_config& sc = src_h->cfg;
    if (sc.dtype != cfg.dtype || sc.n != n || sc.L != L || sc.N != N || sc.output_kind != cfg.output_kind || src_h->device != device)
      FAIL(-3, "kmpc_state_transfer: the handles differ in n, L, N, dtype, output kind or device");
    Impl<T>* const src = static_cast<Impl<T>*>(src_h);  // (same dtype: the same instantiation)
    if (src->q != q || (cfg.output_kind != KMPC_OUT_LIFT && sc.out_row0 != cfg.out_row0)) FAIL(-3, "kmpc_state_transfer: the handles differ in their output rows");
    if (count > B) FAIL(-3, "kmpc_state_transfer: more rows than the destination has trajectories");
    if (!rows_supported("kmpc_state_transfer (destination)")) return -3;
    if (!src->rows_supported("kmpc_state_transfer (source)")) { err = src->err; return -3; }
    if (count == 0) return 0;
    // gather into this handle's staging rows, then scatter: with src == dst and overlapping lists every destination receives what its
    // source held before the call
    RowPlan pl;
    if (!row_plan(&pl)) FAIL(-3, "kmpc_state_transfer: no row layout for this handle");
    { int rc = sync_own(); if (rc) return rc; }  // (the staging rows may still be read by an earlier transfer on another stream)
    HIPCHK(dRowStage.grow((size_t)count * pl.row_elems));
    { const int rc = src->state_pack(src_idx, count, dRowStage.get(), s); if (rc) { err = "kmpc_state_transfer, source: " + src->err; return rc; } }
    return state_unpack(dst_idx, count, dRowStage.get(), s);
  }

  int profile_enable(int on) override {
    prof = on != 0;
    ev_used = 0;
    prof_steps = 0;
    if (core) core->profile_enable(on);
    return 0;
  }
  int profile_read(double* ms2, int64_t* count, int reset_) override {
    double a0 = 0, a1 = 0;
    int64_t core_steps = 0;
    if (core) {  // (the fused launches of a float32 handle are recorded by its core; both halves keep their totals on a non-resetting read)
      double c2[2] = {0, 0}; int64_t cc = 0;
      if (const int rc = on_core([&](Impl<double>& c) { return c.profile_read(c2, &cc, reset_); })) return rc;
      a0 += c2[0]; a1 += c2[1]; core_steps = cc;
    }
    for (size_t i = 0; i + 2 < ev_used + 0 && i + 2 < ev.size(); i += 3) {
      HIPCHK(hipEventSynchronize(ev[i + 2]));
      float t0 = 0, t1 = 0;
      HIPCHK(hipEventElapsedTime(&t0, ev[i], ev[i + 1]));
      HIPCHK(hipEventElapsedTime(&t1, ev[i + 1], ev[i + 2]));
      a0 += t0; a1 += t1;
    }
    if (ms2) { ms2[0] = a0; ms2[1] = a1; }
    if (count) *count = prof_steps + core_steps;  // control steps covered by the recorded launches
    if (reset_) { ev_used = 0; prof_steps = 0; }
    return 0;
  }

  int64_t algorithmic_bytes() const override {
    // s [ 2 (p^2 + L p + L^2 + n L) + (L + L p + n L + N m + n) + (n + m + q N) ]
    const int64_t s = sizeof(T);
    return s * (2 * ((int64_t)p * p + L * p + L * L + n * L) + (L + L * p + n * L + N * m + n) + (n + m + q * N));
  }
};

// every entry point runs on the device the handle was created on (lazy allocations and launches included), whatever
// the caller's current device is, and leaves the caller's device as it found it
struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) { if (hipGetDevice(&prev) != hipSuccess) prev = -1; if (prev != dev) (void)hipSetDevice(dev); else prev = -1; }
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
// ---------------------------------------------------------------------------------------
extern "C" {

int kmpc_version(void) { return 100; }

int kmpc_create(const kmpc_config* cfg, kmpc_handle** out) {
  if (!cfg || !out) { g_create_error = "kmpc_create: null argument"; return -1; }
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    g_create_error = "kmpc_create: no HIP device visible (libkoopmpc has no CPU path)";
    return -5;
  }
  kmpc_handle* h = nullptr;
  int rc;
  if (cfg->dtype == KMPC_F64) { auto* i = new Impl<double>(); rc = i->init(*cfg); h = i; }
  else if (cfg->dtype == KMPC_F32) { auto* i = new Impl<float>(); rc = i->init(*cfg); h = i; }
  else { g_create_error = "kmpc_create: dtype must be KMPC_F32 or KMPC_F64"; return -2; }
  if (rc) { g_create_error = h->err; delete h; return rc; }
  if (hipGetDevice(&h->device) != hipSuccess) h->device = 0;
  *out = h;
  return 0;
}

int kmpc_destroy(kmpc_handle* h) {
  if (!h) return 0;
  DeviceGuard g(h->device);
  delete h;
  return 0;
}
const char* kmpc_last_error(const kmpc_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

#define NN(h) if (!(h)) return -1; DeviceGuard dev_guard_((h)->device)
// (stream-ordered entry points: when the call returns, the handle's event for this stream is recorded behind what it enqueued)
struct StreamMarkAtExit {
  kmpc_handle* h; hipStream_t s;
  ~StreamMarkAtExit() { h->mark_stream(s); }
};
#define NNS(h, s) NN(h); StreamMarkAtExit mark_at_exit_{(h), (hipStream_t)(s)}
int kmpc_set_encoder(kmpc_handle* h, int layer, const double* W, const double* b, int rows, int cols) { NN(h); return h->set_encoder_layer(layer, W, b, rows, cols); }
int kmpc_set_encoder_layer(kmpc_handle* h, int layer, const double* W, const double* b, int rows, int cols) { return kmpc_set_encoder(h, layer, W, b, rows, cols); }
int kmpc_set_centres(kmpc_handle* h, const double* cx, int L, int n) { NN(h); return h->set_centres(cx, L, n); }
int kmpc_set_rbf_order(kmpc_handle* h, int k) { NN(h); return h->set_rbf_order(k); }
int kmpc_set_model(kmpc_handle* h, const double* A, const double* B, const double* C) { NN(h); return h->set_model(A, B, C); }
int kmpc_set_terminal_weight(kmpc_handle* h, const double* PN) { NN(h); return h->set_terminal_weight(PN); }
int kmpc_terminal_from_dare(kmpc_handle* h, const double* Q, double R, int maxiter, double eps, int per_trajectory,
                            double* PN_out, int32_t* iters_out, void* s) {
  NNS(h, s);
  return h->terminal_from_dare(Q, R, maxiter, eps, per_trajectory, PN_out, iters_out, (hipStream_t)s);
}
int kmpc_solve_dare(const void* A, const void* B, const double* Q, double R, int maxiter, double eps, int nb, int L,
                    void* P, void* K, int32_t* iters, void* s) {
  if (nb == 0) return 0;
  if (!A || !B || !Q || !P || nb < 0 || L < 1 || L > 64 || maxiter < 1) return -3;
  DevBuf<double> dQl;
  if (dQl.alloc((size_t)L * L) != hipSuccess) return -1001;
  int rc = 0;
  if (hipMemcpyAsync(dQl, Q, sizeof(double) * (size_t)L * L, hipMemcpyHostToDevice, (hipStream_t)s) != hipSuccess) rc = -1002;
  DareArgs d{};
  d.nb = nb; d.L = L; d.q = 0; d.maxiter = maxiter; d.shared_model = 0;
  d.A = (const double*)A; d.strideA = (long)L * L; d.ldA = L;
  d.B = (const double*)B; d.strideB = L; d.incB = 1;
  d.Q = dQl; d.R = R; d.eps = eps; d.Co = nullptr; d.strideC = 0;
  d.P = (double*)P; d.K = (double*)K; d.PN = nullptr; d.pn_sub_diag = 0.0; d.iters = iters;
  if (!rc && launch_dare(d, (hipStream_t)s) != hipSuccess) rc = -1003;
  if (hipStreamSynchronize((hipStream_t)s) != hipSuccess && !rc) rc = -1004;
  return rc;
}
int kmpc_set_terminal_refresh(kmpc_handle* h, int every, const double* Q, double R, int maxiter, double eps) { NN(h); return h->set_terminal_refresh(every, Q, R, maxiter, eps); }
int kmpc_rollout_is_fused(const kmpc_handle* h) { NN(h); return h->rollout_is_fused(); }
int kmpc_rollout_variant(const kmpc_handle* h) { NN(h); return h->last_rollout_variant; }
int kmpc_rollout_resident(const kmpc_handle* h, int* lds_bytes) {
  NN(h);
  if (lds_bytes) *lds_bytes = h->last_rollout_lds;
  return h->last_rollout_resident;
}
// Makes (or finds) the plug-in a handle of this configuration would load -- no device needed: hipcc cross-compiles.  For builds that
// want the kernel cache filled before the first kmpc_create (__graft_entry__.build(), an installer, the first rank of a node).
static void put_text(char* text, int text_bytes, const std::string& t) { if (text && text_bytes > 0) snprintf(text, (size_t)text_bytes, "%s", t.c_str()); }
// 1: made or found (*text: the object), -1: failed (*text: why), 0: the configuration has no object of this variant
static int prebuild_variant(int n, int L, int N, int q, bool rbf, int hidden_eff, int batch, bool io32, bool term, bool diag, std::string* text, bool rbf_kinds) {
  const EncoderShape e = encoder_shape(hidden_eff, 0, n, L);
  RolloutPluginKey k{};
  if (!rollout_plugin_key(n, L, N, q, rbf, e.Lp, e.KS, e.Hp, batch, io32, &k, term, diag, rbf_kinds)) return 0;
  if (!rollout_plugin_get(k, text)) return -1;
  *text = rollout_plugin_describe(k);
  return 1;
}
int kmpc_rollout_plugin_prebuild(int n, int L, int N, int out_rows, int lift_kind, int hidden_eff, int batch, int dtype, char* text, int text_bytes) {
  auto say = [&](int code, const std::string& t) { put_text(text, text_bytes, t); return code; };
  const bool rbf = lift_kind != KMPC_LIFT_MLP, io32 = dtype == KMPC_F32;
  const int q = out_rows > 0 ? out_rows : n;
  if (lift_kind < KMPC_LIFT_MLP || lift_kind > KMPC_LIFT_RBF_POLYHARMONIC) return say(-3, "lift_kind must be one of KMPC_LIFT_* (0..6)");  // (as kmpc_create)
  if (n != 2 || L < 1 || N < 1 || batch < 1 || (!rbf && (hidden_eff < 1 || hidden_eff > 128)) || (dtype != KMPC_F32 && dtype != KMPC_F64)) return say(-3, "bad arguments");
  if (!(io32 ? rollout_io32_available(n, L, N, q, rbf) : rollout_fused_available<double>(n, L, N, q, 64, rbf))) return say(2, "no fused roll-out for this configuration");
  std::string t;
  const int rc = prebuild_variant(n, L, N, q, rbf, hidden_eff, batch, io32, false, false, &t, lift_kind >= KMPC_LIFT_RBF_GAUSS);
  return rc == 0 ? say(0, "built-in instantiation of libkoopmpc.so") : say(rc, t);
}
int kmpc_rollout_diag_plugin_prebuild(int n, int L, int N, int out_rows, int lift_kind, int hidden_eff, int batch, int with_term, char* text, int text_bytes) {
  auto say = [&](int code, const std::string& t) { put_text(text, text_bytes, t); return code; };
  const bool rbf = lift_kind != KMPC_LIFT_MLP;
  const int q = out_rows > 0 ? out_rows : n;
  if (lift_kind < KMPC_LIFT_MLP || lift_kind > KMPC_LIFT_RBF_POLYHARMONIC) return say(-3, "lift_kind must be one of KMPC_LIFT_* (0..6)");  // (as kmpc_create)
  if (n != 2 || L < 1 || N < 1 || batch < 1 || (!rbf && (hidden_eff < 1 || hidden_eff > 128))) return say(-3, "bad arguments");
  std::string t;
  const int rc = rollout_fused_available<double>(n, L, N, q, 64, rbf) ? prebuild_variant(n, L, N, q, rbf, hidden_eff, batch, false, with_term != 0, true, &t, lift_kind >= KMPC_LIFT_RBF_GAUSS) : 0;
  return rc == 0 ? say(2, "no fused diagnostics variant for this configuration (per-step launches)") : say(rc, t);
}
int kmpc_rollout_plugin_status(const kmpc_handle* h, char* text, int text_bytes) {
  if (!h) return -100;
  std::string t;
  const int rc = h->rollout_plugin_status(&t);
  put_text(text, text_bytes, t);
  return rc;
}
// The placement pass of the fused roll-out as a function of its own (tests, tools): perm_dev receives, in its first B entries, the
// slot -> trajectory table of the card deal for the per-trajectory work counters work_dev[B]; it must hold 3 B int32 (the sort's buffers).
int kmpc_rank_by_work(const int32_t* work_dev, int B, int32_t* perm_dev, void* s) {
  if (!work_dev || !perm_dev) return -3;
  const hipError_t e = kmpc::launch_place(work_dev, B, perm_dev, reinterpret_cast<uint32_t*>(perm_dev + B), (hipStream_t)s);
  return e == hipSuccess ? 0 : -(1000 + (int)e);
}
int kmpc_set_rollout_workgroup(int trajectories) {
  if (trajectories != 0 && trajectories != 4 && trajectories != 8 && trajectories != 16) return -1;
  kmpc::set_rollout_workgroup(trajectories);
  return 0;
}
int kmpc_reset(kmpc_handle* h, void* s) { NNS(h, s); return h->reset((hipStream_t)s); }
int kmpc_state_init(kmpc_handle* h, double P0_scale, double barQ0_scale, void* s) { NNS(h, s); return h->state_init(P0_scale, barQ0_scale, (hipStream_t)s); }
int kmpc_state_init_from(kmpc_handle* h, const double* K_A0, const double* P0, const double* barX0, const double* barQ0, void* s) {
  NNS(h, s);
  return h->state_init_from(K_A0, P0, barX0, barQ0, (hipStream_t)s);
}
int kmpc_lift(kmpc_handle* h, const void* X, void* Psi, int B, void* s) { NNS(h, s); return h->lift(X, Psi, B, (hipStream_t)s); }
int kmpc_rls_update(kmpc_handle* h, const void* psi, const void* u, const void* psin, const void* xn, int B, void* s) { NNS(h, s); return h->rls_update(psi, u, psin, xn, B, (hipStream_t)s); }
int kmpc_get_model(kmpc_handle* h, void* A, void* B, void* C, void* s) { NNS(h, s); return h->get_model(A, B, C, (hipStream_t)s); }
int kmpc_condense(kmpc_handle* h, const void* psi, const void* ref, int rpt, void* H, void* f, int B, void* s) { NNS(h, s); return h->condense(psi, ref, rpt, H, f, nullptr, B, (hipStream_t)s); }
int kmpc_condense_cost(kmpc_handle* h, const void* psi, const void* ref, int rpt, void* H, void* f, void* c, int B, void* s) { NNS(h, s); return h->condense(psi, ref, rpt, H, f, c, B, (hipStream_t)s); }
int kmpc_mpc_solve(kmpc_handle* h, const void* A, const void* Bv, const void* C, int shared, const void* psi, const void* ref, int rpt,
                   double lb, double ub, double Qw, double Rw, const double* PN, void* U, void* U0, void* fun, int32_t* st, int32_t* it,
                   int B, void* s) {
  NNS(h, s);
  return h->mpc_solve(A, Bv, C, shared, psi, ref, rpt, lb, ub, Qw, Rw, PN, U, U0, fun, st, it, B, (hipStream_t)s);
}
int kmpc_generate_and_fit(kmpc_handle* h, int plant, const void* X0, const void* U, int n_traj, int n_steps, double hs, double ridge,
                          int init_rls, void* A, void* B, void* C, void* Xo, void* Yo, void* s) {
  NNS(h, s);
  return h->generate_and_fit(plant, X0, U, n_traj, n_steps, hs, ridge, init_rls, A, B, C, Xo, Yo, (hipStream_t)s);
}
int kmpc_qp_solve(kmpc_handle* h, const void* H, const void* f, void* U, int32_t* st, int32_t* it, int B, void* s) { NNS(h, s); return h->qp_solve(H, f, U, st, it, B, (hipStream_t)s); }
int kmpc_step(kmpc_handle* h, const void* X, const void* ref, int rpt, void* U0, void* Useq, int32_t* st, int32_t* it, void* s) { NNS(h, s); return h->step(X, ref, rpt, U0, Useq, st, it, (hipStream_t)s); }
int kmpc_set_applied_input(kmpc_handle* h, const void* U, int B, void* s) { NNS(h, s); return h->set_applied_input(U, B, (hipStream_t)s); }
int kmpc_set_online_update(kmpc_handle* h, int on) { NN(h); return h->set_online_update(on); }
int kmpc_plant_step(kmpc_handle* h, int plant, void* X, const void* U, double hs, int sw, int B, void* s) { NNS(h, s); return h->plant_step(plant, X, U, hs, sw, B, (hipStream_t)s); }
int kmpc_rollout(kmpc_handle* h, int plant, void* X, const void* ref, int rpt, int steps, int step0, int sw, double hs, void* Ulog, void* Xlog, int32_t* st, int32_t* it, void* s) { NNS(h, s); return h->rollout(plant, X, ref, rpt, steps, step0, sw, hs, Ulog, Xlog, st, it, (hipStream_t)s); }
int kmpc_set_rollout_diagnostics(kmpc_handle* h, int on) { NN(h); return h->set_rollout_diagnostics(on); }
int kmpc_estimator_status(const kmpc_handle* h, double* P0, double* barQ0) { if (!h) return -1; return h->estimator_status(P0, barQ0); }
int kmpc_get_prev_transition(kmpc_handle* h, void* psi_prev, void* u_prev, void* s) { NNS(h, s); return h->get_prev_transition(psi_prev, u_prev, (hipStream_t)s); }
int kmpc_rollout_diag(kmpc_handle* h, int plant, void* X, const void* ref, int rpt, int steps, int step0, int sw, double hs, void* Ulog, void* Xlog,
                      void* Psilog, void* dAlog, void* dBlog, void* dClog, int32_t* st, int32_t* it, void* s) {
  NNS(h, s);
  return h->rollout_diag(plant, X, ref, rpt, steps, step0, sw, hs, Ulog, Xlog, Psilog, dAlog, dBlog, dClog, st, it, (hipStream_t)s);
}
int kmpc_offline_fit(kmpc_handle* h, const void* X, const void* Y, const void* U, int M, double ridge, int init_rls, void* A, void* B, void* C, void* s) { NNS(h, s); return h->offline_fit(X, Y, U, M, ridge, init_rls, A, B, C, (hipStream_t)s); }
int64_t kmpc_gram_elems(const kmpc_handle* h) { return h ? h->gram_elems() : -1; }
// The one collective of the path for native callers: sum of the per-rank Gram blocks over an RCCL communicator.
// RCCL is resolved at run time from the process (the caller created the communicator with the RCCL it loaded; under
// PyTorch that is torch's own copy and KoopmanMPC.shared_step goes through torch.distributed instead) -- the library
// itself does not link against it.
int kmpc_allreduce_gram(kmpc_handle* h, double* delta, void* nccl_comm, void* s) {
  NNS(h, s);
  if (!delta || !nccl_comm) return -3;
  typedef ncclResult_t (*allreduce_fn)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t);
  const allreduce_fn fn = (allreduce_fn)resolve_nccl_allreduce();
  if (!fn) return -4;  // no RCCL in this process
  const ncclResult_t rc = fn(delta, delta, (size_t)h->gram_elems(), ncclDouble, ncclSum, (ncclComm_t)nccl_comm, (hipStream_t)s);
  return rc == ncclSuccess ? 0 : -(2000 + (int)rc);
}
int kmpc_shared_local_gram(kmpc_handle* h, const void* X, double* delta, void* s) { NNS(h, s); return h->shared_local_gram(X, delta, (hipStream_t)s); }
int kmpc_gram_accumulate(kmpc_handle* h, const void* X, double* delta, void* s) { return kmpc_shared_local_gram(h, X, delta, s); }
int kmpc_shared_solve(kmpc_handle* h, const double* delta, const void* ref, void* U0, void* Useq, int32_t* st, int32_t* it, void* s) { NNS(h, s); return h->shared_solve(delta, ref, U0, Useq, st, it, (hipStream_t)s); }
int kmpc_shared_solve_plant(kmpc_handle* h, const double* delta, const void* ref, void* U0, void* Useq, int32_t* st, int32_t* it,
                            int plant, void* X, int switched, double hstep, void* s) {
  NNS(h, s);
  return h->shared_solve_plant(delta, ref, U0, Useq, st, it, plant, X, switched, hstep, (hipStream_t)s);
}
int kmpc_shared_get_model(kmpc_handle* h, void* A, void* B, void* C, void* s) { NNS(h, s); return h->shared_get_model(A, B, C, (hipStream_t)s); }
int kmpc_shared_rollout(kmpc_handle* h, int plant, void* X, const void* ref, int steps, int step0, int switch_step, double hstep, void* comm,
                        void* Ulog, void* Xlog, void* U0out, void* Useq, int32_t* st, int32_t* it, void* s) {
  NNS(h, s);
  return h->shared_rollout(plant, X, ref, steps, step0, switch_step, hstep, comm, Ulog, Xlog, U0out, Useq, st, it, (hipStream_t)s);
}
int64_t kmpc_state_bytes(const kmpc_handle* h) { return h ? h->state_bytes() : -1; }
int kmpc_state_export(kmpc_handle* h, void* blob, int64_t bytes) { NN(h); return h->state_export(blob, bytes); }
int kmpc_state_import(kmpc_handle* h, const void* blob, int64_t bytes) { NN(h); return h->state_import(blob, bytes); }
int64_t kmpc_state_row_elems(const kmpc_handle* h) { return h ? h->state_row_elems() : -1; }
int kmpc_state_pack(kmpc_handle* h, const int32_t* idx, int count, void* rows, void* s) { NNS(h, s); return h->state_pack(idx, count, rows, (hipStream_t)s); }
int kmpc_state_unpack(kmpc_handle* h, const int32_t* idx, int count, const void* rows, void* s) { NNS(h, s); return h->state_unpack(idx, count, rows, (hipStream_t)s); }
int kmpc_state_transfer(kmpc_handle* dst, const int32_t* dst_idx, kmpc_handle* src, const int32_t* src_idx, int count, void* s) {
  NNS(dst, s);
  if (!src) return -1;
  StreamMarkAtExit mark_src{src, (hipStream_t)s};  // (the source's gather runs on this stream too)
  return dst->state_transfer(dst_idx, src, src_idx, count, (hipStream_t)s);
}
int kmpc_profile_enable(kmpc_handle* h, int on) { NN(h); return h->profile_enable(on); }
int kmpc_profile_read(kmpc_handle* h, double* ms2, int64_t* count, int reset) { NN(h); return h->profile_read(ms2, count, reset); }
int64_t kmpc_algorithmic_bytes_per_step(const kmpc_handle* h) { return h ? h->algorithmic_bytes() : -1; }

}  // extern "C"

// state_rows.h -- the list of a handle's state blocks (Sections, filled by Impl::sections in api.hip) and the packed row of
// kmpc_state_pack / kmpc_state_unpack / kmpc_state_transfer that is derived from it (build_row_plan).  Plain structs and host
// arithmetic: api.hip builds the plan, the row kernels of aux_kernels.hip take it by value, tests/state_rows_check.cpp runs it on the CPU.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

namespace kmpc {

// one section of a blob as a handle holds it, and the ordered list of them (Impl::sections)
struct Section {
  void* ptr; size_t elem, count;  // element size, elements
  size_t panel_rows = 0;          // 0: [B][count / B], trajectory-major; else a [panel_rows][B] panel, a trajectory owns one column
  size_t bytes() const { return elem * count; }
};
struct Sections {
  Section s[11];
  int n = 0, n_traj = 0;  // n_traj: the leading sections that hold per-trajectory state (P .. u_prev)
  void add(void* ptr, size_t elem, size_t count, size_t panel_rows = 0) { s[n++] = Section{ptr, elem, count, panel_rows}; }
  int64_t payload_bytes() const { int64_t b = 0; for (int i = 0; i < n; ++i) b += (int64_t)s[i].bytes(); return b; }  // (a blob: header + this)
};

// One per-trajectory section as the row kernels walk it: element j of trajectory b lives at base + (b stride + j step) elements and
// at element off + j of the packed row.  step = 1: a contiguous block (P .. psi_prev, u_prev); else a panel column (warm: step = B).
struct RowSeg {
  char* base;
  long stride, step;
  int off, len;
};
// the packed row of one handle: its segments in blob order, the two flag elements behind them, zero padding up to row_elems
struct RowPlan {
  static constexpr int kMaxSeg = 8;
  RowSeg seg[kMaxSeg];
  int nseg = 0, elem = 0;  // elem: sizeof(T)
  int flag_off = 0;        // have_prev at flag_off, rls_fresh at flag_off + 1
  int row_elems = 0;       // elements of a row: flag_off + 2 rounded up to a multiple of 16 bytes
};

// the plan of the leading n_traj sections of `t` for a batch of B; false: `t` is not a list a row can be made of
inline bool build_row_plan(const Sections& t, int B, RowPlan* out) {
  RowPlan pl;
  if (B < 1 || t.n_traj < 1 || t.n_traj > RowPlan::kMaxSeg || t.n_traj > t.n) return false;
  pl.elem = (int)t.s[0].elem;
  if (pl.elem != 4 && pl.elem != 8) return false;
  long off = 0;
  for (int i = 0; i < t.n_traj; ++i) {
    const Section& sec = t.s[i];
    if ((int)sec.elem != pl.elem || sec.count % (size_t)B != 0) return false;
    RowSeg& g = pl.seg[pl.nseg++];
    g.base = (char*)sec.ptr;
    g.off = (int)off;
    if (sec.panel_rows) {
      if (sec.count != sec.panel_rows * (size_t)B) return false;
      g.len = (int)sec.panel_rows; g.stride = 1; g.step = B;
    } else {
      g.len = (int)(sec.count / (size_t)B); g.stride = g.len; g.step = 1;
    }
    off += g.len;
  }
  const long per16 = 16 / pl.elem;
  pl.flag_off = (int)off;
  pl.row_elems = (int)((off + 2 + per16 - 1) / per16 * per16);
  *out = pl;
  return true;
}

// status word of state_rows_check_kernel: what was wrong (any of the first four), and the flags of row 0
enum { ROWS_BAD_RANGE = 1, ROWS_BAD_DUP = 2, ROWS_BAD_FLAG_VALUE = 4, ROWS_BAD_FLAG_MIXED = 8, ROWS_ROW0_HAVE_PREV = 16, ROWS_ROW0_RLS_FRESH = 32 };

// ---- the row kernels (aux_kernels.hip).  Declared here and not in kernels.h: that header is hashed into every roll-out plug-in object,
// and these calls touch no roll-out kernel.
// Validation, before any copy: reads idx[0 .. count) (null: 0 .. count-1) and, with `rows`, the two flag elements of every row; ORs
// ROWS_* into *status (zeroed by the launcher).  mark (int32[B], zeroed by the launcher; null: no duplicate check).  want_have_prev /
// want_rls_fresh: the pair every row must carry; -1: the pair of row 0 (ROWS_BAD_FLAG_MIXED otherwise).
hipError_t launch_state_rows_check(const int32_t* idx, int count, int B, int32_t* mark, const void* rows, const RowPlan& pl, int want_have_prev,
                                   int want_rls_fresh, int32_t* status, hipStream_t s);
// rows[r] <- trajectory idx[r] (gather; the flags as given) / trajectory idx[r] <- rows[r] (scatter; the flag elements are not read).
// One workgroup per row; a row whose index lies outside [0, B) is skipped.
template <typename T> hipError_t launch_state_rows_gather(const RowPlan& pl, const int32_t* idx, int count, int B, T* rows, int have_prev, int rls_fresh, hipStream_t s);
template <typename T> hipError_t launch_state_rows_scatter(const RowPlan& pl, const int32_t* idx, int count, int B, const T* rows, hipStream_t s);

}  // namespace kmpc

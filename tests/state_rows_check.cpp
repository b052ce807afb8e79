// Stand-alone host program for tests/test_state_rows_cpu.py: the host code of csrc/state_rows.h that turns a handle's list of state
// blocks (Sections, as Impl::sections of api.hip fills it) into the segment table of a packed row.  Built with
// -fsanitize=address,undefined; exits 0 when every check holds.  Every section is a host block of exactly its size, and the program walks
// every address the row kernels would form from the table, so an offset, stride or length that is off by one is an AddressSanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "state_rows.h"

#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      std::exit(1);                                                      \
    }                                                                    \
  } while (0)

static long even_up(long v) { return (v + 1) & ~1L; }

// the blocks of a handle (n, L, N, batch B, element size elem) and its list, in the blob's order; every element holds its own global number
struct Handle {
  int n, L, N, B, elem;
  long sP, sK, sQ, sC;
  std::vector<std::vector<char>> blocks;
  kmpc::Sections t;
  long next_id = 0;
  void put(std::vector<char>& blk, long i, double v) const {
    if (elem == 8) std::memcpy(blk.data() + 8 * i, &v, 8);
    else { const float f = (float)v; std::memcpy(blk.data() + 4 * i, &f, 4); }
  }
  void add(long count, long panel_rows = 0) {
    blocks.emplace_back((size_t)count * elem);
    for (long i = 0; i < count; ++i) put(blocks.back(), i, (double)next_id++);
    t.add(blocks.back().data(), (size_t)elem, (size_t)count, (size_t)panel_rows);
  }
  Handle(int n_, int L_, int N_, int B_, int elem_) : n(n_), L(L_), N(N_), B(B_), elem(elem_) {
    const long p = L + 1;
    sP = even_up(p * p); sK = even_up((long)L * p); sQ = even_up((long)L * L); sC = even_up((long)n * L);
    blocks.reserve(11);
    add(sP * B); add(sK * B); add(sQ * B); add(sC * B); add((long)L * B); add((long)N * B, N); add(B);
    t.n_traj = t.n;
    add(7);  // (a section behind the per-trajectory ones, as a terminal block is: no part of a row)
  }
};

static double value_at(const char* p, int elem) {
  if (elem == 8) { double v; std::memcpy(&v, p, 8); return v; }
  float f; std::memcpy(&f, p, 4); return (double)f;
}

static void check_set(int n, int L, int N, int B, int elem) {
  Handle h(n, L, N, B, elem);
  kmpc::RowPlan pl;
  CHECK(kmpc::build_row_plan(h.t, B, &pl));
  // offsets, lengths and row_elems as the format comment in api.hip gives them
  const long want_len[7] = {h.sP, h.sK, h.sQ, h.sC, L, N, 1};
  CHECK(pl.nseg == 7 && pl.elem == elem);
  long off = 0;
  for (int k = 0; k < 7; ++k) {
    CHECK(pl.seg[k].off == off && pl.seg[k].len == want_len[k] && pl.seg[k].base == (char*)h.t.s[k].ptr);
    if (k == 5) CHECK(pl.seg[k].stride == 1 && pl.seg[k].step == B);
    else CHECK(pl.seg[k].stride == want_len[k] && pl.seg[k].step == 1);
    off += want_len[k];
  }
  CHECK(pl.flag_off == off && pl.row_elems >= off + 2 && pl.row_elems < off + 2 + 16 / elem && ((long)pl.row_elems * elem) % 16 == 0);
  // float64 segments in front of warm start on 16 bytes inside the row (the even strides)
  if (elem == 8) for (int k = 0; k < 5; ++k) CHECK(((long)pl.seg[k].off * elem) % 16 == 0);
  else for (int k = 0; k < 5; ++k) CHECK(((long)pl.seg[k].off * elem) % 8 == 0);
  // gather every trajectory as the kernels address it: every element of the per-trajectory blocks is read exactly once, in blob order
  std::vector<char> rows((size_t)B * pl.row_elems * elem);
  long total = 0;
  for (int k = 0; k < 7; ++k) total += (long)h.t.s[k].count;
  std::vector<int> seen((size_t)total, 0);
  for (int b = 0; b < B; ++b)
    for (int k = 0; k < pl.nseg; ++k)
      for (int j = 0; j < pl.seg[k].len; ++j) {
        const char* src = pl.seg[k].base + ((long)b * pl.seg[k].stride + (long)j * pl.seg[k].step) * elem;
        char* dst = rows.data() + ((size_t)b * pl.row_elems + pl.seg[k].off + j) * elem;
        std::memcpy(dst, src, (size_t)elem);
        const long id = (long)value_at(src, elem);
        CHECK(id >= 0 && id < total);
        seen[(size_t)id] += 1;
      }
  for (long i = 0; i < total; ++i) CHECK(seen[(size_t)i] == 1);
  // a row's segment is the blob's slice of that trajectory: contiguous blocks whole, the panel column element by element
  for (int b = 0; b < B; ++b) {
    const char* row = rows.data() + (size_t)b * pl.row_elems * elem;
    for (int k = 0; k < 7; ++k) {
      const char* blk = (const char*)h.t.s[k].ptr;
      if (k != 5) CHECK(std::memcmp(row + (size_t)pl.seg[k].off * elem, blk + (size_t)b * want_len[k] * elem, (size_t)want_len[k] * elem) == 0);
      else for (int j = 0; j < N; ++j) CHECK(std::memcmp(row + (size_t)(pl.seg[k].off + j) * elem, blk + ((size_t)j * B + b) * elem, (size_t)elem) == 0);
    }
  }
}

int main() {
  // the four dimension sets of tests/test_gpu_state_rows.py, at the batches it uses and at an odd one
  const int sets[4][4] = {{2, 20, 20, 8}, {2, 8, 30, 8}, {3, 9, 5, 8}, {2, 20, 20, 4}};
  const int batches[5] = {32, 16, 1, 3, 24};
  for (const auto& s : sets)
    for (int B : batches) check_set(s[0], s[1], s[2], B, s[3]);
  // row_elems of the four sets (P K Q C psi warm u + 2 flags, rounded up to 16 bytes)
  {
    const int want[4] = {1346, 276, 318, 1348};  // 1343 + 2, 273 + 2, 315 + 2, 1343 + 2 elements, rounded up to 2 / 2 / 2 / 4
    for (int i = 0; i < 4; ++i) {
      Handle h(sets[i][0], sets[i][1], sets[i][2], 32, sets[i][3]);
      kmpc::RowPlan pl;
      CHECK(kmpc::build_row_plan(h.t, 32, &pl) && pl.row_elems == want[i]);
    }
  }
  // lists no row can be made of
  {
    Handle h(2, 3, 3, 4, 8);
    kmpc::RowPlan pl;
    CHECK(!kmpc::build_row_plan(h.t, 0, &pl));
    CHECK(!kmpc::build_row_plan(h.t, 3, &pl));  // (the blocks are no multiple of this batch)
    kmpc::Sections t = h.t;
    t.n_traj = 0;
    CHECK(!kmpc::build_row_plan(t, 4, &pl));
    t = h.t; t.s[2].elem = 4;
    CHECK(!kmpc::build_row_plan(t, 4, &pl));
    t = h.t; t.s[5].panel_rows = 2;
    CHECK(!kmpc::build_row_plan(t, 4, &pl));
  }
  std::puts("state rows ok");
  return 0;
}

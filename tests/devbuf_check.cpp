// Stand-alone host program for tests/test_host_cpu.py: csrc/devbuf.h on a counting host allocator that fails on the k-th request.
// Built with -fsanitize=address,undefined; exits 0 when every check holds.
#include <cstdio>
#include <cstdlib>
#include <set>

#include "devbuf.h"

#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      std::exit(1);                                                      \
    }                                                                    \
  } while (0)

struct HostMem {
  static int requests, fail_at, frees;  // fail_at: the request (counted from 1) that is refused, 0: none
  static std::set<void*> live;
  static void start(int fail) { CHECK(live.empty()); requests = frees = 0; fail_at = fail; }
  static hipError_t alloc(void** p, size_t bytes) {
    if (++requests == fail_at) return hipErrorOutOfMemory;
    *p = std::malloc(bytes ? bytes : 1);
    CHECK(*p && live.insert(*p).second);
    return hipSuccess;
  }
  static void release(void* p) {
    CHECK(live.erase(p) == 1);  // a block of ours that has not been freed yet
    ++frees;
    std::free(p);
  }
};
int HostMem::requests = 0, HostMem::fail_at = 0, HostMem::frees = 0;
std::set<void*> HostMem::live;

template <typename U> using Buf = kmpc::DevBuf<U, HostMem>;

// the shape of Impl::dare_buffers: three blocks for nb models, all or none
struct Dare {
  Buf<double> P, W;
  Buf<int> it;
  int cap = 0;
  hipError_t buffers(int nb) {
    if (cap >= nb) return hipSuccess;
    const hipError_t e = kmpc::replace_together(P, (size_t)nb * 9, it, (size_t)nb, W, (size_t)nb * 4);
    if (e == hipSuccess) cap = nb;
    return e;
  }
};

int main() {
  // every block is freed exactly once: destruction, reset, move construction, move assignment over a live block
  HostMem::start(0);
  {
    Buf<double> a, b, c;
    CHECK(a.alloc(7) == hipSuccess && a.capacity() == 7 && a.get() != nullptr);
    a[6] = 1.0;                                        // (reads as a pointer)
    CHECK(a.alloc(3) == hipErrorInvalidValue && a.capacity() == 7 && HostMem::requests == 1);  // alloc is for an empty buffer
    CHECK(b.alloc(2) == hipSuccess && c.alloc(5) == hipSuccess);
    double* const pa = a;
    Buf<double> d(std::move(a));
    CHECK(d.get() == pa && d.capacity() == 7 && a.get() == nullptr && a.capacity() == 0 && HostMem::frees == 0);
    b = std::move(d);                                  // b's block goes, a's former block is b's
    CHECK(b.get() == pa && b.capacity() == 7 && d.get() == nullptr && HostMem::frees == 1 && HostMem::live.size() == 2);
    c.reset();
    CHECK(!c && c.capacity() == 0 && HostMem::frees == 2);
    c.reset();
    CHECK(HostMem::frees == 2);
  }
  CHECK(HostMem::live.empty() && HostMem::requests == 3 && HostMem::frees == 3);

  // ensure on a non-empty buffer makes no request; on an empty one it is alloc
  HostMem::start(0);
  {
    Buf<float> a;
    CHECK(a.ensure(4) == hipSuccess && HostMem::requests == 1 && a.capacity() == 4);
    float* const pa = a;
    CHECK(a.ensure(4) == hipSuccess && a.ensure(400) == hipSuccess && HostMem::requests == 1 && a.get() == pa && a.capacity() == 4);
  }
  CHECK(HostMem::live.empty() && HostMem::frees == 1);

  // grow: new block first, then the old one goes; a refused request leaves pointer and capacity as they were
  HostMem::start(3);
  {
    Buf<int> a;
    CHECK(a.grow(8) == hipSuccess && a.capacity() == 8 && HostMem::requests == 1);
    CHECK(a.grow(8) == hipSuccess && a.grow(2) == hipSuccess && HostMem::requests == 1);  // large enough already
    CHECK(a.grow(16) == hipSuccess && a.capacity() == 16 && HostMem::requests == 2 && HostMem::frees == 1);
    int* const pa = a;
    a[15] = 5;
    CHECK(a.grow(32) == hipErrorOutOfMemory && a.get() == pa && a.capacity() == 16 && a[15] == 5 && HostMem::frees == 1);
    CHECK(a.grow(32) == hipSuccess && a.capacity() == 32 && HostMem::frees == 2);  // (request 4)
  }
  CHECK(HostMem::live.empty() && HostMem::requests == 4 && HostMem::frees == 3);

  // three buffers grown together: a refusal at request 1, 2 or 3 frees what the call had allocated and leaves the old blocks
  for (int fail = 0; fail <= 3; ++fail) {
    HostMem::start(0);
    {
      Dare d;
      CHECK(d.buffers(2) == hipSuccess && d.cap == 2 && HostMem::requests == 3);
      CHECK(d.buffers(1) == hipSuccess && HostMem::requests == 3);
      double* const pP = d.P; int* const pit = d.it; double* const pW = d.W;
      d.P[17] = 3.0; d.it[1] = 4; d.W[7] = 5.0;
      HostMem::fail_at = fail ? 3 + fail : 0;
      const hipError_t e = d.buffers(5);
      if (fail) {
        CHECK(e == hipErrorOutOfMemory && d.cap == 2 && d.P.get() == pP && d.it.get() == pit && d.W.get() == pW);
        CHECK(d.P.capacity() == 18 && d.it.capacity() == 2 && d.W.capacity() == 8);
        CHECK(d.P[17] == 3.0 && d.it[1] == 4 && d.W[7] == 5.0);
        CHECK(HostMem::requests == 3 + fail && HostMem::frees == fail - 1 && HostMem::live.size() == 3);
      } else {
        CHECK(e == hipSuccess && d.cap == 5 && d.P.capacity() == 45 && d.it.capacity() == 5 && d.W.capacity() == 20);
        CHECK(HostMem::requests == 6 && HostMem::frees == 3 && HostMem::live.size() == 3);
        d.P[44] = 1.0; d.it[4] = 1; d.W[19] = 1.0;
      }
    }
    CHECK(HostMem::live.empty() && HostMem::frees == HostMem::requests - (fail ? 1 : 0));
  }
  std::puts("devbuf ok");
  return 0;
}

// devbuf.h -- owning device buffers of api.hip.  Host code only: no kernel source includes this file, and it is no part of a
// roll-out plug-in's sources.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <utility>

namespace kmpc {

// the two device calls of a buffer (a test replaces them with a host allocator that counts and fails on demand)
struct HipMem {
  static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static void release(void* p) { (void)hipFree(p); }
};

// `count` elements of U on the device, freed when the buffer goes out of scope.  Move-only; reads as a U* wherever one is expected.
// A failed call returns the error and leaves the buffer as it was.
template <typename U, typename Mem = HipMem>
class DevBuf {
  U* p_ = nullptr;
  size_t cap_ = 0;

 public:
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_; cap_ = o.cap_;
      o.p_ = nullptr; o.cap_ = 0;
    }
    return *this;
  }
  ~DevBuf() { reset(); }

  operator U*() const { return p_; }
  U* get() const { return p_; }
  size_t capacity() const { return cap_; }  // elements

  void reset() {
    if (p_) Mem::release(p_);
    p_ = nullptr; cap_ = 0;
  }
  // an empty buffer gets its block
  hipError_t alloc(size_t count) {
    if (p_) return hipErrorInvalidValue;
    void* p = nullptr;
    const hipError_t e = Mem::alloc(&p, sizeof(U) * count);
    if (e != hipSuccess) return e;
    p_ = static_cast<U*>(p); cap_ = count;
    return hipSuccess;
  }
  // lazy allocation: the first call allocates, every later one does nothing
  hipError_t ensure(size_t count) { return p_ ? hipSuccess : alloc(count); }
  // at least `count` elements; the contents are not kept.  The new block is allocated before the old one is released.
  hipError_t grow(size_t count) {
    if (count <= cap_) return hipSuccess;
    DevBuf fresh;
    const hipError_t e = fresh.alloc(count);
    if (e == hipSuccess) *this = std::move(fresh);
    return e;
  }
};

// replace_together(a, na, b, nb, ...): every buffer gets a new block of its count, or -- when one of the requests fails -- none does:
// the blocks allocated so far are freed and the old ones stay.  The contents are not kept.
inline hipError_t replace_together() { return hipSuccess; }
template <typename U, typename Mem, typename... Rest>
hipError_t replace_together(DevBuf<U, Mem>& buf, size_t count, Rest&&... rest) {
  DevBuf<U, Mem> fresh;
  hipError_t e = fresh.alloc(count);
  if (e == hipSuccess) e = replace_together(std::forward<Rest>(rest)...);
  if (e == hipSuccess) buf = std::move(fresh);  // (every later request has succeeded)
  return e;
}

}  // namespace kmpc

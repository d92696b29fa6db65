// gnnb_mem.h -- move-only owners of device memory (hipMalloc / hipFree) and pinned host memory (hipHostMalloc / hipHostFree).
//
// Everything the handle, the bound network and the trainer allocate is held by one of these, so dropping the owner releases the
// memory: no free lists.  Kernel argument structs keep plain pointers, filled from get().  Every operation returns the
// hipError_t of the runtime call that failed (hipSuccess otherwise), so HIPCHK(buf.alloc(n)) reports expression and line as for a raw call.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

namespace gnnb {

template <class T, bool PINNED>
class HipBuf {
  T* p_ = nullptr;
  size_t n_ = 0;      // elements

 public:
  HipBuf() = default;
  HipBuf(HipBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
  HipBuf& operator=(HipBuf&& o) noexcept {
    if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); n_ = std::exchange(o.n_, 0); }
    return *this;
  }
  ~HipBuf() { reset(); }
  T* get() const { return p_; }
  size_t size() const { return n_; }
  void reset() {
    if (p_) (void)(PINNED ? hipHostFree(p_) : hipFree(p_));
    p_ = nullptr; n_ = 0;
  }
  hipError_t alloc(size_t n) {      // a fresh block of n elements (uninitialised); empty on failure
    reset();
    const hipError_t e = PINNED ? hipHostMalloc((void**)&p_, n * sizeof(T), hipHostMallocDefault) : hipMalloc((void**)&p_, n * sizeof(T));
    if (e == hipSuccess) n_ = n; else p_ = nullptr;
    return e;
  }
  hipError_t grow(size_t n) { return n <= n_ ? hipSuccess : alloc(n); }      // keeps a block that is large enough (contents lost otherwise)
  hipError_t upload(const T* host, size_t n) {      // a fresh block holding host[0..n)
    const hipError_t e = alloc(n);
    return e != hipSuccess ? e : hipMemcpy(p_, host, n * sizeof(T), PINNED ? hipMemcpyHostToHost : hipMemcpyHostToDevice);
  }
};
template <class T> using DevBuf = HipBuf<T, false>;
template <class T> using PinnedBuf = HipBuf<T, true>;

}  // namespace gnnb

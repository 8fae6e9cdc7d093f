// devbuf.hpp — the owning buffers of the host library: device memory (DevBuf) and pinned host memory (PinBuf).
//
// Every d_* / h_* member of the context, and every function-local temporary of an entry point, is one of these: it is freed
// when its owner goes (demi_ctx_destroy is `delete ctx`; an early return frees a temporary), and `reserve` is the one grow.
// Growth DISCARDS the contents and allocates exactly what was asked for: the free comes before the allocation, so the peak is
// the larger of the two sizes, not their sum.  A site that has to keep the contents allocates a second buffer, copies, and
// move-assigns it into the member.
//
// A condition the code does not show: hipFree waits for the device to go idle.  The scratch buffers (the pending-set spill,
// the word counters) are grown while an earlier launch of the context may still be running on another stream and using the old
// allocation; it is reset()'s hipFree that makes that safe.  Do not replace it by an asynchronous or pooled free.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <type_traits>

namespace demi_host {
struct DeviceMem {
  static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static void release(void* p) { (void)hipFree(p); }
};
struct PinnedMem {
  static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static void release(void* p) { (void)hipHostFree(p); }
};

template <class T, class Mem>
class Buf {
 public:
  Buf() = default;
  ~Buf() { reset(); }
  Buf(Buf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
  Buf& operator=(Buf&& o) noexcept {
    if (this != &o) { reset(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
    return *this;
  }
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;

  T* get() const { return p_; }
  operator T*() const { return p_; }           // (a buffer is handed to kernels and copies as the pointer it owns)
  size_t capacity() const { return cap_; }     // in elements (Buf<void>: bytes)
  void reset() {
    if (p_) Mem::release(p_);
    p_ = nullptr; cap_ = 0;
  }
  // room for n elements; on failure the buffer is empty and the runtime's error status is cleared
  hipError_t reserve(size_t n) {
    if (n <= cap_) return hipSuccess;
    reset();
    void* p = nullptr;
    const hipError_t e = Mem::alloc(&p, n * kElem);
    if (e != hipSuccess) { (void)hipGetLastError(); return e; }
    p_ = static_cast<T*>(p); cap_ = n;
    return hipSuccess;
  }

 private:
  static constexpr size_t kElem = sizeof(std::conditional_t<std::is_void<T>::value, char, T>);     // (an element of Buf<void> is a byte)
  T* p_ = nullptr;
  size_t cap_ = 0;
};
template <class T> using DevBuf = Buf<T, DeviceMem>;     // (DevBuf<void>: an arena that its user carves by byte offsets)
template <class T> using PinBuf = Buf<T, PinnedMem>;
}  // namespace demi_host

// Owners of what the engine allocates (host C++17, internal): device buffers, pinned host buffers,
// streams and events. Each is move-only, frees in its destructor and calls HIP directly; every
// fallible step returns the hipError_t, which the caller maps to an AV_ERR_* code (engine.h).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <type_traits>
#include <utility>

namespace avmem {

// How reserve() sizes a buffer that has to grow (contents are never kept).
enum class Slack {
  kExact,   // the size asked for
  kMiB,     // at least 1 MiB
  kEighth,  // an eighth more than asked for, at least 1 MiB
};

inline size_t grown_size(size_t want, Slack s) {
  if (s == Slack::kEighth) want += want / 8;
  return s == Slack::kExact ? want : std::max(want, (size_t)1 << 20);
}

// Shared by the two buffer owners: the pointer, its capacity in elements (bytes for T = void), moves.
template <typename T, hipError_t (*Free)(void*)>
class Buf {
 public:
  Buf() = default;
  Buf(Buf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr, o.n_ = 0; }
  Buf& operator=(Buf&& o) noexcept {  // frees what this one held
    if (this != &o) reset(), std::swap(p_, o.p_), std::swap(n_, o.n_);
    return *this;
  }
  ~Buf() { reset(); }
  void reset() {
    if (p_) (void)Free(const_cast<std::remove_cv_t<T>*>(p_));
    p_ = nullptr, n_ = 0;
  }
  T* get() const { return p_; }
  operator T*() const { return p_; }

 protected:
  // an empty request still yields a valid pointer
  static size_t bytes_of(size_t n) {
    return std::max<size_t>(n, 1) * sizeof(std::conditional_t<std::is_void<T>::value, char, T>);
  }
  // the old buffer freed, then where the allocating call puts the new one, and what it returned
  void** fresh() { return reset(), reinterpret_cast<void**>(const_cast<std::remove_cv_t<T>**>(&p_)); }
  hipError_t took(hipError_t e, size_t n) {
    if (e == hipSuccess) n_ = n;
    return e;
  }
  T* p_ = nullptr;
  size_t n_ = 0;
};

// Device memory. alloc* replace whatever the buffer held.
template <typename T>
struct DevBuf : Buf<T, hipFree> {
  hipError_t alloc(size_t n) { return this->took(hipMalloc(this->fresh(), this->bytes_of(n)), n); }
  // allocated, and its memset enqueued on stream
  hipError_t alloc_zeroed(size_t n, hipStream_t stream) {
    const hipError_t e = alloc(n);
    return e != hipSuccess ? e : hipMemsetAsync(this->p_, 0, this->bytes_of(n), stream);
  }
  // hipExtMallocWithFlags: fine-grained, uncached
  hipError_t alloc_flags(size_t n, unsigned flags) {
    return this->took(hipExtMallocWithFlags(this->fresh(), this->bytes_of(n), flags), n);
  }
  // at least n elements, re-allocated (the old one freed first) only if it holds fewer
  hipError_t reserve(size_t n, Slack s = Slack::kExact) {
    return n <= this->n_ ? hipSuccess : alloc(grown_size(n, s));
  }
};

// Pinned host memory; flags: hipHostMallocDefault, hipHostMallocMapped (the device can address it,
// hipHostGetDevicePointer), or hipHostMallocMapped | hipHostMallocCoherent.
template <typename T>
struct PinnedBuf : Buf<T, hipHostFree> {
  hipError_t alloc(size_t n, unsigned flags) {
    return this->took(hipHostMalloc(this->fresh(), this->bytes_of(n), flags), n);
  }
  hipError_t reserve(size_t n, Slack s, unsigned flags) {
    return n <= this->n_ ? hipSuccess : alloc(grown_size(n, s), flags);
  }
};

// A stream or an event: created on demand or adopted, destroyed with its owner (not synchronized first).
template <typename H, hipError_t (*Create)(H*, unsigned), hipError_t (*Destroy)(H)>
class Handle {
 public:
  Handle() = default;
  explicit Handle(H adopted) : h_(adopted) {}
  Handle(Handle&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  ~Handle() { reset(); }
  hipError_t create(unsigned flags) { return reset(), Create(&h_, flags); }
  void reset() {
    if (h_) (void)Destroy(h_);
    h_ = nullptr;
  }
  H get() const { return h_; }
  operator H() const { return h_; }

 private:
  H h_ = nullptr;
};

using Stream = Handle<hipStream_t, hipStreamCreateWithFlags, hipStreamDestroy>;
using Event = Handle<hipEvent_t, hipEventCreateWithFlags, hipEventDestroy>;

}  // namespace avmem

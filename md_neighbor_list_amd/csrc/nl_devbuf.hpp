// nl_devbuf.hpp -- DevBuf<T>: the owner of one hipMalloc allocation.  Move-only, frees in its destructor, converts to T*
// so that launches and pointer arithmetic read as with a raw pointer, and remembers what it was allocated for: the bytes
// asked for and the items the caller counts them in.  Knows nothing of the handle: its operations return hipError_t, and
// what a (re)allocation means for a handle (buffers_epoch, last_hip, the nl_status) is the business of the wrappers in
// nl_api.hip.  Needs only hipMalloc / hipFree (a host compiler builds it against stand-ins: tests/sanitize).
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

namespace nl {

template <typename T> class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept { adopt(o); }
  DevBuf& operator=(DevBuf&& o) noexcept {
    adopt(o);
    return *this;
  }
  ~DevBuf() { release(); }

  T* get() const { return p_; }
  operator T*() const { return p_; }
  // DevBuf<void> only: static_cast<U*>(buf), as on the void* it stands for
  template <typename U, typename V = T, typename = std::enable_if_t<std::is_void<V>::value>> explicit operator U*() const {
    return static_cast<U*>(p_);
  }
  size_t bytes() const { return bytes_; }    // as asked for (0 for the 16 bytes a zero-byte request takes); 0 when empty
  int64_t items() const { return items_; }   // as the caller counted them; 0 when empty
  bool holds(int64_t items) const { return p_ && items_ >= items; }

  // Frees what it holds, then allocates: empty on failure.
  hipError_t replace(size_t bytes, int64_t items = 0) {
    release();
    return take(bytes, items);
  }
  // Allocates first and frees the old allocation only then: a failure leaves the buffer as it was.
  hipError_t replace_keeping(size_t bytes, int64_t items = 0) {
    DevBuf fresh;
    const hipError_t e = fresh.take(bytes, items);
    if (e == hipSuccess) adopt(fresh);
    return e;
  }
  // At least `items` items: nothing where it holds them, else replace() -- a failed growth leaves it holding nothing.
  hipError_t ensure(int64_t items, size_t bytes) { return holds(items) ? hipSuccess : replace(bytes, items); }
  void release() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr, bytes_ = 0, items_ = 0;
  }
  // Frees what it holds and takes over o's allocation; o is left empty.
  void adopt(DevBuf& o) {
    if (this == &o) return;
    release();
    p_ = o.p_, bytes_ = o.bytes_, items_ = o.items_;
    o.p_ = nullptr, o.bytes_ = 0, o.items_ = 0;
  }

 private:
  hipError_t take(size_t bytes, int64_t items) {  // (empty on entry)
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, bytes ? bytes : 16);
    if (e == hipSuccess) p_ = static_cast<T*>(p), bytes_ = bytes, items_ = items;
    return e;
  }
  T* p_ = nullptr;
  size_t bytes_ = 0;
  int64_t items_ = 0;
};

}  // namespace nl

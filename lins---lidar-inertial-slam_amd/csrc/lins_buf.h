// lins_buf.h — the one owning buffer of the C API files: everything they allocate after lins_create (the mapping side's
// state, the lazily allocated parts of the streams context, the temporaries of the debug entry points) is a Buf member
// or local, grown where it is used and released by its destructor.  Grow-only, move-only; contents never survive a
// growth.  The memory source is a policy (int alloc(void**, size_t bytes), int free(void*), 0 = success), so that the
// growth logic compiles without ROCm (-DLINS_BUF_NO_HIP: tests/native/buf_check.cpp); the two HIP policies and the
// event wrapper are the lower part.  A HIP error of grow / grow_all reaches the context through BUF_TRY (lins_ctx_priv.h).
#pragma once
#include <cstddef>

namespace lins {

template <class T, class Mem>
class Buf {
 public:
  Buf() = default;
  Buf(Buf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr, o.cap_ = 0; }
  Buf& operator=(Buf&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_, cap_ = o.cap_;
      o.p_ = nullptr, o.cap_ = 0;
    }
    return *this;
  }
  ~Buf() { reset(); }

  T* get() const { return p_; }
  operator T*() const { return p_; }  // launches, copies and pointer arithmetic take the buffer as the raw pointer it owns
  size_t cap() const { return cap_; }  // elements

  // At least max(need, 1) elements.  A capacity that suffices is left alone (same pointer); otherwise the old block is
  // freed FIRST (a device free waits for the kernels that may still read it, and the two blocks never coexist), then the
  // new one allocated.  On failure the buffer is empty and the policy's error is returned.
  int grow(size_t need) {
    if (need < 1) need = 1;
    if (cap_ >= need) return 0;
    reset();
    void* q = nullptr;
    if (int e = Mem::alloc(&q, need * sizeof(T))) return e;
    p_ = (T*)q, cap_ = need;
    return 0;
  }
  void reset() {
    if (p_) (void)Mem::free(p_);
    p_ = nullptr, cap_ = 0;
  }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
};

// A group of buffers that share one capacity, as (buffer, elements) pairs: grow_all(a, n, b, n, c, 2 * n).  The first
// member answers for the group: where its capacity suffices nothing is touched.  Otherwise ALL are freed, then allocated
// in the order written; after a failure every member is empty.
inline void buf_reset_all() {}
template <class B, class... R>
void buf_reset_all(B& b, size_t, R&&... rest) {
  b.reset();
  buf_reset_all(rest...);
}
inline int buf_alloc_all() { return 0; }
template <class B, class... R>
int buf_alloc_all(B& b, size_t need, R&&... rest) {
  if (int e = b.grow(need)) return e;
  return buf_alloc_all(rest...);
}
template <class B, class... R>
int grow_all(B& first, size_t need, R&&... rest) {
  if (first.cap() >= (need < 1 ? 1 : need)) return 0;
  buf_reset_all(first, need, rest...);
  const int e = buf_alloc_all(first, need, rest...);
  if (e) buf_reset_all(first, need, rest...);
  return e;
}

}  // namespace lins

#ifndef LINS_BUF_NO_HIP
#include <hip/hip_runtime.h>

namespace lins {

struct DeviceMem {
  static int alloc(void** p, size_t bytes) { return (int)hipMalloc(p, bytes); }
  static int free(void* p) { return (int)hipFree(p); }
};
struct PinnedMem {
  static int alloc(void** p, size_t bytes) { return (int)hipHostMalloc(p, bytes); }
  static int free(void* p) { return (int)hipHostFree(p); }
};
template <class T>
using DevBuf = Buf<T, DeviceMem>;
template <class T>
using PinBuf = Buf<T, PinnedMem>;

// an event created on first use, outside lins_create
class Event {
 public:
  Event() = default;
  Event(Event&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
  Event& operator=(Event&& o) noexcept {
    if (this != &o) {
      reset();
      e_ = o.e_, o.e_ = nullptr;
    }
    return *this;
  }
  ~Event() { reset(); }
  operator hipEvent_t() const { return e_; }
  int create(unsigned flags = hipEventDefault) { return e_ ? 0 : (int)hipEventCreateWithFlags(&e_, flags); }
  void reset() {
    if (e_) (void)hipEventDestroy(e_);
    e_ = nullptr;
  }

 private:
  hipEvent_t e_ = nullptr;
};

}  // namespace lins
#endif

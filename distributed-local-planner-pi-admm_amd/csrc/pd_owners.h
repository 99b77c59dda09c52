// pd_owners.h -- the owners of device and pinned memory, for every handle of the library (internal,
// not installed).  A handle type H has `hipStream_t stream` and `std::string err`; a failed runtime
// call is reported through own_fail, which a handle type may specialise (piadmm_ctx.h: the
// planner's also sets the thread's message).  What the library holds at any moment is what its
// dev_buf and arena members hold.
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <utility>
#include <vector>

#include "piadmm.h"

namespace pd_own {

template <class H>
int own_fail(H* h, int code, const std::string& msg) {
  if (h) h->err = msg;
  return code;
}
#define OWN_HIP(h, call)                                                                \
  do {                                                                                  \
    hipError_t _e = (call);                                                             \
    if (_e != hipSuccess)                                                               \
      return pd_own::own_fail(h, PIADMM_E_HIP, std::string(#call ": ") + hipGetErrorString(_e)); \
  } while (0)

// The zero fill is done when this returns: hipMemset of device memory does not wait, and the handle's
// stream does not wait for the null stream, so the fill could otherwise land after a kernel's writes.
template <class H, typename T>
int dalloc(H* h, T** p, size_t count, bool zero) {
  OWN_HIP(h, hipMalloc(p, count * sizeof(T)));
  if (zero) OWN_HIP(h, hipMemset(*p, 0, count * sizeof(T)));
  if (zero) OWN_HIP(h, hipStreamSynchronize(nullptr));
  return 0;
}

// The owner of one hipMalloc'ed array (Pinned: of one hipHostMalloc'ed): move-only, freed when it
// goes.  It converts to the pointer, so a launch or a copy names it as it would the raw pointer.
// Whoever lets one go while the stream may still use it synchronises the stream first.
template <typename T, bool Pinned = false>
class dev_buf {
 public:
  dev_buf() = default;
  dev_buf(dev_buf&& o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
  dev_buf& operator=(dev_buf&& o) noexcept {
    if (this != &o) {
      release();
      p_ = std::exchange(o.p_, nullptr);
    }
    return *this;
  }
  ~dev_buf() { release(); }
  // the project's error code, h->err set; the array is owned even when the memset fails
  template <class H>
  int alloc(H* h, size_t count, bool zero) {
    release();
    if constexpr (Pinned) {
      OWN_HIP(h, hipHostMalloc(reinterpret_cast<void**>(&p_), count * sizeof(T)));
      return 0;
    } else {
      return dalloc(h, &p_, count, zero);
    }
  }
  // the bare allocation, for a caller that words the failure itself
  hipError_t make(size_t count) {
    release();
    if constexpr (Pinned) return hipHostMalloc(reinterpret_cast<void**>(&p_), count * sizeof(T));
    else return hipMalloc(&p_, count * sizeof(T));
  }
  T* get() const { return p_; }
  operator T*() const { return p_; }

 private:
  void release() {
    if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
    p_ = nullptr;
  }
  T* p_ = nullptr;
};

// Device arrays that live and go together: a scenario's (the planner handle), or those of one
// stand-alone call, on the stack.  An array has at least one element; a zero fill runs on the
// handle's stream, so it is ordered before whatever that stream does next.  After a failed take
// every later one hands out nullptr and rc keeps the first failure, so a caller takes all its arrays
// and asks once.  release -- and the destructor, on whichever path a call leaves -- synchronises the
// stream and then frees the arrays.
template <class H>
class arena {
 public:
  explicit arena(H* h) : h_(h) {}
  arena(const arena&) = delete;
  arena& operator=(const arena&) = delete;
  ~arena() { release(); }
  void release() {
    if (h_->stream) (void)hipStreamSynchronize(h_->stream);
    for (void* q : held_) (void)hipFree(q);
    held_.clear();
    rc = 0;
  }
  template <typename T>
  T* take(size_t count, bool zero) {
    if (rc) return nullptr;
    if (count == 0) count = 1;
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, count * sizeof(T));
    if (e != hipSuccess) {
      rc = own_fail(h_, PIADMM_E_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
      return nullptr;
    }
    held_.push_back(q);
    if (zero && (e = hipMemsetAsync(q, 0, count * sizeof(T), h_->stream)) != hipSuccess) {
      rc = own_fail(h_, PIADMM_E_HIP, std::string("hipMemset: ") + hipGetErrorString(e));
      return nullptr;
    }
    return static_cast<T*>(q);
  }
  int rc = 0;

 private:
  H* h_;
  std::vector<void*> held_;
};

}  // namespace pd_own

// fh_memory.h -- what fh_ctx and fh_group own, as four move-only types: DeviceBuffer<T> (hipMalloc), PinnedBuffer<T> (hipHostMalloc), Event and Stream.
// A type frees what it holds and nothing else: whoever resizes or releases a buffer that a stream may still use synchronises first, at the call site, and a
// group makes the owning device current before it releases a member's (group.hip).  Every allocation is at least 16 bytes, so a buffer sized for nothing is
// still a valid pointer.  All eight HIP calls go through fh::seam, which counts what is live (fh_kat_live_allocations); tools/fh_memory_check.cpp defines
// FH_MEMORY_FAKE_SEAM, the HIP names used here and the eight raw_ functions itself and checks the types without a GPU.
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <memory>
#ifndef FH_MEMORY_FAKE_SEAM
#include <hip/hip_runtime.h>
#endif

namespace fh {
namespace seam {
#ifdef FH_MEMORY_FAKE_SEAM
hipError_t raw_device_malloc(void** p, size_t bytes);
hipError_t raw_device_free(void* p);
hipError_t raw_host_malloc(void** p, size_t bytes);
hipError_t raw_host_free(void* p);
hipError_t raw_event_create(hipEvent_t* e, unsigned flags);
hipError_t raw_event_destroy(hipEvent_t e);
hipError_t raw_stream_create(hipStream_t* s, unsigned flags, int priority);
hipError_t raw_stream_destroy(hipStream_t s);
#else
inline hipError_t raw_device_malloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
inline hipError_t raw_device_free(void* p) { return hipFree(p); }
inline hipError_t raw_host_malloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
inline hipError_t raw_host_free(void* p) { return hipHostFree(p); }
inline hipError_t raw_event_create(hipEvent_t* e, unsigned flags) { return hipEventCreateWithFlags(e, flags); }
inline hipError_t raw_event_destroy(hipEvent_t e) { return hipEventDestroy(e); }
inline hipError_t raw_stream_create(hipStream_t* s, unsigned flags, int priority) { return priority ? hipStreamCreateWithPriority(s, flags, priority) : hipStreamCreateWithFlags(s, flags); }
inline hipError_t raw_stream_destroy(hipStream_t s) { return hipStreamDestroy(s); }
#endif
// live allocations and handles of the four types in this process, and the bytes of the buffers among them
inline std::atomic<uint64_t> live_count{0}, live_bytes{0};
inline void took(size_t bytes) { live_count.fetch_add(1, std::memory_order_relaxed); live_bytes.fetch_add(bytes, std::memory_order_relaxed); }
inline void gave(size_t bytes) { live_count.fetch_sub(1, std::memory_order_relaxed); live_bytes.fetch_sub(bytes, std::memory_order_relaxed); }
}  // namespace seam

template <typename T, bool kPinned>
class Buffer {
 public:
  Buffer() = default;
  Buffer(const Buffer&) = delete;
  Buffer& operator=(const Buffer&) = delete;
  Buffer(Buffer&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
  Buffer& operator=(Buffer&& o) noexcept { if (this != std::addressof(o)) { reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; } return *this; }
  ~Buffer() { reset(); }
  Buffer* operator&() = delete;  // ((void**)&ctx->d_x of the days of raw pointers must not compile)

  // n elements, whatever was held before; a failure leaves the buffer empty
  hipError_t alloc(size_t n)
  {
    reset();
    void* raw = nullptr;
    const hipError_t e = kPinned ? seam::raw_host_malloc(&raw, bytes_of(n)) : seam::raw_device_malloc(&raw, bytes_of(n));
    if (e != hipSuccess) return e;
    p_ = static_cast<T*>(raw); n_ = n;
    seam::took(bytes_of(n));
    return hipSuccess;
  }
  // grow only: what is held stays (contents included) when it has room for n elements
  hipError_t ensure(size_t n) { return n_ >= n ? hipSuccess : alloc(n); }
  void reset()
  {
    if (!p_) return;
    (void)(kPinned ? seam::raw_host_free(p_) : seam::raw_device_free(p_));
    seam::gave(bytes_of(n_));
    p_ = nullptr; n_ = 0;
  }
  T* release() { T* p = p_; if (p) seam::gave(bytes_of(n_)); p_ = nullptr; n_ = 0; return p; }  // the caller frees it
  size_t size() const { return n_; }
  T* get() const { return p_; }
  operator T*() const { return p_; }

 private:
  static size_t bytes_of(size_t n) { return n * sizeof(T) > 16 ? n * sizeof(T) : 16; }
  T* p_ = nullptr;
  size_t n_ = 0;
};
template <typename T> using DeviceBuffer = Buffer<T, false>;
template <typename T> using PinnedBuffer = Buffer<T, true>;

class Event {
 public:
  Event() = default;
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  Event(Event&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
  Event& operator=(Event&& o) noexcept { if (this != &o) { reset(); e_ = o.e_; o.e_ = nullptr; } return *this; }
  ~Event() { reset(); }
  hipError_t create(unsigned flags = 0)  // (0: hipEventDefault, a timing event)
  {
    reset();
    const hipError_t e = seam::raw_event_create(&e_, flags);
    if (e != hipSuccess) e_ = nullptr; else seam::took(0);
    return e;
  }
  void reset() { if (e_) { (void)seam::raw_event_destroy(e_); seam::gave(0); e_ = nullptr; } }
  operator hipEvent_t() const { return e_; }

 private:
  hipEvent_t e_ = nullptr;
};

class Stream {
 public:
  Stream() = default;
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  Stream(Stream&& o) noexcept : s_(o.s_) { o.s_ = nullptr; }
  Stream& operator=(Stream&& o) noexcept { if (this != &o) { reset(); s_ = o.s_; o.s_ = nullptr; } return *this; }
  ~Stream() { reset(); }
  hipError_t create(unsigned flags, int priority = 0)  // (priority 0: the default one)
  {
    reset();
    const hipError_t e = seam::raw_stream_create(&s_, flags, priority);
    if (e != hipSuccess) s_ = nullptr; else seam::took(0);
    return e;
  }
  void reset() { if (s_) { (void)seam::raw_stream_destroy(s_); seam::gave(0); s_ = nullptr; } }
  operator hipStream_t() const { return s_; }

 private:
  hipStream_t s_ = nullptr;
};
}  // namespace fh

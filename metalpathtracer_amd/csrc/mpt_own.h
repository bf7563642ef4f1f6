// mpt_own.h — owners of the HIP resources the host side holds: device memory, pinned host memory, events and streams (host code only).
// Each owner is move-only and lets go of what it holds in its destructor; reset() lets go early, release() hands the raw handle over
// and adopt() takes one.  A struct of owners frees itself: nothing lists its fields by hand.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <utility>

namespace mpt_own {

// An event or a stream: create(make, args...) calls make(&handle, args...), e.g. ev.create(hipEventCreateWithFlags, hipEventDisableTiming).
template <class H, hipError_t (*Free)(H)>
class Handle {
  public:
    Handle() = default;
    Handle(Handle&& o) noexcept : h_(o.release()) {}
    Handle& operator=(Handle&& o) noexcept {
        if (this != &o) adopt(o.release());
        return *this;
    }
    Handle(const Handle&) = delete;
    Handle& operator=(const Handle&) = delete;
    ~Handle() { reset(); }
    template <class F, class... A>
    hipError_t create(F make, A... args) {
        reset();
        H h = nullptr;
        const hipError_t e = make(&h, args...);
        if (e == hipSuccess) h_ = h;
        return e;
    }
    void reset() { adopt(nullptr); }
    void adopt(H h) {
        if (h_) (void)Free(h_);
        h_ = h;
    }
    H release() { return std::exchange(h_, nullptr); }
    H get() const { return h_; }
    explicit operator bool() const { return h_ != nullptr; }

  private:
    H h_ = nullptr;
};
using Event = Handle<hipEvent_t, hipEventDestroy>;
using Stream = Handle<hipStream_t, hipStreamDestroy>;

// Memory on the device (hipMalloc) or pinned on the host (hipHostMalloc).  T: what the pointer is read as; bytes(): the size asked for.
template <class T, bool HOST>
class Mem {
  public:
    Mem() = default;
    Mem(Mem&& o) noexcept : bytes_(o.bytes_), p_(o.release()) {}
    Mem& operator=(Mem&& o) noexcept {
        if (this != &o) {
            const size_t b = o.bytes_;
            adopt(o.release(), b);
        }
        return *this;
    }
    Mem(const Mem&) = delete;
    Mem& operator=(const Mem&) = delete;
    ~Mem() { reset(); }
    // lets go of what it held, then allocates (a device allocation of 0 bytes gets 16); it holds nothing if that fails
    hipError_t alloc(size_t bytes, unsigned host_flags = hipHostMallocDefault) {
        reset();
        void* q = nullptr;
        const hipError_t e = HOST ? hipHostMalloc(&q, bytes, host_flags) : hipMalloc(&q, bytes ? bytes : 16);
        if (e == hipSuccess) adopt(q, bytes);
        return e;
    }
    void reset() { adopt(nullptr, 0); }
    void adopt(void* p, size_t bytes) {
        if (p_) (void)(HOST ? hipHostFree(p_) : hipFree(p_));
        p_ = (T*)p;
        bytes_ = p ? bytes : 0;
    }
    T* release() {
        bytes_ = 0;
        return std::exchange(p_, nullptr);
    }
    T* get() const { return p_; }
    size_t bytes() const { return bytes_; }
    explicit operator bool() const { return p_ != nullptr; }

  private:
    size_t bytes_ = 0;
    T* p_ = nullptr;
};
template <class T = void>
using DevMem = Mem<T, false>;
template <class T = void>
using HostMem = Mem<T, true>;

}  // namespace mpt_own

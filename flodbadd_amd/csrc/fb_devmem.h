// fb_devmem.h -- the owners of what the host code holds on the device: one allocation, one event, one
// stream each, move-only, released by the destructor.  A struct of them needs no hand-written teardown,
// and a group of buffers is allocated whole or not at all (alloc_group).  Host-only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

namespace fbk {

int set_err(int code, const char* fmt, ...);         // fb_capi.hip: fb_last_error's text; returns `code`
constexpr int kDevmemNoMem = -2, kDevmemHip = -3;    // FB_ERR_NOMEM, FB_ERR_HIP (asserted in fb_host.h)

// One hipMalloc allocation of size() elements.
template <typename T>
class DevBuf {
  public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept { swap(o); }
    DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { reset(); swap(o); } return *this; }
    ~DevBuf() { reset(); }
    // Frees what it holds, then allocates n elements (none for n == 0); empty after a failure.
    hipError_t alloc(size_t n) {
        reset();
        if (n == 0) return hipSuccess;
        const hipError_t e = hipMalloc((void**)&p_, n * sizeof(T));
        if (e == hipSuccess) n_ = n; else p_ = nullptr;
        return e;
    }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        n_ = 0;
    }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t size() const { return n_; }
    void swap(DevBuf& o) noexcept { std::swap(p_, o.p_); std::swap(n_, o.n_); }

  private:
    T* p_ = nullptr;
    size_t n_ = 0;
};

// The same over hipHostMalloc(flags); dev() is the device alias of a hipHostMallocMapped buffer.
template <typename T>
class PinnedBuf {
  public:
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf&& o) noexcept { swap(o); }
    PinnedBuf& operator=(PinnedBuf&& o) noexcept { if (this != &o) { reset(); swap(o); } return *this; }
    ~PinnedBuf() { reset(); }
    hipError_t alloc(size_t n, unsigned flags) {
        reset();
        if (n == 0) return hipSuccess;
        hipError_t e = hipHostMalloc((void**)&p_, n * sizeof(T), flags);
        if (e != hipSuccess) { p_ = nullptr; return e; }
        n_ = n;
        if (flags & hipHostMallocMapped) e = hipHostGetDevicePointer((void**)&d_, p_, 0);
        if (e != hipSuccess) reset();
        return e;
    }
    void reset() {
        if (p_) (void)hipHostFree(p_);
        p_ = d_ = nullptr;
        n_ = 0;
    }
    T* get() const { return p_; }
    T* dev() const { return d_; }
    operator T*() const { return p_; }
    T* operator->() const { return p_; }
    size_t size() const { return n_; }
    void swap(PinnedBuf& o) noexcept { std::swap(p_, o.p_); std::swap(d_, o.d_); std::swap(n_, o.n_); }

  private:
    T *p_ = nullptr, *d_ = nullptr;
    size_t n_ = 0;
};

// An event without timing / a non-blocking stream: made by the first create(), destroyed once.
class DevEvent {
  public:
    DevEvent() = default;
    DevEvent(DevEvent&& o) noexcept { std::swap(e_, o.e_); }
    DevEvent& operator=(DevEvent&& o) noexcept { if (this != &o) { reset(); std::swap(e_, o.e_); } return *this; }
    ~DevEvent() { reset(); }
    void reset() { if (e_) (void)hipEventDestroy(e_); e_ = nullptr; }
    hipError_t create() {
        if (e_) return hipSuccess;
        const hipError_t e = hipEventCreateWithFlags(&e_, hipEventDisableTiming);
        if (e != hipSuccess) e_ = nullptr;
        return e;
    }
    operator hipEvent_t() const { return e_; }

  private:
    hipEvent_t e_ = nullptr;
};
class DevStream {
  public:
    DevStream() = default;
    DevStream(DevStream&& o) noexcept { std::swap(s_, o.s_); }
    DevStream& operator=(DevStream&& o) noexcept { if (this != &o) { reset(); std::swap(s_, o.s_); } return *this; }
    ~DevStream() { reset(); }
    void reset() { if (s_) (void)hipStreamDestroy(s_); s_ = nullptr; }
    hipError_t create() {
        if (s_) return hipSuccess;
        const hipError_t e = hipStreamCreateWithFlags(&s_, hipStreamNonBlocking);
        if (e != hipSuccess) s_ = nullptr;
        return e;
    }
    operator hipStream_t() const { return s_; }

  private:
    hipStream_t s_ = nullptr;
};

// Allocates (buffer, elements) pairs in order; stops at the first failure.
inline hipError_t alloc_each() { return hipSuccess; }
template <class B, class... Rest>
hipError_t alloc_each(B& b, size_t n, Rest&&... rest) {
    const hipError_t e = b.alloc(n);
    return e != hipSuccess ? e : alloc_each(rest...);
}
// A group of buffers (a movable struct of owners) made whole or not at all: g is dropped, fill(fresh
// group) allocates, and g takes the fresh group only when every allocation succeeded -- else g stays empty.
template <class G, class Fill>
hipError_t alloc_group(G& g, Fill fill) {
    g = G();
    G nw;
    const hipError_t e = fill(nw);
    if (e == hipSuccess) g = std::move(nw);
    return e;
}

// A grow-only scratch buffer that any stream may use: acquire() orders the stream after the previous use
// (the event release() recorded), and a growth waits for that use on the host before the old buffer goes.
class StreamScratch {
  public:
    // `what` names the scratch in the error text.  A failed growth leaves it empty.
    int acquire(size_t bytes, hipStream_t s, const char* what) {
        hipError_t e = ev_.create();
        if (e == hipSuccess) e = hipStreamWaitEvent(s, ev_, 0);  // (an event never recorded is complete)
        if (e == hipSuccess && bytes > buf_.size()) {
            e = hipEventSynchronize(ev_);
            if (e == hipSuccess && buf_.alloc(bytes) != hipSuccess)
                return set_err(kDevmemNoMem, "%s (%llu bytes)", what, (unsigned long long)bytes);
        }
        return e == hipSuccess ? 0 : set_err(kDevmemHip, "%s: %s", what, hipGetErrorString(e));
    }
    int release(hipStream_t s) {
        const hipError_t e = hipEventRecord(ev_, s);
        return e == hipSuccess ? 0 : set_err(kDevmemHip, "hipEventRecord failed: %s", hipGetErrorString(e));
    }
    void* get() const { return buf_.get(); }
    size_t capacity() const { return buf_.size(); }

  private:
    DevBuf<unsigned char> buf_;
    DevEvent ev_;
};

}  // namespace fbk

// qs_devbuf.hpp -- the one owner of device and pinned-host memory in the host code (the C-ABI layer, qs_ctx.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace qs {

// A hipMalloc'ed (Pinned: hipHostMalloc'ed) buffer together with its capacity. Move-only; frees in its destructor.
template <typename T, bool Pinned = false> class DevBuf {
    T *p_ = nullptr;
    size_t bytes_ = 0;

public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; bytes_ = o.bytes_; o.p_ = nullptr; o.bytes_ = 0; }
        return *this;
    }
    ~DevBuf() { reset(); }

    T *get() const { return p_; }
    size_t bytes() const { return bytes_; }
    explicit operator bool() const { return p_ != nullptr; }

    // free now (hipFree waits for the device), back to empty
    void reset() {
        if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr; bytes_ = 0;
    }
    // Grow-only: at least `bytes` afterwards, exactly `bytes` if it had to allocate (slack is the caller's business). The old
    // contents are gone then; `reader` (NULL = nobody: a pointer, because the null stream is a stream too) names the stream whose
    // queued work may still read them and is waited for first. On failure the buffer is empty.
    hipError_t reserve(size_t bytes, const hipStream_t *reader) {
        if (bytes <= bytes_) return hipSuccess;
        hipError_t e = (p_ && reader) ? hipStreamSynchronize(*reader) : hipSuccess;
        reset();
        void *fresh = nullptr;
        if (e == hipSuccess) e = Pinned ? hipHostMalloc(&fresh, bytes, hipHostMallocDefault) : hipMalloc(&fresh, bytes);
        if (e != hipSuccess) return e;
        p_ = static_cast<T *>(fresh); bytes_ = bytes;
        return hipSuccess;
    }
};
template <typename T> using PinBuf = DevBuf<T, true>;

// A non-blocking stream of the context's own, created on first use. Move-less; destroyed (after its work has drained) with its owner.
class DevStream {
    hipStream_t s_ = nullptr;

public:
    DevStream() = default;
    DevStream(const DevStream &) = delete;
    DevStream &operator=(const DevStream &) = delete;
    ~DevStream() { if (s_) (void)hipStreamDestroy(s_); }
    hipStream_t get() const { return s_; }
    explicit operator bool() const { return s_ != nullptr; }
    hipError_t ensure() { return s_ ? hipSuccess : hipStreamCreateWithFlags(&s_, hipStreamNonBlocking); }
};

// An ordering event (no timing), created on first use.
class DevEvent {
    hipEvent_t e_ = nullptr;

public:
    DevEvent() = default;
    DevEvent(const DevEvent &) = delete;
    DevEvent &operator=(const DevEvent &) = delete;
    ~DevEvent() { if (e_) (void)hipEventDestroy(e_); }
    hipEvent_t get() const { return e_; }
    hipError_t ensure() { return e_ ? hipSuccess : hipEventCreateWithFlags(&e_, hipEventDisableTiming); }
};

}  // namespace qs

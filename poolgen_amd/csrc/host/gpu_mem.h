// gpu_mem.h -- the CLI's only callers of the HIP allocator: a throwing status check and move-only owners of device and
// pinned host memory.  An exception on the way (unsorted input, out of memory) releases what an owner holds: the caller may
// carry on into another path (run() falls back to the whole-file path on an unsorted input).
#pragma once
#include <hip/hip_runtime.h>
#include <stdexcept>
#include <string>
#include <utility>

namespace pgh {

inline void hip_ok(hipError_t e, const char *what) {
    if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

template <typename T>
class DeviceBuf {
    T *p_ = nullptr;
    size_t cap_ = 0; // bytes
public:
    DeviceBuf() = default;
    DeviceBuf(size_t bytes, const char *what) { reset(bytes, what); }
    DeviceBuf(DeviceBuf &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    DeviceBuf &operator=(DeviceBuf &&o) noexcept { std::swap(p_, o.p_); std::swap(cap_, o.cap_); return *this; }
    ~DeviceBuf() { reset(); }
    void reset() { if (p_) (void)hipFree(p_); p_ = nullptr; cap_ = 0; }
    void reset(size_t bytes, const char *what = "device memory") {
        reset();
        hip_ok(hipMalloc((void **)&p_, bytes), what);
        cap_ = bytes;
    }
    void reserve(size_t bytes, const char *what = "device memory") { // a reusable buffer: grows with an eighth to spare
        if (bytes > cap_) reset(bytes + bytes / 8, what);
    }
    T *get() const { return p_; }
};

// Pinned host memory.  Its users are allocator callbacks (SyncAlloc), which report a failure as a null pointer: nothing throws here.
class PinnedBuf {
    void *p_ = nullptr;
    size_t cap_ = 0;
public:
    static void *alloc(size_t bytes) {
        void *p = nullptr;
        return hipHostMalloc(&p, bytes, hipHostMallocDefault) == hipSuccess ? p : nullptr;
    }
    static void release(void *p) { (void)hipHostFree(p); }
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    PinnedBuf &operator=(PinnedBuf &&o) noexcept { std::swap(p_, o.p_); std::swap(cap_, o.cap_); return *this; }
    ~PinnedBuf() { reset(); }
    void reset() { if (p_) release(p_); p_ = nullptr; cap_ = 0; }
    bool reset(size_t bytes) {
        reset();
        p_ = alloc(bytes);
        cap_ = p_ ? bytes : 0;
        return p_ != nullptr;
    }
    void *reserve(size_t bytes) { // grows with an eighth to spare; null when the allocation fails
        if (bytes > cap_ && !reset(bytes + bytes / 8)) return nullptr;
        return p_;
    }
    void *get() const { return p_; }
};

} // namespace pgh

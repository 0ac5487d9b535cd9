// qkd_device.h — the one owner of device memory in the library: every
// hipMalloc / hipFree goes through DevBuf.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>

#include <vector>

namespace qkd {

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

// count elements of T on the device that was current when they were allocated;
// freed with that device current, wherever the owner is destroyed. Move-only.
// Every call that allocates returns HIP's error and leaves the buffer empty on
// failure; the caller words the status (QKD_HIP, or an out-of-memory message).
template <class T>
class DevBuf {
    T* p_ = nullptr;
    size_t n_ = 0;
    int dev_ = 0;

public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_), dev_(o.dev_) { o.p_ = nullptr, o.n_ = 0; }
    DevBuf& operator=(DevBuf&&) = delete;
    ~DevBuf() { reset(); }

    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t size() const { return n_; }

    void reset() {
        if (p_) {
            DeviceGuard g(dev_);
            (void)hipFree(p_);
        }
        p_ = nullptr;
        n_ = 0;
    }
    hipError_t alloc(size_t count) {
        reset();
        hipError_t e = hipGetDevice(&dev_);
        if (e == hipSuccess) e = hipMalloc(&p_, count * sizeof(T));
        if (e == hipSuccess) n_ = count;
        else p_ = nullptr;
        return e;
    }
    // grow only, contents not kept: at least count elements afterwards
    hipError_t reserve(size_t count) { return n_ >= count ? hipSuccess : alloc(count); }
    hipError_t upload(const T* host, size_t count) {
        hipError_t e = alloc(count);
        if (e == hipSuccess) e = hipMemcpy(p_, host, count * sizeof(T), hipMemcpyHostToDevice);
        if (e != hipSuccess) reset();
        return e;
    }
    hipError_t upload(const std::vector<T>& v) { return upload(v.data(), v.size()); }
};

}  // namespace qkd

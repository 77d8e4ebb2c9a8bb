// dev_mem.hpp — device memory with one owner: buffers that carry their own capacity, and a scoped
// device selection. Host code only (no kernels): builds with a plain host compiler.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstddef>
#include <utility>

namespace pvhip {

// pointer + capacity (in elements of T) of the two owning buffers below; move-only, never copies
template <typename T>
class dev_owned {
public:
    T* get() const { return p_; }
    size_t capacity() const { return cap_; }

protected:
    dev_owned() = default;
    dev_owned(dev_owned&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    void take(dev_owned& o) {
        p_ = std::exchange(o.p_, nullptr);
        cap_ = std::exchange(o.cap_, 0);
    }
    T* p_ = nullptr;
    size_t cap_ = 0;
};

// hipMalloc / hipFree. grow(need, alloc): nothing when need <= capacity(); else the buffer is freed
// and `alloc` (>= need) elements are allocated. Contents are lost; a failure leaves it empty.
template <typename T>
class dev_buf : public dev_owned<T> {
public:
    dev_buf() {}   // user-provided: the class is no aggregate
    dev_buf(dev_buf&&) noexcept = default;
    dev_buf& operator=(dev_buf&& o) noexcept {
        if (this != &o) {
            release();
            this->take(o);
        }
        return *this;
    }
    ~dev_buf() { release(); }
    void release() {
        if (this->p_) (void)hipFree(this->p_);
        this->p_ = nullptr;
        this->cap_ = 0;
    }
    hipError_t grow(size_t need, size_t alloc) {
        if (need <= this->cap_) return hipSuccess;
        release();
        const hipError_t e = hipMalloc((void**)&this->p_, alloc * sizeof(T));
        if (e == hipSuccess) this->cap_ = alloc;
        else this->p_ = nullptr;
        return e;
    }
    // scratch reused from call to call: a floor of 1,024 elements
    hipError_t grow_floor(size_t need) { return grow(need, std::max<size_t>(need, 1024)); }
};

// hipMallocAsync / hipFreeAsync on the stream given to each call. The destructor has no stream: what
// is still held then goes back through the synchronous hipFree.
template <typename T>
class dev_stream_buf : public dev_owned<T> {
public:
    dev_stream_buf() {}
    dev_stream_buf(dev_stream_buf&&) noexcept = default;
    dev_stream_buf& operator=(dev_stream_buf&& o) noexcept {
        if (this != &o) {
            drop();
            this->take(o);
        }
        return *this;
    }
    ~dev_stream_buf() { drop(); }
    void release(hipStream_t st) {
        if (this->p_) (void)hipFreeAsync(this->p_, st);
        this->p_ = nullptr;
        this->cap_ = 0;
    }
    hipError_t grow(size_t need, size_t alloc, hipStream_t st) {
        if (need <= this->cap_) return hipSuccess;
        release(st);
        const hipError_t e = hipMallocAsync((void**)&this->p_, alloc * sizeof(T), st);
        if (e == hipSuccess) this->cap_ = alloc;
        else this->p_ = nullptr;
        return e;
    }
    // arrays that grow step by step: 1/8 headroom over a floor of 64 elements, and once more without
    // the headroom when the device is out of memory
    hipError_t grow_headroom(size_t need, hipStream_t st) {
        hipError_t e = grow(need, std::max<size_t>(need + need / 8, 64), st);
        if (e == hipErrorOutOfMemory) {
            (void)hipGetLastError();
            e = grow(need, std::max<size_t>(need, 64), st);
        }
        return e;
    }

private:
    void drop() {
        if (this->p_) (void)hipFree(this->p_);
        this->p_ = nullptr;
        this->cap_ = 0;
    }
};

// selects `dev` for the calling thread and puts the previously selected device back on scope exit
class device_guard {
public:
    explicit device_guard(int dev) {
        if (hipGetDevice(&prev_) != hipSuccess) prev_ = -1;
        (void)hipSetDevice(dev);
    }
    ~device_guard() {
        if (prev_ >= 0) (void)hipSetDevice(prev_);
    }
    device_guard(const device_guard&) = delete;
    device_guard& operator=(const device_guard&) = delete;

private:
    int prev_ = -1;
};

}  // namespace pvhip

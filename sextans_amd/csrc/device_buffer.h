// device_buffer.h -- sx::DevBuf<T>: the one owner of a hipMalloc allocation.  Every device array the engine or a plan builder owns is
// one of these; views (pointers into caller memory or into a DevBuf held elsewhere) stay raw const pointers.  The calls are the plain
// synchronous hipMalloc / hipFree: nothing here may run inside a hipGraph capture or a timed region.
// Not a public header.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <utility>

namespace sx {

template <class T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
        return *this;
    }
    ~DevBuf() { reset(); }

    T *get() const { return p_; }
    operator T *() const { return p_; }                                        // kernel arguments, pointer arithmetic, null tests
    size_t size() const { return n_; }                                         // elements asked for
    int64_t bytes() const { return p_ ? (int64_t)(sizeof(T) * (n_ ? n_ : 1)) : 0; }   // bytes asked of hipMalloc
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr; n_ = 0;
    }
    hipError_t alloc(size_t n) {   // exactly n elements (at least one); empty on failure
        reset();
        const hipError_t e = hipMalloc((void **)&p_, sizeof(T) * (n ? n : 1));
        if (e != hipSuccess) { p_ = nullptr; return e; }
        n_ = n;
        return hipSuccess;
    }
    hipError_t reserve(size_t n) { return p_ && n_ >= n ? hipSuccess : alloc(n); }   // grow-only workspace

private:
    T *p_ = nullptr;
    size_t n_ = 0;
};

}  // namespace sx

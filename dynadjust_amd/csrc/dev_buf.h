// Owning buffers: one device (or page-locked host) allocation and its capacity in elements, freed by reset() and the destructor.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <algorithm>
#include <initializer_list>
#include "la_kernels.h"

namespace dnagpu {

struct DeviceMem {      // (through poison_malloc: DNAGPU_POISON_ALLOC still fills every new buffer)
    static hipError_t alloc(void** p, size_t bytes) { return poison_malloc(p, bytes); }
    static void release(void* p) { hipFree(p); }
};
struct PinnedMem {
    static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes); }
    static void release(void* p) { hipHostFree(p); }
};

template <class T, class Mem>
class Buffer {
public:
    Buffer() = default;
    explicit Buffer(T* adopt) : p_(adopt) {}          // takes over an allocation of the same kind (capacity unknown: 0)
    Buffer(const Buffer&) = delete;
    Buffer& operator=(const Buffer&) = delete;
    Buffer(Buffer&& o) noexcept : p_(o.p_), cap_(o.cap_) {
        o.p_ = nullptr;
        o.cap_ = 0;
    }
    Buffer& operator=(Buffer&& o) noexcept {
        if (this != &o) {
            reset();
            std::swap(p_, o.p_);
            std::swap(cap_, o.cap_);
        }
        return *this;
    }
    ~Buffer() { reset(); }

    void reset() {
        if (p_) Mem::release(p_);
        p_ = nullptr;
        cap_ = 0;
    }
    // frees what it holds, then allocates `count` elements; on failure it holds nothing
    hipError_t alloc(size_t count) {
        reset();
        void* p = nullptr;
        hipError_t e = Mem::alloc(&p, count * sizeof(T));
        if (e != hipSuccess) {
            if (p) Mem::release(p);
            return e;
        }
        p_ = static_cast<T*>(p);
        cap_ = count;
        return hipSuccess;
    }
    // at least `count` elements: nothing to do if they are there, else the streams are synchronised (a launch queued on them may still
    // use the buffer), it is freed and max(count, floor) elements are allocated
    hipError_t grow(size_t count, size_t floor, std::initializer_list<hipStream_t> sync = {}) {
        if (cap_ >= count) return hipSuccess;
        for (hipStream_t s : sync) {
            hipError_t e = hipStreamSynchronize(s);
            if (e != hipSuccess) return e;
        }
        return alloc(std::max(count, floor));
    }
    T* release() {
        T* p = p_;
        p_ = nullptr;
        cap_ = 0;
        return p;
    }

    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t cap() const { return cap_; }

private:
    T* p_ = nullptr;
    size_t cap_ = 0;
};

template <class T> using DevBuf = Buffer<T, DeviceMem>;
template <class T> using HostBuf = Buffer<T, PinnedMem>;

}  // namespace dnagpu

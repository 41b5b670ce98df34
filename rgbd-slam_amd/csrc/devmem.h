// devmem.h -- move-only owners of device memory, pinned host memory and events (host runtime only).
//
// A buffer is freed by the destructor of the struct that declares it; structs handed to kernels hold raw
// pointers only.  Fallible operations return hipError_t like the launchers of dispatch.h, so callers write
// check_hip(c, buf.reserve(n), "what").
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>

namespace rgbd {

struct DevAlloc {
    static hipError_t get(void** p, size_t bytes) { return hipMalloc(p, bytes); }
    static void put(void* p) { (void)hipFree(p); }
};
struct PinnedAlloc {
    static hipError_t get(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static void put(void* p) { (void)hipHostFree(p); }
};

template <typename T, typename A>
class Buf {
public:
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    Buf(Buf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    Buf& operator=(Buf&& o) noexcept
    {
        if (this != &o) {
            release();
            p_ = o.p_; cap_ = o.cap_;
            o.p_ = nullptr; o.cap_ = 0;
        }
        return *this;
    }
    ~Buf() { release(); }

    // release, then n elements (at least 16 bytes, so n = 0 still gives a pointer); empty on failure
    hipError_t alloc(size_t n)
    {
        release();
        void* p = nullptr;
        const hipError_t e = A::get(&p, std::max<size_t>(n * sizeof(T), 16));
        if (e == hipSuccess) { p_ = static_cast<T*>(p); cap_ = n; }
        return e;
    }
    // at least n elements, growing by doubling; the contents are NOT kept; empty on failure
    hipError_t reserve(size_t n) { return n <= cap_ ? hipSuccess : alloc(std::max(n, 2 * cap_)); }
    void release()
    {
        if (p_) A::put(p_);
        p_ = nullptr; cap_ = 0;
    }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t capacity() const { return cap_; }   // elements

private:
    T* p_ = nullptr;
    size_t cap_ = 0;
};
template <typename T> using DevBuf = Buf<T, DevAlloc>;
template <typename T> using PinnedBuf = Buf<T, PinnedAlloc>;

class Event {
public:
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    ~Event() { if (e_) (void)hipEventDestroy(e_); }
    // created on first use, without timing
    hipError_t ensure()
    {
        if (e_) return hipSuccess;
        hipEvent_t e = nullptr;
        const hipError_t r = hipEventCreateWithFlags(&e, hipEventDisableTiming);
        if (r == hipSuccess) e_ = e;
        return r;
    }
    operator hipEvent_t() const { return e_; }

private:
    hipEvent_t e_ = nullptr;
};

}  // namespace rgbd

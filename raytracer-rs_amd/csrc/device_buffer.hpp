// device_buffer.hpp — the owner of one HIP allocation: device memory (hipMalloc) or pinned host memory (hipHostMalloc), freed by reset() and by
// the destructor.  It may count its bytes into a running total while it holds them (Renderer::hbm_allocated_bytes) and carry a 0xA5 guard tail.
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstdint>
#include <utility>

namespace mi355rt {

template <class T, bool Pinned>
class HipBuffer {
public:
    HipBuffer() = default;
    HipBuffer(HipBuffer&& o) noexcept : s_(std::exchange(o.s_, State{})) {}
    HipBuffer& operator=(HipBuffer&& o) noexcept { if (this != &o) { reset(); s_ = std::exchange(o.s_, State{}); } return *this; }
    ~HipBuffer() { reset(); }

    // Frees what the buffer holds, then allocates bytes + guard.  On an error the buffer holds nothing.
    hipError_t alloc(size_t bytes, size_t* counter = nullptr, size_t guard = 0)
    {
        reset();
        void* p = nullptr;
        hipError_t e = Pinned ? hipHostMalloc(&p, bytes + guard, hipHostMallocDefault) : hipMalloc(&p, bytes + guard);
        if (e != hipSuccess) return e;
        s_ = State{ static_cast<T*>(p), bytes, guard, counter };
        if (counter) *counter += bytes + guard;
        if (guard && (e = hipMemset(static_cast<char*>(p) + bytes, 0xA5, guard)) != hipSuccess) reset();
        return e;
    }
    void reset()
    {
        if (!s_.p) return;
        if (Pinned) (void)hipHostFree(s_.p); else (void)hipFree(s_.p);
        if (s_.counter) *s_.counter -= s_.bytes + s_.guard;
        s_ = State{};
    }
    T* get() const { return s_.p; }
    size_t bytes() const { return s_.bytes; }                   // without the guard tail
    const uint8_t* guard() const { return s_.guard ? static_cast<const uint8_t*>(static_cast<const void*>(s_.p)) + s_.bytes : nullptr; }
    explicit operator bool() const { return s_.p != nullptr; }

private:
    struct State { T* p = nullptr; size_t bytes = 0, guard = 0; size_t* counter = nullptr; } s_;
};

template <class T = void> using DeviceBuffer = HipBuffer<T, false>;
template <class T = void> using PinnedBuffer = HipBuffer<T, true>;

}  // namespace mi355rt

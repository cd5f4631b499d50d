// staging.hpp — the caller's memory of ONE API call on the device.  A call says for every argument whether it is read (in), written (out) or
// needed by the kernels whether or not the caller wants it (scratch), and gets the pointer the kernels take: the caller's own when the call's memory is device
// memory, a temporary otherwise — uploaded as it is made, copied back by download().  Everything is queued on the call's stream and nothing here waits: the
// call synchronises once, behind download(), and the temporaries go with the object, after that wait.  Every temporary counts into the handle's
// hbm_allocated_bytes while it lives.  The first HIP error sticks (error()); after it every operation returns null and queues nothing.
#pragma once
#include <hip/hip_runtime_api.h>
#include <algorithm>
#include <vector>
#include "device_buffer.hpp"

namespace mi355rt {

class Staging {
public:
    // device: the caller's pointers are device memory of the stream's device, used in place
    Staging(hipStream_t stream, size_t* counter, bool device) : stream_(stream), counter_(counter), device_(device) {}

    // An input of `count` elements.  Host: its copy on the device; null or empty: null — or, with `dummy`, four valid bytes for a callee that needs a pointer
    template <class T> const T* in(const T* p, size_t count, bool dummy = false)
    {
        if (device_) return p;
        const size_t bytes = p ? count * sizeof(T) : 0;
        if (!bytes && !dummy) return nullptr;
        void* d = temp(std::max<size_t>(bytes, 4));
        if (d && bytes) note(hipMemcpyAsync(d, p, bytes, hipMemcpyHostToDevice, stream_));
        return static_cast<const T*>(d);
    }
    // An output of `count` elements; null: null.  Host: a temporary that download() copies back; preload: it starts as the caller's contents, so what the
    // kernels leave unwritten survives the round trip
    template <class T> T* out(T* p, size_t count, bool preload = false) { return p ? scratch(p, count, preload) : nullptr; }
    // An output the kernels write even when the caller passed null: then a temporary that nobody reads back
    template <class T> T* scratch(T* p, size_t count, bool preload = false)
    {
        if (device_ && p) return p;
        const size_t bytes = count * sizeof(T);
        void* d = bytes ? temp(bytes) : nullptr;
        if (d && p) {
            if (preload) note(hipMemcpyAsync(d, p, bytes, hipMemcpyHostToDevice, stream_));
            outs_.push_back(Out{ p, d, bytes });
        }
        return static_cast<T*>(d);
    }
    // download() copies only the first `count` elements of output p (0: nothing); p null or not staged: nothing to do
    template <class T> void only(T* p, size_t count)
    {
        for (Out& o : outs_) if (o.host == p) o.bytes = std::min(o.bytes, count * sizeof(T));
    }
    // Queues the copy of every staged output back to the caller
    hipError_t download()
    {
        for (const Out& o : outs_) if (o.bytes) note(hipMemcpyAsync(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost, stream_));
        outs_.clear();
        return err_;
    }
    hipError_t error() const { return err_; }

private:
    struct Out { void* host; void* dev; size_t bytes; };
    void note(hipError_t e) { if (err_ == hipSuccess) err_ = e; }
    void* temp(size_t bytes)
    {
        if (err_ != hipSuccess) return nullptr;
        DeviceBuffer<> b;
        note(b.alloc(bytes, counter_));
        temps_.push_back(std::move(b));
        return temps_.back().get();
    }
    hipStream_t stream_;
    size_t* counter_;
    bool device_;
    hipError_t err_ = hipSuccess;
    std::vector<DeviceBuffer<>> temps_;
    std::vector<Out> outs_;
};

}  // namespace mi355rt

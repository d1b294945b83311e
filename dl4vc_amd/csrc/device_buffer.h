// The one owner of device resources for the host code of the .hip files and the C-ABI files: device and pinned arrays that grow
// on demand, a handle's list of fixed blocks, events, streams, the guard that restores the caller's device, and the error macros of the functions that use them.
// An array that grows is freed and allocated anew with a quarter and 4096 elements to spare: its contents are not kept
// (Pinned::ensure_keep is the one exception).  A handle declares members only; they are destroyed in reverse order of declaration.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <deque>

#include "capi_shell.h"

namespace dev {

// n elements of T on the device, owned: freed with the object
template <class T>
struct Array {
    T* p = nullptr;
    size_t cap = 0;                                       // elements
    hipError_t ensure(size_t n) { return n <= cap ? hipSuccess : alloc(n + n / 4 + 4096); }
    // exactly n elements, for an array whose size is known when its handle opens
    hipError_t alloc(size_t n) {
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        const hipError_t e = hipMalloc((void**)&p, n * sizeof(T));
        if (e == hipSuccess) cap = n;
        return e;
    }
    T* get() const { return p; }
    size_t capacity() const { return cap; }
    template <class U> U* as() const { return (U*)p; }
    Array() = default;
    Array(const Array&) = delete;
    Array& operator=(const Array&) = delete;
    ~Array() { if (p) (void)hipFree(p); }
};
using Buffer = Array<uint8_t>;                            // bytes

// the blocks of a handle whose sizes are known when it opens (weights, workspaces): each at least 256 bytes, all owned here and
// freed with the list; the handle keeps typed pointers into them
struct Blocks {
    std::deque<Buffer> all;
    template <class T>
    hipError_t take(T** p, size_t count, bool zero) {
        all.emplace_back();
        Buffer& b = all.back();
        hipError_t e = b.alloc(count * sizeof(T) < 256 ? 256 : count * sizeof(T));
        if (e == hipSuccess && zero) e = hipMemset(b.p, 0, b.cap);
        if (e == hipSuccess) *p = (T*)b.p;
        return e;
    }
};

// pinned host bytes, owned
struct Pinned {
    uint8_t* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t n) { return ensure_keep(n, 0); }
    // the first `used` bytes survive the growth
    hipError_t ensure_keep(size_t n, size_t used) { return n <= cap ? hipSuccess : alloc(n + n / 4 + 4096, used); }
    hipError_t alloc(size_t want, size_t used = 0) {
        uint8_t* old = used ? p : nullptr;                // (nothing to keep: freed first, as a device array is)
        if (p && !old) (void)hipHostFree(p);
        p = nullptr; cap = 0;
        const hipError_t e = hipHostMalloc((void**)&p, want, hipHostMallocDefault);
        if (e == hipSuccess) cap = want; else p = nullptr;
        if (e == hipSuccess && old) memcpy(p, old, used);
        if (old) (void)hipHostFree(old);
        return e;
    }
    uint8_t* get() const { return p; }
    size_t capacity() const { return cap; }
    Pinned() = default;
    Pinned(const Pinned&) = delete;
    Pinned& operator=(const Pinned&) = delete;
    ~Pinned() { if (p) (void)hipHostFree(p); }
};

// created by the first ensure(), with the flags of its site
struct Event {
    hipEvent_t e = nullptr;
    hipError_t ensure(unsigned flags = hipEventDefault) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }
    operator hipEvent_t() const { return e; }
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    ~Event() { if (e) (void)hipEventDestroy(e); }
};

struct Stream {
    hipStream_t s = nullptr;
    hipError_t ensure() { return s ? hipSuccess : hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
    operator hipStream_t() const { return s; }
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
};

// the caller's current device, restored when the guard goes
struct DeviceGuard {
    int prev = -1;
    DeviceGuard() { if (hipGetDevice(&prev) != hipSuccess) prev = -1; }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

}  // namespace dev

// in a function that returns int: a failed HIP call is "<prefix><call>: <HIP's text>" in the string dst and -2
#define DEV_TRY(dst, prefix, x)                                                                                          \
    do {                                                                                                                 \
        const hipError_t e_ = (x);                                                                                       \
        if (e_ != hipSuccess) return capi::failf(dst, -2, "%s%s: %s", prefix, #x, hipGetErrorString(e_));                \
    } while (0)

// in a function that returns int and has `const char** msg`: a failed HIP call is its text in *msg and -2
#define HIP_CHECK_MSG(x)                                                   \
    do {                                                                   \
        const hipError_t e_ = (x);                                         \
        if (e_ != hipSuccess) { *msg = hipGetErrorString(e_); return -2; } \
    } while (0)

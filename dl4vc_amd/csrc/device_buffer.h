// Device allocations that grow on demand, and the error macro of the functions that use them (host code of the .hip files and
// the C-ABI files).  A buffer that grows is freed and allocated anew with a quarter to spare: its contents are not kept.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

namespace dev {

// bytes, owned: freed with the object
struct Buffer {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        const size_t want = bytes + bytes / 4 + 256;
        const hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    template <class T> T* as() const { return (T*)p; }
    Buffer() = default;
    Buffer(const Buffer&) = delete;
    Buffer& operator=(const Buffer&) = delete;
    ~Buffer() { if (p) (void)hipFree(p); }
};

// n elements behind a typed pointer its owner frees; cap in elements
template <class T>
bool grow(T*& p, size_t& cap, size_t n) {
    if (n <= cap) return true;
    if (p) (void)hipFree(p);
    p = nullptr; cap = 0;
    const size_t want = n + n / 4 + 64;
    if (hipMalloc((void**)&p, want * sizeof(T)) != hipSuccess) return false;
    cap = want;
    return true;
}

}  // namespace dev

// in a function that returns int and has `const char** msg`: a failed HIP call is its text in *msg and -2
#define HIP_CHECK_MSG(x)                                                   \
    do {                                                                   \
        const hipError_t e_ = (x);                                         \
        if (e_ != hipSuccess) { *msg = hipGetErrorString(e_); return -2; } \
    } while (0)

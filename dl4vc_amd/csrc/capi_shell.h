// What every extern "C" entry of the native libraries shares: the formatter of its error text and the shell that turns whatever
// its body throws into a code, so that the ABI never aborts.  Host only, no HIP include: the host-only builds of tools/asan_*.sh
// and tools/capi_shell_main.cpp compile it with a plain C++ compiler.  Each library keeps its own destination string.
#pragma once

#include <cstdarg>
#include <cstdio>
#include <exception>
#include <string>
#include <utility>

namespace capi {

// dst = the formatted text, cut at 1023 characters; returns code
inline int failf(std::string& dst, int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    dst = buf;
    return code;
}

// body(), or -4 with "<who>: <what()>" / "<who>: unknown exception" in dst
template <class F>
int guarded(std::string& dst, const char* who, F&& body) {
    try {
        return std::forward<F>(body)();
    } catch (const std::exception& e) {
        return failf(dst, -4, "%s: %s", who, e.what());
    } catch (...) {
        return failf(dst, -4, "%s: unknown exception", who);
    }
}

}  // namespace capi

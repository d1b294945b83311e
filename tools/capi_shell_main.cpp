// Stand-alone driver of dl4vc_amd/csrc/capi_shell.h (tests/test_capi_shell_host.py builds and runs it; the same file is clean under
// -fsanitize=address,undefined): what an extern "C" body returns and leaves as its error text when it ends normally and when it
// throws, and the formatter at its buffer's limit.  Prints "ok: N checks, 0 mismatches" or every mismatch.
#include <cstring>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>

#include "../dl4vc_amd/csrc/capi_shell.h"

namespace {

int checks = 0, bad = 0;

void expect(const char* what, int rc, int want_rc, const std::string& text, const std::string& want_text) {
    ++checks;
    if (rc == want_rc && text == want_text) return;
    ++bad;
    printf("MISMATCH %s: rc %d (want %d), text \"%s\" (want \"%s\")\n", what, rc, want_rc, text.c_str(), want_text.c_str());
}

thread_local std::string tl_err;
std::string plain_err;

// every case once, with dst as the destination
void cases(std::string& dst, const char* tag) {
    dst = "stale";
    expect(tag, capi::guarded(dst, "entry", [&] { return 7; }), 7, dst, "stale");
    expect(tag, capi::guarded(dst, "entry", [&] { return capi::failf(dst, -3, "%s at %d", "bad record", 42); }), -3, dst, "bad record at 42");
    expect(tag, capi::guarded(dst, "entry", [&]() -> int { throw std::bad_alloc(); }), -4, dst, std::string("entry: ") + std::bad_alloc().what());
    expect(tag, capi::guarded(dst, "entry", [&]() -> int { throw std::runtime_error("x"); }), -4, dst, "entry: x");
    expect(tag, capi::guarded(dst, "entry", [&]() -> int { throw 5; }), -4, dst, "entry: unknown exception");
    // 2000 characters: cut at 1023, terminated, nothing written past the 1024-byte buffer (the sanitizer build watches the stack)
    const std::string big(2000, 'm');
    expect(tag, capi::failf(dst, -1, "%s", big.c_str()), -1, dst, std::string(1023, 'm'));
    expect(tag, capi::failf(dst, -2, "%s", std::string(1023, 'k').c_str()), -2, dst, std::string(1023, 'k'));
    expect(tag, (int)strlen(dst.c_str()), 1023, "", "");
    expect(tag, capi::guarded(dst, "who", [&]() -> int { throw std::runtime_error(big); }), -4, dst, "who: " + std::string(1018, 'm'));
}

}  // namespace

int main() {
    cases(plain_err, "plain destination");
    cases(tl_err, "thread_local destination");
    // another thread's text is its own: the first thread's stays
    tl_err = "first thread";
    std::thread([] {
        cases(tl_err, "thread_local destination, second thread");
        expect("second thread's text", 0, 0, tl_err.substr(0, 5), "who: ");
    }).join();
    expect("first thread's text", 0, 0, tl_err, "first thread");
    if (bad) return 1;
    printf("ok: %d checks, 0 mismatches\n", checks);
    return 0;
}

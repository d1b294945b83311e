// Stand-alone driver of tools/asan_loader.sh: dan_loader.cpp and dan_pileup.cpp (libdl4vc_loader.so's two sources) compiled into
// this program under the sanitizers, called through their C ABI over the files tests/loader_shell_cases.py writes into the
// directory given as argv[1]:
//   * the candidate files of 24 records in chunks of 8 -- intact, and with chunk 1 inflating short, cut, too long, stored short
//     without the filter -- on 1 and 3 worker threads, batches of 8 from record 0 and from record 4 (pieces straddle chunks),
//     every plane in a heap buffer of exactly its size;
//   * the record types whose fields leave the record (refused by dl_open);
//   * dl_open then dl_close without a dl_next, and dl_close while the workers still hold pieces;
//   * pe_encode on 1 and 3 threads over the damaged BAM records, and over a good one;
//   * every allocation of dl_open .. dl_next .. dl_close and of pe_open .. pe_encode failing in turn (this program replaces
//     operator new to that end): each run ends in a count or in a negative code with a text, never in an abort or a wait
//     without end.
// Exit status 0 and "asan_loader: ok" when every call gave what it must.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <new>
#include <string>
#include <vector>

#include "../include/dl4vc_loader.h"

// ---- allocation failures on request: the g_fail_in'th operator new from now throws (-1: none).  Only the library's allocations
// count: those of its own threads, and those of the main thread while it is inside an entry (lib()).
static std::atomic<long> g_fail_in{-1};
static thread_local bool t_driver = false;
template <class F>
static auto lib(F&& call) {
    t_driver = false;
    const auto rc = call();
    t_driver = true;
    return rc;
}
static void* take(size_t n) {
    if (!t_driver && g_fail_in.load() >= 0 && g_fail_in.fetch_sub(1) == 0) throw std::bad_alloc();
    void* p = malloc(n ? n : 1);
    if (!p) throw std::bad_alloc();
    return p;
}
void* operator new(size_t n) { return take(n); }
void* operator new[](size_t n) { return take(n); }
void* operator new(size_t n, const std::nothrow_t&) noexcept { try { return take(n); } catch (...) { return nullptr; } }
void* operator new[](size_t n, const std::nothrow_t&) noexcept { try { return take(n); } catch (...) { return nullptr; } }
void operator delete(void* p) noexcept { free(p); }
void operator delete[](void* p) noexcept { free(p); }
void operator delete(void* p, size_t) noexcept { free(p); }
void operator delete[](void* p, size_t) noexcept { free(p); }
void operator delete(void* p, const std::nothrow_t&) noexcept { free(p); }
void operator delete[](void* p, const std::nothrow_t&) noexcept { free(p); }

static int g_checks = 0, g_failed = 0;
static void check(bool ok, const char* what, const std::string& detail = "") {
    ++g_checks;
    if (!ok) { ++g_failed; fprintf(stderr, "asan_loader: FAILED %s %s\n", what, detail.c_str()); }
}
static bool has(const std::string& s, const char* part) { return s.find(part) != std::string::npos; }

static const int N = 24, R = 10, L = 201, BATCH = 8;

struct Planes {       // one batch, every buffer ending where its data ends
    std::vector<uint8_t> reads, qual, strand, ref, rmask, vmask, black;
    std::vector<char> vcf;
    std::vector<int32_t> num;
    explicit Planes(int b) : reads((size_t)b * R * L), qual(reads.size()), strand(reads.size()), ref((size_t)b * L), rmask(ref.size()),
                             vmask(ref.size()), black(b), vcf((size_t)b * 129), num(b) {}
};

struct Drained { int rc_open = 0; int64_t rc = 0, delivered = 0; std::string text; std::vector<uint8_t> reads; };

// opens, reads to the end or to the first error, closes
static Drained drain(const std::string& path, int threads, int64_t lo, int batch = BATCH, int max_calls = 1 << 30) {
    Drained d;
    dl_loader_t* l = nullptr;
    d.rc_open = lib([&] { return dl_open(path.c_str(), "", R, lo, -1, batch, 0, 0, threads, 1, &l); });
    if (d.rc_open != 0) { d.text = dl_last_error(nullptr); return d; }
    Planes p(batch);
    for (int call = 0; call < max_calls; ++call) {
        d.rc = lib([&] {
            return dl_next(l, p.reads.data(), p.qual.data(), p.strand.data(), p.ref.data(), p.rmask.data(), p.vmask.data(), p.vcf.data(),
                           p.num.data(), p.black.data());
        });
        if (d.rc <= 0) break;
        d.delivered += d.rc;
        d.reads.insert(d.reads.end(), p.reads.begin(), p.reads.begin() + (size_t)d.rc * R * L);
    }
    if (d.rc < 0) d.text = dl_last_error(l);
    dl_close(l);
    return d;
}

static void chunk_cases(const std::string& dir) {
    static const struct { const char* name; const char* text; } CASES[] = {
        {"intact", nullptr}, {"short_inflate", "chunk 1 holds 15425 bytes once inflated"}, {"truncated", "zlib inflate failed"},
        {"too_long", "zlib inflate failed"}, {"short_raw", "chunk 1 holds 15425 bytes, the piece needs"}};
    std::vector<uint8_t> whole;
    for (const auto& c : CASES)
        for (int threads : {1, 3})
            for (int64_t lo : {0, 4}) {
                const Drained d = drain(dir + "/" + c.name + ".hdf", threads, lo);
                const std::string tag = std::string(c.name) + " threads " + std::to_string(threads) + " lo " + std::to_string(lo);
                if (!c.text) {
                    check(d.rc_open == 0 && d.rc == 0 && d.delivered == N - lo, "an intact file is read to its end", tag + " " + d.text);
                    if (lo == 0) whole = d.reads;
                    else check(d.reads.size() + 4u * R * L == whole.size() && memcmp(d.reads.data(), whole.data() + 4u * R * L, d.reads.size()) == 0,
                               "records 4.. are the same from either start", tag);
                } else {
                    check(d.rc_open == 0 && d.rc == -2 && has(d.text, c.text), "a damaged chunk 1 is refused", tag + ": " + d.text);
                    check(d.delivered == (lo == 0 ? 8 : 0) && (d.reads.empty() || memcmp(d.reads.data(), whole.data(), d.reads.size()) == 0),
                          "nothing of a failed piece is delivered", tag);
                }
            }
    for (const char* name : {"strand_past_record", "ref_bases_in_front"}) {
        const Drained d = drain(dir + "/" + name + ".hdf", 1, 0);
        check(d.rc_open == -1 && has(d.text, "unexpected record layout"), "a record type whose fields leave the record is refused", d.text);
    }
}

static void open_and_close(const std::string& dir) {
    const std::string path = dir + "/intact.hdf";
    for (int i = 0; i < 50; ++i) {                              // never read
        dl_loader_t* l = nullptr;
        check(dl_open(path.c_str(), nullptr, R, 0, -1, BATCH, 0, 0, 4, 3, &l) == 0 && l, "dl_open", dl_last_error(nullptr));
        dl_close(l);
    }
    for (int batch : {1, 2, 8})                                 // closed after one batch, the workers ahead of it
        for (int threads : {1, 3}) {
            const Drained d = drain(path, threads, 0, batch, 1);
            check(d.rc_open == 0 && d.rc == batch, "dl_close while workers hold pieces");
        }
    dl_close(nullptr);
    check(dl_next(nullptr, 0, 0, 0, 0, 0, 0, 0, 0, 0) == -1, "dl_next without a handle");
}

struct Encoded { int rc_open = 0, rc = 0; std::string text; int8_t status[6] = {0}; };

static Encoded encode(const std::string& dir, const std::string& name, int threads) {
    static const char* const CONTIGS[6] = {"ref", "ref", "ref", "ref", "ref", "ref"};
    static const int32_t POS[6] = {110, 115, 120, 125, 130, 135};
    const int W = 33, MR = 50;
    Encoded e;
    const pe_options opt = {16, MR, 10, 50, 0};
    pe_encoder_t* h = nullptr;
    const std::string bam = dir + "/" + name + ".bam", fa = dir + "/" + name + ".fa";
    e.rc_open = lib([&] { return pe_open(bam.c_str(), nullptr, fa.c_str(), &opt, &h); });
    if (e.rc_open != 0) { e.text = pe_last_error(nullptr); return e; }
    std::vector<uint8_t> reads((size_t)6 * MR * W), qual(reads.size()), strand(reads.size()), ref((size_t)6 * W);
    std::vector<int32_t> num(6);
    e.rc = lib([&] {
        return pe_encode(h, CONTIGS, POS, 6, reads.data(), qual.data(), strand.data(), ref.data(), num.data(), e.status, threads);
    });
    if (e.rc != 0) e.text = pe_last_error(h);
    pe_close(h);
    return e;
}

static void bam_cases(const std::string& dir) {
    static const char* const DAMAGED[] = {"l_seq_beyond_record", "negative_l_seq", "negative_block_size", "tiny_block_size",
                                          "cigar_count_beyond_record", "truncated_record", "l_read_name_zero"};
    for (int threads : {1, 3}) {
        for (const char* name : DAMAGED) {
            const Encoded e = encode(dir, name, threads);
            const bool named = has(e.text, "corrupt BAM record") || has(e.text, "truncated BAM record") || has(e.text, "BGZF");
            check(e.rc_open == 0 && e.rc == -1 && named, "a damaged BAM record is refused", std::string(name) + ": " + e.text);
            if (!strcmp(name, "l_read_name_zero")) check(has(e.text, "corrupt BAM record (l_read_name)"), "the core's own text", e.text);
        }
        const Encoded e = encode(dir, "good", threads);
        check(e.rc_open == 0 && e.rc == 0 && e.status[0] == 1 && e.status[5] == 1, "a good BAM is encoded", e.text);
    }
    pe_close(nullptr);
}

// Every allocation of a whole run fails in turn, until a run needs fewer allocations than the countdown.
static void allocation_failures(const std::string& dir) {
    int refused = 0;
    for (long k = 0;; ++k) {
        g_fail_in = k;
        const Drained d = drain(dir + "/intact.hdf", 3, 4, 2);
        const bool fired = g_fail_in.exchange(-1) < 0;
        if (!fired) { check(d.rc_open == 0 && d.rc == 0 && d.delivered == N - 4, "the run no allocation failed in"); break; }
        const bool refusal = d.rc_open != 0 ? (d.rc_open == -4 || d.rc_open == -1) && !d.text.empty() : (d.rc == -2 || d.rc == -4) && !d.text.empty();
        // (an allocation may also fail where its result is not needed: then the run is whole)
        check(refusal || (d.rc == 0 && d.delivered == N - 4), "a failed allocation in the loader is a code and a text",
              "allocation " + std::to_string(k) + ": open " + std::to_string(d.rc_open) + " next " + std::to_string(d.rc) + " " + d.text);
        refused += refusal;
    }
    check(refused > 10, "allocation failures reached the loader");
    refused = 0;
    for (long k = 0;; ++k) {
        g_fail_in = k;
        const Encoded e = encode(dir, "good", 3);
        const bool fired = g_fail_in.exchange(-1) < 0;
        if (!fired) { check(e.rc_open == 0 && e.rc == 0, "the run no allocation failed in"); break; }
        const bool refusal = (e.rc_open != 0 || e.rc != 0) && !e.text.empty();
        check(refusal || (e.rc_open == 0 && e.rc == 0), "a failed allocation in the encoder is a code and a text", "allocation " + std::to_string(k));
        refused += refusal;
    }
    check(refused > 10, "allocation failures reached the encoder");
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: asan_loader DIR (the files of tests/loader_shell_cases.py)\n"); return 2; }
    t_driver = true;
    const std::string dir = argv[1];
    chunk_cases(dir);
    open_and_close(dir);
    bam_cases(dir);
    allocation_failures(dir);
    int32_t rows[8];
    check(dl_select_rows(7, 20, 20, 8, rows) == 8, "dl_select_rows");
    if (g_failed) { fprintf(stderr, "asan_loader: %d of %d checks failed\n", g_failed, g_checks); return 1; }
    printf("asan_loader: ok, %d checks\n", g_checks);
    return 0;
}

// pg_debug_run_records (include/dl4vc_pileup_gpu.h): the framed records of one run by the host path and by the CPU twin of the
// device path, for tests without a GPU.  No device call.  With -DPG_HOST_ONLY a plain C++ compiler builds this file alone
// (tools/asan_pileup_frame.sh runs it under sanitizers, together with the host entry of bgzf_capi.cpp).
#include "../../include/dl4vc_pileup_gpu.h"
#include "capi_shell.h"
#include "pileup_fetch.h"

std::string pgh::g_err;

#ifdef PG_HOST_ONLY
extern "C" const char* pg_last_error(const pg_encoder_t*) { return pgh::g_err.c_str(); }
#endif

extern "C" int pg_debug_run_records(const char* bam_path, const char* bai_path, int32_t tid, int64_t s0, int64_t stop, int path,
                                    pg_rec_view* out, int64_t cap, int64_t* n, int64_t* max_nref, int32_t* sorted) {
    return capi::guarded(pgh::g_err, "pg_debug_run_records", [&] {
        if (!bam_path || !bai_path || !n || !max_nref || !sorted || (cap > 0 && !out)) return capi::failf(pgh::g_err, -1, "pg_debug_run_records: null argument");
        if (path < 0 || path > 2) return capi::failf(pgh::g_err, -1, "pg_debug_run_records: path is 0, 1 or 2");
        bamn::Bai bai;
        if (!bai.load(bai_path)) return capi::failf(pgh::g_err, -3, "cannot read the BAI index %s", bai_path);
        pgh::RunRecs run;
        if (path == 0) {
            bamn::BamFile bam;
            std::vector<uint8_t> blk;
            if (!bam.open(bam_path)) return capi::failf(pgh::g_err, -3, "%s", bam.err.c_str());
            pgh::fetch_records(bai, bam, blk, tid, s0, stop, run);
        } else if (path == 1) {
            pgh::twin_records(bai, bam_path, tid, s0, stop, run);
        } else {                                             // a call that also asks for the contig's first bases
            const pgh::Region first{tid, 0, 64};
            pgh::twin_records(bai, bam_path, tid, s0, stop, run, &first, 1);
        }
        if (!run.err.empty()) return capi::failf(pgh::g_err, -3, "%s", run.err.c_str());
        *n = (int64_t)run.recs.size();
        *max_nref = run.max_nref;
        *sorted = run.sorted ? 1 : 0;
        for (int64_t i = 0; i < *n && i < cap; ++i) {
            const pg::Rec& m = run.recs[(size_t)i];
            pg_rec_view& v = out[i];
            v.pos = m.pos; v.end = m.end; v.res = m.res; v.l_seq = m.l_seq;
            v.cigar_off = m.cigar_off; v.seq_off = m.seq_off; v.qual_off = m.qual_off;
            v.n_cig = m.n_cig; v.l_name = m.l_name; v.bits = m.bits;
            uint64_t hsh = 1469598103934665603ull;           // FNV-1a 64 over the record up to the end of its qualities
            const uint8_t* b = run.bytes.data() + m.off;
            for (uint64_t k = 0; k < (uint64_t)m.qual_off + (uint64_t)m.l_seq; ++k) hsh = (hsh ^ b[k]) * 1099511628211ull;
            v.bytes_hash = hsh;
        }
        return 0;
    });
}

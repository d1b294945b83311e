// FASTA + .fai access (without a .fai: one scan of the file, as dl4vc_amd/bamio.py::FastaFile._scan), shared by the CPU pileup
// encoder (dan_pileup.cpp) and the GPU pileup encoder (pileup_capi.cpp).
#pragma once

#include <algorithm>
#include <cctype>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace fastan {

struct Fasta {
    FILE* f = nullptr;
    struct Entry { int64_t length, offset, lb, lw; };
    std::map<std::string, Entry> index;

    bool open(const std::string& path, std::string& err) {
        f = fopen(path.c_str(), "rb");
        if (!f) { err = "cannot open " + path; return false; }
        FILE* fai = fopen((path + ".fai").c_str(), "r");
        if (fai) {
            char line[4096];
            while (fgets(line, sizeof line, fai)) {
                char name[2048];
                long long a, b, c, d;
                // tab separated: name, length, offset, line bases, line width
                char* tab = strchr(line, '\t');
                if (!tab) continue;
                const size_t nl = (size_t)(tab - line);
                if (nl >= sizeof name) continue;
                memcpy(name, line, nl); name[nl] = 0;
                if (sscanf(tab + 1, "%lld\t%lld\t%lld\t%lld", &a, &b, &c, &d) == 4) index[name] = Entry{a, b, c, d};
            }
            fclose(fai);
        } else {
            // scan (dl4vc_amd/bamio.py::FastaFile._scan)
            std::string name;
            bool have = false;
            Entry e{0, 0, 0, 0};
            int64_t pos = 0;
            std::vector<char> buf(1 << 20);
            std::string line;
            int ch;
            line.reserve(256);
            auto flush_line = [&](const std::string& ln) {
                if (!ln.empty() && ln[0] == '>') {
                    if (have) index[name] = e;
                    size_t a = 1, b = 1;
                    while (b < ln.size() && !isspace((unsigned char)ln[b])) ++b;
                    name = ln.substr(a, b - a);
                    have = true;
                    e = Entry{0, pos + (int64_t)ln.size(), 0, 0};
                } else if (have) {
                    size_t bases = ln.size();
                    while (bases > 0 && (ln[bases - 1] == '\n' || ln[bases - 1] == '\r')) --bases;
                    if (e.lb == 0) { e.lb = (int64_t)bases; e.lw = (int64_t)ln.size(); }
                    e.length += (int64_t)bases;
                }
                pos += (int64_t)ln.size();
            };
            while ((ch = fgetc(f)) != EOF) {
                line.push_back((char)ch);
                if (ch == '\n') { flush_line(line); line.clear(); }
            }
            if (!line.empty()) flush_line(line);
            if (have) index[name] = e;
        }
        return true;
    }
    const Entry* entry(const std::string& ref) const {
        auto it = index.find(ref);
        if (it != index.end()) return &it->second;
        const std::string alt = ref.rfind("chr", 0) == 0 ? ref.substr(3) : "chr" + ref;
        it = index.find(alt);
        return it == index.end() ? nullptr : &it->second;
    }
    // bases of [start, end) as stored; false when the sequence is absent
    bool fetch(const std::string& ref, int64_t start, int64_t end, std::string& out) {
        out.clear();
        const Entry* e = entry(ref);
        if (!e) return false;
        start = std::max<int64_t>(0, start); end = std::min(end, e->length);
        if (end <= start || e->lb <= 0) return true;
        const int64_t first = e->offset + (start / e->lb) * e->lw + start % e->lb;
        const int64_t last = e->offset + ((end - 1) / e->lb) * e->lw + (end - 1) % e->lb;
        std::vector<char> raw((size_t)(last - first + 1));
        fseeko(f, first, SEEK_SET);
        const size_t got = fread(raw.data(), 1, raw.size(), f);
        for (size_t i = 0; i < got; ++i) if (raw[i] != '\n' && raw[i] != '\r') out.push_back(raw[i]);
        return true;
    }
    ~Fasta() { if (f) fclose(f); }
};

}  // namespace fastan

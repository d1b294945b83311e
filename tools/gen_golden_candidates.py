#!/usr/bin/env python
"""Writes tests/golden/candidates_*.json.gz from the REFERENCE's own candidate_generator.py / bedutils.py functions.

Run only where a checkout of the reference exists (``--reference DIR``); never in a test or on the GPU machine.  pysam and
tqdm are stubbed in sys.modules; the reference's functions (detect_variants, build_allele_stats,
filter_alleles_by_frequency, remove_multialleles, generate_contig_regions, generate_contig_subregions,
collate_subregions_into_groups) run on a pysam stand-in: get_aligned_pairs(with_seq=True) rebuilt from CIGAR + MD + SEQ,
get_reference_positions, and fetch with htslib's overlap rule (pos < end and bam_endpos > start, no flag filter).  The
stand-in raises ValueError where this project skips a read on purpose (no MD; N / P CIGAR operations; SEQ '*'; an MD that
disagrees with the CIGAR): the reference then counts the read's coverage and drops its alleles.  The VCF lines are this
project's text (unpinned) over the reference's tuples in the reference's final order.
"""
import argparse
import contextlib
import gzip
import io
import json
import os
import random
import re
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dl4vc_amd import candidates as C   # noqa: E402

M, I, D, N, S, H, P, EQ, X = range(9)


def expand_md(md):
    """MD -> list of ('m', None) / ('x', letter) / ('d', letters); None when it is not in the strict grammar."""
    out = []
    pos = 0
    for m in re.finditer(r"(\d+)|\^([A-Z]+)|([A-Z])", md):
        if m.start() != pos:
            return None
        pos = m.end()
        if m.group(1) is not None:
            out += [("m", None)] * int(m.group(1))
        elif m.group(2) is not None:
            out.append(("d", m.group(2)))
        else:
            out.append(("x", m.group(3)))
    return out if pos == len(md) else None


class Read:
    def __init__(self, d, references):
        self.d = d
        self.reference_name = references[d["tid"]][0]
        self.pos = d["pos"]
        self.flag = d["flag"]
        self.cigartuples = [tuple(c) for c in d["cigar"]]
        self.seq = d["seq"] or None

    def endpos(self):
        rl = sum(l for op, l in self.cigartuples if op in (M, D, N, EQ, X))
        return self.pos + 1 if (self.flag & 4) or rl == 0 else self.pos + rl

    def get_reference_positions(self):
        out, r = [], self.pos
        for op, l in self.cigartuples:
            if op in (M, EQ, X):
                out += range(r, r + l)
            if op in (M, D, N, EQ, X):
                r += l
        return out

    def get_aligned_pairs(self, with_seq=True, matches_only=False):
        if self.d["md"] is None:
            raise ValueError("MD tag not present")
        if not self.cigartuples:
            return []
        if any(op in (N, P) for op, _ in self.cigartuples) or not self.seq:
            raise ValueError("unsupported read (N / P operation or SEQ '*')")
        toks = expand_md(self.d["md"])
        if toks is None:
            raise ValueError("malformed MD")
        # pairs without reference bases first, then the MD laid over them
        pairs, q, r = [], 0, self.pos
        for op, l in self.cigartuples:
            for _ in range(l):
                if op in (M, EQ, X):
                    pairs.append([q, r, None]); q += 1; r += 1
                elif op in (I, S):
                    pairs.append([q, None, None]); q += 1
                elif op == D:
                    pairs.append([None, r, None]); r += 1
        if q != len(self.seq):
            raise ValueError("malformed MD")
        t = 0
        i = 0
        while i < len(pairs):
            p = pairs[i]
            if p[1] is None:
                i += 1
                continue
            if t >= len(toks):
                raise ValueError("malformed MD")
            kind, v = toks[t]
            if p[0] is not None:
                if kind == "d":
                    raise ValueError("malformed MD")
                p[2] = self.seq[p[0]] if kind == "m" else v.lower()
                t += 1
                i += 1
            else:
                j = i
                while j < len(pairs) and pairs[j][0] is None and pairs[j][1] is not None:
                    j += 1
                if kind != "d" or len(v) != j - i:
                    raise ValueError("malformed MD")
                for k in range(i, j):
                    pairs[k][2] = v[k - i]
                t += 1
                i = j
        if t != len(toks):
            raise ValueError("malformed MD")
        return [tuple(p) for p in pairs]


class FakeBam:
    def __init__(self, references, reads):
        self.references = [n for n, _ in references]
        self.lengths = [l for _, l in references]
        self.reads = [Read(r, references) for r in reads]
        self.malformed = 0

    def fetch(self, contig, start, end):
        tid = self.references.index(contig)
        for r in self.reads:
            if r.d["tid"] == tid and r.pos < end and r.endpos() > start:
                if r.d.get("malformed"):
                    self.malformed += 1
                yield r


def load_reference(ref_dir):
    sys.modules["pysam"] = types.ModuleType("pysam")
    tq = types.ModuleType("tqdm")
    tq.tqdm = lambda x, **k: x
    sys.modules["tqdm"] = tq
    sys.path.insert(0, os.path.join(ref_dir, "tools"))
    import candidate_generator as cg          # noqa: E402
    return cg


def flag_table(cg):
    import argparse as ap
    captured = {}
    orig = ap.ArgumentParser.parse_args

    def grab(self, *a, **k):
        captured["p"] = self
        raise SystemExit(0)
    ap.ArgumentParser.parse_args = grab
    try:
        cg.main()
    except SystemExit:
        pass
    finally:
        ap.ArgumentParser.parse_args = orig
    out = []
    for a in captured["p"]._actions:
        if a.dest == "help":
            continue
        out.append({"flags": list(a.option_strings), "dest": a.dest, "default": a.default,
                    "type": a.type.__name__ if a.type else None, "action": type(a).__name__})
    return out


def run_case(cg, refs, reads, params, bed_text, tmp):
    bam = FakeBam(refs, reads)
    bedfile = None
    if bed_text is not None:
        bedfile = os.path.join(tmp, "case.bed")
        open(bedfile, "w").write(bed_text)
    args = types.SimpleNamespace(keep_contig_chr=params["keep_contig_chr"])
    with contextlib.redirect_stdout(io.StringIO()):
        regions = cg.generate_contig_regions(dict(zip(bam.references, bam.lengths)), bam, params["contigs"], bedfile, args)
        size = params["chunk_size"] * 1000
        subs = cg.generate_contig_subregions(regions, size)
        groups = cg.collate_subregions_into_groups(subs, size)
        cands = []
        for g in groups:
            for sub in g:
                cov, freq = cg.build_allele_stats(sub, bam, max_len_indel_allele=params["max_len_indel_allele"])
                f = cg.filter_alleles_by_frequency(cov, freq, params["snp_min_freq"], params["indel_min_freq"])
                if not params["keep_multialleles"]:
                    f = list(cg.remove_multialleles(f))
                cands += f
    lines = [C.record_line(*c) for c in cands]
    order = sorted(range(len(lines)), key=lambda i: (lines[i].split("\t")[0].encode(), int(lines[i].split("\t")[1]), lines[i].encode()))
    return {"regions": [list(r) for r in regions], "subregions": [list(s) for s in subs], "groups": [[list(s) for s in g] for g in groups],
            "tuples": [list(cands[i]) for i in order], "lines": [lines[i] for i in order], "malformed_fetched": bam.malformed}


# ---- reads ------------------------------------------------------------------------------------------------------------------
def md_for(ref, pos, cigar, seq):
    """The standard MD of a read against ``ref`` (mismatch letters upper case, '0' separators where needed)."""
    out, run, q, r, last_del = [], 0, 0, pos, False
    for op, l in cigar:
        if op in (M, EQ, X):
            for _ in range(l):
                if seq[q] == ref[r]:
                    run += 1
                else:
                    out.append("%d%s" % (run, ref[r])); run = 0
                q += 1; r += 1
        elif op in (I, S):
            q += l
        elif op == D:
            out.append("%d^%s" % (run, ref[r:r + l])); run = 0; r += l
    out.append(str(run))
    return "".join(out)


def rd(name, tid, pos, cigar, seq, md="auto", flag=0, ref=None, malformed=False):
    if md == "auto":
        md = md_for(ref, pos, cigar, seq)
    return {"name": name, "tid": tid, "pos": pos, "flag": flag, "cigar": [list(c) for c in cigar], "seq": seq, "md": md,
            "malformed": malformed}


def apply(ref, pos, cigar, subst=()):
    """A read sequence for ``cigar`` at ``pos``: reference bases, inserted / clipped bases random, ``subst`` {query index: base}."""
    rng = random.Random(pos * 7 + len(cigar))
    seq, r = [], pos
    for op, l in cigar:
        if op in (M, EQ, X):
            seq += list(ref[r:r + l]); r += l
        elif op in (I, S):
            seq += [rng.choice("ACGT") for _ in range(l)]
        elif op in (D, N):
            r += l
    for k, b in dict(subst).items():
        seq[k] = b
    return "".join(seq)


def edge_case(rng_seed=11):
    rng = random.Random(rng_seed)
    L = 3200
    ref = "".join(rng.choice("ACGT") for _ in range(L))
    reads = []

    def add(name, pos, cigar, subst=(), **kw):
        seq = kw.pop("seq", None) or apply(ref, pos, cigar, subst)
        reads.append(rd(name, 0, pos, cigar, seq, ref=ref, **kw))

    # a pile-up at 995..1005 so that the 1 kb boundary carries SNPs / indels (chunk_size 1)
    for k in range(8):
        add("b%d" % k, 960 + k, [(M, 80)], {1000 - (960 + k): "A" if ref[1000] != "A" else "C"})
        add("c%d" % k, 950 + k, [(M, 50 - k), (I, 2), (M, 30)])
        add("e%d" % k, 940 + k, [(M, 60 - k), (D, 3), (M, 30)])
    # multi-allelic site at 1500: SNP to two bases and an insertion
    for k in range(6):
        alt = "ACGT".replace(ref[1500], "")[k % 2]
        add("m%d" % k, 1450 + k, [(M, 100)], {1500 - (1450 + k): alt})
    add("mi", 1460, [(M, 41), (I, 1), (M, 40)])
    # clips with insertions next to them (dropped), hard clips
    add("clip1", 1200, [(S, 5), (I, 3), (M, 50), (I, 2), (S, 4)])
    add("clip2", 1210, [(H, 7), (S, 2), (M, 40), (I, 4), (M, 10), (H, 3)])
    # I -> D (all deletions of the read dropped), D -> I (insertion anchored on a deleted position)
    add("id1", 1300, [(M, 20), (D, 2), (M, 10), (I, 2), (D, 3), (M, 20)])
    add("di1", 1305, [(M, 15), (D, 2), (I, 3), (M, 20)])
    add("di2", 1306, [(M, 14), (D, 2), (I, 3), (M, 20)])
    # deletion at the first pair: anchored on the last pair
    add("lead", 1350, [(S, 3), (D, 2), (M, 30)])
    # mismatched anchors: insertion / deletion right after a mismatch
    add("ma1", 1400, [(M, 10), (I, 2), (M, 10)], {9: "A" if ref[1409] != "A" else "G"})
    add("ma2", 1402, [(M, 10), (D, 2), (M, 10)], {9: "T" if ref[1411] != "T" else "G"})
    # N bases: in the read (no SNP), in the MD (reference N, no SNP; an insertion anchored on it keeps N)
    add("n1", 1600, [(M, 30)], {5: "N"})
    s = apply(ref, 1610, [(M, 10), (I, 1), (M, 10)])
    md = md_for(ref, 1610, [(M, 10), (I, 1), (M, 10)], s)
    reads.append(rd("n2", 0, 1610, [(M, 10), (I, 1), (M, 10)], s[:9] + ("A" if ref[1619] != "A" else "C") + s[10:],
                    md="9N10"))
    # no MD; unmapped but placed (with and without a CIGAR); duplicate and secondary flags
    add("nomd", 1650, [(M, 30)], {3: "A" if ref[1653] != "A" else "C"}, md=None)
    add("unm1", 1660, [], seq=apply(ref, 1660, [(M, 20)]), flag=4, md=None)
    reads.append(rd("unm2", 0, 1661, [(M, 20)], apply(ref, 1661, [(M, 20)], {2: "A" if ref[1663] != "A" else "C"}), ref=ref, flag=4))
    add("dup", 1662, [(M, 20)], {2: "A" if ref[1664] != "A" else "C"}, flag=1024)
    add("sec", 1663, [(M, 20)], {2: "A" if ref[1665] != "A" else "C"}, flag=256)
    # over-long indels at max_len 60: REF / ALT of 60 kept, 61 dropped
    add("dl59", 1700, [(M, 20), (D, 59), (M, 20)])
    add("dl60", 1701, [(M, 20), (D, 60), (M, 20)])
    add("il59", 1702, [(M, 20), (I, 59), (M, 20)])
    add("il60", 1703, [(M, 20), (I, 60), (M, 20)])
    # N operation and SEQ '*': coverage only
    add("skip", 1900, [(M, 10), (N, 50), (M, 10)], md="20")
    reads.append(rd("noseq", 0, 1910, [(M, 20)], "", md="20"))
    # MD running past / falling short of the CIGAR, and '^' runs of the wrong length
    for name, cig, md in (("past", [(M, 20)], "25"), ("short", [(M, 20)], "15"), ("dlong", [(M, 10), (D, 2), (M, 10)], None),
                          ("dshort", [(M, 10), (D, 3), (M, 10)], None), ("lower", [(M, 20)], "5a14")):
        s = apply(ref, 2000, cig)
        if md is None:
            md = "10^" + ref[2010:2010 + (3 if name == "dlong" else 2)] + "10"
        reads.append(rd(name, 0, 2000, cig, s, md=md, malformed=True))
    # filler coverage around 2000-2100 so the skipped reads' depth shows
    for k in range(4):
        add("f%d" % k, 1990 + k, [(M, 60)], {15: "A" if ref[1990 + k + 15] != "A" else "G"})
    reads.sort(key=lambda d: (d["tid"], d["pos"]))
    return [("chr1", L)], reads


def random_case(seed=5, n_reads=3000):
    rng = random.Random(seed)
    refs = [("chr1", 20000), ("chr2", 15000)]
    seqs = ["".join(rng.choice("ACGT") for _ in range(l)) for _, l in refs]
    hot = [sorted(rng.sample(range(100, l - 200), 60)) for _, l in refs]
    reads = []
    for i in range(n_reads):
        tid = 0 if rng.random() < 0.6 else 1
        ref = seqs[tid]
        pos = rng.randrange(0, refs[tid][1] - 200)
        cig, q = [], 0
        if rng.random() < 0.15:
            cig.append((S, rng.randint(1, 8)))
        left = 100
        while left > 0:
            m = min(left, rng.randint(10, 60))
            cig.append((M, m)); left -= m
            if left > 0 and rng.random() < 0.25:
                cig.append((I, rng.randint(1, 4)) if rng.random() < 0.5 else (D, rng.randint(1, 5)))
        if rng.random() < 0.15:
            cig.append((S, rng.randint(1, 8)))
        seq = list(apply(ref, pos, cig))
        # variants at hot positions (many reads share them), random errors elsewhere
        qi, r = 0, pos
        for op, l in cig:
            if op in (M, EQ, X):
                for k in range(l):
                    if (r + k in hot[tid] and rng.random() < 0.4) or rng.random() < 0.004:
                        seq[qi + k] = rng.choice("ACGT".replace(ref[r + k], ""))
                qi += l; r += l
            elif op in (I, S):
                qi += l
            elif op == D:
                r += l
        seq = "".join(seq)
        flag = rng.choice([0, 16, 0, 16, 1024]) if rng.random() < 0.9 else 256
        reads.append(rd("r%d" % i, tid, pos, cig, seq, ref=ref, flag=flag, md=md_for(ref, pos, cig, seq)
                        if rng.random() > 0.01 else None))
    reads.sort(key=lambda d: (d["tid"], d["pos"]))
    return refs, reads


def params(**kw):
    p = {"contigs": None, "keep_contig_chr": False, "chunk_size": 1000, "snp_min_freq": 0.01, "indel_min_freq": 0.01,
         "keep_multialleles": False, "max_len_indel_allele": 60}
    p.update(kw)
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    cg = load_reference(a.reference)
    tmp = os.path.join(a.out, ".tmp_gen")
    os.makedirs(tmp, exist_ok=True)
    refs, reads = edge_case()
    rrefs, rreads = random_case()
    nrefs = [("1", 3200)]
    cases = {
        "edge": (refs, reads, [("chunk1", params(chunk_size=1), None), ("chunk1_multi", params(chunk_size=1, keep_multialleles=True), None),
                               ("whole", params(snp_min_freq=0.075, indel_min_freq=0.02, keep_multialleles=True), None),
                               ("contigs", params(contigs="chr1:900:1750", chunk_size=1), None),
                               ("bed_nochr_keep", params(keep_contig_chr=True), "1\t950\t1520\n1\t1600\t2100\n"),
                               ("bed_chr", params(), "chr1\t950\t1520\n")]),
        "nochr": (nrefs, [dict(r) for r in reads], [("bed", params(chunk_size=1), "1\t990\t1010\n1\t1400\t3200\n")]),
        "random": (rrefs, rreads, [("cli", params(snp_min_freq=0.075, indel_min_freq=0.02, keep_multialleles=True), None),
                                   ("chunk5", params(snp_min_freq=0.075, indel_min_freq=0.02, keep_multialleles=True, chunk_size=5), None),
                                   ("default", params(chunk_size=7), None)]),
    }
    for name, (rf, rs, runs) in cases.items():
        out = {"references": rf, "reads": rs, "runs": []}
        for rname, p, bed in runs:
            res = run_case(cg, rf, rs, p, bed, tmp)
            out["runs"].append({"name": rname, "params": p, "bed": bed, **res})
            print(name, rname, "subregions", len(res["subregions"]), "candidates", len(res["tuples"]))
        if name == "edge":
            out["flag_table"] = flag_table(cg)
        with gzip.open(os.path.join(a.out, "candidates_%s.json.gz" % name), "wt") as f:
            json.dump(out, f, separators=(",", ":"))
    for f in os.listdir(tmp):
        os.remove(os.path.join(tmp, f))
    os.rmdir(tmp)


if __name__ == "__main__":
    main()

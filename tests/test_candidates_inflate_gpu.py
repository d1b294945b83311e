"""Candidate generation with the BGZF inflate, the record walk and the framing on the MI355X (``inflate_device="gpu"``):
the same candidates, tuples and counts as the host inflate path on every fixture, on a BAM whose records span BGZF blocks in
every way, and an error (not a signal, not a hang) on corrupt files."""
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

from dl4vc_amd import bamio, candidates as C
from dl4vc_amd.candgen import CandidateCounter, Stats
from dl4vc_amd.vcfpost import BGZF_BLOCK
from tests.candidates_fixture import NAMES, load, write_bam
from tests.test_candidates_host import AUX_KINDS, _bgzf, _blocks, _damaged

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_STATS = [n for n, t in Stats._fields_ if t is not Stats._fields_[-1][1]]


def _body(path):
    return [l.rstrip("\n") for l in open(path) if not l.startswith("#")]


@pytest.mark.parametrize("name", NAMES)
def test_generator_matches_reference_with_device_inflate(name, tmp_path):
    fx = load(name)
    bam = write_bam(fx, str(tmp_path / (name + ".bam")))
    for run in fx["runs"]:
        p = run["params"]
        bed = None
        if run["bed"] is not None:
            bed = str(tmp_path / "r.bed")
            open(bed, "w").write(run["bed"])
        out = str(tmp_path / ("%s.vcf" % run["name"]))
        try:
            stats = C.generate(bam, out, contigs=p["contigs"], bedfile=bed, keep_contig_chr=p["keep_contig_chr"],
                               chunk_size=p["chunk_size"], threads=4, snp_min_freq=p["snp_min_freq"],
                               indel_min_freq=p["indel_min_freq"], keep_multialleles=p["keep_multialleles"],
                               max_len_indel_allele=p["max_len_indel_allele"], inflate_device="gpu")
        except ValueError as e:                    # contigs the BAM does not have: the reference's fetch raises too
            assert run["bed"] is not None and not p["keep_contig_chr"], e
            continue
        assert _body(out) == run["lines"], run["name"]
        assert stats["reads_malformed"] == run["malformed_fetched"], (run["name"], stats)
        assert stats["inflate_records"] >= 0 and "inflate_ms" in stats


def _both(bam, subs, **kw):
    res = []
    for dev in (None, "gpu"):
        with CandidateCounter(bam, threads=4, inflate_device=dev, **kw) as cc:
            counted, stats = cc.run(subs)
        res.append((sorted(counted), {k: stats[k] for k in INT_STATS}, stats))
    return res


def test_tuples_and_stats_equal_the_host_path(tmp_path):
    fx = load("random")
    bam = write_bam(fx, str(tmp_path / "r.bam"))
    run = [r for r in fx["runs"] if r["name"] == "chunk5"][0]
    p = run["params"]
    subs = [tuple(s) for s in run["subregions"]]
    refs = [r[0] for r in fx["references"]]
    host, dev = _both(bam, [(refs.index(c), s, e) for c, s, e in subs], max_len_indel_allele=p["max_len_indel_allele"],
                      snp_min_freq=p["snp_min_freq"], indel_min_freq=p["indel_min_freq"])
    assert dev[0] == host[0]
    assert dev[1] == host[1] and host[1]["reads"] > 3000
    assert sorted(C.candidate_tuples(subs, dev[0], True)) == sorted(tuple(t) for t in run["tuples"])
    assert dev[2]["inflate_blocks"] > 0 and dev[2]["inflate_records"] > 0


# ---- records that span BGZF blocks, several device batches ------------------------------------------------------------------
CONTIG = 9000000


def _spanning_records():
    rng = np.random.default_rng(5)
    ref = rng.choice(np.frombuffer(b"ACGT", np.uint8), CONTIG)
    starts = np.sort(np.concatenate([rng.integers(a, a + 400000, 6700) for a in (100000, 4300000, 8500000)]))[:20000]
    recs = []
    long_at = 4500000
    for i, s in enumerate(starts.tolist()):
        if long_at is not None and s >= long_at:
            seq = ref[long_at:long_at + 50000].tobytes().decode()
            recs.append(bamio.pack_record(0, long_at, "long", 0, 60, [(bamio.CMATCH, 50000)], seq, aux=b"MDZ50000\x00"))
            long_at = None
        seq = ref[s:s + 150].copy()
        md = "150"
        if i % 3 == 0:                                   # a SNP at base 50 (a third of the reads: well above the frequency floor)
            seq[50] = b"ACGT"[(b"ACGT".index(bytes([seq[50]])) + 1) % 4]
            md = "50%s99" % chr(ref[s + 50])
        recs.append(bamio.pack_record(0, s, "r%d" % (i * 7919 % 100003), 16 if i & 1 else 0, 60, [(bamio.CMATCH, 150)],
                                      seq.tobytes().decode(), aux=b"MDZ" + md.encode() + b"\x00"))
    assert long_at is None
    return recs


def _straddles(path):
    """Record starts, from the file, whose 4-byte block_size field lies in two BGZF blocks."""
    sizes = [struct.unpack("<I", b[-4:])[0] for b in _blocks(path)]
    raw = b"".join(zlib.decompress(b[18:-8], -15) for b in _blocks(path))
    cuts = set(np.cumsum(sizes).tolist())
    o = 8 + struct.unpack_from("<i", raw, 4)[0]
    n_ref = struct.unpack_from("<i", raw, o)[0]
    o += 4
    for _ in range(n_ref):
        o += 8 + struct.unpack_from("<i", raw, o)[0]
    found, longest = 0, 0
    while o < len(raw):
        if any(o + k in cuts for k in (1, 2, 3)):
            found += 1
        n = struct.unpack_from("<i", raw, o)[0]
        longest = max(longest, n)
        o += 4 + n
    return found, longest


@pytest.fixture(scope="module")
def spanning(tmp_path_factory):
    d = tmp_path_factory.mktemp("span")
    recs = _spanning_records()
    refs = [("ctg", CONTIG)]
    base = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:ctg\tLN:%d\n" % CONTIG
    head = 12 + len(base) + 4 + 4 + 4                       # magic, l_text, text, n_ref, l_name, "ctg\0", l_ref
    offs = np.cumsum([0] + [len(r) for r in recs[:-1]])
    pad = next(p for p in range(5, 400) if ((head + p + offs) % BGZF_BLOCK > BGZF_BLOCK - 4).any())
    paths = {}
    for level in (0, 1, 6):
        path = str(d / ("span%d.bam" % level))
        with bamio.BamWriter(path, refs, header_text=base + "@CO\t" + "x" * (pad - 5) + "\n", level=level) as w:
            for r in recs:
                w.w.write(r)
        bamio.build_bai(path, path + ".bai")
        paths[level] = path
    return paths


@pytest.mark.parametrize("level", [0, 1, 6])
def test_spanning_records_and_batches(spanning, level):
    bam = spanning[level]
    found, longest = _straddles(bam)
    assert found >= 1 and longest > 65536
    subs = [("ctg", s, e) for _, s, e in C.split_subregions([("ctg", 0, CONTIG)], 1000 * 1000)]
    host, dev = _both(bam, [(0, s, e) for _, s, e in subs], snp_min_freq=0.075, indel_min_freq=0.02)
    assert host[1]["batches"] >= 3 and host[1]["reads"] >= 20001 and host[1]["candidates"] > 1000
    assert dev[0] == host[0]
    assert dev[1] == host[1]


# ---- corrupt files ----------------------------------------------------------------------------------------------------------
def _with_twin_index(tmp_path, kind):
    """The damaged BAM of test_candidates_host._damaged (or one CRC byte flipped) beside the index of its undamaged twin: the
    same bytes in the same blocks."""
    bam = _damaged(tmp_path, "l_seq_past_record" if kind == "crc_flipped" else kind)
    data = b"".join(zlib.decompress(b[18:-8], -15) for b in _blocks(str(tmp_path / "good.bam")))
    step = 30000 if kind == "truncated_bgzf" else 60000
    cuts = list(range(0, len(data), step)) + [len(data)]
    # (_damaged cuts a one-block file inside a block that starts at the first record; the CRC case keeps the header, which
    # cg_open reads on the host, in a block of its own and damages the block of the records)
    if kind == "crc_flipped" or (kind == "truncated_bgzf" and len(data) <= step):
        o = 8 + struct.unpack_from("<i", data, 4)[0]
        n_ref = struct.unpack_from("<i", data, o)[0]
        o += 4
        for _ in range(n_ref):
            o += 8 + struct.unpack_from("<i", data, o)[0]
        cuts = [0, o, len(data)]
    twin = str(tmp_path / "twin.bam")
    open(twin, "wb").write(b"".join(_bgzf(data[a:b]) for a, b in zip(cuts, cuts[1:])) + _bgzf(b""))
    if kind == "crc_flipped":
        raw = bytearray(open(twin, "rb").read())
        two = len(_blocks(twin)[0]) + len(_blocks(twin)[1])
        raw[two - 7] ^= 0x10                                  # a CRC byte of the second block's trailer
        bam = str(tmp_path / "crc_flipped.bam")
        open(bam, "wb").write(bytes(raw))
    bamio.build_bai(twin, bam + ".bai")
    return bam


REFUSED_RECORD = ["block_size_past_eof", "l_seq_past_record", "n_cigar_past_record"] + list(AUX_KINDS)


@pytest.mark.parametrize("kind", ["truncated_bgzf", "crc_flipped"] + REFUSED_RECORD)
def test_corrupt_bam_is_an_error_on_the_device_path(tmp_path, kind):
    """In a child process, so that an abort would show as a signal.  A record the framing refuses is refused with the host
    path's message on the same file: one table of texts, and the same virtual offset."""
    bam = _with_twin_index(tmp_path, kind)
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from dl4vc_amd.candgen import CandidateCounter\n"
            "def refusal(**kw):\n"
            "    try:\n"
            "        CandidateCounter(%r, threads=2, **kw).run([(0, 0, 3200)])\n"
            "    except RuntimeError as e:\n"
            "        return str(e)\n"
            "dev = refusal(inflate_device='gpu')\n"
            "if dev is None:\n"
            "    print('OK'); sys.exit(0)\n"
            "print('ERR', dev)\n"
            "if %r:\n"
            "    print('HOST', refusal())\n"
            "sys.exit(3)\n") % (ROOT, bam, kind in REFUSED_RECORD)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "corrupt BAM record" in r.stdout or "truncated" in r.stdout or "BGZF" in r.stdout, r.stdout
    if kind in REFUSED_RECORD:
        lines = r.stdout.splitlines()
        dev = [l[4:] for l in lines if l.startswith("ERR ")]
        host = [l[5:] for l in lines if l.startswith("HOST ")]
        assert len(dev) == 1 and dev == host and "(record at virtual offset " in dev[0], r.stdout
    if kind in AUX_KINDS:
        assert AUX_KINDS[kind] in r.stdout, r.stdout


def test_no_index_is_refused_with_the_reason(tmp_path):
    bam = write_bam(load("nochr"), str(tmp_path / "x.bam"), index=False)
    with pytest.raises(RuntimeError, match="needs the BAI index"):
        CandidateCounter(bam, inflate_device="gpu")
    with pytest.raises(RuntimeError, match="needs the BAI index"):
        C.generate(bam, str(tmp_path / "o.vcf"), inflate_device="gpu")


def test_cli_flag_writes_the_same_vcf(tmp_path):
    bam = write_bam(load("random"), str(tmp_path / "r.bam"))
    outs = []
    for extra in ([], ["--inflate-device", "gpu"]):
        out = str(tmp_path / ("o%d.vcf" % len(outs)))
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "candidate_generator.py"), "--input", bam, "--output", out,
                            "--snp_min_freq", "0.075", "--indel_min_freq", "0.02", "--keep_multialleles", "--chunk_size", "5"] + extra,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
        assert ('"inflate_records"' in r.stdout) == bool(extra)
        outs.append(open(out, "rb").read())
    assert outs[0] == outs[1] and outs[0].count(b"\n") > 20


def test_call_variants_sh_z(tmp_path):
    """call_variants.sh -z: candidates.vcf equals the run without -z (tests/test_candidates_gpu.py pins that one to the
    fixture's lines, so the fixture's lines are the comparison here) and the log shows the device inflate ran."""
    import torch
    from dl4vc_amd.config import DanConfig
    from oracle.dan_oracle import random_state_dict
    fx = load("random")
    bam = write_bam(fx, str(tmp_path / "r.bam"))
    rng = np.random.default_rng(3)
    fa = str(tmp_path / "ref.fa")
    with open(fa, "w") as f:
        for name, length in fx["references"]:
            s = "".join(rng.choice(list("ACGT"), length))
            f.write(">%s\n%s\n" % (name, "\n".join(s[i:i + 60] for i in range(0, length, 60))))
    sd = random_state_dict(DanConfig(), seed=14)
    ck = str(tmp_path / "ckpt.pth.tar")
    torch.save({"epoch": 1, "best_loss": 0.0, "optimizer": {}, "state_dict": {"module." + k: torch.from_numpy(v) for k, v in sd.items()}}, ck)
    out = tmp_path / "out"
    r = subprocess.run(["bash", os.path.join(ROOT, "call_variants.sh"), "-m", ck, "-o", str(out), "-i", bam, "-r", fa, "-p", "4", "-z"],
                       capture_output=True, text=True, timeout=600)
    log = (out / "candidate_generator.log").read_text() if (out / "candidate_generator.log").exists() else ""
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:], log[-1500:])
    cli = [run for run in fx["runs"] if run["name"] == "cli"][0]
    assert _body(str(out / "candidates.vcf")) == cli["lines"]
    assert '"inflate_records"' in log
    assert (out / "called_variants.vcf.gz").exists()

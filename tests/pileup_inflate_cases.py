"""Inputs for the GPU pileup encoder with the BAM inflated on the device (``inflate_device="gpu"``), shared by
tests/test_pileup_frame_host.py (the CPU twin, no GPU) and tests/test_pileup_inflate_gpu.py.  Plain module.

``grid(tmp, level)``: one BAM of ~3 800 records over two contigs ("chr1", and "2" without the prefix) that holds, on purpose:
a record whose 4-byte block_size lies across two BGZF blocks (the first read's name is padded until one does), a 70 000-base
record (longer than a block), a read with a 20-kb deletion that starts three 16-kb windows left of its location (it sits in a
parent bin), a 5 000-base read over two runs more than RUN_GAP apart, reads at the first and the last base of both contigs, a
stretch without reads, unmapped and placed-unmapped records, flag-masked reads and a site deeper than PG_MAX_TRACKS."""
import os
import struct
import zlib

import numpy as np

from dl4vc_amd import bamio
from dl4vc_amd.vcfpost import BGZF_BLOCK
from tests.pileup_cases import make_ref, read

W, MAX_READS = 16, 20                                   # window_size, max_reads of every grid encoder
LEN1, LEN2 = 300_000, 40_000
DEEP = 120_000                                          # the site over PG_MAX_TRACKS
OPTIONS = (W, MAX_READS, 10, 50, 0)


def _reads():
    r1, r2 = make_ref(LEN1, 301), make_ref(LEN2, 302)
    rs = []
    rng = np.random.default_rng(17)
    # the ends of both contigs
    for i in range(4):
        rs.append(read(r1, i, "40M", "a%d" % i, 16 * (i & 1), 20 + i))
        rs.append(read(r1, LEN1 - 40 - i, "40M", "z%d" % i, 16 * (i & 1), 20 + i))
        rs.append(read(r2, i, "40M", "b%d" % i, 0, 30, tid=1))
        rs.append(read(r2, LEN2 - 38 - i, "30M2I8M", "y%d" % i, 16, 30, tid=1))
    # a 20-kb deletion, from window 0 to window 3; a few plain reads at its far end
    rs.append(read(r1, 16_000, "7000M20000D7000M", "del20k", 0, 33))
    for i in range(6):
        rs.append(read(r1, 49_960 + 3 * i, "40M", "d%d" % i, 16 * (i & 1), 25))
    # 5 000 bases over two runs (locations 4 890 apart: more than RUN_GAP), with short reads at both
    rs.append(read(r1, 100_000, "5000M", "long5k", 16, 31))
    for i in range(5):
        rs.append(read(r1, 99_990 + 4 * i, "18M3I20M", "p%d" % i, 0, 22))
        rs.append(read(r1, 104_880 + 4 * i, "15M4D21M", "q%d" % i, 16, 24))
    # ~12x over 8 kb, every fifth read flag-masked, some placed-unmapped
    flags = [0, 16, 0, 16, bamio.FDUP, 0, 16, 0, 16, bamio.FSECONDARY, 0, 16, 0, 16, bamio.FQCFAIL]
    for i, p in enumerate(np.sort(rng.integers(110_000, 118_000, 1000)).tolist()):
        cigar = ["100M", "40M2I58M", "50M5D50M", "3S97M", "100M"][i % 5]
        rs.append(read(r1, p, cigar, "g%d" % i, flags[i % 15], 5 + i % 40))
        if i % 97 == 0:
            rs.append(bamio.BamRecord(0, p, 0, bamio.FUNMAP, "pu%d" % i, (), "ACGTACGTAC", np.full(10, 20, np.uint8)))
    # a site deeper than PG_MAX_TRACKS
    for i in range(1100):
        rs.append(read(r1, DEEP - 20 + i % 11, "40M", "t%d" % i, 16 * (i & 1), 30))
    # longer than a BGZF block
    rs.append(read(r1, 200_000, "70000M", "long70k", 0, 28))
    for i in range(8):
        rs.append(read(r1, 229_980 + 5 * i, "40M", "m%d" % i, 16 * (i & 1), 27))
    # the second contig: ~8x over 20 kb
    for i, p in enumerate(np.sort(rng.integers(5_000, 25_000, 1600)).tolist()):
        rs.append(read(r2, p, ["100M", "60M3D40M", "30M4I66M"][i % 3], "h%d" % i, 16 * (i % 3 == 1), 10 + i % 30, tid=1))
    rs.sort(key=lambda r: (r.tid, r.pos))
    for i in range(5):                                   # unmapped, at the end of the file
        rs.append(bamio.BamRecord(-1, -1, 0, bamio.FUNMAP, "un%d" % i, (), "ACGT" * 10, np.full(40, 11, np.uint8)))
    return [("chr1", r1), ("2", r2)], rs


def locations():
    """-> (contigs, positions): both spellings of both contigs, every feature of the grid, and a stretch without reads."""
    locs = [("chr1", 1), ("1", 2), ("chr1", LEN1), ("1", LEN1 - 20), ("2", 1), ("chr2", LEN2), ("2", LEN2 - 5),
            ("chr1", 49_990), ("chr1", 16_010), ("chr1", 30_000), ("chr1", 100_010), ("chr1", 104_900),
            ("chr1", 150_000), ("chr1", 160_000), ("chr1", DEEP), ("chr1", DEEP + 60), ("chr1", 230_000), ("chr1", 200_001),
            ("chr1", 269_999), ("chrX", 5)]
    locs += [("chr1", p) for p in range(110_050, 118_000, 173)]
    locs += [("2" if p % 2 else "chr2", p) for p in range(5_100, 25_000, 331)]
    return [c for c, _ in locs], [p for _, p in locs]


def _pack(r, name=None):
    return bamio.pack_record(r.tid, r.pos, name or r.name, r.flag, r.mapq, list(r.cigar), r.seq, r.qual.tolist())


_CACHE = {}


def _packed():
    if not _CACHE:
        refs, rs = _reads()
        recs = [_pack(r) for r in rs]
        base = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % (n, len(s)) for n, s in refs)
        head = 12 + len(base) + sum(4 + len(n) + 1 + 4 for n, _ in refs)
        offs = np.cumsum([0] + [len(r) for r in recs[:-1]])
        # pad the first read's name until some record's block_size field lies across a block boundary
        pad = next(p for p in range(0, 200) if ((head + p + offs[1:]) % BGZF_BLOCK > BGZF_BLOCK - 4).any())
        recs[0] = _pack(rs[0], rs[0].name + "x" * pad)
        _CACHE.update(refs=refs, recs=recs, base=base)
    return _CACHE["refs"], _CACHE["recs"], _CACHE["base"]


def write_fasta(path, refs):
    with open(path, "w") as f:
        for name, seq in refs:
            f.write(">%s\n" % name + "\n".join(seq[i:i + 70] for i in range(0, len(seq), 70)) + "\n")


def grid(tmp, level):
    """-> (bam, fasta); the BAI lies beside the BAM."""
    refs, recs, base = _packed()
    d = os.path.join(str(tmp), "grid%d" % level)
    os.makedirs(d, exist_ok=True)
    bam, fa = os.path.join(d, "grid.bam"), os.path.join(d, "ref.fa")
    write_fasta(fa, refs)
    with bamio.BamWriter(bam, [(n, len(s)) for n, s in refs], header_text=base, level=level) as w:
        for r in recs:
            w.w.write(r)
    bamio.build_bai(bam, bam + ".bai")
    return bam, fa


def blocks(path):
    raw = open(path, "rb").read()
    out, o = [], 0
    while o < len(raw):
        bsize = struct.unpack_from("<H", raw, o + 16)[0] + 1
        out.append(raw[o:o + bsize])
        o += bsize
    return out


def straddles(path):
    """-> (records whose block_size field lies in two BGZF blocks, the longest record, the number of blocks)."""
    bl = blocks(path)
    sizes = [struct.unpack("<I", b[-4:])[0] for b in bl]
    raw = b"".join(zlib.decompress(b[18:-8], -15) for b in bl)
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
    return found, longest, len(bl)


def windows():
    """The fetch windows [s0, stop) of the runs the grid's locations form (tid, s0, stop), as encode_batch cuts them
    (RUN_GAP 4096, RUN_SPAN 2^20), for the CPU twin."""
    contigs, pos = locations()
    tid = {"chr1": 0, "1": 0, "2": 1, "chr2": 1}
    es = sorted((tid[c], p, c) for c, p in zip(contigs, pos) if c in tid)
    out = []
    for t, p, c in es:
        s0, stop = max(p - (W + 2), 0), p + W + 3
        if out and out[-1][0] == t and out[-1][3] == c and s0 <= out[-1][2] + 4096 and stop - out[-1][1] <= (1 << 20):
            out[-1][2] = max(out[-1][2], stop)
        else:
            out.append([t, s0, stop, c])
    return [(t, a, b) for t, a, b, _ in out]


# ---- two runs whose byte ranges share a BGZF block without merging ------------------------------------------------------------
SHARED_LOCS = (["ctg", "ctg", "ctg"], [150, 39_990, 40_000])
SHARED_WINDOWS = [(0, 150 - (W + 2), 150 + W + 3), (0, 39_990 - (W + 2), 40_000 + W + 3)]


def shared_block(tmp):
    """-> (bam, fasta).  30 reads at 100, 5 at 20 000 that no location asks for, 600 at 39 000: the chunks of the first and
    the third 16-kb bin begin in the same BGZF block, are not adjacent (the second bin's records lie between them), and the
    third continues into the next block.  A call for locations in the first and the third bin has two byte ranges that touch
    one block."""
    ref = make_ref(60_000, 91)
    rs = [read(ref, 100 + i, "100M", "a%d" % i, 16 * (i & 1), 30) for i in range(30)]
    rs += [read(ref, 20_000 + i, "100M", "b%d" % i, 0, 30) for i in range(5)]
    rs += [read(ref, 39_000 + 2 * i, "100M", "c%d" % i, 16 * (i & 1), 20 + i % 20) for i in range(600)]
    d = os.path.join(str(tmp), "shared")
    os.makedirs(d, exist_ok=True)
    bam, fa = os.path.join(d, "shared.bam"), os.path.join(d, "ref.fa")
    write_fasta(fa, [("ctg", ref)])
    with bamio.BamWriter(bam, [("ctg", len(ref))]) as w:
        for r in rs:
            w.w.write(_pack(r))
    idx = bamio.build_bai(bam, bam + ".bai")
    (a0, a1), (c0, c1) = idx.bins[0][4681][0], idx.bins[0][4683][0]
    assert a0 >> 16 == c0 >> 16 and a1 < c0 and c1 >> 16 > c0 >> 16, "the fixture no longer shares a block between two ranges"
    return bam, fa


# ---- damaged inputs: the file of one contig below, damaged, beside the index of its undamaged twin --------------------------
DAMAGED = ["crc_flipped", "truncated_bgzf", "block_size_past_eof", "l_seq_past_record", "n_cigar_past_record", "cigar_600m",
           "aux_string_without_nul", "aux_value_type"]
# what the error says: (the host path, the device path and its CPU twin).  A cut block is met by the host's block reader and by
# the device path's range planner (the index points past the end of the cut file), which have their own words for it.
EXPECT = {"crc_flipped": ("BGZF block fails its CRC / size check", "BGZF block fails its CRC / size check (CRC mismatch, block at file offset"),
          "truncated_bgzf": ("truncated BGZF block", "BGZF: truncated file (the index points at offset"),
          "block_size_past_eof": ("truncated BAM record (record at virtual offset", "truncated BAM record (record at virtual offset"),
          "l_seq_past_record": ("corrupt BAM record (l_seq exceeds the record) (record at virtual offset",) * 2,
          "n_cigar_past_record": ("corrupt BAM record (n_cigar_op exceeds the record) (record at virtual offset",) * 2,
          "cigar_600m": ("corrupt BAM record (CIGAR reference length) (record at virtual offset",) * 2,
          "aux_string_without_nul": ("corrupt BAM record (aux string without its NUL) (record at virtual offset",) * 2,
          "aux_value_type": ("corrupt BAM record (aux value type) (record at virtual offset",) * 2}
DAMAGED_WINDOW = (0, 0, 3200)


def _bgzf(data):
    c = zlib.compressobj(0, zlib.DEFLATED, -15)           # stored: the damaged file's blocks lie where its twin's do
    body = c.compress(data) + c.flush()
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(body) + 25) + body +
            struct.pack("<II", zlib.crc32(data) & 0xffffffff, len(data)))


def damaged(tmp, kind):
    """-> (bam, bai, fasta).  The header is a block of its own (the encoder reads it on the host when it opens the file); the
    records follow in blocks of 20 000 bytes; the third record is the damaged one (for the aux kinds it carries an MD:Z tag, in
    the twin as well)."""
    ref = make_ref(4000, 77)
    rs = [read(ref, 20 + 7 * i, "20M20M20M", "k%d" % i, 16 * (i & 1), 30) for i in range(500)]
    recs = [_pack(r) for r in rs]
    if kind.startswith("aux_"):
        r = rs[2]
        recs[2] = bamio.pack_record(r.tid, r.pos, r.name, r.flag, r.mapq, list(r.cigar), r.seq, r.qual.tolist(), aux=b"NMC\x00MDZ60\x00")
    text = "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:ctg\tLN:4000\n".encode()
    head = bamio.BAM_MAGIC + struct.pack("<i", len(text)) + text + struct.pack("<i", 1) + struct.pack("<i", 4) + b"ctg\x00" + struct.pack("<i", 4000)
    d = os.path.join(str(tmp), kind)
    os.makedirs(d, exist_ok=True)

    def write(path, recs, cut=None, flip=False):
        body = b"".join(recs)
        bl = [_bgzf(head)] + [_bgzf(body[i:i + 20000]) for i in range(0, len(body), 20000)] + [_bgzf(b"")]
        if flip:
            b = bytearray(bl[2])
            b[-7] ^= 0x10                                    # a CRC byte of the second record block's trailer
            bl[2] = bytes(b)
        blob = b"".join(bl)
        if cut:
            blob = b"".join(bl[:2]) + bl[2][:len(bl[2]) // 2]
        open(path, "wb").write(blob)

    twin, bam, fa = os.path.join(d, "twin.bam"), os.path.join(d, kind + ".bam"), os.path.join(d, "ref.fa")
    write(twin, recs)
    bad = bytearray(recs[2])
    if kind == "block_size_past_eof":
        bad[0:4] = struct.pack("<i", 1 << 20)
    elif kind == "l_seq_past_record":
        bad[20:24] = struct.pack("<i", 5000)
    elif kind == "n_cigar_past_record":
        bad[16:18] = struct.pack("<H", 4000)
    elif kind == "cigar_600m":                               # 600 000 000 M, as three operations of 200 000 000 M (28 bits each)
        o = 4 + 32 + bad[12]
        bad[o:o + 12] = struct.pack("<I", (200_000_000 << 4) | bamio.CMATCH) * 3
    elif kind == "aux_string_without_nul":                   # the MD terminator, the record's last byte
        bad[-1] = ord("A")
    elif kind == "aux_value_type":
        bad[-4] = ord("x")                                   # MD:Z -> MD:x
    recs2 = list(recs)
    recs2[2] = bytes(bad)
    write(bam, recs2, cut=kind == "truncated_bgzf", flip=kind == "crc_flipped")
    bamio.build_bai(twin, bam + ".bai")
    write_fasta(fa, [("ctg", ref)])
    return bam, bam + ".bai", fa

"""The case grid of the BGZF inflate tests (host: test_bgzf_inflate_host.py, GPU: test_bgzf_inflate_gpu.py).

Valid cases are raw DEFLATE bodies from Python's zlib (every level / strategy that changes the block types it emits) plus two
streams assembled by hand for what zlib never emits and libdeflate does (a distance of 32 768, 15-bit codes); Python's zlib is
the judge of each: ``check_grid()`` inflates every valid body with it and requires it to refuse every damaged stream.  Each
case is wrapped as one BGZF block the way ``vcfpost._bgzf_block`` does.

A damaged case names the statuses its damage may end in and ``legit``, an upper bound of the bytes a decoder may have
produced before it met the damage; its slot beyond that must stay untouched."""
from __future__ import annotations

import functools
import struct
import zlib
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from dl4vc_amd import candgen

HEADER = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00"
FILL = 0xAB

# include/dl4vc_bgzf.h
OK, BAD_BLOCK_TYPE, BAD_STORED_LEN, BAD_CODE_LENGTHS, BAD_SYMBOL, DISTANCE_BEFORE_START, OUTPUT_EXCEEDS_ISIZE, \
    OUTPUT_SHORT_OF_ISIZE, INPUT_EXHAUSTED, TRAILING_INPUT, CRC_MISMATCH, BAD_HEADER, BAD_SLOT = range(13)
STREAM_DAMAGE = frozenset(range(BAD_BLOCK_TYPE, TRAILING_INPUT + 1))


class Case(NamedTuple):
    name: str
    block: bytes                   # one whole BGZF block
    data: Optional[bytes]          # what it inflates to (valid cases)
    isize: int                     # its ISIZE field: the size of its slot
    expect: frozenset = frozenset()  # damaged cases: the statuses the damage may end in
    legit: int = 0                 # damaged cases: bytes that may have been produced before the damage


def wrap(body: bytes, data: bytes, isize: Optional[int] = None, crc: Optional[int] = None) -> bytes:
    bsize = len(body) + 25
    assert bsize < 65536, bsize
    return (HEADER + struct.pack("<H", bsize) + body +
            struct.pack("<II", (zlib.crc32(data) if crc is None else crc) & 0xffffffff, len(data) if isize is None else isize))


def deflate(data: bytes, level: int = 6, strategy: int = zlib.Z_DEFAULT_STRATEGY) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return c.compress(data) + c.flush()


class BitWriter:
    """DEFLATE bit order: fields from the least significant bit, Huffman codes most significant bit first."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, value: int, n: int) -> None:
        self.acc |= (value & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xff)
            self.acc >>= 8
            self.n -= 8

    def code(self, code: int, n: int) -> None:
        for i in range(n - 1, -1, -1):
            self.bits((code >> i) & 1, 1)

    def done(self) -> bytes:
        if self.n:
            self.out.append(self.acc & 0xff)
            self.acc = self.n = 0
        return bytes(self.out)


def fixed_code(sym: int) -> Tuple[int, int]:
    if sym < 144:
        return 0x30 + sym, 8
    if sym < 256:
        return 0x190 + sym - 144, 9
    if sym < 280:
        return sym - 256, 7
    return 0xc0 + sym - 280, 8


def canonical(lens: Sequence[int]) -> List[int]:
    code, codes = 0, [0] * len(lens)
    for n in range(1, 16):
        for s, l in enumerate(lens):
            if l == n:
                codes[s] = code
                code += 1
        code <<= 1
    return codes


def bam_like(n: int, seed: int) -> bytes:
    rng = np.random.default_rng(seed)
    out = bytearray()
    pos = 10000
    i = 0
    while len(out) < n:
        pos += int(rng.integers(0, 40))
        name = b"read%07d\0" % i
        seq = rng.integers(0, 4, 75, dtype=np.uint8)
        seq = ((1 << seq) << 4 | (1 << rng.integers(0, 4, 75, dtype=np.uint8))).astype(np.uint8).tobytes()
        qual = rng.integers(28, 41, 150, dtype=np.uint8).tobytes()
        rec = struct.pack("<iiBBHHHiiii", 0, pos, len(name), 60, 4681, 1, 99, 150, 0, pos + 200, 350) + name + \
            struct.pack("<I", 150 << 4) + seq + qual + b"MDZ150\0NMC\0"
        out += struct.pack("<i", len(rec)) + rec
        i += 1
    return bytes(out[:n])


def far_match_stream() -> Tuple[bytes, bytes]:
    """One fixed-Huffman block: 32 768 literals, then a match of length 258 at distance 32 768."""
    lit = np.random.default_rng(7).integers(0, 256, 32768, dtype=np.uint8).tobytes()
    w = BitWriter()
    w.bits(1, 1); w.bits(1, 2)
    for v in lit:
        w.code(*fixed_code(v))
    w.code(*fixed_code(285))              # length 258, no extra bits
    w.code(29, 5); w.bits(32768 - 24577, 13)
    w.code(*fixed_code(256))
    return w.done(), lit + lit[:258]


def long_code_stream() -> Tuple[bytes, bytes]:
    """One dynamic block whose literal/length code has the lengths 1, 2, ..., 14, 15, 15; both 15-bit codes are used, and
    one match (length 3, distance 1) through a distance code of a single 1-bit code."""
    syms = [ord("a") + i for i in range(14)] + [256, 257]        # ascending, so lengths 1.. go to 'a'.. and 15, 15 to 256, 257
    lens = [0] * 258
    for s, l in zip(syms, list(range(1, 15)) + [15, 15]):
        lens[s] = l
    codes = canonical(lens)
    cl_lens = [4] * 13 + [5] * 6                                  # the code-length code: 13 / 16 + 6 / 32 = 1
    cl_codes = canonical(cl_lens)
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    w = BitWriter()
    w.bits(1, 1); w.bits(2, 2)
    w.bits(258 - 257, 5); w.bits(0, 5); w.bits(19 - 4, 4)
    for s in order:
        w.bits(cl_lens[s], 3)
    for l in lens + [1]:                                          # 258 literal/length lengths, one distance length
        w.code(cl_codes[l], cl_lens[l])
    text = bytes(ord("a") + (i * 7 + i // 5) % 14 for i in range(400))
    out = bytearray()
    for v in text:
        w.code(codes[v], lens[v]); out.append(v)
    w.code(codes[257], 15); w.code(0, 1); out += bytes([out[-1]]) * 3      # the first 15-bit code: a match
    for v in text[:50]:
        w.code(codes[v], lens[v]); out.append(v)
    w.code(codes[256], 15)                                        # the second: end of block
    return w.done(), bytes(out)


@functools.lru_cache(maxsize=None)
def valid_cases() -> Tuple[Case, ...]:
    rng = np.random.default_rng(11)
    cases: List[Tuple[str, bytes, bytes]] = []

    def add(name, data, body):
        cases.append((name, data, body))

    add("eof", b"", deflate(b""))
    add("one_byte", b"Q", deflate(b"Q"))
    bam = bam_like(0xff00, 3)
    for level in (1, 6, 9):
        add("bam_level%d" % level, bam, deflate(bam, level))
    add("level0", bam[:0xff00 - 10], deflate(bam[:0xff00 - 10], 0))
    # (65 536 incompressible bytes cannot be one BGZF block: stored blocks add 5 bytes each and the whole block, header and
    # trailer included, holds 65 536 at most; zeros_65536 below is the case with ISIZE at the format's limit)
    rnd = rng.integers(0, 256, 65480, dtype=np.uint8).tobytes()
    add("random_65480", rnd, deflate(rnd, 6))
    add("fixed_4000", bam[:4000], deflate(bam[:4000], 6, zlib.Z_FIXED))
    add("huffman_only", bam, deflate(bam, 6, zlib.Z_HUFFMAN_ONLY))
    runs = b"".join(bytes([int(v)]) * int(n) for v, n in zip(rng.integers(0, 256, 200), rng.integers(1, 600, 200)))[:60000]
    add("rle_runs", runs, deflate(runs, 6, zlib.Z_RLE))
    add("zeros_65536", bytes(65536), deflate(bytes(65536), 9))
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 8)
    body = b""
    for k, i in enumerate(range(0, 20000, 777)):
        body += c.compress(bam[i:min(i + 777, 20000)]) + c.flush(zlib.Z_SYNC_FLUSH if k % 2 == 0 else zlib.Z_FULL_FLUSH)
    add("flushed_777", bam[:20000], body + c.flush())
    body, data = far_match_stream()
    add("hand_far_match", data, body)
    body, data = long_code_stream()
    add("hand_15_bit_codes", data, body)
    return tuple(Case(n, wrap(b, d), d, len(d)) for n, d, b in cases)


@functools.lru_cache(maxsize=None)
def damaged_cases() -> Tuple[Case, ...]:
    bam = bam_like(30000, 5)
    good = deflate(bam, 6)
    out: List[Case] = []

    def add(name, body, isize, expect, legit, data=bam, crc=None):
        out.append(Case(name, wrap(body, data, isize, crc), None, isize, frozenset(expect), legit))

    add("btype3", b"\x07\x00", 10, {BAD_BLOCK_TYPE}, 0)
    add("stored_nlen", b"\x01\x05\x00\x00\x00hello", 5, {BAD_STORED_LEN}, 0)
    add("cut_bsize", good[:-30], len(bam), {INPUT_EXHAUSTED}, len(bam))
    add("cut_zeroed", good[:-20] + bytes(20), len(bam), STREAM_DAMAGE, len(bam))
    w = BitWriter()
    w.bits(1, 1); w.bits(2, 2); w.bits(0, 5); w.bits(0, 5); w.bits(15, 4)
    for _ in range(19):
        w.bits(1, 3)                       # nineteen codes of one bit
    w.bits(0, 32)
    add("oversubscribed", w.done(), 100, {BAD_CODE_LENGTHS}, 0)
    w = BitWriter()
    w.bits(1, 1); w.bits(1, 2)
    for v in b"abcdefgh":
        w.code(*fixed_code(v))
    w.code(*fixed_code(286)); w.code(0, 5); w.code(*fixed_code(256))
    add("symbol_286", w.done(), 100, {BAD_SYMBOL}, 8)
    w = BitWriter()
    w.bits(1, 1); w.bits(1, 2)
    for v in b"abc":
        w.code(*fixed_code(v))
    w.code(*fixed_code(257)); w.code(3, 5)  # length 3 at distance 4, three bytes in
    w.code(*fixed_code(256))
    add("distance_before_start", w.done(), 100, {DISTANCE_BEFORE_START}, 3)
    add("isize_minus_1", good, len(bam) - 1, {OUTPUT_EXCEEDS_ISIZE}, len(bam) - 1)
    add("isize_plus_1", good, len(bam) + 1, {OUTPUT_SHORT_OF_ISIZE}, len(bam))
    add("crc_flipped", good, len(bam), {CRC_MISMATCH}, len(bam), crc=zlib.crc32(bam) ^ 0x00010000)
    add("trailing_garbage", good + b"\x5a\x00\x17", len(bam), {TRAILING_INPUT}, len(bam))
    return tuple(out)


def body_of(block: bytes) -> bytes:
    return block[18:-8]


def check_grid() -> None:
    """Python's zlib as the judge: every valid body inflates to its data, every stream damage is refused."""
    for c in valid_cases():
        assert zlib.decompress(body_of(c.block), -15) == c.data, c.name
        crc, isize = struct.unpack("<II", c.block[-8:])
        assert isize == len(c.data) and crc == zlib.crc32(c.data), c.name
    for c in damaged_cases():
        body = body_of(c.block)
        crc, isize = struct.unpack("<II", c.block[-8:])
        if c.expect == {CRC_MISMATCH}:
            assert zlib.crc32(zlib.decompress(body, -15)) != crc, c.name
        elif c.expect <= {OUTPUT_EXCEEDS_ISIZE, OUTPUT_SHORT_OF_ISIZE}:
            assert len(zlib.decompress(body, -15)) != isize, c.name
        elif c.expect == {TRAILING_INPUT}:
            d = zlib.decompressobj(-15)
            d.decompress(body)
            assert d.eof and d.unused_data, c.name            # (zlib.decompress itself ignores what follows the stream)
        else:
            try:
                zlib.decompress(body, -15)
            except zlib.error:
                continue
            raise AssertionError("zlib accepts the damaged case %s" % c.name)


def layout(cases: Sequence[Case], gap: int = 5, order: Optional[Sequence[int]] = None):
    """The call's arrays: blocks back to back, slots in ``order`` (default: as given) with ``gap`` bytes between them."""
    blob = b"".join(c.block for c in cases)
    block_off = np.cumsum([0] + [len(c.block) for c in cases[:-1]]).astype(np.uint64)
    out_off = np.zeros(len(cases), np.uint64)
    at = gap
    for i in (range(len(cases)) if order is None else order):
        out_off[i] = at
        at += cases[i].isize + gap
    return blob, block_off, out_off, at


def run(cases: Sequence[Case], device: Optional[int], gap: int = 5, order: Optional[Sequence[int]] = None):
    blob, block_off, out_off, cap = layout(cases, gap, order)
    out = np.full(cap, FILL, np.uint8)
    status = candgen.inflate_blocks(blob, block_off, out, out_off, device=device)
    return out, out_off, status


def assert_outside_untouched(cases: Sequence[Case], out: np.ndarray, out_off: np.ndarray) -> None:
    mask = np.ones(len(out), bool)
    for c, o in zip(cases, out_off):
        mask[int(o):int(o) + c.isize] = False
    assert (out[mask] == FILL).all()


def assert_valid(cases: Sequence[Case], out: np.ndarray, out_off: np.ndarray, status: Sequence[int]) -> None:
    for c, o, st in zip(cases, out_off, status):
        assert st == OK, (c.name, st)
        assert out[int(o):int(o) + c.isize].tobytes() == c.data, c.name
    assert_outside_untouched(cases, out, out_off)


def check_damaged(bad: Case, device: Optional[int]) -> None:
    """The damaged block between two good ones in one call."""
    good = valid_cases()
    trio = [good[3], bad, good[7]]
    out, out_off, status = run(trio, device)
    assert status[1] != OK and status[1] in bad.expect, (bad.name, status[1], sorted(bad.expect))
    for k in (0, 2):
        assert status[k] == OK, (bad.name, k, status[k])
        assert out[int(out_off[k]):int(out_off[k]) + trio[k].isize].tobytes() == trio[k].data, (bad.name, k)
    o = int(out_off[1])
    assert (out[o + min(bad.legit, bad.isize):o + bad.isize] == FILL).all(), bad.name
    assert_outside_untouched(trio, out, out_off)

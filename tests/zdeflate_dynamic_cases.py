"""Cases of the zlib compressor's dynamic mode (csrc/zdeflate.h, ``ZD_DYNAMIC``), shared by tests/test_zdeflate_dynamic_host.py
(CPU) and tests/test_compress_dynamic_gpu.py: contents at which the code construction takes another path -- a literal code
deeper than 15 bits without the limit, a segment without a single match, contents that fixed codes hold as well -- with the
tools to say so: the parse of a segment in Python (its histograms) and a ``heapq`` Huffman code (its cost and depth)."""
import heapq
import struct
import zlib

import numpy as np

from tests import zdeflate_cases as ZC          # noqa: F401  (the grid, for the modules that import this one)

SEGMENT = 16384


def fibonacci_bytes(seed=11):
    """Byte value k occurs F(k + 1) times -- 1, 1, 2, 3, ... 1 597, 4 180 bytes -- in an order shuffled with a fixed seed."""
    fib = [1, 1]
    while fib[-1] < 1597:
        fib.append(fib[-1] + fib[-2])
    data = np.concatenate([np.full(f, k, np.uint8) for k, f in enumerate(fib)])
    np.random.default_rng(seed).shuffle(data)
    return data.tobytes()


def fibonacci_run_bytes(seed=11):
    """4 179 runs of one byte value, 0 and 1 in turn, each a literal and one match at distance 1; the matches' lengths are drawn so
    that the 16 length symbols 258..273 occur 1 597, 987, ... 3, 2, 1 times, shuffled with a fixed seed.  With the end-of-block
    symbol's 1 that is a Fibonacci chain in the literal / length alphabet which the parse leaves as it is: 27 879 bytes, one
    segment of 32 768."""
    fib = [1, 2]
    while fib[-1] < 1597:
        fib.append(fib[-1] + fib[-2])
    lengths = [4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35][::-1]        # one length of each symbol; the rarest the longest
    runs = np.concatenate([np.full(f, n) for f, n in zip(fib, lengths)])
    np.random.default_rng(seed).shuffle(runs)
    return b"".join(bytes([k % 2]) * (int(n) + 1) for k, n in enumerate(runs))


def de_bruijn_bytes(k=3, n=4):
    """Every n-gram over k byte values exactly once: k^n + n - 1 = 84 bytes without a repeated 4-gram, so without a match."""
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    s = seq + seq[:n - 1]
    assert len(s) == k ** n + n - 1 and len({tuple(s[i:i + n]) for i in range(len(s) - n + 1)}) == k ** n
    return bytes(65 + v for v in s)


def permutation_bytes(seed=4):
    """Every byte value once: 256 literals of one count, which fixed codes hold in fewer bits than a dynamic header costs."""
    return np.random.default_rng(seed).permutation(256).astype(np.uint8).tobytes()


def special_cases():
    """-> [(name, segment size, bytes)]: each is one segment."""
    return [("fibonacci", SEGMENT, fibonacci_bytes()), ("fibonacci runs", 32768, fibonacci_run_bytes()),
            ("de bruijn", SEGMENT, de_bruijn_bytes()), ("permutation", SEGMENT, permutation_bytes())]


def _length_symbol(n):
    l = n - 3
    if n == 258:
        return 285, 0
    if l < 8:
        return 257 + l, 0
    e = l.bit_length() - 3
    return 261 + 4 * e + ((l >> e) & 3), e


def _dist_symbol(dist):
    d = dist - 1
    if d < 4:
        return d, 0
    e = d.bit_length() - 2
    return 2 * e + 2 + ((d >> e) & 1), e


def parse_histograms(data):
    """The compressor's parse of one segment (greedy, one candidate per position from a 256-entry hash of 4 bytes, entered at
    every literal, match start and match end) -> (literal / length counts [286] with the end-of-block symbol, distance counts
    [30], extra bits)."""
    n, head = len(data), [0] * 256
    ll, dd, extra, i = [0] * 286, [0] * 30, 0, 0
    h4 = lambda p: ((struct.unpack_from("<I", data, p)[0] * 2654435761) & 0xffffffff) >> 24       # noqa: E731
    while i < n:
        mlen = 0
        if i + 4 <= n:
            h = h4(i)
            cand, head[h] = head[h], i + 1
            if cand:
                c, l, maxl = cand - 1, 0, min(n - i, 258)
                while l < maxl and data[c + l] == data[i + l]:
                    l += 1
                if l >= 4:
                    mlen, dist = l, i - c
        if mlen:
            s, e = _length_symbol(mlen)
            t, f = _dist_symbol(dist)
            ll[s] += 1
            dd[t] += 1
            extra += e + f
            i += mlen
            if i + 3 <= n:
                head[h4(i - 1)] = i
        else:
            ll[data[i]] += 1
            i += 1
    ll[256] += 1
    return ll, dd, extra


def fixed_segment_bytes(data):
    """Size of ``data`` as one last segment in fixed codes, from the histograms: what pins the Python parse to the compressor's."""
    ll, dd, extra = parse_histograms(data)
    bits = 3 + extra + 5 * sum(dd) + sum(c * (8 if s < 144 else 9 if s < 256 else 7 if s < 280 else 8) for s, c in enumerate(ll))
    return (bits + 7) // 8


def huffman(freq):
    """``heapq`` Huffman over the used symbols -> (cost = sum of count x length, depth); on equal weights the shallower tree is
    joined first, which gives the least depth an optimal code can have."""
    heap = [(f, 0, s) for s, f in enumerate(freq) if f]
    if len(heap) < 2:
        return sum(f for f, _d, _s in heap), 1
    heapq.heapify(heap)
    cost, tick = 0, len(freq)
    while len(heap) > 1:
        f1, d1, _ = heapq.heappop(heap)
        f2, d2, _ = heapq.heappop(heap)
        cost += f1 + f2
        heapq.heappush(heap, (f1 + f2, max(d1, d2) + 1, tick))
        tick += 1
    return cost, heap[0][1]


def bgzf_block(data, stream):
    """The zlib stream of ``data`` (at most 65 536 bytes) as one BGZF block: its DEFLATE blocks between the gzip header with the
    BC field and CRC-32 | ISIZE."""
    body = stream[2:-4]
    bsize = 18 + len(body) + 8
    assert bsize <= 65536 and len(data) <= 65536
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", bsize - 1) + body +
            struct.pack("<II", zlib.crc32(data), len(data)))

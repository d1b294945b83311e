"""Fixtures of the compact record format's tests (tests/test_train_cache_compact_host.py on the CPU,
tests/test_train_cache_compact_gpu.py on the GPU): hand-made records around the edges of a row's span as three plane arrays
``[n][S][W]`` at any shape, and the numpy statements of the format of dl4vc_amd/csrc/store_host.h -- a record's spans, its span
in a slab and its bytes."""
import numpy as np

from dl4vc_amd.hdf5_schema import PLANE_FIELDS, record_dtype

SHAPES = [(5, 7), (3, 16), (200, 201)]          # (S, W): rowtab, ts and q start at every alignment; the production planes
# edge_planes(): what each record is there for, and the format it must come out in (1 compact, 0 rows: it fell back)
EDGES = (("kept = 0", 1), ("row 0: one byte at column 0", 1), ("row 1: one byte at column W - 1, row 0 all zero", 1),
         ("one byte in the quality plane only", 1), ("one byte in the strand plane only", 1), ("an all-zero row between two used rows", 1),
         ("zero cells inside a span", 1), ("a row that spans all W columns", 1), ("token 15 with strand 15", 1), ("token 16", 0),
         ("strand 16", 0), ("every row used, quality bytes up to 255", 1), ("the last stored row only", 1), ("dense, one token of 200", 0))
N_EDGES = len(EDGES)


def edge_planes(S, W, seed=0):
    """-> [reads, qual, strand], each ``[N_EDGES][S][W]`` uint8 (S >= 3, W >= 3)."""
    rng = np.random.default_rng(100 * S + W + seed)
    a, q, b = (np.zeros((N_EDGES, S, W), np.uint8) for _ in range(3))
    a[1, 0, 0] = 3
    a[2, 1, W - 1] = 4
    q[3, 0, W // 2] = 40
    b[4, S // 2, 1] = 2
    lo, hi = 1, max(2, W - 2)
    for p, top in ((a, 9), (q, 41), (b, 3)):
        p[5, 0, lo:hi] = rng.integers(1, top, hi - lo)
        p[5, 2, :hi] = rng.integers(1, top, hi)
    a[6, 0, 0], q[6, 0, W - 1] = 5, 17                                   # the span is the whole row, all zero between its ends
    a[6, 1, 1], b[6, 1, W - 2] = 1, 1
    for p, top in ((a, 9), (q, 41), (b, 3)):
        p[7, :2] = rng.integers(1, top, (2, W))
    a[8, 0, 1:3], b[8, 0, 1:3], q[8, 0, 1:3] = 15, 15, 255
    a[9, 0, 1], a[9, 1, :] = 16, 7
    b[10, 1, W - 1], a[10, 0, :2] = 16, 2
    for r in range(S):                                                   # a span of its own in every row
        c0 = int(rng.integers(0, W - 1))
        n = int(rng.integers(1, W - c0 + 1))
        a[11, r, c0:c0 + n], b[11, r, c0:c0 + n] = rng.integers(0, 16, n), rng.integers(0, 16, n)
        q[11, r, c0:c0 + n] = rng.integers(0, 256, n)
        a[11, r, c0], q[11, r, c0 + n - 1] = 1, 9                       # (the ends of the span are not zero)
    q[12, S - 1, W // 3] = 1
    for p in (a, q, b):
        p[13] = rng.integers(0, 5, (S, W)) * rng.integers(1, 4, (S, W))
    a[13, S - 1, 0] = 200
    return [a, q, b]


def edge_records(S=20, W=201):
    """The same records in the candidate file's layout (``record_dtype``: an odd record size, planes at every alignment)."""
    planes = edge_planes(S, W)
    recs = np.zeros(N_EDGES, record_dtype(S, W))
    for f, p in zip(PLANE_FIELDS, planes):
        recs[f] = p
    kept = spans_definition(planes)[0]
    recs["num_reads"] = kept.reshape(recs["num_reads"].shape)
    return recs


def record_planes(recs):
    return [np.ascontiguousarray(recs[f]) for f in PLANE_FIELDS]


def spans_definition(planes):
    """-> (kept [n], cells [n], mergeable [n], rowspans [n][S] = c0 | n << 8): per row the smallest column range that contains every
    non-zero byte of the three planes (0, 0 for a row without one); kept = 1 + the last row with one; cells = the sum of n;
    mergeable = no byte >= 16 in the reads or strand plane."""
    a, q, b = planes
    n_rec, S, W = a.shape
    nz = (a | q | b) != 0
    used = nz.any(axis=2)
    first = np.argmax(nz, axis=2)
    last = W - 1 - np.argmax(nz[:, :, ::-1], axis=2)
    n = np.where(used, last - first + 1, 0)
    c0 = np.where(used, first, 0)
    kept = np.where(used.any(axis=1), S - np.argmax(used[:, ::-1], axis=1), 0).astype(np.int32)
    mergeable = ((a < 16).all(axis=(1, 2)) & (b < 16).all(axis=(1, 2))).astype(np.int32)
    return kept, n.sum(axis=1).astype(np.int32), mergeable, (c0 | n << 8).astype(np.uint16)


def pad16(x):
    return (np.asarray(x, np.int64) + 15) & ~np.int64(15)


def compact_span(kept, cells):
    kept, cells = np.asarray(kept, np.int64), np.asarray(cells, np.int64)
    return np.where(kept > 0, pad16(4 * (kept + 1) + 2 * cells), 0)


def rows_span(kept, W):
    return pad16(3 * np.asarray(kept, np.int64) * W)


def format_spans(planes, record_format="compact"):
    """-> (format [n], span [n]) of the records in a store of ``record_format``: a record that is not mergeable keeps the rows layout."""
    kept, cells, mergeable, _ = spans_definition(planes)
    fmt = mergeable if record_format == "compact" else np.zeros(len(kept), np.int32)
    return fmt, np.where(fmt == 1, compact_span(kept, cells), rows_span(kept, planes[0].shape[2]))


def stored_bytes_definition(planes, i, fmt):
    """The bytes of record ``i``: rowtab[kept + 1] (off | c0 << 24, little-endian) | ts | q | zeros, or the rows layout."""
    a, q, b = (p[i] for p in planes)
    kept, cells, _m, rowspans = (x[0] for x in spans_definition([p[i:i + 1] for p in planes]))
    W = a.shape[1]
    if fmt == 0:
        body = b"".join(np.ascontiguousarray(p[:kept]).tobytes() for p in (a, q, b))
        return np.frombuffer(body + bytes(int(rows_span(kept, W)) - len(body)), np.uint8)
    if kept == 0:
        return np.zeros(0, np.uint8)
    c0, n = (rowspans[:kept] & 255).astype(np.int64), (rowspans[:kept] >> 8).astype(np.int64)
    off = np.concatenate(([0], np.cumsum(n)))
    rowtab = (off | np.concatenate((c0, [0])) << 24).astype("<u4")
    ts = np.concatenate([a[r, c0[r]:c0[r] + n[r]] | b[r, c0[r]:c0[r] + n[r]] << 4 for r in range(kept)]).astype(np.uint8)
    qs = np.concatenate([q[r, c0[r]:c0[r] + n[r]] for r in range(kept)]).astype(np.uint8)
    assert len(ts) == cells == off[-1]
    body = rowtab.tobytes() + ts.tobytes() + qs.tobytes()
    return np.frombuffer(body + bytes(int(compact_span(kept, cells)) - len(body)), np.uint8)


def layout_definition(spans, slab_bytes):
    """``train_cache_cases.layout_definition`` by explicit spans -> ([(slab, offset)], used bytes per slab)."""
    places, used = [], []
    for s in np.asarray(spans).tolist():
        if s == 0:
            places.append((0, 0))
            continue
        assert s <= slab_bytes and s % 16 == 0
        if not used or used[-1] + s > slab_bytes:
            used.append(0)
        places.append((len(used) - 1, used[-1]))
        used[-1] += s
    return places, used


def check_store_against_the_definition(st, planes, order, slab_bytes, data_off=0, fill=0xAB):
    """Every record of the store ``st`` (record k = slot ``order[k]`` of ``planes``, appended in that order into slabs pre-filled with
    ``fill``) against the numpy statements: format, span, place, bytes; the pad is zeros (it is part of the stated bytes) and
    every byte of every slab's allocation outside the records still holds ``fill``."""
    fmt, spans = format_spans(planes, st.record_format)
    kept = spans_definition(planes)[0]
    places, used = layout_definition(spans[order], slab_bytes)
    slabs = [st.slab(k) for k in range(len(used))]
    covered = [np.zeros(len(s[0]), bool) for s in slabs]
    for k, slot in enumerate(order):
        slab, off, got_kept = st.record(k)
        assert (slab, off) == places[k] and got_kept == kept[slot] and off % 16 == 0, (k, slot)
        assert st.record_span(k) == (fmt[slot], spans[slot]), (k, slot, EDGES[slot] if len(kept) == N_EDGES else "")
        if spans[slot] == 0:
            continue
        buf, d_off, _used, cap = slabs[slab]
        assert d_off == data_off and cap <= slab_bytes and off + spans[slot] <= cap       # (the last slab: what the capacity leaves)
        lo = d_off + off
        want = stored_bytes_definition(planes, slot, fmt[slot])
        assert len(want) == spans[slot] and buf[lo:lo + len(want)].tobytes() == want.tobytes(), (k, slot)
        assert not covered[slab][lo:lo + len(want)].any()
        covered[slab][lo:lo + len(want)] = True
    for k, (buf, d_off, n_used, _cap) in enumerate(slabs):
        assert n_used == used[k]
        assert covered[k][d_off:d_off + n_used].all() and (buf[~covered[k]] == fill).all(), k
    return fmt, spans

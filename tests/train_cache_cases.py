"""Fixtures of the record store's tests (tests/test_train_cache_host.py on the CPU, tests/test_train_cache_gpu.py on the GPU): the
45 records of tests/train_loader_device_cases.py as inflated bytes, six records made by hand around the edges of the extent, and the
numpy statements of a record's extent, of the store's layout and of its bytes."""
import numpy as np

from dl4vc_amd.hdf5_schema import PLANE_FIELDS, record_dtype
from dl4vc_amd.site_assembly import SitePlan
from tests.train_loader_device_cases import READS, STORED, labelled_records

W = 201
# extents of hand_made_records(): no byte; one byte in row 0 of the strand plane only; a byte in the last stored row; fewer rows
# than num_reads says; a row beyond num_reads; exactly the rows the model reads
HAND_KEPT = (0, 1, STORED, 6, 10, READS)


def hand_made_records():
    recs = np.zeros(len(HAND_KEPT), record_dtype(STORED, W))
    rng = np.random.default_rng(12)
    recs[1]["strand"][0, 77] = 2
    recs[1]["num_reads"] = 1
    for f in PLANE_FIELDS:
        recs[2][f][:9] = rng.integers(1, 9, (9, W))
    recs[2]["single_reads"][STORED - 1, W - 1] = 3                 # the very last byte of the reads plane
    recs[2]["num_reads"] = 9
    for f in PLANE_FIELDS:
        recs[3][f][:6] = rng.integers(0, 9, (6, W))
    recs[3]["q-scores"][5, 0] = 40
    recs[3]["num_reads"] = 15                                      # num_reads larger than kept
    for f in PLANE_FIELDS:
        recs[4][f][:3] = rng.integers(1, 9, (3, W))
    recs[4]["q-scores"][9, 100] = 1                                # a non-zero row beyond num_reads
    recs[4]["num_reads"] = 3
    for f in PLANE_FIELDS:
        recs[5][f][:READS] = rng.integers(0, 9, (READS, W))
    recs[5]["strand"][READS - 1, 200] = 1
    recs[5]["num_reads"] = READS
    return recs


def plane_offsets(dtype):
    return [dtype.fields[f][1] for f in PLANE_FIELDS]


def inflated(recs):
    """The records as the inflate leaves them: packed, ``itemsize`` bytes each."""
    return np.frombuffer(recs.tobytes(), np.uint8).copy()


def kept_definition(recs):
    """1 + the last stored row with a non-zero byte in any of the three planes (0: none)."""
    used = np.zeros((len(recs), recs.dtype["single_reads"].shape[0]), bool)
    for f in PLANE_FIELDS:
        used |= (recs[f] != 0).any(axis=2)
    last = used.shape[1] - np.argmax(used[:, ::-1], axis=1)
    return np.where(used.any(axis=1), last, 0).astype(np.int32)


def span(kept):
    return (3 * np.asarray(kept, np.int64) * W + 15) & ~np.int64(15)


def layout_definition(kept, slab_bytes):
    """-> ([(slab, offset)] per record in order, used bytes per slab): 16-byte boundaries, a record that does not fit what is
    left of the last slab opens the next, a record without rows lies at (0, 0) and takes nothing."""
    places, used = [], []
    for b in span(kept).tolist():
        if b == 0:
            places.append((0, 0))
            continue
        assert b <= slab_bytes
        if not used or used[-1] + b > slab_bytes:
            used.append(0)
        places.append((len(used) - 1, used[-1]))
        used[-1] += b
    return places, used


def stored_bytes_definition(rec, kept):
    """reads[kept][W] | qual[kept][W] | strand[kept][W] | zeros to the next multiple of 16."""
    body = b"".join(np.ascontiguousarray(rec[f][:kept]).tobytes() for f in PLANE_FIELDS)
    return np.frombuffer(body + bytes(int(span(kept)) - len(body)), np.uint8)


def hand_plan(records, rows, first_rows, seed=3):
    """A plan over hand-made records: the row lists as given, arbitrary bytes in the three [m][W] lines."""
    m = len(records)
    rng = np.random.default_rng(seed)
    lines = [rng.integers(0, 255, (m, W)).astype(np.uint8) for _ in range(3)]
    return SitePlan(np.asarray(records, np.int32), np.asarray(rows, np.int16).reshape(m, -1), np.asarray(first_rows, np.uint8), lines[0],
                    lines[1], lines[2], [""] * m, np.zeros(m, np.int32), np.zeros(m, bool))


def hand_plans():
    """Rows >= kept (zeros) in every position, rows below it, and first-rows sites with kept <, = and > the rows read."""
    n = len(HAND_KEPT)
    rng = np.random.default_rng(5)
    rows = np.sort(rng.integers(0, STORED, (n, READS)), axis=1)
    rows[2] = np.arange(STORED - READS, STORED)                    # up to the last stored row
    rows[4, -1] = 9                                                # the row beyond num_reads
    yield hand_plan(np.arange(n), rows, np.zeros(n))
    yield hand_plan(np.arange(n), np.tile(np.arange(READS), (n, 1)), np.ones(n))        # kept 0, 1, 20, 6, 10, 12 against 12 rows read
    mixed = np.array([3, 5, 2, 0, 3, 1, 4], np.int32)
    yield hand_plan(mixed, rows[mixed], np.array([1, 0, 1, 0, 0, 1, 0]))

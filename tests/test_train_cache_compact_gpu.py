"""``--train-cache-format compact`` on the MI355X: ``record_spans`` and ``store_pack_compact`` against the host store's bytes through
both sources (three plane arrays at every alignment, records inflated through a loader handle), ``store_assemble`` from a compact
store against the rows store and the CPU definition, the resident records from a file and from a BAM with their source gone, whole
runs of ``main.py`` with the flag against runs without it, and a budget that only the compact format fits.  The shapes are the
edge grid of tests/train_cache_compact_cases.py at (5, 7), (3, 16) and (200, 201), not the workload's sizes."""
import os
import shutil

import numpy as np
import pytest

from dl4vc_amd import hdf5io
from dl4vc_amd.chunk_loader import RecordStore, ResidentRecords
from tests import train_bam_cases as TC
from tests import train_cache_compact_cases as CC
from tests.train_cache_cases import W, hand_plans, inflated, plane_offsets
from tests.train_loader_device_cases import N, PLANES, READS, STORED, draw_seed, index_lists, labelled_records

pytestmark = pytest.mark.gpu

GUARD = 64                                       # 0xAB bytes behind every output plane (and 0..15 in front of it)
ORDER = np.array([11, 0, 9, 13, 7, 1, 2, 3, 10, 4, 5, 12, 6, 8], np.int32)       # slots in the order they are appended
ROWS_READ = {5: 4, 3: 3, 200: 100}               # rows a site reads at each shape's S


def same_stores(st, twin, n_records):
    """The device store against the host store: every record's table entry, format and span, every slab's bytes, and 0xAB in the
    guard in front of a device slab's data, behind the records and in the 16-byte pad."""
    s, t = st.stats(), twin.stats()
    assert (s.records, s.stored_bytes, s.slabs, s.inflated_bytes) == (t.records, t.stored_bytes, t.slabs, t.inflated_bytes)
    a, b = st.format_stats(), twin.format_stats()
    assert [getattr(a, f) for f, _t in a._fields_[:5]] == [getattr(b, f) for f, _t in b._fields_[:5]]
    for i in range(n_records):
        assert st.record(i) == twin.record(i) and st.record_span(i) == twin.record_span(i), i
    for k in range(s.slabs):
        buf, off, used, cap = st.slab(k)
        want, _o, want_used, want_cap = twin.slab(k)
        assert (off, used, cap) == (256, want_used, want_cap) and len(buf) == 256 + cap + 16
        assert buf[off:off + used].tobytes() == want[:used].tobytes(), k
        assert (buf[:off] == 0xAB).all() and (buf[off + used:] == 0xAB).all(), k


def assemble_both(st, twin, records, rows, first, R, Wp, lines, use_q, use_strand, shift, stream=0):
    """``cl_store_assemble_device`` into planes ``shift`` bytes into 0xAB-filled buffers against ``twin.assemble_host``."""
    import torch
    m = len(records)
    sizes = [m * R * Wp] * 3 + [m * Wp] * 3
    bufs = [torch.full((shift + n + GUARD,), 0xAB, dtype=torch.uint8, device="cuda") for n in sizes]
    torch.cuda.synchronize()
    st.assemble_device(records, rows, first, R, lines, use_q, use_strand, [t.data_ptr() + shift for t in bufs], stream)
    torch.cuda.synchronize()
    want = twin.assemble_host(records, rows, first, R, lines, use_q, use_strand)
    got = []
    for name, t, n, y in zip(PLANES, bufs, sizes, want):
        h = t.cpu().numpy()
        assert h[shift:shift + n].tobytes() == y.tobytes(), (name, shift, use_q, use_strand)
        assert (h[:shift] == 0xAB).all() and (h[shift + n:] == 0xAB).all(), (name, shift)
        got.append(h[shift:shift + n])
    return got


# ---- the three kernels with the planar source ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shifts", [(0, 1, 8), (15, 8, 1), (8, 15, 15)])
@pytest.mark.parametrize("S,Wp", CC.SHAPES)
def test_spans_pack_and_assemble_from_planes_equal_the_host_store(S, Wp, shifts):
    """The edge grid as three arrays whose views start 0, 1, 8 and 15 bytes past a 16-byte boundary, in two appends and an order of
    its own, slabs of a third of the bytes (three or more), the budget exactly enough: the device's extents, formats, spans and
    slabs equal the host store's and the numpy statement, the source is unchanged; then sites over compact and fallback records
    alike, row lists and first rows, with and without the quality and strand planes."""
    import torch
    planes = CC.edge_planes(S, Wp)
    n = CC.N_EDGES * S * Wp
    bufs = [torch.full((16 + sh + n + 64,), 0xCD, dtype=torch.uint8, device="cuda") for sh in shifts]
    views = []
    for b, sh, p in zip(bufs, shifts, planes):
        lo = (-b.data_ptr()) % 16 + sh
        views.append(b[lo:lo + n])
        views[-1].copy_(torch.from_numpy(p.reshape(-1)))
    ptrs = [v.data_ptr() for v in views]
    assert [p % 16 for p in ptrs] == list(shifts)
    before = [b.cpu().numpy().copy() for b in bufs]
    fmt, spans = CC.format_spans(planes)
    need = int(spans[ORDER].sum())
    slab = int(max(spans.max(), CC.pad16(need // 3)))
    records = np.arange(len(ORDER), dtype=np.int32)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with RecordStore(Wp, S, len(ORDER), need, slab, device=-1, record_format="compact") as twin, \
            RecordStore(Wp, S, len(ORDER), need, slab, device=0, record_format="compact") as st, \
            RecordStore(Wp, S, len(ORDER), 1 << 30, 1 << 20, device=0) as rows_store:
        twin.debug_fill(0xAB)
        st.debug_fill(0xAB)
        want_kept = twin.pack_planes_host(*planes, ORDER, records)
        kept = np.concatenate([st.append_planes_device(ptrs, CC.N_EDGES, ORDER[:5], records[:5], side.cuda_stream),
                               st.append_planes_device(ptrs, CC.N_EDGES, ORDER[5:], records[5:])])
        assert (kept == want_kept).all() and (kept == CC.spans_definition(planes)[0][ORDER]).all()
        same_stores(st, twin, len(ORDER))
        CC.check_store_against_the_definition(st, planes, ORDER, slab, data_off=256)
        s, by = st.stats(), st.format_stats()
        assert s.slabs >= 3 and s.stored_bytes == need and by.rows_records == 3 and by.compact_records == len(ORDER) - 3
        assert by.spans_ms > 0 and s.extent_ms == 0 and s.pack_ms > 0
        # one byte short of what the records need in compact spans
        from dl4vc_amd.chunk_loader import StoreFull
        with RecordStore(Wp, S, len(ORDER), need - 1, slab, device=0, record_format="compact") as tight:
            with pytest.raises(StoreFull, match="capacity of %d bytes would be exceeded" % (need - 1)):
                tight.append_planes_device(ptrs, CC.N_EDGES, ORDER, records)
            assert (tight.stats().records, tight.stats().slabs) == (0, 0)
            fit = int((np.cumsum(spans[ORDER]) <= need - 1).sum())
            assert (tight.stats().refused_fit_records, tight.stats().refused_fit_bytes) == (fit, int(spans[ORDER][:fit].sum()))
        # the gather: every record as a site, row lists that name rows >= kept and first rows, three output alignments
        rows_store.append_planes_device(ptrs, CC.N_EDGES, ORDER, records)
        assert rows_store.format_stats().compact_records == 0
        R = ROWS_READ[S]
        rng = np.random.default_rng(S)
        sites = np.concatenate((records, records[::-1])).astype(np.int32)
        m = len(sites)
        lines = [rng.integers(0, 255, (m, Wp)).astype(np.uint8) for _ in range(3)]
        pick = np.sort(rng.integers(0, S, (m, R)), axis=1).astype(np.int16)
        first = (np.arange(m) % 3 == 0).astype(np.uint8)
        for k, (use_q, use_strand) in enumerate([(True, True), (False, True), (True, False), (False, False)]):
            shift = (5 * k + shifts[0]) % 16
            got = assemble_both(st, twin, sites, pick, first, R, Wp, lines, use_q, use_strand, shift, side.cuda_stream)
            also = assemble_both(rows_store, twin, sites, pick, first, R, Wp, lines, use_q, use_strand, shift)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(got, also))
        got = assemble_both(st, twin, sites, None, None, R, Wp, lines, True, True, 3)            # rows = NULL: every site its first rows
        # against the untrimmed planes themselves
        for p, x in zip(planes, got):
            assert x.reshape(m, R, Wp).tobytes() == p[ORDER[sites], :R].tobytes()
    torch.cuda.synchronize()
    for b, was in zip(bufs, before):
        assert b.cpu().numpy().tobytes() == was.tobytes()                  # the three source arrays are read only


# ---- records inflated through a loader handle ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def recs():
    return labelled_records()


@pytest.fixture(scope="module")
def files(tmp_path_factory, recs):
    d = tmp_path_factory.mktemp("train_cache_compact")
    hdf5io.write_candidates(str(d / "labelled.hdf"), recs)
    hdf5io.write_candidates(str(d / "edges.hdf"), CC.edge_records())
    return {"labelled": str(d / "labelled.hdf"), "edges": str(d / "edges.hdf"), "dir": str(d)}


def host_twin(records, slab_bytes, record_format="compact"):
    st = RecordStore(W, STORED, len(records), 1 << 30, slab_bytes, device=-1, record_format=record_format)
    st.debug_fill(0xAB)
    st.pack_host(inflated(records), records.dtype.itemsize, plane_offsets(records.dtype), np.arange(len(records)), np.arange(len(records)))
    return st


@pytest.mark.parametrize("which,group", [("labelled", 2), ("edges", 1), ("labelled", 6)])
def test_spans_and_pack_of_inflated_records_equal_the_host_store(files, recs, which, group):
    """The fill from a file (an odd record size: planes at every alignment) in groups of 2, 1 and 6 chunks."""
    records = recs if which == "labelled" else CC.edge_records()
    assert records.dtype.itemsize % 2 == 1
    planes = CC.record_planes(records)
    slab = int(2 * CC.format_spans(planes)[1].max())
    with host_twin(records, slab) as twin, \
            ResidentRecords(files[which], READS, 37, capacity_bytes=1 << 30, slab_bytes=slab, group_chunks=group, debug_fill=0xAB,
                            record_format="compact") as rr:
        assert len(rr) == len(records)
        same_stores(rr.store, twin, len(records))
        CC.check_store_against_the_definition(rr.store, planes, np.arange(len(records)), slab, data_off=256)
        by = twin.format_stats()
        assert rr.stage["store_compact_records"] == by.compact_records and rr.stage["store_compact_bytes"] == by.compact_bytes
        assert rr.stage["store_rows_records"] == by.rows_records == (0 if which == "labelled" else 3)
        assert rr.stage["store_bytes"] == by.compact_bytes + by.rows_bytes and rr.stage["spans_ms"] > 0 and rr.stage["extent_ms"] == 0


def test_assemble_device_from_a_compact_store_equals_the_rows_store_and_the_host_definition(files, recs):
    """The index lists of the training loader over the 45 labelled records (deep sites with drawn rows), and the hand plans over the
    edge records (a batch whose sites mix compact and fallback records, rows >= kept in every position, first rows with kept <, =
    and > the rows read): outputs 0..15 bytes into their buffers, with and without the quality and strand planes."""
    from tests.test_train_cache_host import plan_of
    slab = 1 << 16
    edges = CC.edge_records()
    with host_twin(recs, slab, "rows") as twin, ResidentRecords(files["labelled"], READS, 37, capacity_bytes=1 << 30, slab_bytes=slab,
                                                                record_format="compact") as rr:
        assert rr.store.format_stats().compact_records == N
        call = 0
        for epoch in (0, 1):
            for idx in index_lists():
                plan = plan_of(recs, idx, draw_seed(epoch))
                first = np.ascontiguousarray(plan.first_rows, np.uint8)
                use_q, use_strand = call % 2 == 0, call % 4 < 2
                assemble_both(rr.store, twin, plan.slots, None if first.all() else plan.rows, first, READS, W,
                              (plan.ref, plan.ref_mask, plan.var_mask), use_q, use_strand, call % 16)
                call += 1
        assert call >= 16
    with host_twin(edges, slab, "rows") as twin, ResidentRecords(files["edges"], READS, 37, capacity_bytes=1 << 30, slab_bytes=slab,
                                                                 record_format="compact") as rr:
        assert rr.store.format_stats().rows_records == 3
        call = 0
        for plan in hand_plans():
            plan.slots[:] = (plan.slots * 5 + 9) % len(edges)
            fmts = {rr.store.record_span(int(i))[0] for i in plan.slots}
            assert fmts == {0, 1}                                          # the batch mixes compact and fallback records
            for use_q, use_strand in ((True, True), (False, True), (True, False), (False, False)):
                got = assemble_both(rr.store, twin, plan.slots, plan.rows, plan.first_rows, READS, W, (plan.ref, plan.ref_mask, plan.var_mask),
                                    use_q, use_strand, (7 * call) % 16)
                call += 1
                for p, f, used in zip(got[:3], ("single_reads", "q-scores", "strand"), (True, use_q, use_strand)):
                    want = np.stack([edges[f][s][np.arange(READS) if fr else r] for s, r, fr in zip(plan.slots, plan.rows, plan.first_rows)])
                    assert p.tobytes() == (want if used else np.zeros_like(want)).tobytes(), f


# ---- resident records ------------------------------------------------------------------------------------------------------------
def batches_equal(a, b, lists, seeds, reads, B):
    """Every batch of ``assemble_list`` of the resident records ``a`` equals that of ``b``: the six planes, labels and counts."""
    import torch
    sizes = [B * reads * 201] * 3 + [B * 201] * 3
    outs_a, outs_b = ([torch.zeros(n, dtype=torch.uint8, device="cuda") for n in sizes] for _ in range(2))
    for seed in seeds:
        for idx in lists:
            m = len(idx)
            ga = a.assemble_list(idx, seed, [t.data_ptr() for t in outs_a])
            gb = b.assemble_list(idx, seed, [t.data_ptr() for t in outs_b])
            torch.cuda.synchronize()
            for name, x, y, n in zip(PLANES, outs_a, outs_b, sizes):
                assert torch.equal(x[:n // B * m], y[:n // B * m]), (name, idx)
            assert (ga.label == gb.label).all() and (ga.counts == gb.counts).all() and list(ga.plan.vcfrec) == list(gb.plan.vcfrec)
    assert outs_a[0].any()


def test_resident_records_from_a_file_give_the_batches_of_the_rows_store_with_the_file_gone(files):
    gone = os.path.join(files["dir"], "gone.hdf")
    shutil.copy(files["labelled"], gone)
    lists = index_lists() + [np.random.RandomState(18).permutation(N).astype(np.int64)[:37]]
    with ResidentRecords(gone, READS, 37, capacity_bytes=1 << 30, slab_bytes=1 << 16, record_format="compact") as rr, \
            ResidentRecords(files["labelled"], READS, 37, capacity_bytes=1 << 30, slab_bytes=1 << 16) as rows:
        os.remove(gone)
        assert rr.record_format == "compact" and rr.stage["store_records"] == N and rr.stage["store_bytes"] < rows.stage["store_bytes"]
        assert rows.stage["store_compact_records"] == 0 and rows.stage["spans_ms"] == 0 and rows.stage["extent_ms"] > 0
        batches_equal(rr, rows, lists, (draw_seed(0), draw_seed(1)), READS, 37)


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    return TC.labelled_fixture(tmp_path_factory.mktemp("train_cache_compact_bam"))


def test_resident_records_from_a_bam_give_the_batches_of_the_rows_store_with_the_bam_gone(fx):
    gone = os.path.join(fx["dir"], "gone")
    os.makedirs(gone)
    for path in (fx["bam"], fx["bam"] + ".bai", fx["fasta"]):
        shutil.copy(path, gone)
    bam, fasta = os.path.join(gone, os.path.basename(fx["bam"])), os.path.join(gone, os.path.basename(fx["fasta"]))
    locations = TC.locations(fx, "train")
    n = TC.TRAIN_RECORDS
    perm = np.random.RandomState(5).permutation(n).astype(np.int64)
    lists = [perm[k:k + 8] for k in range(0, n, 8)] + [np.arange(0, 8, dtype=np.int64)]
    with ResidentRecords.from_bam(bam, fasta, locations, 100, 8, capacity_bytes=1 << 30, slab_bytes=1 << 20, round_locations=16,
                                  record_format="compact") as rr, \
            ResidentRecords.from_bam(fx["bam"], fx["fasta"], locations, 100, 8, capacity_bytes=1 << 30, slab_bytes=1 << 20,
                                     round_locations=16) as rows, \
            ResidentRecords.from_bam(fx["bam"], fx["fasta"], locations, 100, 8, device=-1, capacity_bytes=1 << 30, slab_bytes=1 << 20,
                                     round_locations=16, record_format="compact") as host:
        shutil.rmtree(gone)
        assert len(rr) == len(rows) == len(host) == n and rr.blob.tobytes() == rows.blob.tobytes()
        same_stores_any_fill(rr.store, host.store, n)
        assert rr.stage["store_compact_records"] == n and rr.stage["store_bytes"] < rows.stage["store_bytes"] and rr.stage["spans_ms"] > 0
        print("the BAM fixture's %d records: %d bytes in rows, %d compact" % (n, rows.stage["store_bytes"], rr.stage["store_bytes"]))
        batches_equal(rr, rows, lists, (7, 7 + n), 100, 8)


def same_stores_any_fill(st, twin, n_records):
    """``same_stores`` without the fill byte (no ``debug_fill``): table entries, formats, spans and the records' bytes."""
    assert st.stats().stored_bytes == twin.stats().stored_bytes and st.stats().slabs == twin.stats().slabs
    for i in range(n_records):
        assert st.record(i) == twin.record(i) and st.record_span(i) == twin.record_span(i), i
    for k in range(st.stats().slabs):
        buf, off, used, _cap = st.slab(k)
        want, _o, want_used, _c = twin.slab(k)
        assert used == want_used and buf[off:off + used].tobytes() == want[:used].tobytes(), k


# ---- main.py -----------------------------------------------------------------------------------------------------------------------
# (the fixture ``train_files`` writes its 17 training and 16 test records of 100 reads into this module's ``files["dir"]``)
from tests.test_train_loader_device_gpu import assert_same_training, run_training, train_files  # noqa: E402,F401

CACHE = ["--train-loader-device", "gpu", "--train-cache-device", "gpu"]
COMPACT = CACHE + ["--train-cache-format", "compact"]
LINE = r"--train-cache-format compact: (\d+) records in (\d+) bytes \(([\d.]+) of their \d+ (?:inflated|plane) bytes\), (\d+) records fell back"


@pytest.fixture(scope="module")
def file_runs(train_files):  # noqa: F811
    """The runs from a file that several tests compare against, made once."""
    return {"rows": run_training(train_files, "compact_rows", CACHE + ["--train-cache-bytes", str(64 << 20)])}


def fill_lines(stdout):
    import re
    return [tuple(m) for m in re.findall(LINE, stdout)]


def test_main_py_trains_the_same_from_a_file_with_the_flag(train_files, file_runs):  # noqa: F811
    got = run_training(train_files, "compact_file", COMPACT + ["--train-cache-bytes", str(64 << 20)])
    assert_same_training(got, file_runs["rows"])
    fills = fill_lines(got[0].stdout)
    assert [(f[0], f[3]) for f in fills] == [("17", "0"), ("16", "0")] and all(0 < float(f[2]) < 1 for f in fills), got[0].stdout[-2000:]
    assert "--train-cache-format" not in file_runs["rows"][0].stdout.split("\n", 1)[1]      # (after the line of the arguments)


def test_main_py_trains_the_same_on_two_ranks_with_the_flag(train_files):  # noqa: F811
    rows = run_training(train_files, "compact_rows2", CACHE + ["--train-cache-bytes", str(64 << 20)], 2)
    got = run_training(train_files, "compact_file2", COMPACT + ["--train-cache-bytes", str(64 << 20)], 2)
    assert_same_training(got, rows)
    assert len(fill_lines(got[0].stdout)) == 4                             # a store per file and rank


def test_main_py_trains_the_same_from_the_bam_with_the_flag(fx):
    from tests.test_train_bam_gpu import assert_same_runs, run_main
    rows = run_main(fx, "compact_bam_rows", "bam")
    got = run_main(fx, "compact_bam", "bam", extra=["--train-cache-format", "compact"])
    assert_same_runs(got, rows, TC.TEST_RECORDS, 5)
    fills = fill_lines(got[0].stdout)
    assert [int(f[0]) + int(f[3]) for f in fills] == [TC.TRAIN_RECORDS, TC.TEST_RECORDS], got[0].stdout[-3000:]
    assert not fill_lines(rows[0].stdout)


def test_a_budget_between_the_two_formats_trains_only_with_the_flag(train_files, file_runs):  # noqa: F811
    """``--train-cache-bytes`` between what the two files take in the compact format and what they take in rows, both from the CPU
    twins: without the flag the run ends during the fill with the store's refusal, with it the run trains and matches the
    unrestricted run."""
    d, _sample = train_files
    need = {"rows": 0, "compact": 0}
    for name in ("train.hdf", "test.hdf"):
        with hdf5io.CandidateFile(os.path.join(d, name)) as f:
            records = f.read(0, len(f))
        planes = CC.record_planes(records)
        S, Wp = planes[0].shape[1:]
        for record_format in need:
            with RecordStore(Wp, S, len(records), 1 << 40, 1 << 24, device=-1, record_format=record_format) as st:
                st.pack_planes_host(*planes, np.arange(len(records)), np.arange(len(records)))
                need[record_format] += st.stats().stored_bytes
    assert need["compact"] < need["rows"]
    budget = (need["compact"] + need["rows"]) // 2
    print("the two files take %d bytes in rows, %d compact; the budget is %d" % (need["rows"], need["compact"], budget))
    r, _ = run_training(train_files, "compact_budget_rows", CACHE + ["--train-cache-bytes", str(budget)], ok=False)
    assert "--train-cache-device gpu: " in r.stderr and "does not fit the record store: " in r.stderr and "Traceback" not in r.stderr
    assert "of the budget of" in r.stderr and "raise --train-cache-bytes or drop --train-cache-device" in r.stderr
    assert "Average loss" not in r.stdout                                  # (it ended during the fill)
    got = run_training(train_files, "compact_budget", COMPACT + ["--train-cache-bytes", str(budget)])
    assert_same_training(got, file_runs["rows"])

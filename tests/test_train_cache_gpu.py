"""The training file resident on the MI355X (``main.py ... --train-loader-device gpu --train-cache-device gpu``): the three kernels of
the record store against their CPU definitions (extents, every slab's bytes, the record table in device memory, the assembled
planes), the budget, the resident prefetcher against the host definition of the device training loader over two epochs and an
evaluation pass with the file gone, a damaged chunk named at the fill, and whole runs of ``main.py`` with the flag against runs
with ``--train-loader-device gpu`` alone."""
import os
import shutil

import numpy as np
import pytest

from dl4vc_amd import hdf5io
from dl4vc_amd.chunk_loader import DamagedChunk, RecordStore, ResidentRecords, StoreFull
from dl4vc_amd.site_assembly import plan_records
from tests.loader_device_cases import chunk_written, write_chunks
from tests.test_train_loader_device_gpu import assert_same_training, run_training
from tests.train_cache_cases import W, inflated, kept_definition, plane_offsets, span
from tests.train_loader_device_cases import N, PLANES, READS, STORED, draw_seed, host_definition, index_lists, labelled_records

pytestmark = pytest.mark.gpu

B = 37                                           # sites per batch: the longest index list of these tests
SLAB = 2 * int(span(STORED))                     # two of the largest records: the 45 records span several slabs
GUARD = 64                                       # 0xAB bytes behind every output plane (and 0..15 in front of it)


@pytest.fixture(scope="module")
def recs():
    return labelled_records()


@pytest.fixture(scope="module")
def files(tmp_path_factory, recs):
    d = tmp_path_factory.mktemp("train_cache")
    hdf5io.write_candidates(str(d / "gzip4.hdf"), recs)
    chunk_written(str(d / "fixed.hdf"), recs, "fixed")
    write_chunks(str(d / "raw.hdf"), recs, raw=(2,))
    write_chunks(str(d / "damaged.hdf"), recs, damage=(2,))
    return {"libhdf5 gzip 4": str(d / "gzip4.hdf"), "ChunkWriter fixed": str(d / "fixed.hdf"), "a raw chunk": str(d / "raw.hdf"),
            "damaged": str(d / "damaged.hdf"), "dir": str(d)}


@pytest.fixture(scope="module")
def twin(recs):
    """The CPU definition of the store over the 45 records, slabs of ``SLAB`` bytes."""
    st = RecordStore(W, STORED, N, 1 << 30, SLAB, device=-1)
    kept = st.pack_host(inflated(recs), recs.dtype.itemsize, plane_offsets(recs.dtype), np.arange(N), np.arange(N))
    assert (kept == kept_definition(recs)).all()
    yield st
    st.close()


def many_lists():
    """Index lists of 1, 3, 5, 8 and 37 sites: the ten of ``index_lists`` and 37 and 5 records of another permutation."""
    perm = np.random.RandomState(18).permutation(N).astype(np.int64)
    lists = index_lists() + [perm[:37], perm[37:42]]
    assert {1, 5, 8, 37} <= {len(i) for i in lists}
    return lists


def plan_of(recs, idx, seed):
    texts = [bytes(v).decode() for v in recs["vcfrec"]]
    idx = np.asarray(idx, np.int64)
    return plan_records(idx.astype(np.int32), idx, recs["num_reads"].reshape(-1), recs["ref_bases"], texts, READS, STORED, seed)


@pytest.mark.parametrize("kind,group", [("libhdf5 gzip 4", 2), ("ChunkWriter fixed", 6), ("a raw chunk", 4)])
def test_store_kernels_equal_their_cpu_definitions(files, recs, twin, kind, group):
    """The fill in groups of 2, 6 and 4 chunks (three appends, one, two): every record's table entry as device memory holds it, every
    slab's bytes, and 0xAB everywhere else in the slabs' allocations; then every index list assembled into planes that start 0..15
    bytes into 0xAB-filled buffers, twice, and with the lists reversed."""
    import torch
    want_kept = kept_definition(recs)
    with ResidentRecords(files[kind], READS, B, capacity_bytes=1 << 30, slab_bytes=SLAB, group_chunks=group, debug_fill=0xAB) as rr:
        assert len(rr) == N and rr.stage["chunks"] == 6 and rr.stage["store_records"] == N
        assert rr.stage["store_bytes"] == int(span(want_kept).sum()) == twin.stats().stored_bytes
        assert rr.stage["raw_chunks"] == (1 if kind == "a raw chunk" else 0)
        assert rr.blob.tobytes() == hdf5io_blob(recs, rr.blob_dtype).tobytes()
        stats = rr.store.stats()
        assert stats.slabs == twin.stats().slabs >= 3 and stats.inflated_bytes == N * recs.dtype.itemsize
        assert stats.extent_ms > 0 and stats.pack_ms > 0
        for i in range(N):
            assert rr.store.record(i) == twin.record(i), i             # (slab, offset, kept) from the device's table
        for k in range(stats.slabs):
            buf, off, used, cap = rr.store.slab(k)
            want, _o, want_used, want_cap = twin.slab(k)
            assert (off, used, cap) == (256, want_used, want_cap)
            assert buf[off:off + used].tobytes() == want[:used].tobytes(), k
            assert (buf[:off] == 0xAB).all() and (buf[off + used:] == 0xAB).all(), k     # in front, behind the records, the 16-byte pad
        side = torch.cuda.Stream()
        call = 0
        for rep in range(2):
            for order in (1, -1):
                for idx in many_lists()[::order]:
                    idx = idx[::order]
                    plan = plan_of(recs, idx, draw_seed(rep))
                    first = np.ascontiguousarray(plan.first_rows, np.uint8)
                    rows = None if first.all() else plan.rows
                    lines = (plan.ref, plan.ref_mask, plan.var_mask)
                    m = len(idx)
                    shift = call % 16
                    call += 1
                    sizes = [m * READS * W] * 3 + [m * W] * 3
                    bufs = [torch.full((shift + n + GUARD,), 0xAB, dtype=torch.uint8, device="cuda") for n in sizes]
                    torch.cuda.synchronize()
                    rr.store.assemble_device(plan.slots, rows, first, READS, lines, True, True, [t.data_ptr() + shift for t in bufs],
                                             side.cuda_stream)
                    side.synchronize()
                    want = twin.assemble_host(plan.slots, rows, first, READS, lines)
                    for name, t, n, y in zip(PLANES, bufs, sizes, want):
                        h = t.cpu().numpy()
                        assert h[shift:shift + n].tobytes() == y.tobytes(), (name, idx, shift)
                        assert (h[:shift] == 0xAB).all() and (h[shift + n:] == 0xAB).all(), (name, idx, shift)
        assert call >= 48                                              # every alignment 0..15 three times


def hdf5io_blob(recs, blob_dtype):
    """The records' members outside the three planes, as the loader keeps them on the host."""
    blob = np.zeros(len(recs), blob_dtype)
    for name in blob_dtype.names:
        blob[name] = recs[name]
    return blob


@pytest.mark.parametrize("m", [1, 5, 8, 37])
def test_store_assemble_at_every_output_alignment(files, recs, twin, m):
    """m = 1, 5, 8 and 37 sites (deep sites with drawn rows among them), outputs 0..15 bytes into their buffers, with and without
    the quality and strand planes."""
    import torch
    perm = np.random.RandomState(40 + m).permutation(N).astype(np.int64)
    idx = np.concatenate(([2], perm[perm != 2]))[:m]                   # record 2 is deeper than the rows read
    plan = plan_of(recs, idx, draw_seed(1))
    assert not plan.first_rows.all()
    lines = (plan.ref, plan.ref_mask, plan.var_mask)
    sizes = [m * READS * W] * 3 + [m * W] * 3
    with ResidentRecords(files["ChunkWriter fixed"], READS, B, capacity_bytes=1 << 30, slab_bytes=SLAB) as rr:
        for shift in range(16):
            use_q, use_strand = shift % 2 == 0, shift % 4 < 2
            bufs = [torch.full((shift + n + GUARD,), 0xAB, dtype=torch.uint8, device="cuda") for n in sizes]
            torch.cuda.synchronize()
            rr.store.assemble_device(plan.slots, plan.rows, plan.first_rows, READS, lines, use_q, use_strand, [t.data_ptr() + shift for t in bufs])
            torch.cuda.synchronize()
            want = twin.assemble_host(plan.slots, plan.rows, plan.first_rows, READS, lines, use_q, use_strand)
            for name, t, n, y in zip(PLANES, bufs, sizes, want):
                h = t.cpu().numpy()
                assert h[shift:shift + n].tobytes() == y.tobytes(), (name, shift)
                assert (h[:shift] == 0xAB).all() and (h[shift + n:] == 0xAB).all(), (name, shift)
        # the range checks, before anything is enqueued: the outputs keep their bytes and the store goes on
        bufs = [torch.full((n,), 0xAB, dtype=torch.uint8, device="cuda") for n in sizes]
        ptrs = [t.data_ptr() for t in bufs]
        bad = plan.slots.copy()
        bad[-1] = N
        with pytest.raises(ValueError, match="names record %d of %d" % (N, N)):
            rr.store.assemble_device(bad, plan.rows, plan.first_rows, READS, lines, True, True, ptrs)
        rows = plan.rows.copy()
        rows[0, 3] = STORED
        with pytest.raises(ValueError, match="site 0 row 3 names stored row %d of %d" % (STORED, STORED)):
            rr.store.assemble_device(plan.slots, rows, plan.first_rows, READS, lines, True, True, ptrs)
        rows[0, 3] = -1
        with pytest.raises(ValueError, match="site 0 row 3 names stored row -1"):
            rr.store.assemble_device(plan.slots, rows, plan.first_rows, READS, lines, True, True, ptrs)
        torch.cuda.synchronize()
        assert all(bool((t == 0xAB).all()) for t in bufs)
        rr.store.assemble_device(plan.slots, plan.rows, plan.first_rows, READS, lines, True, True, ptrs)
        torch.cuda.synchronize()
        assert bufs[0].cpu().numpy().tobytes() == twin.assemble_host(plan.slots, plan.rows, plan.first_rows, READS, lines)[0].tobytes()


def test_a_budget_one_byte_short_is_refused_and_the_exact_budget_fits(files, recs):
    kept = kept_definition(recs)
    need = int(span(kept).sum())
    fit = int((np.cumsum(span(kept)) <= need - 1).sum())
    assert fit == N - 1                                                # (the last record has rows)
    text = r"gzip4\.hdf does not fit the record store: %d of its %d records fit, in %d bytes of the budget of %d bytes; raise " \
           r"--train-cache-bytes or drop --train-cache-device" % (fit, N, int(span(kept[:fit]).sum()), need - 1)
    for group in (2, 6):                                               # refused at the third append, and at the only one
        with pytest.raises(StoreFull, match=text):
            ResidentRecords(files["libhdf5 gzip 4"], READS, B, capacity_bytes=need - 1, slab_bytes=SLAB, group_chunks=group)
    with ResidentRecords(files["libhdf5 gzip 4"], READS, B, capacity_bytes=need, slab_bytes=SLAB, group_chunks=2) as rr:
        assert rr.stage["store_bytes"] == need and rr.stage["store_records"] == N


@pytest.mark.parametrize("ahead,release", [(1, True), (4, True), (2, False)])
def test_resident_prefetcher_batches_equal_the_host_definition_with_the_file_gone(files, ahead, release):
    """Two epochs with different seeds and one sequential evaluation pass from a prefetcher whose file is REMOVED once it is
    filled: nothing can be read again.  The consumer holds every batch until it has taken the next one and compares it then."""
    import torch
    from dl4vc_amd.train_data import DeviceBatchPrefetcher
    path = files["libhdf5 gzip 4"]
    gone = os.path.join(files["dir"], "resident_%d_%d.hdf" % (ahead, release))
    shutil.copy(path, gone)
    shuffled = index_lists() + [np.random.RandomState(18).permutation(N).astype(np.int64)[k:k + 8] for k in range(0, N, 8)]
    sequential = [np.arange(k, min(N, k + 8), dtype=np.int64) for k in range(0, N, 8)]

    def check(batch, idx, seed):
        planes, targets, blacklist, vcfrec = host_definition(path, idx, seed)
        batch.event.synchronize()
        for name, t, want in zip(PLANES, batch.planes(), planes):
            assert t.is_cuda and t.cpu().numpy().tobytes() == want.tobytes(), (name, idx)
        assert sorted(batch.targets) == sorted(targets)
        for k, v in targets.items():
            assert batch.targets[k].dtype == v.dtype and batch.targets[k].tobytes() == v.tobytes(), (k, idx)
        assert (batch.blacklist == blacklist).all() and batch.vcfrec == vcfrec and (batch.index == idx).all()

    with DeviceBatchPrefetcher(gone, READS, 8, ahead=ahead, wait_s=60.0, resident=True, cache_bytes=1 << 30, slab_bytes=SLAB) as pf:
        os.remove(gone)
        stage = dict(pf.stage)
        assert stage["chunks"] == 6 and stage["store_records"] == N and stage["store_bytes"] > 0 and stage["fill_ms"] > 0
        assert pf.loader.store.stats().slabs >= 3
        for lists, seed in ((shuffled, draw_seed(1)), (shuffled[::-1], draw_seed(2)), (sequential, draw_seed(0))):
            held, seen = None, 0
            for k, batch in enumerate(pf.batches(iter(lists), max_reads=READS, seed=seed, non_snp_train_weight=2.0, keep_candidate_af=True)):
                torch.cuda.synchronize()
                if held is not None:
                    check(held, lists[k - 1], seed)
                    if release:
                        held.release()
                held, seen = batch, seen + 1
            check(held, lists[-1], seed)
            held.release()
            assert seen == len(lists)
        for k in ("chunks", "compressed_bytes", "inflate_ms", "inflated_bytes", "read_ms", "store_bytes", "fill_ms"):
            assert pf.stage[k] == stage[k], k                          # after the fill nothing is read or inflated
        assert pf.stage["records"] == 2 * sum(len(i) for i in shuffled) + N and pf.stage["assemble_ms"] > 0


def test_a_damaged_chunk_no_index_touches_is_named_at_the_fill(files):
    from dl4vc_amd.train_data import DeviceBatchPrefetcher
    with pytest.raises(DamagedChunk, match="chunk at record 16: "):
        DeviceBatchPrefetcher(files["damaged"], READS, 8, resident=True, cache_bytes=1 << 30)
    with pytest.raises(DamagedChunk, match="chunk at record 16: "):
        ResidentRecords(files["damaged"], READS, 8, capacity_bytes=1 << 30, group_chunks=2)


# ---- main.py ---------------------------------------------------------------------------------------------------------------
from tests.test_train_loader_device_gpu import train_files  # noqa: E402,F401  (the fixture: 17 training and 16 test records of 100 reads)

CACHE = ["--train-loader-device", "gpu", "--train-cache-device", "gpu"]


@pytest.mark.parametrize("gpus", [1, 2])
def test_main_py_trains_the_same_with_the_files_resident(train_files, gpus):  # noqa: F811
    """Two epochs, ``--train-cache-device gpu`` against ``--train-loader-device gpu`` alone: the loss lines, both epochs' scored
    evaluation VCFs and every tensor of both checkpoints, bit for bit.  gpus = 2: two ranks on device 0 over gloo, a store each."""
    plain = run_training(train_files, "cache_plain%d" % gpus, ["--train-loader-device", "gpu"], gpus)
    kept = run_training(train_files, "cache_resident%d" % gpus, CACHE + ["--train-cache-bytes", str(64 << 20)], gpus)
    assert_same_training(kept, plain)
    lines = [l for l in kept[0].stdout.splitlines() if l.startswith("--train-cache-device gpu: ")]
    assert len(lines) == 2 * gpus and all(" records resident in " in l and "filled in" in l for l in lines)
    assert sum("17 records resident" in l for l in lines) == gpus and sum("16 records resident" in l for l in lines) == gpus
    assert "--train-cache-device" not in plain[0].stdout


def test_main_py_ends_with_the_refusal_when_the_budget_is_too_small(train_files):  # noqa: F811
    r, _ = run_training(train_files, "cache_small", CACHE + ["--train-cache-bytes", "100000"], ok=False)
    assert "--train-cache-device gpu: " in r.stderr and "does not fit the record store: " in r.stderr and "Traceback" not in r.stderr
    assert "of the budget of 100000 bytes; raise --train-cache-bytes or drop --train-cache-device" in r.stderr


def test_main_py_names_a_damaged_chunk_at_the_fill(train_files):  # noqa: F811
    r, _ = run_training(train_files, "cache_damaged", CACHE, train="train_damaged.hdf", ok=False)
    assert "chunk at record 8: " in r.stderr and "Traceback" not in r.stderr

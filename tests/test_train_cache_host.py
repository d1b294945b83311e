"""``--train-cache-device gpu`` where no device is needed: the CPU definitions of the record store (``cl_store_extent_host``,
``cl_store_pack_host``, ``cl_store_assemble_host``) against their numpy statements (tests/train_cache_cases.py) and against the host
definition of the device training loader, the store's refusals, what the command line refuses, the header against the exports and
the bindings, and the sanitizer pass of tools/asan_store.sh."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from dl4vc_amd import capi, chunk_loader, hdf5io, pileup_gpu
from dl4vc_amd.chunk_loader import RecordStore, StoreFull
from dl4vc_amd.hdf5_schema import PLANE_FIELDS
from dl4vc_amd.site_assembly import assemble_host, plan_records
from tests.train_cache_cases import (HAND_KEPT, W, hand_made_records, hand_plans, inflated, kept_definition, layout_definition, plane_offsets,
                                     span, stored_bytes_definition)
from tests.train_loader_device_cases import DEEP, N, NO_READ, PLANES, READS, STORED, draw_seed, host_definition, index_lists, labelled_records


@pytest.fixture(scope="module", autouse=True)
def lib():
    if not pileup_gpu.available() or not os.path.isfile(capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return chunk_loader.load_library()


@pytest.fixture(scope="module")
def recs():
    return labelled_records()


def host_store(records, slab_bytes=1 << 20, capacity=1 << 30, fill=0xAB):
    """A host store holding ``records`` in order -> (store, kept)."""
    st = RecordStore(W, STORED, len(records), capacity, slab_bytes, device=-1)
    st.debug_fill(fill)
    kept = st.pack_host(inflated(records), records.dtype.itemsize, plane_offsets(records.dtype), np.arange(len(records)), np.arange(len(records)))
    return st, kept


# ---- extents ---------------------------------------------------------------------------------------------------------------
def test_extents_equal_the_numpy_definition(recs):
    kept = chunk_loader.record_extents_host(inflated(recs), recs.dtype.itemsize, plane_offsets(recs.dtype), STORED, W)
    want = kept_definition(recs)
    assert kept.dtype == np.int32 and (kept == want).all()
    assert kept[NO_READ] == 0 and all(kept[i] > READS for i in DEEP) and 1 < len(set(kept.tolist()))
    assert recs.dtype.itemsize % 2 == 1                            # (planes at every byte alignment)
    # a subset in another order
    slots = np.array([44, 0, 17, 17], np.int32)
    assert (chunk_loader.record_extents_host(inflated(recs), recs.dtype.itemsize, plane_offsets(recs.dtype), STORED, W, slots) == want[slots]).all()


def test_extents_of_the_hand_made_records():
    hand = hand_made_records()
    kept = chunk_loader.record_extents_host(inflated(hand), hand.dtype.itemsize, plane_offsets(hand.dtype), STORED, W)
    assert kept.tolist() == list(HAND_KEPT) == kept_definition(hand).tolist()
    assert hand[3]["num_reads"] > kept[3] and hand[4]["num_reads"] < kept[4]          # num_reads disagrees with the planes, both ways
    assert not any(hand[1][f].any() for f in PLANE_FIELDS[:2]) and hand[1]["strand"][0].any()


def test_extent_host_refuses_what_it_cannot_follow(lib):
    hand = hand_made_records()
    buf, offs = inflated(hand), plane_offsets(hand.dtype)
    with pytest.raises(ValueError, match="names slot 6 of 6"):
        chunk_loader.record_extents_host(buf, hand.dtype.itemsize, offs, STORED, W, [0, 6])
    with pytest.raises(ValueError, match="names slot -1 of 6"):
        chunk_loader.record_extents_host(buf, hand.dtype.itemsize, offs, STORED, W, [-1])
    with pytest.raises(ValueError, match="does not lie inside a record"):
        chunk_loader.record_extents_host(buf, hand.dtype.itemsize, [offs[0], offs[1], offs[2] + 1], STORED, W)
    with pytest.raises(ValueError, match="bad shape"):
        chunk_loader.record_extents_host(buf, hand.dtype.itemsize, offs, 0, W)


# ---- pack ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["45 records", "hand-made"])
def test_pack_equals_the_numpy_statement_of_the_layout(recs, which):
    records = recs if which == "45 records" else hand_made_records()
    want_kept = kept_definition(records)
    slab_bytes = int(2 * span(want_kept).max())                    # just large enough for two of the largest records
    st, kept = host_store(records, slab_bytes)
    with st:
        assert (kept == want_kept).all()
        places, used = layout_definition(want_kept, slab_bytes)
        stats = st.stats()
        assert stats.records == len(records) and stats.slabs == len(used)
        assert stats.stored_bytes == int(span(want_kept).sum()) == sum(used)
        assert stats.inflated_bytes == len(records) * records.dtype.itemsize
        if which == "45 records":
            assert len(used) >= 3
        slabs = [st.slab(k) for k in range(len(used))]
        covered = [np.zeros(slab_bytes, bool) for _ in used]
        for i in range(len(records)):
            slab, off, k = st.record(i)
            assert (slab, off) == places[i] and k == want_kept[i] and off % 16 == 0
            b = int(span(k))
            assert off + b <= slab_bytes                           # none straddles
            buf, data_off, _used, cap = slabs[slab]
            assert data_off == 0 and cap == slab_bytes
            assert buf[off:off + b].tobytes() == stored_bytes_definition(records[i], k).tobytes(), i
            assert not covered[slab][off:off + b].any()
            covered[slab][off:off + b] = True
        for k, (buf, _o, n_used, _cap) in enumerate(slabs):
            assert n_used == used[k] and covered[k][:n_used].all() and not covered[k][n_used:].any()
            assert (buf[n_used:] == 0xAB).all()                    # nothing behind the records is written


def test_pack_in_groups_and_any_record_order_gives_the_layout_of_the_append_order(recs):
    """Three appends (the last in reverse slot order): records lie in the order they were appended."""
    kept = kept_definition(recs)
    buf, offs = inflated(recs), plane_offsets(recs.dtype)
    order = np.concatenate((np.arange(0, 16), np.arange(16, 40), np.arange(44, 39, -1)))
    with RecordStore(W, STORED, N, 1 << 30, 1 << 16, device=-1) as st:
        for a, b in ((0, 16), (16, 40), (40, 45)):
            got = st.pack_host(buf, recs.dtype.itemsize, offs, order[a:b], order[a:b])
            assert (got == kept[order[a:b]]).all()
        places, _used = layout_definition(kept[order], 1 << 16)
        for i, rec in enumerate(order):
            assert st.record(rec)[:2] == places[i]
            slab, off, k = st.record(rec)
            assert st.slab(slab)[0][off:off + int(span(k))].tobytes() == stored_bytes_definition(recs[rec], k).tobytes()


# ---- assemble --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gzip_file(tmp_path_factory, recs):
    path = str(tmp_path_factory.mktemp("train_cache") / "gzip4.hdf")
    hdf5io.write_candidates(path, recs)
    return path


def plan_of(recs, idx, seed):
    texts = [bytes(v).decode() for v in recs["vcfrec"]]
    idx = np.asarray(idx, np.int64)
    return plan_records(idx.astype(np.int32), idx, recs["num_reads"].reshape(-1), recs["ref_bases"], texts, READS, STORED, seed)


@pytest.mark.parametrize("use_q,use_strand", [(True, True), (False, True), (True, False), (False, False)])
def test_assemble_host_equals_the_host_definition(recs, gzip_file, use_q, use_strand):
    """Every index list at the seeds of evaluation and of the first epoch: the six planes byte for byte -- against the loader's
    host definition (raw chunks -> zi_inflate_host -> plan_records -> assemble_host) where both planes are used, against the
    numpy assembly of the untrimmed records for every setting."""
    st, _kept = host_store(recs, slab_bytes=1 << 16)
    with st:
        for epoch in (0, 1):
            seed = draw_seed(epoch)
            for idx in index_lists():
                plan = plan_of(recs, idx, seed)
                first = np.ascontiguousarray(plan.first_rows, np.uint8)
                got = st.assemble_host(plan.slots, None if first.all() else plan.rows, first, READS, (plan.ref, plan.ref_mask, plan.var_mask),
                                       use_q, use_strand)
                want = assemble_host(recs["single_reads"], recs["q-scores"], recs["strand"], plan, use_q, use_strand)
                for name, x, y in zip(PLANES, got, want):
                    assert x.dtype == np.uint8 and x.shape == y.shape and x.tobytes() == y.tobytes(), (name, idx)
                if use_q and use_strand:
                    planes = host_definition(gzip_file, idx, seed)[0]
                    for name, x, y in zip(PLANES, got, planes):
                        assert x.tobytes() == y.tobytes(), (name, idx)
        assert any(not plan_of(recs, idx, draw_seed(1)).first_rows.all() for idx in index_lists())


def test_assemble_host_writes_rows_that_were_not_kept_as_zeros():
    """Plans over the hand-made records: row lists that name rows >= kept, and first-rows sites with kept <, = and > the rows read."""
    hand = hand_made_records()
    st, kept = host_store(hand, slab_bytes=1 << 16)
    with st:
        assert min(kept) < READS and READS in kept and max(kept) > READS
        for plan in hand_plans():
            assert any((plan.rows[i] >= kept[plan.slots[i]]).any() for i in range(len(plan)) if not plan.first_rows[i]) or plan.first_rows.all()
            got = st.assemble_host(plan.slots, plan.rows, plan.first_rows, READS, (plan.ref, plan.ref_mask, plan.var_mask))
            want = assemble_host(hand["single_reads"], hand["q-scores"], hand["strand"], plan)
            for name, x, y in zip(PLANES, got, want):
                assert x.tobytes() == y.tobytes(), name
            # rows = NULL: every site takes its first rows
            got = st.assemble_host(plan.slots, None, None, READS, (plan.ref, plan.ref_mask, plan.var_mask))
            plan.first_rows[:] = 1
            want = assemble_host(hand["single_reads"], hand["q-scores"], hand["strand"], plan)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(got, want))


# ---- range checks ----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_store_unchanged_and_usable(recs):
    buf, offs, item = inflated(recs), plane_offsets(recs.dtype), recs.dtype.itemsize
    kept = kept_definition(recs)
    need = int(span(kept[:16]).sum())
    with RecordStore(W, STORED, N, need + int(span(kept[16:24]).sum()) - 1, 1 << 16, device=-1) as st:
        st.pack_host(buf, item, offs, np.arange(16), np.arange(16))
        plan = plan_of(recs, [3, 9, 2], draw_seed(1))
        lines = (plan.ref, plan.ref_mask, plan.var_mask)
        good = lambda: [a.tobytes() for a in st.assemble_host(plan.slots, plan.rows, plan.first_rows, READS, lines)]   # noqa: E731
        before, state = good(), [st.record(i) for i in range(16)]

        def unchanged():
            s = st.stats()
            assert (s.records, s.stored_bytes) == (16, need) and [st.record(i) for i in range(16)] == state and good() == before

        with pytest.raises(ValueError, match="site 1 names record 45 of 45"):
            st.assemble_host([3, N, 2], plan.rows, plan.first_rows, READS, lines)
        with pytest.raises(ValueError, match="site 0 names record -1 of 45"):
            st.assemble_host([-1, 9, 2], plan.rows, plan.first_rows, READS, lines)
        with pytest.raises(ValueError, match="names record 20, which is not in the store"):
            st.assemble_host([3, 20, 2], plan.rows, plan.first_rows, READS, lines)
        rows = plan.rows.copy()
        rows[2, 4] = -1
        with pytest.raises(ValueError, match="site 2 row 4 names stored row -1 of %d" % STORED):
            st.assemble_host(plan.slots, rows, np.zeros(3, np.uint8), READS, lines)
        rows[2, 4] = STORED
        with pytest.raises(ValueError, match="site 2 row 4 names stored row %d of %d" % (STORED, STORED)):
            st.assemble_host(plan.slots, rows, np.zeros(3, np.uint8), READS, lines)
        with pytest.raises(ValueError, match="%d rows per site but only %d are stored" % (STORED + 1, STORED)):
            st.assemble_host(plan.slots, None, None, STORED + 1, lines)
        unchanged()
        # an append beyond the capacity: one byte short of what records 16..23 need
        with pytest.raises(StoreFull, match=r"capacity of %d bytes would be exceeded: it holds 16 records in %d bytes, and 7 of the 8 records"
                                            % (st.capacity_bytes, need)):
            st.pack_host(buf, item, offs, np.arange(16, 24), np.arange(16, 24))
        s = st.stats()
        assert (s.refused_fit_records, s.refused_fit_bytes) == (7, need + int(span(kept[16:23]).sum()))
        unchanged()
        for slots, records, why in (([45], [16], "names slot 45 of 45"), ([16], [45], "names record 45 of 45"), ([16], [-1], "names record -1"),
                                    ([16], [3], "record 3 is in the store already"), ([16, 17], [20, 20], "record 20 is named twice")):
            with pytest.raises(ValueError, match=why):
                st.pack_host(buf, item, offs, slots, records)
        unchanged()
        st.pack_host(buf, item, offs, np.arange(16, 23), np.arange(16, 23))        # what fits still goes in
        assert st.stats().records == 23 and [st.record(i) for i in range(16)] == state and good() == before
    with pytest.raises(ValueError, match="multiple of 16"):
        RecordStore(W, STORED, N, 1 << 20, 1000, device=-1)
    with RecordStore(W, STORED, N, 1 << 30, 4096, device=-1) as st:
        with pytest.raises(ValueError, match="does not fit a slab of 4096"):
            st.pack_host(buf, item, offs, [2], [2])
        assert st.stats().records == 0


def test_device_entries_refuse_a_host_store(lib):
    with RecordStore(W, STORED, 4, 1 << 20, 1 << 16, device=-1) as st:
        one = np.zeros(1, np.int32)
        assert lib.cl_store_append_device(st._h, None, one.ctypes.data_as(C.c_void_p), one.ctypes.data_as(C.c_void_p), 1, None,
                                          one.ctypes.data_as(C.c_void_p)) == -1
        assert b"opened in host memory" in lib.cl_store_last_error(st._h)
    assert lib.cl_store_get_stats(None, None) == -1 and lib.cl_store_append_device(None, None, None, None, 0, None, None) == -1
    lib.cl_store_close(None)


# ---- the header, the exports, the bindings ----------------------------------------------------------------------------------
def test_header_exports_and_bindings_agree_on_the_store(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dl4vc_chunks.h")).read(), flags=re.S)
    declared = {n for n in re.findall(r"\b(cl_[a-z_]+)\s*\(", text) if n.startswith("cl_store_")}
    assert {"cl_store_open", "cl_store_close", "cl_store_last_error", "cl_store_append_device", "cl_store_assemble_device", "cl_store_get_stats",
            "cl_store_extent_host", "cl_store_pack_host", "cl_store_assemble_host"} <= declared
    assert declared == {n for n in chunk_loader.CL_SYMBOLS if n.startswith("cl_store_")}
    out = subprocess.run(["nm", "-D", "--defined-only", pileup_gpu.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {l.split()[-1] for l in out.splitlines() if l.split() and l.split()[-1].startswith("cl_store_")} == declared
    kinds = {"int64_t": C.c_int64, "uint64_t": C.c_uint64, "int32_t": C.c_int32}
    for fn in sorted(declared - {"cl_store_close", "cl_store_last_error"}):
        decl = re.search(r"int %s\((.*?)\);" % fn, text, flags=re.S).group(1)
        params = [re.sub(r"\s+", " ", p.strip()) for p in decl.split(",")]
        want = [None if "*" in p else kinds[p.split()[0]] for p in params]
        have = getattr(lib, fn).argtypes
        assert len(have) == len(want), fn
        for p, w, t in zip(params, want, have):
            assert (t is C.c_void_p or issubclass(t, C._Pointer)) if w is None else t is w, (fn, p)
    a = re.search(r"int cl_store_assemble_device\((.*?)\);", text, flags=re.S).group(1)
    b = re.search(r"int cl_store_assemble_host\((.*?)\);", text, flags=re.S).group(1)
    assert re.sub(r"\s+", " ", a) == re.sub(r"\s+", " ", b)         # (the CPU definition takes the same arguments)
    body = re.search(r"typedef struct \{([^}]*)\} cl_store_stats;", text, flags=re.S).group(1)
    names = [n.strip() for decl in re.findall(r"(?:int64_t|double)\s+([a-z_, ]+);", body) for n in decl.split(",")]
    assert names == [f[0] for f in chunk_loader.StoreStats._fields_]


# ---- the command line ------------------------------------------------------------------------------------------------------
def _main(argv):
    import sys
    sys.path.insert(0, ROOT)
    import main as cli
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    return str(e.value)


BASE = ["--model_pool_combine_dimension", "0", "--sample_vcf", "c.vcf"]
TRAIN = ["--train_file", "t.hdf", "--test_file", "v.hdf"]


def test_the_flags_parse_and_leave_no_trace_when_absent():
    from arguments import parse_args
    args = parse_args(BASE + TRAIN + ["--train-loader-device", "gpu", "--train-cache-device", "gpu", "--train-cache-bytes", "123456"])
    assert args.train_cache_device == "gpu" and args.train_cache_bytes == 123456
    plain = parse_args(BASE + TRAIN + ["--train-loader-device", "gpu"])
    assert "train_cache" not in repr(plain)                        # (the line main.py prints of its arguments is the parent's)
    assert parse_args(BASE + TRAIN + ["--train-loader-device", "gpu", "--train-cache-device", "gpu"]).train_cache_device == "gpu"


def test_refusals_name_their_reason():
    on = ["--train-loader-device", "gpu"]
    assert "--train-cache-device must be gpu" in _main(BASE + TRAIN + on + ["--train-cache-device", "cpu"])
    assert "--train-cache-device must be gpu" in _main(BASE + TRAIN + on + ["--train-cache-device", ""])
    why = _main(BASE + TRAIN + ["--train-cache-device", "gpu"])
    assert "--train-cache-device gpu keeps the records of --train-loader-device gpu resident: it needs that option" in why
    why = _main(BASE + TRAIN + ["--num-data-workers", "0", "--train-cache-device", "gpu", "--train-cache-bytes", "5"])
    assert "it needs that option" in why
    why = _main(BASE + TRAIN + on + ["--train-cache-bytes", "1000"])
    assert "--train-cache-bytes is the budget of --train-cache-device gpu, which is not given" in why
    why = _main(BASE + TRAIN + on + ["--train-cache-device", "gpu", "--train-cache-bytes", "-1"])
    assert "--train-cache-bytes must not be negative" in why
    # the older options keep their texts
    assert "--train-loader-device must be gpu" in _main(BASE + TRAIN + ["--train-loader-device", "cpu", "--train-cache-device", "gpu"])
    why = _main(BASE + ["--modelload", "c.pt", "--test_file", "v.hdf", "--train-loader-device", "gpu", "--train-cache-device", "gpu"])
    assert "option of --train_file" in why and "--loader-device gpu" in why
    why = _main(BASE + ["--modelload", "c.pt"] + TRAIN + ["--loader-device", "gpu"])
    assert "--loader-device gpu is an inference option: training and its evaluation keep the host loaders" in why
    assert "--loader-device must be gpu" in _main(BASE + ["--modelload", "c.pt", "--test_file", "x.hdf", "--loader-device", "cpu"])


def test_files_the_device_loader_refuses_are_refused_with_the_flag_too(tmp_path):
    from dl4vc_amd import synth
    from tests.loader_device_cases import create_dataset
    good, flat, few = (str(tmp_path / n) for n in ("good.hdf", "flat.hdf", "few_rows.hdf"))
    hdf5io.write_candidates(good, synth.make_labelled_records(16, 100, 900))
    create_dataset(flat, synth.make_labelled_records(16, 100, 900), chunked=False, shuffle=False)
    hdf5io.write_candidates(few, labelled_records(16))
    flags = ["--train-loader-device", "gpu", "--train-cache-device", "gpu"]
    why = _main(BASE + flags + ["--train_file", flat, "--test_file", good])
    assert why.startswith("--train-loader-device gpu: ") and "is not chunked" in why
    why = _main(BASE + flags + ["--train_file", good, "--test_file", few])
    assert "the model reads 100 rows per site but %s stores only %d" % (few, STORED) in why


def test_the_help_text_says_when_a_damaged_chunk_ends_the_run():
    from arguments import create_arg_parser
    text = re.sub(r"\s+", " ", create_arg_parser().format_help())
    assert "--train-cache-device" in text and "a damaged chunk ends the run during the fill" in text and "--train-cache-bytes" in text


# ---- the sanitizer pass ----------------------------------------------------------------------------------------------------
def test_the_host_twins_run_clean_under_the_sanitizers():
    """tools/asan_store.sh: a stand-alone program, every buffer ending where its data ends, source and destination alignments
    0..15."""
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "asan_store.sh")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "asan_store: " in r.stdout and "ok" in r.stdout

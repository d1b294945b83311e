"""``--train-cache-format compact`` where no device is needed: the CPU twins of the compact record format (``cl_store_spans_host``,
``cl_store_pack_host`` / ``cl_store_pack_planes_host`` and ``cl_store_assemble_host`` on a host store opened with
``record_format="compact"``) against the numpy statements of tests/train_cache_compact_cases.py and against the rows store, the
budget counted in compact spans, the refusals of the store and of the command line, the header against the exports and the
bindings, the sanitizer pass of tools/asan_store_compact.sh and the bytes a synthetic 30x pileup takes in both formats."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from dl4vc_amd import capi, chunk_loader, hdf5io, pileup_gpu
from dl4vc_amd.chunk_loader import RecordStore, StoreFull
from dl4vc_amd.site_assembly import assemble_host
from tests import train_cache_compact_cases as CC
from tests.train_cache_cases import W, hand_made_records, hand_plans, inflated, kept_definition, plane_offsets
from tests.train_loader_device_cases import N, PLANES, READS, STORED, draw_seed, host_definition, index_lists, labelled_records


@pytest.fixture(scope="module", autouse=True)
def lib():
    if not pileup_gpu.available() or not os.path.isfile(capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return chunk_loader.load_library()


@pytest.fixture(scope="module")
def recs():
    return labelled_records()


def planes_store(planes, order, slab_bytes, record_format="compact", capacity=1 << 30):
    """A host store of the slots ``order`` of three plane arrays, slabs pre-filled with 0xAB."""
    n, S, Wp = planes[0].shape
    st = RecordStore(Wp, S, len(order), capacity, slab_bytes, device=-1, record_format=record_format)
    st.debug_fill(0xAB)
    kept = st.pack_planes_host(*planes, order, np.arange(len(order)))
    assert (kept == CC.spans_definition(planes)[0][order]).all()
    return st


def records_store(records, slab_bytes=1 << 20, record_format="compact", capacity=1 << 30):
    st = RecordStore(W, STORED, len(records), capacity, slab_bytes, device=-1, record_format=record_format)
    st.debug_fill(0xAB)
    st.pack_host(inflated(records), records.dtype.itemsize, plane_offsets(records.dtype), np.arange(len(records)), np.arange(len(records)))
    return st


# ---- spans -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["45 records", "hand-made", "edges"])
def test_spans_of_records_equal_the_numpy_definition(recs, which):
    records = {"45 records": recs, "hand-made": hand_made_records(), "edges": CC.edge_records()}[which]
    got = chunk_loader.record_spans_host(inflated(records), records.dtype.itemsize, plane_offsets(records.dtype), STORED, W)
    want = CC.spans_definition(CC.record_planes(records))
    for name, x, y in zip(("kept", "cells", "mergeable", "rowspans"), got, want):
        assert x.dtype == y.dtype and (x == y).all(), name
    assert (got[0] == kept_definition(records)).all()                      # kept is the extent, as today
    assert records.dtype.itemsize % 2 == 1                                 # (planes at every byte alignment)
    slots = np.array([len(records) - 1, 0, 2, 2], np.int32)
    sub = chunk_loader.record_spans_host(inflated(records), records.dtype.itemsize, plane_offsets(records.dtype), STORED, W, slots)
    assert all((x == y[slots]).all() for x, y in zip(sub, want))


@pytest.mark.parametrize("S,Wp", CC.SHAPES + [(4, 255)])
def test_spans_of_the_edge_grid_equal_the_numpy_definition(S, Wp):
    planes = CC.edge_planes(S, Wp)
    kept, cells, mergeable, rowspans = chunk_loader.plane_spans_host(*planes)
    want = CC.spans_definition(planes)
    assert (kept == want[0]).all() and (cells == want[1]).all() and (mergeable == want[2]).all() and (rowspans == want[3]).all()
    assert mergeable.tolist() == [f for _why, f in CC.EDGES]
    assert kept[0] == 0 and cells[0] == 0 and kept[12] == S and cells[12] == 1
    assert rowspans[1, 0] == 0 | 1 << 8 and rowspans[2, 1] == (Wp - 1) | 1 << 8 and rowspans[2, 0] == 0
    assert rowspans[5, 1] == 0 and rowspans[5, 0] and rowspans[5, 2]       # the all-zero row between two used rows
    assert rowspans[6, 0] == Wp << 8 and rowspans[7, 0] == Wp << 8         # zeros inside a span; a row of all W columns
    assert rowspans[3, 0] == Wp // 2 | 1 << 8 and rowspans[4, S // 2] == 1 | 1 << 8     # the quality / the strand plane only


def test_spans_host_refuses_what_it_cannot_follow():
    planes = CC.edge_planes(3, 16)
    with pytest.raises(ValueError, match="names slot %d of %d" % (CC.N_EDGES, CC.N_EDGES)):
        chunk_loader.plane_spans_host(*planes, slots=[0, CC.N_EDGES])
    with pytest.raises(ValueError, match="a window of 256 columns exceeds the compact format's 255"):
        chunk_loader.plane_spans_host(*[np.zeros((1, 3, 256), np.uint8)] * 3)


# ---- pack --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,Wp", CC.SHAPES + [(4, 255)])
def test_packed_bytes_of_the_edge_grid_equal_the_numpy_statement(S, Wp):
    """A mixed store (compact records and the three that fall back) over at least three slabs, in an order of its own."""
    planes = CC.edge_planes(S, Wp)
    order = np.array([11, 0, 9, 13, 7, 1, 2, 3, 10, 4, 5, 12, 6, 8, 0], np.int32)       # (slot 0 twice: a record per append entry)
    _fmt, spans = CC.format_spans(planes)
    slab_bytes = int(max(spans.max(), CC.pad16(spans[order].sum() // 3)))
    with planes_store(planes, order, slab_bytes) as st:
        fmt, spans = CC.check_store_against_the_definition(st, planes, order, slab_bytes)
        have, by = st.stats(), st.format_stats()
        assert have.slabs >= 3 and have.records == len(order) and have.stored_bytes == int(spans[order].sum())
        assert by.format == 1 and by.rows_records == 3 and by.compact_records == len(order) - 3
        assert by.rows_bytes == int(spans[order][fmt[order] == 0].sum()) and by.compact_bytes == int(spans[order][fmt[order] == 1].sum())
        assert have.inflated_bytes == len(order) * 3 * S * Wp
    # the same planes in a rows store keep today's bytes
    with planes_store(planes, order, 1 << 20, "rows") as st:
        fmt, spans = CC.check_store_against_the_definition(st, planes, order, 1 << 20)
        assert not fmt.any() and st.format_stats().compact_records == 0 and st.format_stats().format == 0


@pytest.mark.parametrize("which", ["45 records", "hand-made", "edges"])
def test_packed_bytes_of_records_equal_the_numpy_statement(recs, which):
    records = {"45 records": recs, "hand-made": hand_made_records(), "edges": CC.edge_records()}[which]
    planes = CC.record_planes(records)
    _fmt, spans = CC.format_spans(planes)
    slab_bytes = int(2 * spans.max())
    with records_store(records, slab_bytes) as st:
        CC.check_store_against_the_definition(st, planes, np.arange(len(records)), slab_bytes)
        assert st.stats().slabs >= (3 if which == "45 records" else 1) and st.stats().stored_bytes == int(spans.sum())
        assert st.stats().inflated_bytes == len(records) * records.dtype.itemsize


# ---- the budget --------------------------------------------------------------------------------------------------------------
def test_the_exact_budget_fits_and_one_byte_short_is_refused_in_compact_spans(recs):
    planes = CC.record_planes(recs)
    _fmt, spans = CC.format_spans(planes)
    need = int(spans.sum())
    assert need < int(CC.rows_span(kept_definition(recs), W).sum())
    with records_store(recs, 1 << 16, capacity=need) as st:
        assert st.stats().stored_bytes == need and st.stats().records == N
    buf, offs, item = inflated(recs), plane_offsets(recs.dtype), recs.dtype.itemsize
    first = int(spans[:16].sum())
    with RecordStore(W, STORED, N, first + int(spans[16:24].sum()) - 1, 1 << 16, device=-1, record_format="compact") as st:
        st.pack_host(buf, item, offs, np.arange(16), np.arange(16))
        state = [st.record(i) + st.record_span(i) for i in range(16)]
        with pytest.raises(StoreFull, match=r"capacity of %d bytes would be exceeded: it holds 16 records in %d bytes, and 7 of the 8 records"
                                            % (st.capacity_bytes, first)):
            st.pack_host(buf, item, offs, np.arange(16, 24), np.arange(16, 24))
        s = st.stats()
        assert (s.refused_fit_records, s.refused_fit_bytes) == (7, first + int(spans[16:23].sum()))
        assert (s.records, s.stored_bytes) == (16, first) and [st.record(i) + st.record_span(i) for i in range(16)] == state
        assert st.format_stats().compact_records + st.format_stats().rows_records == 16
        st.pack_host(buf, item, offs, np.arange(16, 23), np.arange(16, 23))        # what fits still goes in
        assert st.stats().records == 23 and st.stats().stored_bytes == first + int(spans[16:23].sum())


# ---- the gather --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gzip_file(tmp_path_factory, recs):
    path = str(tmp_path_factory.mktemp("train_cache_compact") / "gzip4.hdf")
    hdf5io.write_candidates(path, recs)
    return path


@pytest.mark.parametrize("use_q,use_strand", [(True, True), (False, True), (True, False), (False, False)])
def test_the_gather_from_a_compact_store_equals_the_rows_store_and_the_host_definition(recs, gzip_file, use_q, use_strand):
    from tests.test_train_cache_host import plan_of
    with records_store(recs, 1 << 16) as st, records_store(recs, 1 << 16, "rows") as rows:
        assert st.format_stats().compact_records == N and rows.format_stats().rows_records == N
        for epoch in (0, 1):
            seed = draw_seed(epoch)
            for idx in index_lists():
                plan = plan_of(recs, idx, seed)
                first = np.ascontiguousarray(plan.first_rows, np.uint8)
                args = (plan.slots, None if first.all() else plan.rows, first, READS, (plan.ref, plan.ref_mask, plan.var_mask), use_q, use_strand)
                got, want = st.assemble_host(*args), rows.assemble_host(*args)
                for name, x, y in zip(PLANES, got, want):
                    assert x.dtype == np.uint8 and x.shape == y.shape and x.tobytes() == y.tobytes(), (name, idx)
                if use_q and use_strand:
                    for name, x, y in zip(PLANES, got, host_definition(gzip_file, idx, seed)[0]):
                        assert x.tobytes() == y.tobytes(), (name, idx)


@pytest.mark.parametrize("which", ["hand-made", "edges"])
@pytest.mark.parametrize("use_q,use_strand", [(True, True), (False, True), (True, False), (False, False)])
def test_the_gather_writes_zeros_outside_the_spans_and_for_rows_that_were_not_kept(which, use_q, use_strand):
    """The hand plans (rows >= kept in every position, first rows with kept <, = and > the rows read) over the hand-made records,
    and over the edge records (a mixed store: three of them fell back), against the numpy assembly of the untrimmed records."""
    records = hand_made_records() if which == "hand-made" else CC.edge_records()
    n = len(records)
    with records_store(records, 1 << 16) as st, records_store(records, 1 << 16, "rows") as rows:
        assert st.format_stats().rows_records == (0 if which == "hand-made" else 3)
        for plan in hand_plans():
            if which == "edges":
                plan.slots[:] = (plan.slots * 5 + 9) % n                   # (sites over compact and fallback records alike)
            got = st.assemble_host(plan.slots, plan.rows, plan.first_rows, READS, (plan.ref, plan.ref_mask, plan.var_mask), use_q, use_strand)
            want = assemble_host(records["single_reads"], records["q-scores"], records["strand"], plan, use_q, use_strand)
            also = rows.assemble_host(plan.slots, plan.rows, plan.first_rows, READS, (plan.ref, plan.ref_mask, plan.var_mask), use_q, use_strand)
            for name, x, y, z in zip(PLANES, got, want, also):
                assert x.tobytes() == y.tobytes() == z.tobytes(), name
            got = st.assemble_host(plan.slots, None, None, READS, (plan.ref, plan.ref_mask, plan.var_mask), use_q, use_strand)
            plan.first_rows[:] = 1
            want = assemble_host(records["single_reads"], records["q-scores"], records["strand"], plan, use_q, use_strand)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(got, want))


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_set_format_refusals(recs):
    with RecordStore(255, 4, 2, 1 << 20, 1 << 16, device=-1, record_format="compact") as st:
        assert st.format_stats().format == 1                               # W = 255 is accepted
    for wide in (256, 300):
        with pytest.raises(ValueError, match="a window of %d columns exceeds its 255" % wide):
            RecordStore(wide, 4, 2, 1 << 20, 1 << 16, device=-1, record_format="compact")
        with RecordStore(wide, 4, 2, 1 << 20, 1 << 16, device=-1) as st:   # (the rows format has no such limit)
            assert st.format_stats().format == 0
    with pytest.raises(ValueError, match="record_format must be one of rows, compact"):
        RecordStore(W, STORED, N, 1 << 20, 1 << 16, device=-1, record_format="dense")
    with RecordStore(W, STORED, N, 1 << 30, 1 << 16, device=-1) as st:
        for bad in (2, -1):
            with pytest.raises(ValueError, match=r"format %d: 0 \(rows\) or 1 \(compact\)" % bad):
                st.set_format(bad)
        st.set_format("compact")
        st.set_format("rows")                                              # before the first append it may still change
        st.pack_host(inflated(recs), recs.dtype.itemsize, plane_offsets(recs.dtype), [3], [3])
        with pytest.raises(ValueError, match="the store holds records already: the format is chosen before the first append"):
            st.set_format("compact")
        assert st.format_stats().format == 0 and st.record_span(3)[0] == 0
        with pytest.raises(ValueError, match="record 4 is not in the store"):
            st.record_span(4)
        with pytest.raises(ValueError, match="record %d of %d" % (N, N)):
            st.record_span(N)
    lib = chunk_loader.load_library()
    assert lib.cl_store_set_format(None, 1) == -1 and lib.cl_store_get_format_stats(None, None) == -1
    assert lib.cl_store_record_span(None, 0, None, None) == -1


def _main(argv):
    import sys
    sys.path.insert(0, ROOT)
    import main as cli
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    return str(e.value)


BASE = ["--model_pool_combine_dimension", "0", "--sample_vcf", "c.vcf"]
TRAIN = ["--train_file", "t.hdf", "--test_file", "v.hdf"]


def test_the_flag_parses_and_leaves_no_trace_when_absent():
    from arguments import create_arg_parser, parse_args
    on = ["--train-loader-device", "gpu", "--train-cache-device", "gpu"]
    assert parse_args(BASE + TRAIN + on + ["--train-cache-format", "compact"]).train_cache_format == "compact"
    assert parse_args(BASE + TRAIN + on + ["--train-cache-format", "rows"]).train_cache_format == "rows"
    plain = parse_args(BASE + TRAIN + on)
    assert not hasattr(plain, "train_cache_format") and "train_cache_format" not in repr(plain)
    text = re.sub(r"\s+", " ", create_arg_parser().format_help())
    assert "--train-cache-format" in text and "token and strand merged into one byte" in text


def test_the_command_line_refusals_name_their_reason():
    on = ["--train-loader-device", "gpu"]
    why = _main(BASE + TRAIN + on + ["--train-cache-format", "compact"])
    assert "--train-cache-format is the record format of --train-cache-device gpu, which is not given" in why
    why = _main(BASE + TRAIN + on + ["--train-cache-device", "gpu", "--train-cache-format", "dense"])
    assert "--train-cache-format must be rows or compact" in why
    why = _main(BASE + TRAIN + on + ["--train-cache-device", "gpu", "--train-cache-format", ""])
    assert "--train-cache-format must be rows or compact" in why
    # the older refusals keep their texts with the flag beside them
    why = _main(BASE + TRAIN + on + ["--train-cache-bytes", "1000", "--train-cache-format", "compact"])
    assert "--train-cache-bytes is the budget of --train-cache-device gpu, which is not given" in why
    why = _main(BASE + TRAIN + ["--train-cache-device", "gpu", "--train-cache-format", "compact"])
    assert "it needs that option" in why


def test_make_training_data_sh_prints_the_flag_as_an_option(tmp_path):
    out = tmp_path / "out"
    (out / "isec").mkdir(parents=True)
    for name in ("candidates.vcf", "isec/0001.vcf", "isec/0002.vcf", "isec/0003.vcf"):
        (out / name).write_text("##fileformat=VCFv4.2\n")
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "make_training_data.sh"), "-i", "x.bam", "-r", "ref.fa", "-t", "truth.vcf", "-o", str(out),
                        "-n"], capture_output=True, text=True)
    assert r.returncode == 0 and "--train-cache-device gpu [--train-cache-format compact]" in r.stdout, (r.stdout, r.stderr)


def test_header_exports_and_bindings_agree_on_the_new_entries(lib):
    new = {"cl_store_set_format", "cl_store_record_span", "cl_store_get_format_stats", "cl_store_spans_host", "cl_store_spans_planes_host"}
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dl4vc_chunks.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(cl_store_[a-z_]+)\s*\(", text))
    assert new <= declared and new <= set(chunk_loader.CL_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", pileup_gpu.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert new <= {l.split()[-1] for l in out.splitlines() if l.split()}
    kinds = {"int64_t": C.c_int64, "uint64_t": C.c_uint64, "int32_t": C.c_int32}
    for fn in sorted(new):
        decl = re.search(r"int %s\((.*?)\);" % fn, text, flags=re.S).group(1)
        params = [re.sub(r"\s+", " ", p.strip()) for p in decl.split(",")]
        have = getattr(lib, fn).argtypes
        assert len(have) == len(params), fn
        for p, t in zip(params, have):
            assert (t is C.c_void_p or issubclass(t, C._Pointer)) if "*" in p else t is kinds[p.split()[0]], (fn, p)
    a = re.search(r"int cl_store_spans_host\((.*?)\);", text, flags=re.S).group(1).split("const int32_t* slots")[1]
    b = re.search(r"int cl_store_spans_planes_host\((.*?)\);", text, flags=re.S).group(1).split("const int32_t* slots")[1]
    assert re.sub(r"\s+", " ", a) == re.sub(r"\s+", " ", b)
    body = re.search(r"typedef struct \{([^}]*)\} cl_store_format_stats;", text, flags=re.S).group(1)
    names = [n.strip() for decl in re.findall(r"(?:int64_t|double)\s+([a-z_, ]+);", body) for n in decl.split(",")]
    assert names == [f[0] for f in chunk_loader.StoreFormatStats._fields_]
    # cl_store_stats keeps its layout
    assert [f[0] for f in chunk_loader.StoreStats._fields_] == ["records", "stored_bytes", "inflated_bytes", "slabs", "refused_fit_records",
                                                                "refused_fit_bytes", "extent_ms", "pack_ms", "assemble_ms"]


# ---- the sanitizer pass ------------------------------------------------------------------------------------------------------
def test_the_compact_twins_run_clean_under_the_sanitizers():
    """tools/asan_store_compact.sh: a stand-alone program, every buffer ending where its data ends."""
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "asan_store_compact.sh")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "asan_store_compact: ok" in r.stdout


# ---- sizes -------------------------------------------------------------------------------------------------------------------
def test_the_bytes_of_a_synthetic_30x_pileup_in_both_formats(tmp_path):
    """143 records of the Python builder over a 12-kbp instance of tools/score_bam_rate.py's inputs (every eighth location): the
    compact store's bytes equal the sum of the numpy statement's spans.  Bytes per record in both formats are printed, no ratio
    is a bar."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from score_bam_rate import make_inputs
    from dl4vc_amd.location_round import default_encoder_options
    from dl4vc_amd.pileup_encoder import encode_locations, locations_from_vcf
    bam, fa, vcf, n_loc = make_inputs(str(tmp_path), 12000)
    locations = locations_from_vcf(vcf, 2)[::8]
    records, none = encode_locations(bam, fa, locations, default_encoder_options(), native=False)
    assert len(records) == 143 and none == 0
    planes = CC.record_planes(records)
    S, Wp = planes[0].shape[1:]
    kept, cells, mergeable, _ = CC.spans_definition(planes)
    assert mergeable.all()
    sizes = {}
    for record_format in ("rows", "compact"):
        with planes_store(planes, np.arange(len(records), dtype=np.int32), 1 << 24, record_format) as st:
            sizes[record_format] = st.stats().stored_bytes
            assert st.stats().stored_bytes == int(CC.format_spans(planes, record_format)[1].sum())
    assert sizes["rows"] == int(CC.rows_span(kept, Wp).sum()) and sizes["compact"] == int(CC.compact_span(kept, cells).sum())
    inside = sum(int(cells[i]) for i in range(len(records)))
    zeros = sum(int(((planes[0][i] | planes[1][i] | planes[2][i]) == 0)[:kept[i]].sum()) - (int(kept[i]) * Wp - int(cells[i]))
                for i in range(len(records)))
    print("\n%d records of %d x %d, %.1f kept rows each: rows %.0f bytes a record, compact %.0f bytes a record; largest token %d, strand %d, "
          "quality %d; %.4f %% of the cells inside a span are zero"
          % (len(records), S, Wp, kept.mean(), sizes["rows"] / len(records), sizes["compact"] / len(records), planes[0].max(),
             planes[2].max(), planes[1].max(), 100.0 * zeros / max(1, inside)))

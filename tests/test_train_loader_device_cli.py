"""``--train-loader-device gpu`` where no device is needed: what the command line refuses, the new entries in the headers against
the exports and the bindings, ``cl_center_counts_host`` against ``alleles.count_center_support``, and the host definition of the
device training loader (tests/train_loader_device_cases.py) against ``assemble_training_batch`` byte for byte."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from dl4vc_amd import alleles, capi, chunk_loader, hdf5io, pileup_gpu, vocab as V
from tests.loader_device_cases import chunk_written, create_dataset, write_chunks
from tests.train_loader_device_cases import (BLACK, DEEP, N, NO_READ, READS, STORED, assert_equals_reference, draw_seed, host_definition,
                                             index_lists, labelled_records, reference_batch)


@pytest.fixture(scope="module", autouse=True)
def lib():
    if not pileup_gpu.available() or not os.path.isfile(capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return chunk_loader.load_library()


def _main(argv):
    import sys
    sys.path.insert(0, ROOT)
    import main as cli
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    return str(e.value)


BASE = ["--model_pool_combine_dimension", "0", "--sample_vcf", "c.vcf"]


def test_the_flag_parses():
    from arguments import parse_args
    args = parse_args(BASE + ["--train_file", "t.hdf", "--test_file", "v.hdf", "--train-loader-device", "gpu", "--num-data-workers", "5"])
    assert args.train_loader_device == "gpu" and args.num_data_workers == 5
    assert parse_args(BASE + ["--train_file", "t.hdf", "--test_file", "v.hdf"]).train_loader_device is None


def test_refusals_name_their_reason():
    train = ["--train_file", "t.hdf", "--test_file", "v.hdf"]
    assert "--train-loader-device must be gpu" in _main(BASE + train + ["--train-loader-device", "cpu"])
    assert "--train-loader-device must be gpu" in _main(BASE + train + ["--train-loader-device", ""])
    why = _main(BASE + ["--modelload", "c.pt", "--test_file", "v.hdf", "--train-loader-device", "gpu"])
    assert "option of --train_file" in why and "--loader-device gpu" in why
    # the inference option keeps its meaning, its refusal of --train_file and its texts
    why = _main(BASE + ["--modelload", "c.pt"] + train + ["--loader-device", "gpu"])
    assert "--loader-device gpu is an inference option: training and its evaluation keep the host loaders" in why
    assert "--loader-device must be gpu" in _main(BASE + ["--modelload", "c.pt", "--test_file", "x.hdf", "--loader-device", "cpu"])


def test_files_the_device_loader_refuses_are_refused_with_its_texts(tmp_path):
    """Before any device is touched: not chunked, filters other than deflate alone, a model that reads more rows than the file
    stores -- for the training file and for the test file."""
    from dl4vc_amd import synth
    recs = synth.make_labelled_records(16, 100, 900)                 # (main.py's model reads 100 rows: the production layout)
    good, flat, shuf, few = (str(tmp_path / n) for n in ("good.hdf", "flat.hdf", "shuffle.hdf", "few_rows.hdf"))
    hdf5io.write_candidates(good, recs)
    create_dataset(flat, recs, chunked=False, shuffle=False)
    create_dataset(shuf, recs, chunked=True, shuffle=True)
    hdf5io.write_candidates(few, labelled_records(16))
    flag = ["--train-loader-device", "gpu"]
    why = _main(BASE + flag + ["--train_file", flat, "--test_file", good])
    assert why.startswith("--train-loader-device gpu: ") and "is not chunked" in why
    why = _main(BASE + flag + ["--train_file", good, "--test_file", shuf])
    assert "--train-loader-device gpu: " in why and "has the filters [2, 1], not deflate alone" in why
    why = _main(BASE + flag + ["--train_file", good, "--test_file", few])
    assert "the model reads 100 rows per site but %s stores only %d" % (few, STORED) in why


def test_a_window_other_than_201_is_refused(tmp_path):
    """By ``check_layout`` and, with the same text, by the command line."""
    from dl4vc_amd.hdf5_schema import record_dtype
    path = str(tmp_path / "narrow.hdf")
    hdf5io.write_candidates(path, np.zeros(8, record_dtype(STORED, 101)))
    with hdf5io.RawChunkFile(path) as f:
        with pytest.raises(ValueError, match="holds windows of 101 columns"):
            chunk_loader.check_layout(f, READS)
    why = _main(BASE + ["--train-loader-device", "gpu", "--train_file", path, "--test_file", path])
    assert why.startswith("--train-loader-device gpu: ") and "holds windows of 101 columns" in why and "201-column window" in why


def test_a_libhdf5_without_read_chunk_is_refused(tmp_path, monkeypatch):
    """The refusal of ``RawChunkFile`` for HDF5 older than 1.10.3, through the command line."""
    class Older:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            if name == "H5Dread_chunk":
                raise AttributeError(name)
            return getattr(self._lib, name)

    path = str(tmp_path / "good.hdf")
    hdf5io.write_candidates(path, labelled_records(8))
    bind = hdf5io._chunk_api
    monkeypatch.setattr(hdf5io, "_chunk_api", lambda lib: Older(bind(lib)))
    why = _main(BASE + ["--train-loader-device", "gpu", "--train_file", path, "--test_file", path])
    assert why.startswith("--train-loader-device gpu: ") and "this libhdf5 has no H5Dread_chunk" in why


def test_candidate_file_reads_the_row_count_the_item_size_implies(tmp_path):
    """``CandidateFile`` knew six stored row counts; the small files of these tests store 20."""
    recs = labelled_records(11)
    path = str(tmp_path / "rows20.hdf")
    hdf5io.write_candidates(path, recs)
    with hdf5io.CandidateFile(path) as f:
        assert f.dtype == recs.dtype and len(f) == 11 and f.read(0, 11).tobytes() == recs.tobytes()
    odd = np.zeros(3, np.dtype([("name", "S16"), ("pad", np.uint8, (recs.dtype.itemsize - 16 + 7,))]))
    hdf5io.write_candidates(str(tmp_path / "odd.hdf"), odd)
    with pytest.raises(ValueError, match="unrecognised record layout"):
        hdf5io.CandidateFile(str(tmp_path / "odd.hdf"))


def test_header_exports_and_bindings_agree_on_the_new_entries(lib):
    from dl4vc_amd import train
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dl4vc_chunks.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(cl_[a-z_]+)\s*\(", text))
    assert {"cl_center_counts_device", "cl_center_counts_host"} <= declared == set(chunk_loader.CL_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", pileup_gpu.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {l.split()[-1] for l in out.splitlines() if l.split() and l.split()[-1].startswith("cl_")} == declared
    params = {}
    for fn in ("cl_center_counts_device", "cl_center_counts_host"):
        decl = re.search(r"int %s\((.*?)\);" % fn, text, flags=re.S).group(1)
        params[fn] = [re.sub(r"\s+", " ", p.strip()) for p in decl.split(",")]
        assert [C.c_void_p if "*" in p else C.c_int64 if p.startswith("int64_t") else C.c_int32 for p in params[fn]] == getattr(lib, fn).argtypes
    assert params["cl_center_counts_device"] == params["cl_center_counts_host"]      # (the CPU definition takes the same arguments)
    # the training ABI: _begin_device is _begin's argument list and an event
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dl4vc_dan_train.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(dan_train_[a-z_]+)\s*\(", text)) == set(train.TRAIN_SYMBOLS) and "dan_train_backward_begin_device" in train.TRAIN_SYMBOLS
    args = {fn: [re.sub(r"\s+", " ", p.strip()) for p in re.search(r"int %s\((.*?)\);" % fn, text, flags=re.S).group(1).split(",")]
            for fn in ("dan_train_backward_begin", "dan_train_backward_begin_device")}
    assert args["dan_train_backward_begin_device"] == args["dan_train_backward_begin"] + ["void* ready_event"]
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "dan_train_backward_begin_device" in {l.split()[-1] for l in out.splitlines() if l.split()}
    dan = train._bind(capi.load_library())
    assert dan.dan_train_backward_begin_device.argtypes == dan.dan_train_backward_begin.argtypes + [C.c_void_p]


def test_center_counts_host_equals_count_center_support():
    """Planes holding every token 0..9 and bytes above 15 in columns 100 and 101, for the three variant modes and every reference
    token at the counted column."""
    rng = np.random.default_rng(8)
    m, R = 12, 37
    reads = rng.integers(0, 10, (m, R, 201)).astype(np.uint8)
    pool = np.array(list(range(10)) + [16, 17, 200, 255], np.uint8)
    reads[:, :, 100:102] = pool[rng.integers(0, len(pool), (m, R, 2))]
    for c in (100, 101):
        assert set(range(10)) <= set(reads[:, :, c].ravel().tolist()) and (reads[:, :, c] > 15).any()
    reads[3, :, 100:102] = 255                                       # a site where nothing is counted
    counts = chunk_loader.center_counts_host(reads)
    assert counts.shape == (m, 2, 16) and counts.dtype == np.int32 and not counts[3].any()
    for i in range(m):
        for k in (0, 1):
            assert (counts[i, k] == np.bincount(reads[i, :, 100 + k], minlength=256)[:16]).all()
        ref = rng.integers(0, 10, 201).astype(np.uint8)
        for mode in (V.MUTATION_SNP, V.MUTATION_DELETE, V.MUTATION_INSERT):
            for tok in range(10):
                ref[100:102] = tok
                assert alleles.center_support_from_counts(counts[i], ref, mode) == \
                    alleles.count_center_support(np.ascontiguousarray(reads[i].T), ref, mode), (i, mode, tok)
    h = np.zeros((1, 2, 16), np.int32)
    assert lib_call(reads[:1], 1, 0, 201, h) == -1 and lib_call(reads[:1], 1, 4, 2, h) == -1 and lib_call(reads[:1], -1, 4, 201, h) == -1
    assert lib_call(None, 1, 4, 201, h) == -1 and b"null argument" in chunk_loader.load_library().cl_last_error(None)
    assert lib_call(None, 0, 4, 201, None) == 0


def lib_call(reads, m, rows, window, out):
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None   # noqa: E731
    return chunk_loader.load_library().cl_center_counts_host(None, p(reads), m, rows, window, p(out), None)


def test_plan_records_is_plan_sites_with_the_sites_named():
    """``plan_sites`` keeps its behaviour: it is ``plan_records`` on the slots its status array selects, seeded with
    ``first_record + i``."""
    from dl4vc_amd.site_assembly import plan_records, plan_sites
    recs = labelled_records()
    status = np.ones(N, np.int8)
    status[[4, 20]] = 0
    texts = [bytes(v).decode() for v in recs["vcfrec"]]
    a = plan_sites(status, recs["num_reads"], recs["ref_bases"], texts, READS, STORED, 9, first_record=100)
    slots = np.flatnonzero(status == 1)
    b = plan_records(slots, 100 + np.arange(len(slots)), recs["num_reads"], recs["ref_bases"], texts, READS, STORED, 9)
    for f in ("slots", "rows", "first_rows", "ref", "ref_mask", "var_mask", "num_reads", "blacklist"):
        assert (getattr(a, f) == getattr(b, f)).all(), f
    assert a.vcfrec == b.vcfrec and (a.first_rows == 0).sum() == len(DEEP)
    with pytest.raises(ValueError, match="record indices for"):
        plan_records(slots, np.arange(3), recs["num_reads"], recs["ref_bases"], texts, READS, STORED, 9)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("train_loader_device")
    recs = labelled_records()
    hdf5io.write_candidates(str(d / "gzip4.hdf"), recs)
    chunk_written(str(d / "fixed.hdf"), recs, "fixed")
    write_chunks(str(d / "raw.hdf"), recs, raw=(2,))
    return {"libhdf5 gzip 4": str(d / "gzip4.hdf"), "ChunkWriter fixed": str(d / "fixed.hdf"), "a raw chunk": str(d / "raw.hdf")}


def test_the_fixture_holds_deep_empty_and_blacklisted_sites(files):
    want = reference_batch(files["libhdf5 gzip 4"], np.arange(N), draw_seed(0))
    nr = want.sites.num_reads
    assert (nr > READS).sum() == len(DEEP) and nr[NO_READ] == 0 and want.blacklist[BLACK] and want.blacklist.sum() < 10
    assert len(set(want.targets["label"].tolist())) > 1 and len(set(want.targets["var_type"].tolist())) > 1
    # the second epoch's seed draws other subsets of the deep sites
    other = reference_batch(files["libhdf5 gzip 4"], np.arange(N), draw_seed(1))
    assert any((want.sites.reads[i] != other.sites.reads[i]).any() for i in DEEP)


@pytest.mark.parametrize("epoch", [0, 1])
@pytest.mark.parametrize("kind", ["libhdf5 gzip 4", "ChunkWriter fixed", "a raw chunk"])
def test_host_definition_equals_assemble_training_batch(files, kind, epoch):
    """The six planes, every target array bitwise, blacklist, index and record text, for every index list of the issue."""
    seed = draw_seed(epoch)
    for idx in index_lists():
        assert_equals_reference(host_definition(files[kind], idx, seed), reference_batch(files[kind], idx, seed), idx)


def test_counted_allele_fraction_equals_the_host_loaders(files):
    """``keep_candidate_af=False``: the allele frequency is the counted variant fraction, which only the histogram gives."""
    path = files["libhdf5 gzip 4"]
    for idx in index_lists()[:2]:
        want = reference_batch(path, idx, draw_seed(1), keep_candidate_af=False)
        assert_equals_reference(host_definition(path, idx, draw_seed(1), keep_candidate_af=False), want, idx)
    kept = reference_batch(path, index_lists()[0], draw_seed(1))
    assert (kept.targets["allele_freq"] != reference_batch(path, index_lists()[0], draw_seed(1), keep_candidate_af=False).targets["allele_freq"]).any()

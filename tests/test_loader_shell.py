"""libdl4vc_loader.so on the shared C-ABI shell: what the native loader refuses (a chunk that holds fewer bytes than the piece
takes from it, a record type whose fields do not fit the record), what the native pileup encoder refuses through the one BAM
framing core, and that a loader closed without being read leaves no thread behind.  CPU only; 24 records of 15 425 bytes in
chunks of 8 (tests/loader_shell_cases.py), 1 and 3 worker threads, batches of 8 from record 0 and from record 4, where every
piece straddles two chunks."""
import os
import subprocess

import numpy as np
import pytest

import loader_shell_cases as CASES
from dl4vc_amd import loader
from dl4vc_amd.dataset import assemble_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANES = ("reads", "qual", "strand", "ref", "ref_mask", "var_mask", "num_reads")
RUNS = [(threads, lo) for threads in (1, 3) for lo in (0, 4)]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    if not loader.available():
        import __graft_entry__ as g
        g.build()
    d = str(tmp_path_factory.mktemp("loader_shell"))
    CASES.write_all(d)
    recs = CASES.make_records()
    want = {lo: assemble_batch(recs[lo:], CASES.READS) for lo in (0, 4)}
    return d, want


def delivered(path, threads, lo):
    """The batches a loader yields before it ends or fails -> (batches, the error or None)."""
    got = []
    with loader.NativeLoader(path, reads=CASES.READS, batch_sites=8, lo=lo, threads=threads) as nl:
        try:
            for b in nl:
                got.append(b)
        except ValueError as e:
            return got, e
    return got, None


def assert_prefix_of(got, want):
    n = sum(len(b) for b in got)
    for k in PLANES:
        have = np.concatenate([getattr(b, k) for b in got]) if got else getattr(want, k)[:0]
        np.testing.assert_array_equal(have, getattr(want, k)[:n], err_msg=k)
    assert sum((b.vcfrec for b in got), []) == want.vcfrec[:n]
    return n


@pytest.mark.parametrize("threads,lo", RUNS)
def test_an_intact_file_loads_as_the_python_assembly(files, threads, lo):
    d, want = files
    got, err = delivered(os.path.join(d, "intact.hdf"), threads, lo)
    assert err is None and assert_prefix_of(got, want[lo]) == CASES.N - lo


@pytest.mark.parametrize("threads,lo", RUNS)
def test_a_chunk_that_inflates_short_is_refused_by_name(files, threads, lo):
    """Chunk 1 inflates to its first record.  The inflate buffer is reused from chunk to chunk, so at ``lo`` 4 the bytes behind
    that record are chunk 0's records: nothing past record 7 may be delivered, and what is delivered is the file's."""
    d, want = files
    got, err = delivered(os.path.join(d, "short_inflate.hdf"), threads, lo)
    assert err is not None and "chunk 1 holds 15425 bytes once inflated" in str(err), err
    assert ("needs %d" % (15425 * (8 if lo == 0 else 4))) in str(err)
    assert assert_prefix_of(got, want[lo]) == (8 if lo == 0 else 0)


@pytest.mark.parametrize("case", ["truncated", "too_long"])
def test_a_cut_stream_and_a_stream_too_long_are_refused_as_before(files, case):
    d, want = files
    for threads, lo in RUNS:
        got, err = delivered(os.path.join(d, case + ".hdf"), threads, lo)
        assert err is not None and "zlib inflate failed" in str(err), (case, threads, lo, err)
        assert assert_prefix_of(got, want[lo]) == (8 if lo == 0 else 0)


@pytest.mark.parametrize("threads,lo", RUNS)
def test_a_short_unfiltered_chunk_is_refused_not_read_past_its_end(files, threads, lo):
    d, want = files
    got, err = delivered(os.path.join(d, "short_raw.hdf"), threads, lo)
    assert err is not None and "chunk 1 holds 15425 bytes, the piece needs" in str(err), err
    assert assert_prefix_of(got, want[lo]) == (8 if lo == 0 else 0)


@pytest.mark.parametrize("case", CASES.LAYOUT_CASES)
def test_a_record_type_whose_fields_leave_the_record_is_refused_at_open(files, case):
    d, _ = files
    with pytest.raises(OSError, match="unexpected record layout"):
        loader.NativeLoader(os.path.join(d, case + ".hdf"), reads=CASES.READS, batch_sites=8, threads=1)


@pytest.mark.parametrize("threads", [1, 3])
def test_a_bam_record_without_a_name_is_refused_by_the_framing_core(files, threads):
    d, _ = files
    bam, fa = (os.path.join(d, "l_read_name_zero." + e) for e in ("bam", "fa"))
    with loader.NativePileupEncoder(bam, fa, 16, 50, 10, 50) as enc:
        with pytest.raises(RuntimeError, match=r"corrupt BAM record \(l_read_name\)"):
            enc.encode(*CASES.BAM_QUERY, threads)


def test_loaders_closed_unread_leave_no_thread_behind(files):
    d, _ = files
    threads_now = lambda: len(os.listdir("/proc/self/task"))   # noqa: E731
    before = threads_now()
    for _ in range(50):
        loader.NativeLoader(os.path.join(d, "intact.hdf"), reads=CASES.READS, batch_sites=8, threads=4).close()
    assert threads_now() == before


def test_the_loader_library_runs_clean_under_the_sanitizers():
    """tools/asan_loader.sh: a stand-alone program over the files above, the damaged ones included."""
    r = subprocess.run(["bash", os.path.join(ROOT, "tools", "asan_loader.sh")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "asan_loader: ok" in r.stdout

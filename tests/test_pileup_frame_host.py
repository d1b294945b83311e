"""The framing of the GPU pileup encoder's device inflate path, on the CPU: ``pg_debug_run_records`` runs the host path
(``fetch_run``) and the CPU twin of the device path (index ranges, the host form of the inflate, the shared frame core) over
the same runs and must give the same records.  No GPU.  ``DL4VC_PILEUP_HOST_LIB``: another build of the entry point
(tools/asan_pileup_frame.sh sets it to the sanitizer build)."""
import ctypes
import os

import pytest

from dl4vc_amd import pileup_gpu
from tests import pileup_inflate_cases as IC


def _lib():
    alt = os.environ.get("DL4VC_PILEUP_HOST_LIB")
    return ctypes.CDLL(alt) if alt else None


def test_new_symbols_exist():
    lib = _lib() or pileup_gpu.load_library()
    names = ("pg_debug_run_records",) if _lib() else ("pg_set_inflate_device", "pg_get_stats", "pg_debug_run_records")
    assert [n for n in names if not hasattr(lib, n)] == []
    assert _lib() or set(names) <= set(pileup_gpu.SYMBOLS)


@pytest.mark.parametrize("level", [0, 1, 6])
def test_twin_gives_the_host_paths_records_on_the_grid(tmp_path, level):
    bam, _ = IC.grid(tmp_path, level)
    found, longest, n_blocks = IC.straddles(bam)
    assert found >= 1 and longest > 65536 and n_blocks >= 5
    lib, total, shared = _lib(), 0, 0
    wins = IC.windows()
    assert len(wins) >= 12
    for tid, s0, stop in wins:
        host = pileup_gpu.debug_run_records(bam, bam + ".bai", tid, s0, stop, 0, lib)
        twin = pileup_gpu.debug_run_records(bam, bam + ".bai", tid, s0, stop, 1, lib)
        assert twin == host, (tid, s0, stop)
        assert pileup_gpu.debug_run_records(bam, bam + ".bai", tid, s0, stop, 2, lib) == host, (tid, s0, stop)
        total += len(host[0])
        shared += any(r[0] == 100_000 and r[1] == 105_000 for r in host[0])
    assert total > 2500 and shared == 2                    # the 5 000-base read is listed for both of its runs
    # the 20-kb deletion governs max_nref of its run; an empty run; a run over PG_MAX_TRACKS
    assert pileup_gpu.debug_run_records(bam, bam + ".bai", 0, 49_972, 50_009, 1, lib)[1] == 34_000
    assert pileup_gpu.debug_run_records(bam, bam + ".bai", 0, 149_982, 150_019, 1, lib)[0] == []
    assert len(pileup_gpu.debug_run_records(bam, bam + ".bai", 0, IC.DEEP - 18, IC.DEEP + 19, 1, lib)[0]) >= 1100


@pytest.mark.parametrize("kind", IC.DAMAGED)
def test_both_paths_refuse_damaged_input_with_the_message(tmp_path, kind):
    bam, bai, _ = IC.damaged(tmp_path, kind)
    lib = _lib()
    said = []
    for path in (0, 1, 2):
        with pytest.raises(RuntimeError) as e:
            pileup_gpu.debug_run_records(bam, bai, *IC.DAMAGED_WINDOW, path, lib)
        assert IC.EXPECT[kind][min(path, 1)] in str(e.value), (path, str(e.value))
        said.append(str(e.value))
    if kind not in ("crc_flipped", "truncated_bgzf"):      # a refused record: the same text and the same offset on every path
        assert said[0] == said[1] == said[2], said


def test_two_ranges_that_share_a_block(tmp_path):
    """The second run's range begins in the block the first run's range lies in and continues into the next: planned alone
    (path 1) and inside a call that also asks for the first run (path 2, where the blocks come from the call's plan)."""
    bam, _ = IC.shared_block(tmp_path)
    lib = _lib()
    counts = []
    for tid, s0, stop in IC.SHARED_WINDOWS:
        host = pileup_gpu.debug_run_records(bam, bam + ".bai", tid, s0, stop, 0, lib)
        for path in (1, 2):
            assert pileup_gpu.debug_run_records(bam, bam + ".bai", tid, s0, stop, path, lib) == host, (s0, path)
        counts.append(len(host[0]))
    assert counts[0] == 30 and 40 <= counts[1] <= 120

"""The BGZF decode core on the CPU (``bz_inflate_host``, dl4vc_amd/csrc/bgzf_inflate.h): the case grid of tests/bgzf_cases.py
against Python's zlib, and the byte ranges the device path takes from the BAI bins.  No GPU.  ``tools/asan_bgzf.sh`` runs the
same grid through a sanitizer build of the same header."""
import pytest

from dl4vc_amd import bamio, candgen
from dl4vc_amd.vcfpost import reg2bins
from tests import bgzf_cases as G
from tests.candidates_fixture import load, write_bam


def test_grid_is_what_it_says():
    G.check_grid()


def test_valid_cases_equal_zlib():
    cases = G.valid_cases()
    out, out_off, status = G.run(cases, None)
    G.assert_valid(cases, out, out_off, status)


@pytest.mark.parametrize("bad", G.damaged_cases(), ids=lambda c: c.name)
def test_damaged_case_is_a_status(bad):
    G.check_damaged(bad, None)


def test_not_a_block_and_bad_slot_are_statuses():
    good = G.valid_cases()[2]
    junk = G.Case("junk", b"\x1f\x8b\x08\x00" + bytes(40), None, 0)
    import numpy as np
    blob = good.block + junk.block
    out = np.full(good.isize + 10, G.FILL, np.uint8)
    status = candgen.inflate_blocks(blob, [0, len(good.block), len(blob) - 5, 0], out, [0, 0, 0, 11])
    assert status == [G.OK, G.BAD_HEADER, G.BAD_HEADER, G.BAD_SLOT]
    assert out[:good.isize].tobytes() == good.data and (out[good.isize:] == G.FILL).all()
    assert candgen.status_text(G.CRC_MISMATCH) == "CRC mismatch"


def test_ranges_from_the_bins_hold_every_overlapping_record(tmp_path):
    """cg_debug_ranges against BaiIndex.bins and reg2bins computed here: the merged ranges are the merged chunks of the
    overlapping bins (less those that end before the linear index's offset), every record the Python reader finds overlapping
    the region starts inside one, and every walk boundary is a record start or a range end."""
    fx = load("random")
    bam = write_bam(fx, str(tmp_path / "r.bam"))
    idx = bamio.BaiIndex.load(bam + ".bai")
    starts = {}
    with bamio.BamFile(bam, index="") as f:
        f.r.seek(f.first_record)
        while True:
            nx = f._next()
            if nx is None:
                break
            at, rec = nx
            starts[at] = (rec, f.r.tell())
    span = max(r.reference_end for r, _ in starts.values())
    with candgen.CandidateCounter(bam) as cc:
        regions = [(0, 0, span + 10), (0, span // 3, span // 3 + 50), (0, span // 2, span // 2 + 1), (0, span + 100, span + 200)]
        regions += [(t, 0, 1 << 29) for t in range(1, len(cc.references))]
        for tid, s, e in regions:
            ranges, bounds = cc.debug_ranges(tid, s, e)
            min_off = idx.linear_offset(tid, s)
            want = []
            if min_off:
                for b in reg2bins(s, e):
                    want += [c for c in idx.bins[tid].get(b, []) if c[1] > min_off]
            merged = []
            for c in sorted(want):
                if merged and c[0] <= merged[-1][1]:
                    merged[-1] = (merged[-1][0], max(merged[-1][1], c[1]))
                else:
                    merged.append(tuple(c))
            assert ranges == merged, (tid, s, e)
            inside = lambda v: any(a <= v < b for a, b in ranges)
            n = 0
            for at, (rec, end_v) in starts.items():
                if rec.tid == tid and rec.pos < e and rec.reference_end > s:
                    assert inside(at) and any(a < end_v <= b for a, b in ranges), (tid, s, e, at)
                    n += 1
            if (tid, s, e) == regions[0]:
                assert n > 0
            ends = {b for _, b in ranges}
            assert bounds == sorted(bounds)
            for v in bounds:
                assert v in starts or v in ends, (tid, s, e, v)
            for a, b in ranges:
                assert a in bounds and b in bounds


def test_inflate_device_needs_the_index(tmp_path):
    bam = write_bam(load("nochr"), str(tmp_path / "x.bam"), index=False)
    with pytest.raises(RuntimeError, match="needs the BAI index"):
        candgen.CandidateCounter(bam, inflate_device="gpu")
    with pytest.raises(ValueError):
        candgen.CandidateCounter(bam, inflate_device="cpu")

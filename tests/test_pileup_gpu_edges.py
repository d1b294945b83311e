"""The GPU pileup encoder (libdl4vc_pileup.so) on the hand-built grid of tests/pileup_cases.py and on a call of 1 301 locations.

Per location: the GPU's status is ``pe_encode``'s, or 2 where ``expected_decline`` names a reason; where the case says the GPU
encodes, status 1 is required, where it says the GPU declines, status 2; at status 1 all six outputs are byte-equal to
``pe_encode``'s; at status 0 / 2 every byte of the slot is zero (the output buffers are handed over filled with 0xAB, through
``pg_encode`` and ``pg_encode_device``).  tests/test_pileup_edges.py holds ``pe_encode`` itself to the Python builder on the
same grid, without a GPU."""
import ctypes as C

import numpy as np
import pytest

from dl4vc_amd import loader, pileup_gpu
from dl4vc_amd import pileup_encoder as PE
from tests import pileup_cases as PC
from tests.test_pileup_edges import ERRORS, _location, _options

pytestmark = pytest.mark.gpu
FIELDS = ("reads", "qual", "strand", "ref", "num_reads", "status")
FILL = 0xAB


def raw_encode(g, contigs, positions, device=False):
    """``pg_encode`` / ``pg_encode_device`` on output buffers pre-filled with a non-zero byte -> six host arrays."""
    n = len(positions)
    names = (C.c_char_p * max(n, 1))(*[c.encode() for c in contigs])
    pos = np.ascontiguousarray(positions, np.int32)
    ref = np.full((n, g.window), FILL, np.uint8)
    num = np.full(n, 0x2B2B2B2B, np.int32)
    status = np.full(n, 0x2B, np.int8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    if device:
        import torch
        dev = torch.device("cuda", g.device)
        planes = [torch.full((n, g.max_reads, g.window), FILL, dtype=torch.uint8, device=dev) for _ in range(3)]
        torch.cuda.synchronize(dev)
        t = lambda x: C.c_void_p(x.data_ptr() if x.numel() else None)   # noqa: E731
        g._check(g.lib.pg_encode_device(g._h, C.cast(names, C.c_void_p), p(pos), n, t(planes[0]), t(planes[1]), t(planes[2]),
                                        p(ref), p(num), p(status), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
                 "pg_encode_device")
        torch.cuda.synchronize(dev)
        planes = [x.cpu().numpy() for x in planes]
    else:
        planes = [np.full((n, g.max_reads, g.window), FILL, np.uint8) for _ in range(3)]
        g._check(g.lib.pg_encode(g._h, C.cast(names, C.c_void_p), p(pos), n, p(planes[0]), p(planes[1]), p(planes[2]), p(ref),
                                 p(num), p(status)), "pg_encode")
    return planes + [ref, num, status]


def check_against_cpu(want, got, why, labels):
    """The contract, location by location; ``why[i]``: the decline reasons that hold there.  -> number of status-1 locations."""
    ws, gs = want[5], got[5]
    for i in range(len(gs)):
        assert gs[i] == ws[i] or (gs[i] == 2 and why[i]), (labels[i], "cpu %d gpu %d" % (ws[i], gs[i]), why[i])
        if gs[i] == 1:
            for k in range(5):
                assert np.array_equal(got[k][i], want[k][i]), (labels[i], FIELDS[k])
        else:
            for k in range(5):
                assert not np.any(got[k][i]), (labels[i], FIELDS[k], "not zero at status %d" % gs[i])
    return int((gs == 1).sum())


@pytest.mark.parametrize("name", PC.CASE_NAMES)
def test_case_on_the_gpu(tmp_path, name):
    case = PC.get_case(name)
    bam, fa = PC.write_case(tmp_path, case)
    pile = PC.Pileup.of_case(case)
    contigs, pos = [l.contig for l in case.locs], [l.pos for l in case.locs]
    labels = ["%s:%d %s" % (l.contig, l.pos, l.note) for l in case.locs]
    why = [PC.expected_decline(pile, l.contig, l.pos, case.w, case.mbq) for l in case.locs]
    with loader.NativePileupEncoder(bam, fa, *case.options()) as e:
        want = e.encode(contigs, pos, 1)
    assert want[5].tolist() == [l.cpu for l in case.locs]
    with pileup_gpu.GpuPileupEncoder(bam, fa, *case.options()) as g:
        got = raw_encode(g, contigs, pos)
        dev = raw_encode(g, contigs, pos, device=True)
        again = g.encode(contigs, pos)
    check_against_cpu(want, got, why, labels)
    for i, l in enumerate(case.locs):
        if l.must_encode():
            assert got[5][i] == 1, (labels[i], "the GPU must encode this location", int(got[5][i]))
        if l.gpu_declines:
            assert got[5][i] == 2 and why[i], (labels[i], "the GPU must decline this location", int(got[5][i]))
    for k in range(6):
        assert np.array_equal(dev[k], got[k]), ("pg_encode_device", FIELDS[k])
        assert np.array_equal(again[k], got[k]), ("encode", FIELDS[k])
    # the hand-down chain GPU -> pe_encode -> Python builder against native=True
    locs, opt = [_location(l) for l in case.locs], _options(case)
    raises = [l.py for l in case.locs if l.py]
    if raises:
        for i, l in enumerate(case.locs):
            if l.py:
                for kw in (dict(native=True), dict(device="gpu")):
                    with pytest.raises(ERRORS[l.py]):
                        PE.encode_locations(bam, fa, [locs[i]], opt, **kw)
        locs = [x for x, l in zip(locs, case.locs) if not l.py]
    nat, e_nat = PE.encode_locations(bam, fa, locs, opt, native=True)
    gpu, e_gpu = PE.encode_locations(bam, fa, locs, opt, device="gpu")
    assert e_gpu == e_nat and len(gpu) == len(nat) and gpu.tobytes() == nat.tobytes()


def test_zero_length_alignments_are_declined_on_the_device(tmp_path):
    """The kernel draws a track's head column from ``Qp[0]`` and its tail from ``k = nb - 1``: a track without a reference
    position must never reach it (``m.end > m.pos`` in the track filter).  Here such reads are the ONLY reads in the window
    and around it, alone and between ordinary reads."""
    ref = PC.make_ref(600, 5)
    reads = [PC.read(ref, 200, "0M5I", "z1"), PC.read(ref, 205, "5S0D", "z2", PC.FREV), PC.read(ref, 210, "0M", "z3"),
             PC.read(ref, 390, "30M", "a"), PC.read(ref, 400, "0M5I", "z4"), PC.read(ref, 400, "30M", "b", PC.FREV)]
    case = PC.Case("zero_only", [("ref", ref)], reads, [PC.Loc("ref", 206, 2, py="ValueError", gpu_declines=True),
                                                        PC.Loc("ref", 401, 2, py="ValueError", gpu_declines=True),
                                                        PC.Loc("ref", 300, 0)])
    bam, fa = PC.write_case(tmp_path, case)
    pile = PC.Pileup.of_case(case)
    contigs, pos = [l.contig for l in case.locs], [l.pos for l in case.locs]
    with loader.NativePileupEncoder(bam, fa, *case.options()) as e:
        want = e.encode(contigs, pos, 1)
    with pileup_gpu.GpuPileupEncoder(bam, fa, *case.options()) as g:
        got = raw_encode(g, contigs, pos)
    assert want[5].tolist() == [2, 2, 0] and got[5].tolist() == [2, 2, 0]
    check_against_cpu(want, got, [PC.expected_decline(pile, c, p, case.w) for c, p in zip(contigs, pos)], pos)


def test_three_batches_runs_cut_by_gap_and_span_and_one_encoder_called_again(tmp_path):
    """1 301 locations in one call: three device batches (512, 512, 277: an odd count times an odd width in the small-output
    layout), two contigs, runs cut by the gap and by the span limit; sorted, shuffled and with every location listed twice;
    ``encode`` against ``pe_encode``, ``encode_device`` against ``encode``; then a 5-location call, the 1 301 and the 5 again on
    the SAME encoder (buffers regrown, nothing stale)."""
    case, contigs, pos = PC.big_call()
    bam, fa = PC.write_case(tmp_path, case)
    pile = PC.Pileup.of_case(case)
    n = len(pos)
    assert n == 1301
    why = [PC.expected_decline(pile, c, p, case.w) for c, p in zip(contigs, pos)]
    assert not any(why)
    with loader.NativePileupEncoder(bam, fa, *case.options()) as e:
        want = e.encode(contigs, pos, 4)
    assert (want[5] == 1).all()
    rng = np.random.default_rng(17)
    five = [0, 300, 301, 650, 1300]
    with pileup_gpu.GpuPileupEncoder(bam, fa, *case.options()) as g:
        small_first = raw_encode(g, [contigs[i] for i in five], [pos[i] for i in five])
        for order in (np.arange(n), rng.permutation(n), np.repeat(rng.permutation(n), 2)):
            c, p = [contigs[i] for i in order], [pos[i] for i in order]
            w_o = [a[order] for a in want]
            got = raw_encode(g, c, p)
            assert check_against_cpu(w_o, got, [why[i] for i in order], ["%s:%d" % x for x in zip(c, p)]) == len(order)
            dev = raw_encode(g, c, p, device=True)
            for k in range(6):
                assert np.array_equal(dev[k], got[k]), ("pg_encode_device", FIELDS[k])
        small = raw_encode(g, [contigs[i] for i in five], [pos[i] for i in five])
        big = raw_encode(g, contigs, pos)
        small_again = raw_encode(g, [contigs[i] for i in five], [pos[i] for i in five])
    for k in range(6):
        assert np.array_equal(big[k], want[k]), FIELDS[k]
        assert np.array_equal(small[k], want[k][five]) and np.array_equal(small_again[k], small[k]), FIELDS[k]
        assert np.array_equal(small_first[k], small[k]), FIELDS[k]

"""GPU pileup encoder (libdl4vc_pileup.so, ``pg_*``) against the CPU encoder it restates (``pe_encode``), location by location.

The contract: the GPU's status is ``pe_encode``'s status or 2 (declined), never 1 or 0 where ``pe_encode`` says otherwise, and
every status-1 record is byte-equal to ``pe_encode``'s.  ``encode_locations(device="gpu")`` (GPU, then ``pe_encode`` for what
the GPU declines, then the Python encoder for what that declines) gives the bytes and error count of ``native=True``.  A decline
needs a reason: every status 2 must be one ``tests/pileup_cases.py::expected_decline`` explains from the records themselves."""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

from dl4vc_amd import bamio, loader, pileup_gpu
from dl4vc_amd import pileup_encoder as PE
from oracle.gen_golden_pileup import simulate_reads
from tests.candidates_fixture import load, write_bam
from tests.pileup_cases import Pileup, expected_decline
from tests.test_pileup_native import _big_case, write_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
FIELDS = ("reads", "qual", "strand", "ref", "num_reads")


def _both(bam, fa, contigs, pos, w=100, mr=200, mil=10, milv=50, mbq=0):
    with loader.NativePileupEncoder(bam, fa, w, mr, mil, milv, mbq) as e:
        want = e.encode(contigs, pos, 1)
    with pileup_gpu.GpuPileupEncoder(bam, fa, w, mr, mil, milv, mbq) as g:
        got = g.encode(contigs, pos)
    pile = Pileup.of_files(bam, fa)
    why = [expected_decline(pile, c, int(p), w, mbq) if s == 2 else None for c, p, s in zip(contigs, pos, got[5])]
    return want, got, why


def _agree(want, got, why):
    """The contract, location by location -> (locations the GPU encoded, locations pe_encode encoded).  ``why[i]``: the decline
    reasons that hold at a location the GPU gave status 2."""
    ws, gs = want[5], got[5]
    bad = np.flatnonzero((gs != ws) & (gs != 2))
    assert len(bad) == 0, [(int(i), int(ws[i]), int(gs[i])) for i in bad[:10]]
    unexplained = [int(i) for i in np.flatnonzero(gs == 2) if not why[i]]
    assert not unexplained, ("declined without a reason", unexplained[:10])
    one = np.flatnonzero(gs == 1)
    for k, name in enumerate(FIELDS):
        diff = [int(i) for i in one if not np.array_equal(got[k][i], want[k][i])]
        assert not diff, (name, diff[:10])
    return len(one), int((ws == 1).sum())


def test_simulated_pileups(tmp_path):
    """The 40 simulate_reads pileups of tests/test_pileup_native.py: insertions beyond both caps, deletions, soft clips, both
    strands, duplicated names, soft-masked reference, depth above max_reads, windows 100 / 30 / 16, with and without a BAI."""
    gpu = cpu = 0
    for seed in range(40):
        w = [100, 100, 30, 16][seed % 4]
        dup = seed % 10 == 9
        ref, center, reads = simulate_reads(100 + seed, w, [8, 40, 90, 300][seed % 4], duplicate_ids=dup)
        bam, fa = write_inputs(tmp_path, ref, reads, tag="s%d" % seed, index=seed % 2 == 0)
        want, got, why = _both(bam, fa, ["ref"], [center], w, 200, [10, 3, 0][seed % 3], [50, 5, 0][seed % 3])
        g, c = _agree(want, got, why)
        if not dup:
            gpu, cpu = gpu + g, cpu + c
    assert cpu >= 20 and gpu >= 0.9 * cpu, (gpu, cpu)


@pytest.mark.parametrize("index", [True, False])
def test_runs_sorted_shuffled_missing_contig_and_past_the_data(tmp_path, index):
    """The 6-kbp 20x contig (insertions, deletions, duplicate-flagged reads), 150 locations in order and shuffled, a position
    past the contig's end and one on a contig neither file has; through the BAI and by a linear scan."""
    bam, fa, ref = _big_case(tmp_path)
    if not index:
        os.remove(bam + ".bai")
    rng = np.random.default_rng(9)
    pos = np.sort(rng.integers(150, 5850, 150)).tolist() + [5990, 7000, 100]
    contigs = ["chr20"] * (len(pos) - 1) + ["chrX"]
    for order in (np.arange(len(pos)), rng.permutation(len(pos))):
        c, p = [contigs[i] for i in order], [pos[i] for i in order]
        want, got, why = _both(bam, fa, c, p)
        g, n = _agree(want, got, why)
        assert n >= 140 and g >= 0.9 * n, (g, n)
        assert got[5][int(np.flatnonzero(order == len(pos) - 1)[0])] == 0       # chrX
        assert got[5][int(np.flatnonzero(order == len(pos) - 2)[0])] == 0       # past the data


@pytest.mark.parametrize("w,mr", [(100, 40), (30, 20), (16, 200)])
def test_windows_and_depth_above_max_reads(tmp_path, w, mr):
    bam, fa, ref = _big_case(tmp_path, n_reads=2400, length=6000, seed=3)        # ~50x
    pos = list(range(200, 5800, 37))
    want, got, why = _both(bam, fa, ["chr20"] * len(pos), pos, w, mr)
    g, n = _agree(want, got, why)
    assert n >= 0.8 * len(pos) and g >= 0.9 * n, (g, n)
    if mr < 50:
        assert (got[4][got[5] == 1] == mr).any()                                 # deep sites keep their middle rows


def test_duplicate_secondary_unmapped_and_qc_fail_reads(tmp_path):
    ref, center, reads = simulate_reads(7, 100, 200)
    rng = np.random.default_rng(1)
    flags = [0, 0, bamio.FDUP, bamio.FSECONDARY, bamio.FUNMAP, bamio.FQCFAIL, bamio.FSUPPLEMENTARY, bamio.FREVERSE]
    reads = [dataclasses.replace(r, flag=r.flag | int(rng.choice(flags))) for r in reads]
    bam, fa = write_inputs(tmp_path, ref, reads, tag="flags")
    pos = list(range(center - 60, center + 61, 3))
    want, got, why = _both(bam, fa, ["ref"] * len(pos), pos)
    g, n = _agree(want, got, why)
    assert n >= 20 and g >= 0.9 * n, (g, n)


def test_candidates_fixture_bam(tmp_path):
    """The candidate generator's random fixture: two contigs, MD tags, duplicate and secondary reads, every candidate."""
    fx = load("random")
    bam = write_bam(fx, str(tmp_path / "r.bam"))
    rng = np.random.default_rng(3)
    fa = str(tmp_path / "ref.fa")
    with open(fa, "w") as f:
        for name, length in fx["references"]:
            s = "".join(rng.choice(list("ACGT"), length))
            f.write(">%s\n%s\n" % (name, "\n".join(s[i:i + 60] for i in range(0, length, 60))))
    lines = [run for run in fx["runs"] if run["name"] == "cli"][0]["lines"]
    contigs, pos = [l.split("\t")[0] for l in lines], [int(l.split("\t")[1]) for l in lines]
    want, got, why = _both(bam, fa, contigs, pos)
    g, n = _agree(want, got, why)
    assert n >= 0.8 * len(pos) and g >= 0.9 * n, (g, n)


def test_encode_locations_gpu_equals_native(tmp_path):
    bam, fa, ref = _big_case(tmp_path)
    rng = np.random.default_rng(4)
    locs = [PE.Location("chr20", int(p), "chr20:%d" % p, 2, "chr20\t%d\t.\t%s\tG" % (p, ref[p - 1])) for p in rng.integers(150, 5850, 120)]
    locs.append(PE.Location("chrX", 100, "chrX:100", 2, "chrX\t100\t.\tA\tC"))
    opt = PE.EncoderOptions(window_size=100, max_reads=200)
    nat, e_nat = PE.encode_locations(bam, fa, locs, opt, native=True)
    gpu, e_gpu = PE.encode_locations(bam, fa, locs, opt, device="gpu")
    assert e_gpu == e_nat and len(gpu) == len(nat) and gpu.tobytes() == nat.tobytes()
    # two reads sharing name AND sequence: the GPU declines, so does pe_encode, the Python encoder writes the record
    sref = "ACGT" * 100
    mk = lambda p, name, seq: bamio.BamRecord(0, p, 30, 0, name, ((bamio.CMATCH, len(seq)),), seq, np.full(len(seq), 30, np.uint8))   # noqa: E731
    twins = [mk(140, "t", sref[140:180]), mk(149, "t", sref[140:180]), mk(150, "u", sref[150:190])]
    bam2, fa2 = write_inputs(tmp_path, sref, twins, tag="twins")
    with pileup_gpu.GpuPileupEncoder(bam2, fa2, 16, 50, 10, 50) as g:
        assert g.encode(["ref"], [160])[5][0] == 2
    loc = [PE.Location("ref", 160, "ref:160", 2, "ref\t160\t.\tA\tC")]
    o16 = PE.EncoderOptions(window_size=16, max_reads=50)
    nat, e_nat = PE.encode_locations(bam2, fa2, loc, o16, native=True)
    gpu, e_gpu = PE.encode_locations(bam2, fa2, loc, o16, device="gpu")
    assert e_gpu == e_nat and gpu.tobytes() == nat.tobytes() and len(gpu) == 1


def test_encode_device_equals_host_encode(tmp_path):
    import torch
    bam, fa, ref = _big_case(tmp_path)
    pos = list(range(200, 5800, 53))
    with pileup_gpu.GpuPileupEncoder(bam, fa, 100, 200, 10, 50) as g:
        host = g.encode(["chr20"] * len(pos), pos)
        dev = g.encode_device(["chr20"] * len(pos), pos)
    torch.cuda.synchronize()
    assert (host[5] == 1).sum() > 0.8 * len(pos)
    for k in range(3):
        assert np.array_equal(dev[k].cpu().numpy(), host[k]), FIELDS[k]
    for k in range(3, 6):
        assert np.array_equal(dev[k], host[k])


@pytest.mark.parametrize("kind", ["truncated_bgzf", "block_size_past_eof", "l_seq_past_record", "n_cigar_past_record",
                                  "cigar_span_overflow", "aux_string_without_nul", "aux_value_type"])
def test_corrupt_bam_is_an_error_not_a_crash(tmp_path, kind):
    """Run in a child process so that an abort would show as a signal, not take the test run down."""
    if kind == "cigar_span_overflow":        # nine D operations of 2^28 - 1: the span overflows 32 bits
        fa_ref = "ACGT" * 250
        r = bamio.BamRecord(0, 100, 30, 0, "big", tuple([(bamio.CMATCH, 10)] + [(bamio.CDEL, (1 << 28) - 1)] * 9 + [(bamio.CMATCH, 10)]),
                            "A" * 20, np.full(20, 30, np.uint8))
        bam, fa = write_inputs(tmp_path, fa_ref, [r], tag="overflow", index=False)
        name = "ref"
    else:
        from tests.test_candidates_host import AUX_KINDS, _damaged
        bam = _damaged(tmp_path, kind)
        name, length = load("nochr")["references"][0]
        fa = str(tmp_path / "r.fa")
        open(fa, "w").write(">%s\n%s\n" % (name, "A" * length))
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from dl4vc_amd.pileup_gpu import GpuPileupEncoder\n"
            "try:\n"
            "    with GpuPileupEncoder(%r, %r, 100, 200, 10, 50) as g:\n"
            "        g.encode([%r] * 3, [150, 1500, 3000])\n"
            "except RuntimeError as e:\n"
            "    print('ERR', e); sys.exit(3)\n"
            "print('OK')\n") % (ROOT, bam, fa, name)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 3, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "corrupt BAM record" in r.stdout or "truncated" in r.stdout or "BGZF" in r.stdout, r.stdout
    if kind.startswith("aux_"):
        assert AUX_KINDS[kind] in r.stdout, r.stdout

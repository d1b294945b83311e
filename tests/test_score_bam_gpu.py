"""Scoring straight from a BAM on the GPU: ``pg_assemble_device`` against its host definition (``site_assembly.assemble_host``),
``main.py --test_bam`` against converter + ``main.py --test_file`` byte for byte, and ``call_variants.sh -d`` against the script
without it."""
import gzip
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from dl4vc_amd import pileup_gpu
from dl4vc_amd.config import DanConfig
from dl4vc_amd.site_assembly import SitePlan, assemble_host
from oracle.dan_oracle import random_state_dict
from tests import pileup_cases as PC
from tests.test_cli_gpu import MODEL_FLAGS
from tests.test_score_bam import vcf_line

pytestmark = pytest.mark.gpu
FILL = 0xAB


# ---- the kernel ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def encoder(tmp_path_factory):
    """Any open encoder: ``pg_assemble_device`` uses its device and staging, not its files."""
    bam, fa = PC.write_case(tmp_path_factory.mktemp("enc"), PC.get_case("window_100"))
    with pileup_gpu.GpuPileupEncoder(bam, fa, 100, 200, 10, 50) as g:
        yield g


def _plan(rng, n, S, R, L, slots, first):
    m = len(slots)
    rows = np.stack([np.sort(rng.choice(S, R, replace=False)) for _ in range(m)]).astype(np.int16) if m else np.zeros((0, R), np.int16)
    lines = [rng.integers(0, 256, (m, L), dtype=np.uint8) for _ in range(3)]
    return SitePlan(np.asarray(slots, np.int32), rows, np.asarray(first, np.uint8), lines[0], lines[1], lines[2], [""] * m,
                    np.zeros(m, np.int32))


@pytest.mark.parametrize("S,R,L", [(200, 100, 201), (200, 64, 201), (200, 100, 61), (40, 40, 201), (37, 5, 7)])
def test_assemble_kernel_equals_the_host_definition(encoder, S, R, L):
    """Stored planes of random bytes, n = 23 slots; the output sites skip slots at both ends and in the middle (m < n), take
    the first R rows, seeded-style sorted subsets, or a mix; q-scores / strands on and off.  The outputs sit one site into
    buffers filled with 0xAB (so the slab's alignment moves with R * L, and a byte written outside it, or not written, shows).
    L = 61 and L = 7 move every row's alignment; at L = 7 a 16-byte store spans three rows."""
    import torch
    rng = np.random.default_rng(S * 1000 + R + L)
    n = 23
    dev = torch.device("cuda", 0)
    host = [rng.integers(0, 256, (n, S, L), dtype=np.uint8) for _ in range(3)]
    stored = [torch.from_numpy(h).to(dev) for h in host]
    keep = [i for i in range(n) if i not in (0, 1, 9, 10, 15, n - 1)]
    cases = [("first rows", keep, [1] * len(keep)), ("subsets", keep, [0] * len(keep)),
             ("mixed", keep, [i % 3 == 0 for i in range(len(keep))]), ("one site", [n - 2], [0]),
             ("every slot, reversed", list(range(n))[::-1], [i % 2 for i in range(n)])]
    for name, slots, first in cases:
        plan = _plan(rng, n, S, R, L, slots, first)
        m = len(plan)
        for use_q, use_strand in ((True, True), (False, True), (True, False), (False, False)):
            outs = [torch.full((m + 2, R, L), FILL, dtype=torch.uint8, device=dev) for _ in range(3)] + \
                   [torch.full((m + 2, L), FILL, dtype=torch.uint8, device=dev) for _ in range(3)]
            torch.cuda.synchronize(dev)
            s = torch.cuda.Stream(dev)
            encoder.assemble_device([t.data_ptr() for t in stored], n, plan, [t[1:].data_ptr() for t in outs], use_q, use_strand,
                                    stream=s.cuda_stream, stored_rows=S, window=L)
            s.synchronize()
            want = assemble_host(host[0], host[1], host[2], plan, use_q, use_strand)
            for k, field in enumerate(("reads", "qual", "strand", "ref", "ref_mask", "var_mask")):
                got = outs[k].cpu().numpy()
                assert np.array_equal(got[1:m + 1], want[k]), (name, field, use_q, use_strand)
                assert (got[0] == FILL).all() and (got[m + 1] == FILL).all(), (name, field, "wrote outside its sites")


def test_assemble_refuses_indices_outside_the_stored_planes(encoder):
    import torch
    dev = torch.device("cuda", 0)
    stored = [torch.zeros((2, 8, 201), dtype=torch.uint8, device=dev) for _ in range(3)]
    outs = [torch.zeros((1, 4, 201), dtype=torch.uint8, device=dev) for _ in range(3)] + [torch.zeros((1, 201), dtype=torch.uint8, device=dev) for _ in range(3)]
    rng = np.random.default_rng(0)
    for slots, rows, what in (([2], [0, 1, 2, 3], "slot"), ([-1], [0, 1, 2, 3], "slot"), ([0], [0, 1, 2, 8], "row"), ([1], [-1, 1, 2, 3], "row")):
        plan = _plan(rng, 2, 8, 4, 201, slots, [0])
        plan.rows[0] = rows
        with pytest.raises(RuntimeError, match=what):
            encoder.assemble_device([t.data_ptr() for t in stored], 2, plan, [t.data_ptr() for t in outs], stored_rows=8, window=201)
    with pytest.raises(RuntimeError, match="only 8 are stored"):
        encoder.assemble_device([t.data_ptr() for t in stored], 2, _plan(rng, 2, 9, 9, 201, [0], [1]), [t.data_ptr() for t in outs],
                                stored_rows=8, window=201)
    torch.cuda.synchronize(dev)


def test_score_bam_raises_the_value_error_of_the_python_builder(tmp_path):
    """A zero-length alignment (0M 5I) over a candidate: the GPU encoder and pe_encode decline, the Python builder raises
    ValueError naming the read -- in the worker thread; ``score_bam`` raises it in the caller and leaves no thread behind."""
    import threading
    import types
    from dl4vc_amd import pileup_encoder as PE
    from dl4vc_amd.inference import score_bam
    ref = PC.make_ref(1200, 5)
    reads = [PC.read(ref, 380, "100M", "a"), PC.read(ref, 390, "100M", "b", PC.FREV), PC.read(ref, 420, "0M5I", "zero"),
             PC.read(ref, 800, "100M", "c")]
    bam, fa = PC.write_case(tmp_path, PC.Case("zero_w100", [("chr20", ref)], reads, [], w=100, max_reads=200))
    locs = [PE.Location("chr20", p, "chr20:%d" % p, 2, vcf_line(ref, p)) for p in (850, 425)]
    net = types.SimpleNamespace(config=DanConfig())          # never reached: the first round fails
    lines = []
    with pytest.raises(ValueError, match="zero"):
        score_bam(net, bam, fa, locs, lines.append, sites_per_launch=8)
    assert not lines and not [t for t in threading.enumerate() if t.name == "score_bam-encoder"]


# ---- end to end ------------------------------------------------------------------------------------------------------------
# Locations of the fixture below that pg_encode itself encodes (status 1) / all locations, as the first run on an MI355X
# reported them: 2 of the 65 are declined (the twin reads, more than PG_MAX_TRACKS tracks), 6 hold no read.
FIXTURE_LOCATIONS = 65
FIXTURE_EMPTY = 6
FIXTURE_ON_GPU = 57
GPU_SHARE_FLOOR = 0.85          # of all locations; pg_encode alone gives 57 / 65 = 0.877 on this fixture


def _fixture(d):
    """Coordinate-sorted BAM + FASTA + candidates.vcf: ~24x background with SNPs, insertions and deletions, a 170-deep and a
    260-deep site (more than R = 100 and more than the 200 stored rows), locations without a read at the start, in the middle
    (a 100-base hole) and at the end, two reads sharing name and sequence (the GPU and pe_encode decline, the Python builder encodes), a site
    with 1 100 tracks (the GPU declines, pe_encode encodes), a record text longer than the 128 stored bytes."""
    ref = PC.make_ref(9000, 77)
    reads = []
    for i, s in enumerate(range(200, 5000, 4)):
        if 3600 <= s < 3800:
            continue                                       # a hole: the location at 3800 has no read
        cigar = ["100M", "50M1X49M", "40M2I58M", "30M3D67M", "5S95M"][i % 5]
        reads.append(PC.read(ref, s, cigar, "bg%d" % i, PC.FREV if i % 2 else 0, 10 + i % 30))
    reads += [PC.read(ref, 1950 + i % 45, "100M" if i % 3 else "47M1X52M", "deep%d" % i, PC.FREV if i % 2 else 0, 20 + i % 20) for i in range(150)]
    reads += [PC.read(ref, 2930 + i % 60, "90M", "deeper%d" % i, PC.FREV if i % 3 else 0, 25) for i in range(240)]
    reads += [PC.read(ref, 5500, "40M", "solo", 0, 30), PC.read(ref, 5505, "30M", "twin", 0, 32, seq=ref[5505:5535]),
              PC.read(ref, 5509, "30M", "twin", PC.FREV, 32, seq=ref[5505:5535])]
    reads += [PC.read(ref, 6200 + i % 25, "30M", "many%d" % i, PC.FREV if i % 2 else 0, 30) for i in range(1100)]
    case = PC.Case("score_bam", [("chr20", ref)], reads, [], w=100, max_reads=200)
    bam, fa = PC.write_case(d, case)
    pos = [60, 120] + list(range(330, 4900, 83)) + [2000, 2990, 3800, 5520, 6215, 8000, 8500]
    assert len(pos) == FIXTURE_LOCATIONS
    head = "##fileformat=VCFv4.2\n##contig=<ID=chr20,length=9000>\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tCALLED\n"
    vcf, plain = os.path.join(str(d), "candidates.vcf"), os.path.join(str(d), "candidates_plain.vcf")
    for path, pad in ((vcf, 150), (plain, 0)):      # (format_vcf, like the reference's, cannot read a record cut at 128 bytes)
        with open(path, "w") as f:
            f.write(head + "".join(vcf_line(ref, p, i % 3, pad if i == 11 else 0) + "\n" for i, p in enumerate(pos)))
    return bam, fa, vcf, plain, pos


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    import torch
    d = tmp_path_factory.mktemp("score_bam")
    bam, fa, vcf, plain, pos = _fixture(d)
    ck = str(d / "ckpt.pth.tar")
    torch.save({"epoch": 1, "best_loss": 0.0, "optimizer": {},
                "state_dict": {"module." + k: torch.from_numpy(v) for k, v in random_state_dict(DanConfig(), seed=21).items()}}, ck)
    return d, bam, fa, vcf, plain, pos, ck


def _run(cmd, **kw):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, **kw)
    assert r.returncode == 0, (cmd[:3], r.stdout[-2000:], r.stderr[-2000:])
    return r


def test_test_bam_equals_convert_then_test_file(inputs):
    d, bam, fa, vcf, _plain, pos, ck = inputs
    # (a) candidates.hdf, then --test_file
    two = d / "two_step"
    two.mkdir()
    _run([sys.executable, os.path.join(ROOT, "tools", "convert_bam_single_reads.py"), "--input", bam, "--fp_vcf", vcf, "--fasta-input", fa,
          "--output", str(two / "candidates.hdf"), "--max-reads", "200", "--num-processes", "2", "--max-insert-length", "10",
          "--max-insert-length-variant", "50", "--save-q-scores", "--save-strand"])
    common = ["--modelload", ck, "--sample_vcf", vcf, "--save_vcf_records", "--reads-seed", "5", "--sites-per-launch", "16"] + MODEL_FLAGS
    _run([sys.executable, os.path.join(ROOT, "main.py"), "--test_file", str(two / "candidates.hdf"), "--save_vcf_records_file",
          str(two / "model_test.vcf")] + common)
    # (b) --test_bam
    one = d / "direct"
    one.mkdir()
    r = _run([sys.executable, os.path.join(ROOT, "main.py"), "--test_bam", bam, "--test_fasta", fa, "--save_vcf_records_file",
              str(one / "model_test.vcf")] + common)
    want = open(str(two / "epoch1_model_test.vcf"), "rb").read()
    got = open(str(one / "epoch1_model_test.vcf"), "rb").read()
    body = [l for l in want.decode().splitlines() if not l.startswith("#")]
    assert len(body) == FIXTURE_LOCATIONS - FIXTURE_EMPTY and got == want             # every location with a read, none left out
    assert max(len(l) for l in body) > 128 + 30                          # (the record cut at 128 bytes went through both)
    # nothing but the scored VCF was written
    assert sorted(os.listdir(str(one))) == ["epoch1_model_test.vcf"]
    # the device path carried the sites
    c = re.search(r"pileup encoder: (\d+) locations: (\d+) on the GPU, (\d+) by pe_encode, (\d+) by the Python builder, (\d+) without a record",
                  r.stdout)
    assert c, r.stdout[-1500:]
    n, gpu, native, py, empty = map(int, c.groups())
    print("pg_encode took %d of %d locations (pe_encode %d, Python %d, no record %d)" % (gpu, n, native, py, empty))
    assert n == FIXTURE_LOCATIONS and empty == FIXTURE_EMPTY and native >= 1 and py >= 1 and gpu + native + py + empty == n
    assert gpu / n >= GPU_SHARE_FLOOR and FIXTURE_ON_GPU / FIXTURE_LOCATIONS >= GPU_SHARE_FLOOR, (gpu, n)
    assert re.search(r"(\d+) of %d sites lie within 1e-4 of a genotype threshold" % len(body), r.stdout)
    # --max-test-batches stops after the same number of records on both paths
    lim = ["--max-test-batches", "1", "--test-batch-size", "10"]
    _run([sys.executable, os.path.join(ROOT, "main.py"), "--test_bam", bam, "--test_fasta", fa, "--save_vcf_records_file",
          str(one / "limited.vcf")] + common + lim)
    limited = [l for l in open(str(one / "epoch1_limited.vcf")).read().splitlines() if not l.startswith("#")]
    assert limited == body[:20]


def test_call_variants_sh_direct_equals_the_two_step_script(inputs):
    d, bam, fa, _long, vcf, pos, ck = inputs
    outs = {}
    for name, flag in (("script_two", []), ("script_direct", ["-d"])):
        out = d / name
        out.mkdir()
        open(str(out / "candidates.vcf"), "w").write(open(vcf).read())
        r = subprocess.run(["bash", os.path.join(ROOT, "call_variants.sh"), "-m", ck, "-o", str(out), "-i", bam, "-r", fa, "-p", "2"] + flag,
                           capture_output=True, text=True, timeout=900)
        log = open(str(out / "training.log")).read()[-1500:] if (out / "training.log").exists() else ""
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:], log)
        outs[name] = out
    assert (outs["script_two"] / "candidates.hdf").exists() and not (outs["script_direct"] / "candidates.hdf").exists()
    assert not (outs["script_direct"] / "training_data.log").exists()
    a = gzip.open(str(outs["script_two"] / "called_variants.vcf.gz"), "rb").read()
    b = gzip.open(str(outs["script_direct"] / "called_variants.vcf.gz"), "rb").read()
    assert a == b and a.startswith(b"##fileformat")
    assert open(str(outs["script_two"] / "epoch1_model_test.vcf"), "rb").read() == open(str(outs["script_direct"] / "epoch1_model_test.vcf"), "rb").read()
    # -d without the BAM is refused, and -d on several GPUs is main.py's refusal
    r = subprocess.run(["bash", os.path.join(ROOT, "call_variants.sh"), "-m", ck, "-o", str(outs["script_direct"]), "-d"], capture_output=True, text=True)
    assert r.returncode == 1 and "-d needs -i BAM -r REFERENCE" in r.stdout


def test_converter_on_the_gpu_encoder_writes_the_same_file(inputs):
    from dl4vc_amd import hdf5io
    d, bam, fa, vcf, _plain, pos, ck = inputs
    out = d / "conv"
    out.mkdir()
    files = []
    for name, extra in (("host.hdf", []), ("gpu.hdf", ["--pileup-device", "gpu"])):
        _run([sys.executable, os.path.join(ROOT, "tools", "convert_bam_single_reads.py"), "--input", bam, "--fp_vcf", vcf, "--fasta-input", fa,
              "--output", str(out / name), "--max-reads", "200", "--num-processes", "2", "--max-insert-length", "10",
              "--max-insert-length-variant", "50", "--save-q-scores", "--save-strand"] + extra)
        with hdf5io.CandidateFile(str(out / name)) as f:
            files.append(f.read(0, len(f)))
    assert len(files[0]) == FIXTURE_LOCATIONS - FIXTURE_EMPTY and files[0].tobytes() == files[1].tobytes()

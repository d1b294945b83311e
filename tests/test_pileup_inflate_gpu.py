"""The GPU pileup encoder with the BGZF blocks inflated and the records framed on the MI355X (``inflate_device="gpu"``,
``pg_set_inflate_device``) against the same encoder with the option off: status, num_reads, the ref row and the three planes of
every location are byte-equal, through ``pg_encode`` and ``pg_encode_device``, and a damaged file is an error with the host
path's text.  Every comparison also asserts that the device path ran (no record framed on the host, blocks inflated)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from dl4vc_amd import pileup_gpu
from tests import pileup_cases as PC
from tests import pileup_inflate_cases as IC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("reads", "qual", "strand", "ref", "num_reads", "status")


def _ran_on_the_device(st):
    assert st["host_records"] == 0 and st["blocks"] > 0 and st["records"] > 0 and st["groups"] >= 1, st


def _equal(got, want):
    for k, name in enumerate(FIELDS):
        a, b = (x.cpu().numpy() if hasattr(x, "cpu") else x for x in (got[k], want[k]))
        bad = [int(i) for i in range(len(b)) if not np.array_equal(a[i], b[i])]
        assert not bad, (name, bad[:10])


# cases in which no location forms a run (every location is decided before a record is read: a window or a quality floor the
# plan does not hold), so neither path reads a block or a record
NO_RUN = {"window_101", "min_base_quality_1"}


@pytest.mark.parametrize("name", [n for n in PC.CASE_NAMES if PC.get_case(n).index])
def test_every_indexed_case_equals_the_host_path(tmp_path, name):
    case = PC.get_case(name)
    bam, fa = PC.write_case(tmp_path, case)
    contigs, pos = [l.contig for l in case.locs], [l.pos for l in case.locs]
    with pileup_gpu.GpuPileupEncoder(bam, fa, *case.options()) as g:
        want = g.encode(contigs, pos)
        host = g.stats()
        assert (host["host_records"] == 0) == (name in NO_RUN), host
    with pileup_gpu.GpuPileupEncoder(bam, fa, *case.options(), inflate_device="gpu") as g:
        got = g.encode(contigs, pos)
        st = g.stats()
    _equal(got, want)
    assert st["host_records"] == 0 and st["records"] == host["records"], (st, host)
    if name not in NO_RUN:
        _ran_on_the_device(st)


def test_two_runs_whose_ranges_share_a_block(tmp_path):
    """Two runs more than a 16-kb window apart whose byte ranges touch the same BGZF block without merging (the records of the
    window between them are not asked for), the second continuing into the next block: the call's block table lists that block
    for both ranges, and each group takes a range's blocks from its own stretch of the table.  One group, then one per run."""
    bam, fa = IC.shared_block(tmp_path)
    contigs, pos = IC.SHARED_LOCS
    with pileup_gpu.GpuPileupEncoder(bam, fa, *IC.OPTIONS) as g:
        want = g.encode(contigs, pos)
        host = g.stats()
        for budget in (0, 1):
            g.set_inflate_device(True, budget)
            got = g.encode(contigs, pos)
            st = g.stats()
            _equal(got, want)
            _ran_on_the_device(st)
            assert st["records"] == host["records"] and st["groups"] == (2 if budget else 1), (st, host)
    assert want[5].tolist() == [1, 1, 1] and st["blocks"] == 3                  # the shared block once for each range


def test_an_encoder_without_an_index_is_refused_with_the_reason(tmp_path):
    case = PC.get_case("unsorted_no_bai")
    assert not case.index
    bam, fa = PC.write_case(tmp_path, case)
    with pytest.raises(RuntimeError, match="needs the BAI index"):
        pileup_gpu.GpuPileupEncoder(bam, fa, *case.options(), inflate_device="gpu")
    with pileup_gpu.GpuPileupEncoder(bam, fa, *case.options()) as g:
        g.encode(["ref"], [321])                            # (the scan builds the linear index only: still no bins)
        with pytest.raises(RuntimeError, match="needs the BAI index"):
            g.set_inflate_device(True)


@pytest.mark.parametrize("level", [0, 1, 6])
def test_grid_equals_the_host_path(tmp_path, level):
    bam, fa = IC.grid(tmp_path, level)
    found, longest, n_blocks = IC.straddles(bam)
    assert found >= 1 and longest > 65536 and n_blocks >= 5
    contigs, pos = IC.locations()
    with pileup_gpu.GpuPileupEncoder(bam, fa, *IC.OPTIONS) as g:
        want = g.encode(contigs, pos)
        g.set_inflate_device(True)
        got = g.encode(contigs, pos)
        st = g.stats()
    _equal(got, want)
    _ran_on_the_device(st)
    status = dict(zip(zip(contigs, pos), want[5].tolist()))
    assert status[("chr1", IC.DEEP)] == 2                                   # over PG_MAX_TRACKS, on both paths
    assert status[("chr1", 150_000)] == 0 and status[("chrX", 5)] == 0      # a hole; a contig the BAM does not have
    for key in (("chr1", 1), ("chr1", IC.LEN1), ("2", 1), ("chr2", IC.LEN2), ("chr1", 49_990), ("chr1", 100_010), ("chr1", 104_900),
                ("chr1", 230_000)):
        assert status[key] == 1, key
    assert st["blocks"] >= 4 and st["inflated_bytes"] > 4 * 60000


def test_big_call_on_off_on_and_many_groups(tmp_path):
    case, contigs, pos = PC.big_call()
    bam, fa = PC.write_case(tmp_path, case)
    with pileup_gpu.GpuPileupEncoder(bam, fa, *case.options()) as g:
        g.set_inflate_device(True)
        first = g.encode(contigs, pos)
        _ran_on_the_device(g.stats())
        g.set_inflate_device(False)
        want = g.encode(contigs, pos)
        assert g.stats()["host_records"] > 0 and g.stats()["blocks"] == 0
        g.set_inflate_device(True)
        again = g.encode(contigs, pos)
        st1 = g.stats()
        g.set_inflate_device(True, 65536)
        small = g.encode(contigs, pos)
        st = g.stats()
    assert (want[5] == 1).all()
    for got in (first, again, small):
        _equal(got, want)
    _ran_on_the_device(st1)
    _ran_on_the_device(st)
    assert st["groups"] > 10 > st1["groups"]


def test_encode_device_writes_every_slot(tmp_path):
    import torch
    bam, fa = IC.grid(tmp_path, 6)
    contigs, pos = IC.locations()
    n = len(pos)
    dev = torch.device("cuda", 0)
    with pileup_gpu.GpuPileupEncoder(bam, fa, *IC.OPTIONS) as g:
        outs = []
        for on in (False, True):
            g.set_inflate_device(on)
            buf = [torch.full((n, IC.MAX_READS, 2 * IC.W + 1), 0xAB, dtype=torch.uint8, device=dev) for _ in range(3)]
            outs.append(g.encode_device(contigs, pos, out=buf))
            torch.cuda.synchronize()
            st = g.stats()
        _ran_on_the_device(st)
    _equal(outs[1], outs[0])
    zero = outs[1][5] != 1
    assert zero.any() and not outs[1][0].cpu().numpy()[zero].any()          # written, not left at 0xAB


@pytest.mark.parametrize("kind", IC.DAMAGED)
def test_damaged_input_is_an_error_on_the_device_path(tmp_path, kind):
    """In a child process, so that an abort would show as a signal.  The CPU twin (tests/test_pileup_frame_host.py) runs the
    same files through the same text under sanitizers."""
    bam, bai, fa = IC.damaged(tmp_path, kind)
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from dl4vc_amd.pileup_gpu import GpuPileupEncoder\n"
            "try:\n"
            "    with GpuPileupEncoder(%r, %r, 16, 20, 10, 50, bai_path=%r, inflate_device='gpu') as g:\n"
            "        g.encode(['ctg'] * 3, [150, 1500, 3000])\n"
            "except RuntimeError as e:\n"
            "    print('ERR', e); sys.exit(3)\n"
            "print('OK')\n") % (ROOT, bam, fa, bai)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert IC.EXPECT[kind][1] in r.stdout, r.stdout
    if kind not in ("crc_flipped", "truncated_bgzf"):
        with pytest.raises(RuntimeError) as e:
            pileup_gpu.debug_run_records(bam, bai, *IC.DAMAGED_WINDOW, 0)
        assert str(e.value).split("failed: ")[1] in r.stdout                # the host path's text and offset


# ---- command lines ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli_inputs(tmp_path_factory):
    import torch
    from dl4vc_amd.config import DanConfig
    from oracle.dan_oracle import random_state_dict
    from tests.test_score_bam_gpu import _fixture
    d = tmp_path_factory.mktemp("inflate_cli")
    bam, fa, vcf, plain, pos = _fixture(d)
    ck = str(d / "ckpt.pth.tar")
    torch.save({"epoch": 1, "best_loss": 0.0, "optimizer": {},
                "state_dict": {"module." + k: torch.from_numpy(v) for k, v in random_state_dict(DanConfig(), seed=21).items()}}, ck)
    return d, bam, fa, vcf, plain, ck


def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (cmd[:3], r.stdout[-2000:], r.stderr[-2000:])
    return r


def test_main_test_bam_with_the_flag_writes_the_same_vcf(cli_inputs):
    from tests.test_score_bam_gpu import MODEL_FLAGS
    d, bam, fa, vcf, _plain, ck = cli_inputs
    common = ["--modelload", ck, "--sample_vcf", vcf, "--save_vcf_records", "--reads-seed", "5", "--sites-per-launch", "16"] + MODEL_FLAGS
    outs = []
    for name, extra in (("off", []), ("on", ["--inflate-device", "gpu"])):
        out = d / ("main_" + name)
        out.mkdir()
        r = _run([sys.executable, os.path.join(ROOT, "main.py"), "--test_bam", bam, "--test_fasta", fa, "--save_vcf_records_file",
                  str(out / "model_test.vcf")] + common + extra)
        outs.append(open(str(out / "epoch1_model_test.vcf"), "rb").read())
        assert ("BGZF inflate and framing on the device" in r.stdout) == bool(extra), r.stdout[-1500:]
        if extra:
            assert "host_records 0," in r.stdout and "blocks 0," not in r.stdout, r.stdout[-1500:]
    assert outs[0] == outs[1] and outs[0].count(b"\n") > 50


def test_converter_with_the_flag_writes_the_same_file(cli_inputs):
    from dl4vc_amd import hdf5io
    d, bam, fa, vcf, _plain, ck = cli_inputs
    out = d / "conv"
    out.mkdir()
    files = []                                                    # (the records: the container stamps its objects with the time)
    for name, extra in (("gpu.hdf", []), ("gpu_inflate.hdf", ["--inflate-device", "gpu"])):
        _run([sys.executable, os.path.join(ROOT, "tools", "convert_bam_single_reads.py"), "--input", bam, "--fp_vcf", vcf, "--fasta-input", fa,
              "--output", str(out / name), "--max-reads", "200", "--num-processes", "2", "--max-insert-length", "10",
              "--max-insert-length-variant", "50", "--save-q-scores", "--save-strand", "--pileup-device", "gpu"] + extra)
        with hdf5io.CandidateFile(str(out / name)) as f:
            files.append(f.read(0, len(f)))
    assert len(files[0]) > 50 and files[0].tobytes() == files[1].tobytes()


def test_call_variants_sh_d_z_equals_d(cli_inputs):
    import gzip
    d, bam, fa, _long, vcf, ck = cli_inputs
    outs = {}
    for name, flag in (("script_d", ["-d"]), ("script_dz", ["-d", "-z"])):
        out = d / name
        out.mkdir()
        open(str(out / "candidates.vcf"), "w").write(open(vcf).read())
        r = subprocess.run(["bash", os.path.join(ROOT, "call_variants.sh"), "-m", ck, "-o", str(out), "-i", bam, "-r", fa, "-p", "2"] + flag,
                           capture_output=True, text=True, timeout=900)
        log = open(str(out / "training.log")).read() if (out / "training.log").exists() else ""
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:], log[-1500:])
        assert ("BGZF inflate and framing on the device" in log) == ("-z" in flag)
        outs[name] = out
    a = gzip.open(str(outs["script_d"] / "called_variants.vcf.gz"), "rb").read()
    b = gzip.open(str(outs["script_dz"] / "called_variants.vcf.gz"), "rb").read()
    assert a == b and a.startswith(b"##fileformat")


def test_the_two_refusals_give_their_messages(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "main.py"), "--test_file", str(tmp_path / "x.hdf"), "--inflate-device", "gpu"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--inflate-device gpu is an option of --test_bam" in r.stderr
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "convert_bam_single_reads.py"), "--input", "a.bam", "--output", "b.hdf",
                        "--inflate-device", "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "give --pileup-device gpu as well" in r.stderr

"""The record census (``pg_census``, ``--record-census gpu``) and what it makes possible: ``main.py --test_bam`` on several
GPUs, with ``--test_holdout_chromosomes`` and ``--max-test-batches`` selecting and seeding the records as ``--test_file`` does,
and ``tools/candidate_generator.py --gpus N``.  Every comparison is byte for byte against the one-process path.

The fixture of tests/test_score_bam_gpu.py has 65 locations: 6 without a read (60 and 120 at the start, 3733 and 3800 in the
hole, 8000 and 8500 at the end), 2 the GPU declines (the twins, 1 100 tracks), and its 170-deep and 260-deep sites come late in
the location order: a two-way split puts empty locations into shard 0 and seeded sites into shard 1."""
import gzip
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from dl4vc_amd import pileup_gpu
from dl4vc_amd import pileup_encoder as PE
from dl4vc_amd.config import DanConfig
from dl4vc_amd.shard import plan_bam_shard, shard_range
from oracle.dan_oracle import random_state_dict
from tests import pileup_cases as PC
from tests.candidates_fixture import load, write_bam
from tests.test_cli_gpu import MODEL_FLAGS
from tests.test_pileup_edges import ERRORS, _location, _options
from tests.test_score_bam import vcf_line
from tests.test_score_bam_gpu import FIXTURE_EMPTY, FIXTURE_LOCATIONS, _fixture

pytestmark = pytest.mark.gpu
MAIN = os.path.join(ROOT, "main.py")
CONVERTER = os.path.join(ROOT, "tools", "convert_bam_single_reads.py")
GENERATOR = os.path.join(ROOT, "tools", "candidate_generator.py")
CONVERT_FLAGS = ["--max-reads", "200", "--num-processes", "2", "--max-insert-length", "10", "--max-insert-length-variant", "50",
                 "--save-q-scores", "--save-strand"]
FORCE0 = dict(os.environ, DL4VC_FORCE_DEVICE0="1")


def _run_all(cmds, timeout=600, **kw):
    """The commands side by side (fresh processes, at most seven): every one must end with 0.  -> their stdouts."""
    procs = [subprocess.Popen(c, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, **kw) for c in cmds]
    outs = [p.communicate(timeout=timeout) for p in procs]
    for c, p, (o, e) in zip(cmds, procs, outs):
        assert p.returncode == 0, (c[1:6], o[-2000:], e[-2000:])
    return [o for o, _e in outs]


def _body(path):
    return [l for l in open(path).read().splitlines() if not l.startswith("#")]


def _record_flags(locs, records):
    """Records in input order (``encode_locations``) -> one flag per location."""
    names = [bytes(r["name"]).rstrip(b"\0").decode() for r in records]
    flags, k = [], 0
    for l in locs:
        hit = k < len(names) and names[k] == l.name
        flags.append(int(hit))
        k += hit
    assert k == len(names)
    return flags


def _census_and_encode(bam, fa, options, contigs, pos, mode):
    """-> (census statuses, encode_device statuses, stats of the census call, stats of the encode call) of one encoder."""
    with pileup_gpu.GpuPileupEncoder(bam, fa, *options, inflate_device=mode) as g:
        want = g.encode_device(contigs, pos)[5]
        enc = g.stats()
        got = g.census(contigs, pos)
        st = g.stats()
        again = g.encode_device(contigs, pos)[5]           # (a census leaves the encoder as it was)
    assert again.tolist() == want.tolist()
    return got, want, st, enc


def _check_census(bam, fa, options, contigs, pos, indexed=True, label=""):
    for mode in (None, "gpu") if indexed else (None,):
        got, want, st, enc = _census_and_encode(bam, fa, options, contigs, pos, mode)
        assert got.dtype == np.int8 and got.tolist() == want.tolist(), (label, mode, got.tolist(), want.tolist())
        assert st["encode_ms"] == 0 and enc["census_ms"] == 0 and st["records"] == enc["records"], (label, mode, st, enc)
        assert st["census_ms"] > 0 or st["records"] == 0, (label, mode, st)
        if mode == "gpu":
            assert st["host_records"] == 0
    return want


# ---- 1. census == encode --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PC.CASE_NAMES)
def test_census_equals_encode_on_every_case(tmp_path, name):
    """Element by element, host framing and (where the case has a BAI: the device path refuses a file without) BGZF inflate and
    framing on the device; then the record flags behind the shared fallback against today's three-level encode."""
    from dl4vc_amd.inference import census_bam
    case = PC.get_case(name)
    bam, fa = PC.write_case(tmp_path, case)
    _check_census(bam, fa, case.options(), [l.contig for l in case.locs], [l.pos for l in case.locs], case.index, name)
    opt = _options(case)
    locs = [_location(l) for l in case.locs if not l.py]
    records, _errors = PE.encode_locations(bam, fa, locs, opt, device="gpu")
    assert census_bam(bam, fa, locs, opt).tolist() == _record_flags(locs, records)
    for l in case.locs:
        if l.py:                                           # (the fallback ends where the encoder's does: in the builder's error)
            with pytest.raises(ERRORS[l.py]):
                census_bam(bam, fa, [_location(l)], opt)


def _two_contigs(d, extra_contig=False):
    """chrA: ~25x with a 400-base hole (one location without a read); chrB: ~25x and a site 160 reads deeper (more than R = 100
    rows).  -> (bam, fasta, candidates.vcf, locations).  ``extra_contig``: chrC, in the BAM but not in the FASTA."""
    ra, rb, rc = PC.make_ref(3400, 201), PC.make_ref(3400, 202), PC.make_ref(600, 203)
    reads = []
    for i, s in enumerate(range(100, 3200, 4)):
        if not 1500 <= s < 1900:
            reads.append(PC.read(ra, s, ["100M", "40M2I58M", "30M3D67M"][i % 3], "a%d" % i, PC.FREV if i % 2 else 0, 12 + i % 25, tid=0))
        reads.append(PC.read(rb, s, ["100M", "50M1X49M", "5S95M"][i % 3], "b%d" % i, PC.FREV if i % 2 else 0, 14 + i % 20, tid=1))
    reads += [PC.read(rb, 2350 + i % 50, "100M" if i % 4 else "47M1X52M", "deep%d" % i, PC.FREV if i % 2 else 0, 22, tid=1) for i in range(160)]
    refs = [("chrA", ra), ("chrB", rb)]
    if extra_contig:
        refs.append(("chrC", rc))
        reads += [PC.read(rc, 100 + 5 * i, "80M", "c%d" % i, 0, 30, tid=2) for i in range(20)]
    case = PC.Case("two_contigs", refs, reads, [], w=100, max_reads=200, fasta=["chrA", "chrB"] if extra_contig else None)
    bam, fa = PC.write_case(d, case)
    pos = {"chrA": list(range(300, 3000, 235)), "chrB": list(range(310, 3000, 235)) + [2400]}
    assert 1710 in pos["chrA"]                             # (its window [1608, 1813) lies inside the hole)
    head = "##fileformat=VCFv4.2\n##contig=<ID=chrA,length=3400>\n##contig=<ID=chrB,length=3400>\n" \
           "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tCALLED\n"
    vcf = os.path.join(str(d), "two.vcf")
    with open(vcf, "w") as f:
        f.write(head)
        for c, ref in (("chrA", ra), ("chrB", rb)):
            for i, p in enumerate(pos[c]):
                f.write(vcf_line(ref, p, i % 3).replace("chr20", c, 1) + "\n")
    return bam, fa, vcf, PE.locations_from_vcf(vcf, label=2)


def test_census_equals_encode_on_the_fixture_and_at_the_edges(tmp_path):
    from dl4vc_amd.inference import census_bam
    bam, fa, vcf, _plain, pos = _fixture(tmp_path)
    locs = PE.locations_from_vcf(vcf, label=2)
    options = (100, 200, 10, 50, 0)
    want = _check_census(bam, fa, options, [l.contig for l in locs], [l.pos for l in locs], label="fixture")
    assert (want == 2).sum() == 2 and len(want) == FIXTURE_LOCATIONS
    for mode in (None, "gpu"):
        stage = {}
        flags = census_bam(bam, fa, locs, inflate_device=mode, stage=stage, batch=20)      # (four calls, the last of 5)
        assert flags.dtype == np.uint8 and int(flags.sum()) == FIXTURE_LOCATIONS - FIXTURE_EMPTY == 59
        assert [l.pos for l, f in zip(locs, flags) if not f] == [60, 120, 3733, 3800, 8000, 8500]
        assert stage["census_ms"] > 0 and stage["encode_ms"] == 0
    # the edges: one location; none with a record; a contig the FASTA lacks, one the BAM lacks; positions below 1; two contigs
    bam2, fa2, _vcf2, _locs2 = _two_contigs(tmp_path, extra_contig=True)
    calls = {"n = 1": (["chrB"], [2400]), "n = 0": ([], []), "no candidate record": (["chrA", "chrA"], [1700, 3390]),
             "contig missing from the FASTA": (["chrC", "chrA"], [140, 500]), "contig missing from the BAM": (["chrZ"], [5]),
             "positions below 1": (["chrA", "chrA", "chrB"], [0, -7, 1]),
             "two contigs in one call": (["chrB", "chrA", "chrB", "chrA", "chrC", "chrA"], [2400, 500, 400, 1700, 150, 2900])}
    seen = set()
    for label, (contigs, p) in calls.items():
        seen |= set(_check_census(bam2, fa2, options, contigs, p, label=label).tolist())
    assert seen == {0, 1, 2}


# ---- 2. and 5.: the Python API ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    import torch
    d = tmp_path_factory.mktemp("census")
    bam, fa, vcf, plain, pos = _fixture(d)
    ck = str(d / "ckpt.pth.tar")
    torch.save({"epoch": 1, "best_loss": 0.0, "optimizer": {},
                "state_dict": {"module." + k: torch.from_numpy(v) for k, v in random_state_dict(DanConfig(), seed=21).items()}}, ck)
    return d, bam, fa, vcf, plain, pos, ck


def test_sharded_score_bam_equals_one_run_and_a_wrong_seed_shows(inputs):
    """One run against 2 and 3 runs planned from the census; then shard 1 of 2 seeded with its first LOCATION's index instead of
    its first record's (off by the two empty locations in front).

    The issue words the sensitivity check as "the lines of the 170-deep and 260-deep sites and no others".  A site is seeded
    when its window holds more than R = 100 rows, and the windows of the grid locations next to those two sites hold the same
    deep reads, as does the 1 100-track site.  So the check is: every changed line belongs to a site with more than R rows
    (nothing else may move), and the lines of the 170-deep (POS 2000) and the 260-deep (POS 2990) site are among them."""
    import torch                                            # noqa: F401 -- before the network's library (one HIP runtime)
    from dl4vc_amd.inference import census_bam, score_bam
    from dl4vc_amd.model import DanNet
    _d, bam, fa, vcf, _plain, _pos, _ck = inputs
    cfg = DanConfig()
    net = DanNet(cfg, device_id=0, max_batch=16).load_state_dict(random_state_dict(cfg, seed=21))
    locs = PE.locations_from_vcf(vcf, label=2)
    try:
        flags = census_bam(bam, fa, locs)

        def score(a, b, first, census=None):
            lines = []
            n = score_bam(net, bam, fa, locs[a:b], lines.append, sites_per_launch=16, reads_seed=5, first_record=first, census=census)
            text = "".join(lines)
            assert n == text.count("\n")
            return text.splitlines()

        whole = score(0, len(locs), 0)
        assert len(whole) == 59
        for count in (2, 3):
            parts = []
            for g in range(count):
                runs = plan_bam_shard(flags, None, 0, g, count)
                assert len(runs) == 1
                part = []
                for a, b, first in runs:
                    part += score(a, b, first, flags[a:b])
                assert len(part) == np.diff(shard_range(59, g, count))[0]
                parts += part
            assert parts == whole, count
        (a, b, first), = plan_bam_shard(flags, None, 0, 1, 2)
        assert first == 29 and a == first + 2               # (60 and 120 are empty)
        wrong = score(a, b, a)
        right = whole[first:]
        opt = PE.EncoderOptions(window_size=100, max_reads=200, max_insert_length=10, max_insert_length_variant=50, min_base_quality=0)
        records, _errors = PE.encode_locations(bam, fa, locs, opt, device="gpu")
        deep = {bytes(r["name"]).rstrip(b"\0").decode().replace(":", "\t") + "\t" for r in records if r["num_reads"] > cfg.reads}
        changed = [r for r, w in zip(right, wrong) if r != w]
        print("%d of %d lines change with the wrong seed; %d sites of the list hold more than %d rows" % (len(changed), len(right), len(deep), cfg.reads))
        assert len(wrong) == len(right) and changed
        assert all(any(l.startswith(p) for p in deep) for l in changed), changed
        for pos in (2000, 2990):
            assert any(l.startswith("chr20\t%d\t" % pos) for l in changed), pos
        # 5. a census that is wrong about one location is an error, not another seed
        for i, name in ((0, "chr20:60"), (5, "chr20:%d" % locs[5].pos)):
            bad = flags.copy()
            bad[i] ^= 1
            assert flags[i] == (0 if i == 0 else 1)
            with pytest.raises(RuntimeError, match=r"record census mismatch at location %s .*census says status %d, the encoder %d"
                                                   % (name, bad[i], flags[i])):
                score(0, 20, 0, bad[:20])
    finally:
        net.close()


# ---- 3. the CLI, two processes on one GPU ------------------------------------------------------------------------------------
def test_test_bam_on_two_processes_equals_one_and_the_parts_of_test_file(inputs):
    d, bam, fa, vcf, _plain, _pos, ck = inputs
    out = d / "cli"
    out.mkdir()
    hdf = str(out / "candidates.hdf")
    _run_all([[sys.executable, CONVERTER, "--input", bam, "--fp_vcf", vcf, "--fasta-input", fa, "--output", hdf] + CONVERT_FLAGS])
    common = ["--modelload", ck, "--sample_vcf", vcf, "--save_vcf_records", "--reads-seed", "5", "--sites-per-launch", "16"] + MODEL_FLAGS
    direct = [sys.executable, MAIN, "--test_bam", bam, "--test_fasta", fa] + common
    for name in ("one", "two", "file", "alone"):
        (out / name).mkdir()
    to = lambda name: ["--save_vcf_records_file", str(out / name / "model_test.vcf")]   # noqa: E731
    outs = _run_all([direct + to("one"),
                     direct + to("two") + ["--record-census", "gpu", "--gpus", "2"]] +
                    [[sys.executable, MAIN, "--test_file", hdf] + common + to("file") + ["--shard", "%d/2" % g] for g in (0, 1)] +
                    [direct + to("alone") + ["--record-census", "gpu", "--shard", "%d/2" % g] for g in (0, 1)], env=FORCE0)
    want = open(str(out / "one" / "epoch1_model_test.vcf"), "rb").read()
    assert len(_body(str(out / "one" / "epoch1_model_test.vcf"))) == 59
    assert open(str(out / "two" / "epoch1_model_test.vcf"), "rb").read() == want
    assert sorted(os.listdir(str(out / "two"))) == ["epoch1_model_test.vcf"]          # no part, statistics or census file
    for g in (0, 1):
        part = "epoch1_model_test.vcf.part%d" % g
        a, b = shard_range(59, g, 2)
        assert open(str(out / "alone" / part)).read() == open(str(out / "file" / part)).read() == "".join(l + "\n" for l in _body(str(out / "one" / "epoch1_model_test.vcf"))[a:b])
        assert re.search(r"shard %d/2 on device 0: %d sites, .*census_s \d+\.\d+ for \d+ locations" % (g, b - a), outs[1]), outs[1][-2000:]
        assert "without sibling processes: this process censuses all 65 locations itself" in outs[4 + g]
    assert not [f for f in os.listdir(str(out / "alone")) if "census" in f]


# ---- 4. holdout and limit ------------------------------------------------------------------------------------------------------
def test_holdout_and_limit_select_the_records_of_test_file(tmp_path):
    import torch
    bam, fa, vcf, locs = _two_contigs(tmp_path)
    assert len(locs) == 25
    ck = str(tmp_path / "ckpt.pth.tar")
    torch.save({"epoch": 1, "best_loss": 0.0, "optimizer": {},
                "state_dict": {"module." + k: torch.from_numpy(v) for k, v in random_state_dict(DanConfig(), seed=22).items()}}, ck)
    hdf = str(tmp_path / "candidates.hdf")
    _run_all([[sys.executable, CONVERTER, "--input", bam, "--fp_vcf", vcf, "--fasta-input", fa, "--output", hdf] + CONVERT_FLAGS])
    common = ["--modelload", ck, "--sample_vcf", vcf, "--save_vcf_records", "--reads-seed", "9", "--sites-per-launch", "16"] + MODEL_FLAGS
    direct = [sys.executable, MAIN, "--test_bam", bam, "--test_fasta", fa, "--record-census", "gpu"] + common
    to = lambda name: ["--save_vcf_records_file", str(tmp_path / (name + ".vcf"))]   # noqa: E731
    hold, lim = ["--test_holdout_chromosomes", "chrB"], ["--max-test-batches", "1", "--test-batch-size", "10"]
    _run_all([[sys.executable, MAIN, "--test_file", hdf] + common + to("file_all"),
              [sys.executable, MAIN, "--test_file", hdf] + common + hold + to("file_hold"),
              direct + hold + to("bam_hold"), direct + lim + ["--gpus", "2"] + to("bam_lim")], env=FORCE0)
    everything, held = _body(str(tmp_path / "epoch1_file_all.vcf")), _body(str(tmp_path / "epoch1_file_hold.vcf"))
    assert len(everything) == 24 and len(held) == 13 and all(l.startswith("chrB\t") for l in held)      # (one empty location on chrA)
    assert open(str(tmp_path / "epoch1_bam_hold.vcf"), "rb").read() == open(str(tmp_path / "epoch1_file_hold.vcf"), "rb").read()
    assert _body(str(tmp_path / "epoch1_bam_lim.vcf")) == everything[:20]


# ---- 6. candidate generation -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inflate", [[], ["--inflate-device", "gpu"]], ids=["host", "inflate_gpu"])
def test_candidate_generator_on_two_processes_writes_the_same_file(tmp_path, inflate):
    """chunk_size 5 kb: seven groups, dealt 3 + 4."""
    from dl4vc_amd.candidates import merge_parts
    fx = load("random")
    bam = write_bam(fx, str(tmp_path / "r.bam"))
    base = [sys.executable, GENERATOR, "--input", bam, "--chunk_size", "5", "--snp_min_freq", "0.075", "--indel_min_freq", "0.02",
            "--keep_multialleles", "--threads", "2"] + inflate
    to = lambda name: ["--output", str(tmp_path / (name + ".vcf"))]   # noqa: E731
    _run_all([base + to("one"), base + to("two") + ["--gpus", "2"], base + to("merged") + ["--shard", "0/2"],
              base + to("merged") + ["--shard", "1/2"]], env=FORCE0)
    want = open(str(tmp_path / "one.vcf"), "rb").read()
    run = [r for r in fx["runs"] if r["name"] == "chunk5"][0]
    assert _body(str(tmp_path / "one.vcf")) == run["lines"]
    assert open(str(tmp_path / "two.vcf"), "rb").read() == want
    parts = [len(open(str(tmp_path / ("merged.vcf.part%d" % g))).read().splitlines()) for g in (0, 1)]
    assert min(parts) > 0 and sum(parts) == len(run["lines"])
    stats = merge_parts(str(tmp_path / "merged.vcf"), 2)
    assert open(str(tmp_path / "merged.vcf"), "rb").read() == want
    assert stats["records"] == len(run["lines"]) and stats["groups"] == 7 and stats["subregions"] == 7
    assert not [f for f in os.listdir(str(tmp_path)) if ".part" in f]


# ---- 7. the script ---------------------------------------------------------------------------------------------------------------
def test_call_variants_sh_direct_on_two_gpus_equals_one(inputs):
    d, bam, fa, _long, vcf, _pos, ck = inputs
    outs = {}
    for name in ("sh_one", "sh_two"):
        (d / name).mkdir()
        open(str(d / name / "candidates.vcf"), "w").write(open(vcf).read())
        outs[name] = d / name
    script = ["bash", os.path.join(ROOT, "call_variants.sh"), "-m", ck, "-i", bam, "-r", fa, "-p", "2", "-d"]
    _run_all([script + ["-o", str(outs["sh_one"])], script + ["-o", str(outs["sh_two"]), "-g", "2"]], timeout=900, env=FORCE0)
    a = gzip.open(str(outs["sh_one"] / "called_variants.vcf.gz"), "rb").read()
    b = gzip.open(str(outs["sh_two"] / "called_variants.vcf.gz"), "rb").read()
    assert a == b and a.startswith(b"##fileformat")
    assert open(str(outs["sh_one"] / "epoch1_model_test.vcf"), "rb").read() == open(str(outs["sh_two"] / "epoch1_model_test.vcf"), "rb").read()
    log = open(str(outs["sh_two"] / "training.log")).read()
    assert "record_census='gpu'" in log and "shard 1/2 on device 0" in log and "census_s" in log
    assert "record_census=None" in open(str(outs["sh_one"] / "training.log")).read()

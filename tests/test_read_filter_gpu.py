"""The read filter by flags and mapping quality and the read census on the GPU: every BAM consumer run on X with ``--min-mapq /
--exclude-flags / --require-flags`` equals the same consumer run on X' = the filtered file (tools/subsample_bam.py) without them,
byte for byte -- the candidate generator (host framing and the device's frame kernel, MD and --reference walks), the GPU pileup
encoder (host framing and pileup_frame_kernel; pg_encode, pg_encode_device, pg_census) and main.py end to end -- and the census the
frame kernels count in LDS equals the host threads' and numpy's.  Fixture and filters: tests/read_filter_cases.py."""
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT
from dl4vc_amd import candgen, loader, pileup_gpu, read_filter
from tests import read_filter_cases as RC
from tests import subsample_cases as SC

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not pileup_gpu.available(), reason="libdl4vc_pileup.so not built")]
MAIN = os.path.join(ROOT, "main.py")
FORCE0 = dict(os.environ, DL4VC_FORCE_DEVICE0="1")
CHUNK_KB = 1                                                   # subregions of 1 kb: reads overlap two of them


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    return RC.write_fixture(tmp_path_factory.mktemp("read_filter_gpu"))


# ---- candidates ----------------------------------------------------------------------------------------------------------------
def candidates(bam, out, **kw):
    from dl4vc_amd.candidates import generate
    stats = generate(bam, out, chunk_size=CHUNK_KB, threads=2, snp_min_freq=0.075, indel_min_freq=0.02, **kw)
    return open(out, "rb").read(), stats


def positions(vcf):
    return {(l.split("\t")[0], int(l.split("\t")[1])) for l in vcf.decode().splitlines() if not l.startswith("#")}


@pytest.mark.parametrize("source", ["md", "reference"])
@pytest.mark.parametrize("inflate_device", [None, "gpu"])
def test_candidates_from_x_with_the_flags_are_those_of_the_filtered_file(fx, tmp_path, inflate_device, source):
    bam = fx["bam"] if source == "md" else fx["bare"]
    kw = dict(inflate_device=inflate_device, reference=fx["fasta"] if source == "reference" else None)
    plain, plain_stats = candidates(bam, str(tmp_path / "plain.vcf"), **kw)
    assert ("ctgB", RC.ISLAND) in positions(plain) and "read_seen" not in plain_stats
    for k, flt in enumerate(RC.FILTERS):
        for subsample in (None, RC.SUBSAMPLE):
            extra = {"subsample": subsample} if subsample else {}
            got, stats = candidates(bam, str(tmp_path / "with.vcf"), read_filter=flt, **extra, **kw)
            want, want_stats = candidates(RC.filtered(bam, flt, subsample), str(tmp_path / "prime.vcf"), **kw)
            assert got == want and got != plain, (flt, subsample, inflate_device, source)
            assert stats["reads"] == want_stats["reads"] == stats["read_kept"] and stats["candidates"] == want_stats["candidates"]
            # the census the device (or the host threads) counted: numpy over the records of every subregion
            assert read_filter.census_of(stats) == RC.census_numpy(RC.subregion_records(bam, CHUNK_KB), flt, subsample), (flt, subsample)
            if subsample:                                     # its records_seen is what passed region and filter: a run on the filtered file
                only, _ = candidates(RC.filtered(bam, flt), str(tmp_path / "only.vcf"), **kw)
                assert stats["subsample_records_seen"] == _["reads"] and stats["subsample_records_kept"] == stats["reads"]
        # a site that exists only through MAPQ-0 reads: the candidate disappears where the filter drops them
        assert (("ctgB", RC.ISLAND) in positions(got)) == (flt not in RC.ISLAND_DROPPED)
    # the census without a filter, and a filter of zeros
    stats_only, st = candidates(bam, str(tmp_path / "stats.vcf"), read_stats=True, **kw)
    assert stats_only == plain and read_filter.census_of(st) == RC.census_numpy(RC.subregion_records(bam, CHUNK_KB))
    assert st["read_seen"] == st["read_kept"] == plain_stats["reads"]
    zeros, zst = candidates(bam, str(tmp_path / "zeros.vcf"), read_filter=(0, 0, 0), **kw)
    assert zeros == plain and "read_seen" not in zst


def test_the_census_off_leaves_the_stats_zero_and_the_setter_refuses(fx):
    import ctypes as C
    with candgen.CandidateCounter(fx["bam"], inflate_device="gpu") as cc:
        cc.run([(0, 0, 4000), (1, 0, 3000)])
        st = read_filter.ReadStats()
        assert cc.lib.cg_get_read_stats(cc.h, C.byref(st)) == 0 and not any(st.flat().values())
        for bad in ((0x10000, 0, 0), (0, -1, 0), (0, 0, 256), (0x5, 0x4, 0)):
            assert cc.lib.cg_set_read_filter(cc.h, *bad) != 0 and "cg_set_read_filter: " in cc.lib.cg_last_error().decode()


def test_a_corrupt_record_with_an_excluded_flag_is_still_an_error(tmp_path):
    bam, fa, loc = RC.corrupt_bam(tmp_path)
    for inflate_device in (None, "gpu"):
        for flt in (None, (0x400, 0, 0)):
            with candgen.CandidateCounter(bam, inflate_device=inflate_device, read_filter=flt) as cc:
                with pytest.raises(RuntimeError, match="l_seq"):
                    cc.run([(0, 0, 600)])
            with pileup_gpu.GpuPileupEncoder(bam, fa, 16, 50, 10, 50, inflate_device=inflate_device, read_filter=flt) as enc:
                with pytest.raises(RuntimeError, match="l_seq"):
                    enc.encode([loc.contig], [loc.pos])


def test_candidate_generator_prints_its_line_and_sums_the_census_of_its_parts(fx, tmp_path):
    flt = RC.FILTERS[0]
    a = SC.run_tool("candidate_generator.py", "--input", fx["bam"], "--output", tmp_path / "a.vcf", "--inflate-device", "gpu", "--chunk_size",
                    CHUNK_KB, "--read-stats", *RC.flags_of(flt))
    b = SC.run_tool("candidate_generator.py", "--input", RC.filtered(fx["bam"], flt), "--output", tmp_path / "b.vcf", "--chunk_size", CHUNK_KB)
    two = SC.run_tool("candidate_generator.py", "--input", fx["bam"], "--output", tmp_path / "two.vcf", "--chunk_size", CHUNK_KB, "--gpus", 2,
                      "--read-stats", *RC.flags_of(flt), env=FORCE0)
    assert a.returncode == 0 and b.returncode == 0 and two.returncode == 0, (a.stderr[-1500:], b.stderr[-1500:], two.stderr[-1500:])
    read = lambda n: open(str(tmp_path / n), "rb").read()     # noqa: E731
    assert read("a.vcf") == read("b.vcf") == read("two.vcf")
    want = RC.census_numpy(RC.subregion_records(fx["bam"], CHUNK_KB), flt)
    line = "read filter: %d records seen, %d dropped by flags, %d dropped by MAPQ, %d kept" % tuple(want[k] for k in read_filter.TOTALS)
    for r in (a, two):                                        # the census of --gpus 2 is the sum of the parts'
        assert line in r.stdout and "read census:" in r.stdout and "  MAPQ 19 " in r.stdout, r.stdout[-1500:]
    assert "read filter" not in b.stdout and "read census" not in b.stdout


# ---- the GPU pileup encoder ------------------------------------------------------------------------------------------------------
def gpu_encoder(bam, fa, case, inflate_device=None, flt=None, subsample=None, read_stats=False):
    return pileup_gpu.GpuPileupEncoder.from_options(bam, fa, RC.options(case, flt, subsample, read_stats), 0, inflate_device)


def all_three(bam, fa, case, inflate_device, flt=None, subsample=None, read_stats=False):
    """-> (pg_encode's six arrays, pg_census' statuses, pg_encode_device's planes / num_reads / statuses, the census of each call)."""
    import torch
    contigs, pos = [l.contig for l in case.locs], [l.pos for l in case.locs]
    with gpu_encoder(bam, fa, case, inflate_device, flt, subsample, read_stats) as enc:
        planes = enc.encode(contigs, pos)
        c1 = enc.read_stats()
        census = enc.census(contigs, pos)
        c2 = enc.read_stats()
        out = [torch.zeros((len(pos), case.max_reads, 2 * case.w + 1), dtype=torch.uint8, device="cuda:0") for _ in range(3)]
        r = enc.encode_device(contigs, pos, out=out)
        torch.cuda.synchronize()
        c3 = enc.read_stats()
        dev = [o.cpu().numpy() for o in out] + [np.asarray(r[4]), np.asarray(r[5])]
        return planes, census, dev, (c1, c2, c3)


def counts_of_rule(bam, fa, case, inflate_device, flt, subsample):
    """The records the sample rule drops behind the filter, from the encoder's subsample stats (seen = passed region and filter)."""
    with gpu_encoder(bam, fa, case, inflate_device, flt, subsample) as enc:
        enc.encode([l.contig for l in case.locs], [l.pos for l in case.locs])
        st = enc.subsample_stats()
    return st["records_seen"] - st["records_kept"]


def same_device(a, b, what):
    assert np.array_equal(a[4], b[4]) and np.array_equal(a[3], b[3]), (what, "status / num_reads")
    enc = a[4] == 1
    for k in range(3):
        assert np.array_equal(a[k][enc], b[k][enc]), (what, k)


@pytest.mark.parametrize("inflate_device", [None, "gpu"])
def test_the_gpu_encoder_on_x_with_the_flags_is_itself_on_the_filtered_file(fx, inflate_device):
    bam, fa, case = fx["bam"], fx["fasta"], fx["case"]
    plain, plain_census, plain_dev, plain_counts = all_three(bam, fa, case, inflate_device)
    assert not any(v for c in plain_counts for v in c.values())          # the census off leaves the stats zero
    deep = [i for i, l in enumerate(case.locs) if l.pos == RC.DEEP][0]
    island = [i for i, l in enumerate(case.locs) if l.pos == RC.ISLAND][0]
    assert plain[5][deep] == 2 and plain[5][island] == 1                  # 1 038 tracks: declined without the filter
    zeros, zc, zd, _ = all_three(bam, fa, case, inflate_device, (0, 0, 0))
    SC.same_planes(zeros, plain, "a filter of zeros is not calling the setter")
    assert np.array_equal(zc, plain_census)
    same_device(zd, plain_dev, "zeros")
    stats_only, sc, sd, counted = all_three(bam, fa, case, inflate_device, read_stats=True)
    SC.same_planes(stats_only, plain, "the census changes no plane")
    assert counted[0] == counted[1] == counted[2] and counted[0]["read_seen"] == counted[0]["read_kept"] > 1000
    for flt in RC.FILTERS:
        for subsample in (None, RC.SUBSAMPLE):
            prime = RC.filtered(bam, flt, subsample)
            got, got_census, got_dev, counts = all_three(bam, fa, case, inflate_device, flt, subsample)
            want, want_census, want_dev, prime_counts = all_three(prime, fa, case, inflate_device, read_stats=True)
            SC.same_planes(got, want, (flt, subsample, inflate_device))
            assert np.array_equal(got_census, want_census), (flt, subsample)
            same_device(got_dev, want_dev, (flt, subsample))
            assert counts[0] == counts[1] == counts[2]                   # the same census from encode, census and encode_device
            c = read_filter.census_of(counts[0])
            assert c["seen"] == counted[0]["read_seen"] and c["mapq_hist"] == read_filter.census_of(counted[0])["mapq_hist"]
            # kept is what the filtered (and subsampled) file holds for the same runs; without the rule nothing else is lost
            assert c["kept"] == prime_counts[0]["read_seen"] == prime_counts[0]["read_kept"]
            assert c["seen"] - c["dropped_flags"] - c["dropped_mapq"] - c["kept"] == (0 if subsample is None else
                                                                                         counts_of_rule(bam, fa, case, inflate_device, flt, subsample))
            assert (got[5][island] == 0) == (flt in RC.ISLAND_DROPPED)


def test_the_device_census_is_the_host_census_and_numpy(fx):
    """The census the frame kernel counted in LDS (inflate on) equals the host threads' (inflate off) and numpy: with the filter
    off, on, and with subsample.  One location per call is one run, its fetch window; all locations in one call are fewer runs
    (near locations share one), where the two paths must still agree with each other."""
    bam, fa, case = fx["bam"], fx["fasta"], fx["case"]
    contigs, pos = [l.contig for l in case.locs], [l.pos for l in case.locs]
    for flt, subsample in ((None, None), (RC.FILTERS[0], None), (RC.FILTERS[1], None), (RC.FILTERS[2], RC.SUBSAMPLE)):
        whole = []
        for inflate_device in (None, "gpu"):
            with gpu_encoder(bam, fa, case, inflate_device, flt, subsample, read_stats=True) as enc:
                enc.census(contigs, pos)
                whole.append(enc.read_stats())
        assert whole[0] == whole[1] and whole[0]["read_seen"] > 1000, (flt, subsample)
    for inflate_device in (None, "gpu"):
        for flt, subsample in ((None, None), (RC.FILTERS[0], None), (RC.FILTERS[2], RC.SUBSAMPLE)):
            with gpu_encoder(bam, fa, case, inflate_device, flt, subsample, read_stats=True) as enc:
                total = {}
                for l in case.locs:
                    enc.encode([l.contig], [l.pos])
                    for k, v in enc.read_stats().items():
                        total[k] = total.get(k, 0) + v
            assert read_filter.census_of(total) == RC.census_numpy(RC.window_records(bam, case), flt or (0, 0, 0), subsample), (inflate_device, flt)


def test_the_track_limit_sees_the_kept_reads_alone(fx):
    """The site of 1 060 records, 22 of them duplicates and 22 supplementary: declined without the filter (1 038 tracks), encoded
    with -F 0x800 (1 016 tracks) -- the bytes pe_encode writes on the filtered file.

    The issue asked for this with the duplicates and -F 0x400.  That cannot hold: the encoder's own mask 0x704 drops duplicates in
    front of its track limit (pinned by the depth case of tests/pileup_cases.py, "flag-masked reads between the tracks: they do
    not count"), and the issue leaves that mask and every decline reason as they are.  So the case is carried by a flag outside
    0x704, and the duplicates are held to what is true of them: -F 0x400 gives the answer of the filtered file, here a decline."""
    bam, fa, case = fx["bam"], fx["fasta"], fx["case"]
    flt = (0x800, 0, 0)
    contigs, pos = ["ctgB"], [RC.DEEP]
    for inflate_device in (None, "gpu"):
        with gpu_encoder(bam, fa, case, inflate_device) as enc:
            assert enc.encode(contigs, pos)[5].tolist() == [2]
        with gpu_encoder(bam, fa, case, inflate_device, (0x400, 0, 0)) as enc, \
                gpu_encoder(RC.filtered(bam, (0x400, 0, 0)), fa, case, inflate_device) as prime:
            assert enc.encode(contigs, pos)[5].tolist() == prime.encode(contigs, pos)[5].tolist() == [2]
        with gpu_encoder(bam, fa, case, inflate_device, flt) as enc:
            got = enc.encode(contigs, pos)
        assert got[5].tolist() == [1]
        with loader.NativePileupEncoder.from_options(RC.filtered(bam, flt), fa, RC.options(case)) as cpu:
            SC.same_planes(got, cpu.encode(contigs, pos, 1), ("track limit", inflate_device))


def test_pg_set_read_filter_refuses_with_the_reason(fx):
    with gpu_encoder(fx["bam"], fx["fasta"], fx["case"]) as enc:
        for bad in ((0x10000, 0, 0), (0, 0x10000, 0), (0, 0, 256), (0, 0, -1), (0x5, 0x4, 0)):
            with pytest.raises(RuntimeError, match="pg_set_read_filter: "):
                enc.set_read_filter(*bad)


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def test_main_py_test_bam_with_the_flags_writes_the_scored_vcf_of_the_filtered_file(fx, tmp_path):
    import torch
    from dl4vc_amd.config import DanConfig
    from oracle.dan_oracle import random_state_dict
    from tests.test_cli_gpu import MODEL_FLAGS
    from tests.test_record_census_gpu import _run_all
    flt = RC.FILTERS[0]
    bam, fa, prime = fx["bam"], fx["fasta"], RC.filtered(fx["bam"], RC.FILTERS[0])
    vcf = str(tmp_path / "candidates.vcf")
    candidates(bam, vcf)                                          # (the candidates of the unfiltered BAM: more locations than X' has records for)
    ck = str(tmp_path / "ckpt.pth.tar")
    torch.save({"epoch": 1, "best_loss": 0.0, "optimizer": {},
                "state_dict": {"module." + k: torch.from_numpy(v) for k, v in random_state_dict(DanConfig(), seed=21).items()}}, ck)
    common = ["--modelload", ck, "--sample_vcf", vcf, "--save_vcf_records", "--reads-seed", "5", "--sites-per-launch", "64"] + MODEL_FLAGS
    flags = RC.flags_of(flt) + ["--read-stats"]
    runs = {"plain": (bam, []), "with": (bam, flags), "prime": (prime, []), "with2": (bam, flags + ["--record-census", "gpu", "--gpus", "2"])}
    cmds = []
    for name, (b, extra) in runs.items():
        (tmp_path / name).mkdir()
        cmds.append([sys.executable, MAIN, "--test_bam", b, "--test_fasta", fa, "--save_vcf_records_file", str(tmp_path / name / "model_test.vcf")] +
                    common + extra)
    outs = dict(zip(runs, _run_all(cmds, env=FORCE0)))
    text = {name: open(str(tmp_path / name / "epoch1_model_test.vcf"), "rb").read() for name in runs}
    assert text["with"] == text["prime"] == text["with2"]
    assert text["with"] != text["plain"] and len(text["with"].splitlines()) > 40
    m = re.search(r"read filter: (\d+) records seen, (\d+) dropped by flags, (\d+) dropped by MAPQ, (\d+) kept", outs["with"])
    assert m and int(m.group(3)) > 0 and int(m.group(1)) == int(m.group(2)) + int(m.group(3)) + int(m.group(4)), outs["with"][-1500:]
    assert "read census:" in outs["with"] and "read filter" not in outs["prime"] and "read filter" not in outs["plain"]
    # the two shards of the census run print their own scoring calls' counts (the census pass keeps a stage of its own): each line
    # adds up, and together they are not the double of the one-process run
    lines = re.findall(r"read filter: (\d+) records seen, (\d+) dropped by flags, (\d+) dropped by MAPQ, (\d+) kept", outs["with2"])
    assert len(lines) == 2 and all(int(a) == int(b) + int(c) + int(d) for a, b, c, d in lines), outs["with2"][-2000:]
    assert 0.75 * int(m.group(1)) <= sum(int(a) for a, _b, _c, _d in lines) <= 1.25 * int(m.group(1))


def test_one_train_bam_epoch_gives_the_losses_and_checkpoint_of_the_filtered_file(tmp_path):
    """--exclude-flags 16 on the labelled fixture of the training tests (its reads differ in strand, not in MAPQ): both BAMs of the
    run take the filter, and the loss lines, the scored VCF and the checkpoint are those of the run on the filtered file."""
    import torch
    from tests import train_bam_cases as TC
    from tests.test_train_bam_gpu import run_main
    from tests.test_train_loader_device_gpu import loss_lines
    fx = TC.labelled_fixture(tmp_path)
    flt = (16, 0, 0)
    recs = RC.parsed(fx["bam"])
    assert 0.2 < sum(bool(r.flag & 16) for r in recs) / len(recs) < 0.8
    prime = dict(fx, bam=RC.filtered(fx["bam"], flt))
    (ra, da), (rb, db) = run_main(fx, "rf_with", "bam", extra=RC.flags_of(flt) + ["--epochs", "1"]), run_main(prime, "rf_prime", "bam", extra=["--epochs", "1"])
    la, lb = loss_lines(ra.stdout), loss_lines(rb.stdout)
    assert len(la) >= 2 and la == lb
    va, vb = (open(os.path.join(x, "epoch1_model_test.vcf"), "rb").read() for x in (da, db))
    assert va == vb and len(va.splitlines()) > 15
    sa, sb = (torch.load(os.path.join(x, "model.pth_epoch1.tar"), map_location="cpu", weights_only=False) for x in (da, db))
    assert sorted(sa["state_dict"]) == sorted(sb["state_dict"]) and len(sa["state_dict"]) > 20
    for k, v in sa["state_dict"].items():
        assert torch.equal(v, sb["state_dict"][k]), k

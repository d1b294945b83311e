"""Read subsampling by name hash on the GPU: every BAM consumer run on X with ``--subsample F --subsample-seed S`` equals the same
consumer run on X' = tools/subsample_bam.py(X, F, S) without it, byte for byte -- the candidate generator (host framing and the
device's frame kernel, MD and --reference), the GPU pileup encoder (host framing and pileup_frame_kernel) with its census, and the
tools end to end.  The fixtures and the conditions that keep the equalities from being vacuous are those of
tests/test_subsample_host.py / tests/subsample_cases.py."""
import gzip
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from dl4vc_amd import bamio, candgen, loader, pileup_gpu
from tests import pileup_cases as PC
from tests import subsample_cases as SC
from tests import train_bam_cases as TC

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not pileup_gpu.available(), reason="libdl4vc_pileup.so not built")]
F = SC.FRACTION
MAIN = os.path.join(ROOT, "main.py")
FORCE0 = dict(os.environ, DL4VC_FORCE_DEVICE0="1")


# ---- candidates ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def blocks(tmp_path_factory):
    fx = SC.write_block_bams(tmp_path_factory.mktemp("subsample_blocks_gpu"))
    layout = SC.block_layout(fx["md"])
    assert layout[0] >= 3 and layout[1] >= 1, layout         # the device arms inflate several blocks, records across their ends
    return fx


def candidates(bam, out, inflate_device=None, reference=None, subsample=None):
    """candidates.vcf of the whole BAM in subregions of 4 kb (reads overlap two of them) -> (the file's bytes, the summary)."""
    from dl4vc_amd.candidates import generate
    stats = generate(bam, out, chunk_size=4, threads=2, inflate_device=inflate_device, reference=reference, subsample=subsample)
    return open(out, "rb").read(), stats


@pytest.mark.parametrize("source", ["md", "reference"])
@pytest.mark.parametrize("inflate_device", [None, "gpu"])
def test_candidates_from_x_with_the_option_are_those_of_x_prime(blocks, tmp_path, inflate_device, source):
    bam = blocks["md"] if source == "md" else blocks["bare"]
    kw = dict(inflate_device=inflate_device, reference=blocks["fasta"] if source == "reference" else None)
    plain, plain_stats = candidates(bam, str(tmp_path / "plain.vcf"), **kw)
    body = [l for l in plain.decode().splitlines() if not l.startswith("#")]
    assert len(body) > 100 and plain_stats["reads"] > 3212       # (reads across a subregion's end are listed in both)
    for seed in SC.SEEDS:
        assert 0.35 <= SC.kept_share(bam, F, seed) <= 0.65
        sub = SC.subsampled(bam, F, seed)
        got, stats = candidates(bam, str(tmp_path / ("with_%d.vcf" % seed)), subsample=(F, seed), **kw)
        want, want_stats = candidates(sub, str(tmp_path / ("prime_%d.vcf" % seed)), **kw)
        assert got == want, (seed, inflate_device, source)
        assert got != plain                                   # at least one candidate moves: the equality is not vacuous
        assert stats["subsample_records_kept"] == stats["reads"] == want_stats["reads"]
        assert stats["subsample_records_seen"] == plain_stats["reads"] > stats["reads"]
        assert stats["candidates"] == want_stats["candidates"]
    whole, whole_stats = candidates(bam, str(tmp_path / "whole.vcf"), subsample=(1.0, 5), **kw)
    assert whole == plain and whole_stats["subsample_records_kept"] == whole_stats["subsample_records_seen"] == plain_stats["reads"]


def test_candidate_generator_prints_its_line_and_the_setter_refuses(blocks, tmp_path):
    bam = blocks["md"]
    sub = SC.subsampled(bam, F, 7)
    a = SC.run_tool("candidate_generator.py", "--input", bam, "--output", tmp_path / "a.vcf", "--subsample", F, "--subsample-seed", 7,
                    "--inflate-device", "gpu", "--chunk_size", 4)
    b = SC.run_tool("candidate_generator.py", "--input", sub, "--output", tmp_path / "b.vcf", "--inflate-device", "gpu", "--chunk_size", 4)
    assert a.returncode == 0 and b.returncode == 0, (a.stderr[-1500:], b.stderr[-1500:])
    assert open(str(tmp_path / "a.vcf"), "rb").read() == open(str(tmp_path / "b.vcf"), "rb").read()
    m = re.search(r"subsample: (\d+) records seen, (\d+) kept \((0\.\d+)\); asked 0\.5, seed 7", a.stdout)
    assert m and 0.35 <= int(m.group(2)) / int(m.group(1)) <= 0.65, a.stdout[-800:]
    assert "subsample:" not in b.stdout
    with candgen.CandidateCounter(bam) as cc:
        for bad in (-0.1, 1.5, float("nan")):
            assert cc.lib.cg_set_subsample(cc.h, bad, 0) != 0
            assert "fraction must lie in [0, 1]" in cc.lib.cg_last_error().decode()


# ---- the GPU pileup encoder ------------------------------------------------------------------------------------------------------
def gpu_encoder(bam, fa, case, inflate_device=None, subsample=None):
    return pileup_gpu.GpuPileupEncoder.from_options(bam, fa, SC.options(case, subsample), 0, inflate_device)


def both(bam, fa, case, contigs, pos, inflate_device, subsample=None):
    """-> (the six arrays of ``encode``, the census statuses, the counts of the encode call)."""
    with gpu_encoder(bam, fa, case, inflate_device, subsample) as enc:
        planes = enc.encode(contigs, pos)
        counts = (enc.subsample_stats(), enc.stats()["records"])
        return planes, enc.census(contigs, pos), counts


@pytest.mark.parametrize("name", PC.CASE_NAMES + ["subsample_names"])
def test_the_gpu_encoder_on_x_with_the_option_is_itself_on_x_prime(tmp_path, name):
    case = SC.named_case() if name == "subsample_names" else PC.get_case(name)
    bam, fa = PC.write_case(tmp_path, case)
    contigs, pos = [l.contig for l in case.locs], [l.pos for l in case.locs]
    for inflate_device in ([None, "gpu"] if case.index else [None]):
        plain, plain_census, (plain_counts, _n) = both(bam, fa, case, contigs, pos, inflate_device)
        assert plain_counts["records_seen"] == plain_counts["records_kept"]
        whole, _c, _k = both(bam, fa, case, contigs, pos, inflate_device, (1.0, 9))
        SC.same_planes(whole, plain, "F = 1.0 keeps all")
        differs = False
        for seed in SC.SEEDS:
            sub = SC.subsampled(bam, F, seed)
            if not case.index and os.path.isfile(sub + ".bai"):
                os.remove(sub + ".bai")
            got, got_census, (counts, n_records) = both(bam, fa, case, contigs, pos, inflate_device, (F, seed))
            want, want_census, (_wc, want_records) = both(sub, fa, case, contigs, pos, inflate_device)
            SC.same_planes(got, want, (name, inflate_device, seed))
            assert np.array_equal(got_census, want_census), (name, inflate_device, seed)
            assert counts["records_kept"] == n_records == want_records
            assert counts["records_seen"] == plain_counts["records_seen"] >= counts["records_kept"]
            differs = differs or any(not np.array_equal(a, b) for a, b in zip(got, plain))
        if len(case.reads) >= 200:
            assert differs, "the sampled planes equal the unsampled ones"


@pytest.mark.parametrize("inflate_device", [None, "gpu"])
def test_the_rule_sits_in_front_of_the_plan(tmp_path, inflate_device):
    """The 1 500-track site is declined unsampled (more than 1 024 tracks); at F = 0.5 its ~750 kept tracks are encoded on the GPU
    and the planes are ``pe_encode``'s on X'."""
    case = PC.get_case("depth")
    bam, fa = PC.write_case(tmp_path, case)
    i = [k for k, l in enumerate(case.locs) if l.note == "1500 tracks"][0]
    contigs, pos = [case.locs[i].contig], [case.locs[i].pos]
    with gpu_encoder(bam, fa, case, inflate_device) as enc:
        assert enc.encode(contigs, pos)[5].tolist() == [2]
    for seed in SC.SEEDS:
        sub = SC.subsampled(bam, F, seed)
        with gpu_encoder(bam, fa, case, inflate_device, (F, seed)) as enc:
            got = enc.encode(contigs, pos)
        assert got[5].tolist() == [1]
        with loader.NativePileupEncoder.from_options(sub, fa, SC.options(case)) as cpu:
            SC.same_planes(got, cpu.encode(contigs, pos, 1), ("track limit", inflate_device, seed))


def test_the_names_of_1_and_254_characters_are_among_the_tracks(tmp_path):
    case = SC.named_case()
    bam, _fa = PC.write_case(tmp_path, case)
    for seed in SC.SEEDS:
        with bamio.BamFile(bam, subsample=(F, seed)) as b:
            lengths = {len(r.name) for r in b.fetch(0, 282, 319)}         # the window of the location at 300 (w = 16)
        assert {1, 254} <= lengths, (seed, sorted(lengths))


def test_pg_set_subsample_refuses_with_the_reason(tmp_path):
    case = PC.get_case("qualities")
    bam, fa = PC.write_case(tmp_path, case)
    with gpu_encoder(bam, fa, case) as enc:
        for bad in (-0.1, 1.5, float("nan")):
            with pytest.raises(RuntimeError, match=r"fraction must lie in \[0, 1\]"):
                enc.set_subsample(bad, 0)
        enc.set_subsample(0.5, 1)
        enc.set_subsample(0.0, 0)                             # off again
        contigs, pos = [l.contig for l in case.locs], [l.pos for l in case.locs]
        off = enc.encode(contigs, pos)
    with gpu_encoder(bam, fa, case) as enc:
        SC.same_planes(off, enc.encode(contigs, pos), "fraction 0 turns it off again")


# ---- end to end ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    import torch
    from dl4vc_amd.config import DanConfig
    from oracle.dan_oracle import random_state_dict
    from tests.test_score_bam_gpu import _fixture
    d = tmp_path_factory.mktemp("subsample_score_bam")
    bam, fa, vcf, plain, _pos = _fixture(d)
    ck = str(d / "ckpt.pth.tar")
    torch.save({"epoch": 1, "best_loss": 0.0, "optimizer": {},
                "state_dict": {"module." + k: torch.from_numpy(v) for k, v in random_state_dict(DanConfig(), seed=21).items()}}, ck)
    assert 0.35 <= SC.kept_share(bam, F, 7) <= 0.65
    return d, bam, fa, vcf, plain, ck, SC.subsampled(bam, F, 7)


def test_main_py_test_bam_with_the_option_writes_the_scored_vcf_of_x_prime(inputs):
    from tests.test_cli_gpu import MODEL_FLAGS
    from tests.test_record_census_gpu import _run_all
    d, bam, fa, vcf, _plain, ck, sub = inputs
    common = ["--modelload", ck, "--sample_vcf", vcf, "--save_vcf_records", "--reads-seed", "5", "--sites-per-launch", "16"] + MODEL_FLAGS
    flags = ["--subsample", str(F), "--subsample-seed", "7"]
    runs = {"plain": (bam, []), "with": (bam, flags), "prime": (sub, []), "with2": (bam, flags + ["--record-census", "gpu", "--gpus", "2"]),
            "prime2": (sub, ["--record-census", "gpu", "--gpus", "2"])}
    cmds = []
    for name, (b, extra) in runs.items():
        (d / name).mkdir()
        cmds.append([sys.executable, MAIN, "--test_bam", b, "--test_fasta", fa, "--save_vcf_records_file", str(d / name / "model_test.vcf")] +
                    common + extra)
    outs = dict(zip(runs, _run_all(cmds, env=FORCE0)))
    text = {name: open(str(d / name / "epoch1_model_test.vcf"), "rb").read() for name in runs}
    assert text["with"] == text["prime"] == text["with2"] == text["prime2"]
    assert text["with"] != text["plain"] and len(text["with"].splitlines()) > 40
    m = re.search(r"subsample: (\d+) records seen, (\d+) kept \(0\.\d+\); asked 0\.5, seed 7", outs["with"])
    assert m and 0.35 <= int(m.group(2)) / int(m.group(1)) <= 0.65, outs["with"][-1500:]
    assert "subsample:" not in outs["prime"] and "subsample:" not in outs["plain"]


def test_call_variants_sh_direct_with_s_equals_the_script_on_x_prime(inputs):
    """-d -f -s 0.5 -S 7: candidate generation (reads without MD, walked against the reference) and main.py --test_bam thin the
    same reads, so every file of the run is that of the script on X'."""
    d, bam, fa, _vcf, _plain, ck, sub = inputs
    outs = {}
    for name, b, flag in (("cv_with", bam, ["-s", str(F), "-S", "7"]), ("cv_prime", sub, []), ("cv_plain", bam, [])):
        out = d / name
        r = subprocess.run(["bash", os.path.join(ROOT, "call_variants.sh"), "-m", ck, "-o", str(out), "-i", b, "-r", fa, "-p", "2", "-d", "-f"] + flag,
                           capture_output=True, text=True, timeout=900)
        logs = "".join(open(str(out / f)).read()[-1200:] for f in ("candidate_generator.log", "training.log") if (out / f).exists())
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:], logs)
        outs[name] = out
    read = lambda name, f: open(str(outs[name] / f), "rb").read()   # noqa: E731
    cands = read("cv_with", "candidates.vcf")
    assert cands == read("cv_prime", "candidates.vcf") != read("cv_plain", "candidates.vcf")
    assert len([l for l in cands.decode().splitlines() if not l.startswith("#")]) > 20
    assert read("cv_with", "epoch1_model_test.vcf") == read("cv_prime", "epoch1_model_test.vcf") != read("cv_plain", "epoch1_model_test.vcf")
    a, b = (gzip.open(str(outs[n] / "called_variants.vcf.gz"), "rb").read() for n in ("cv_with", "cv_prime"))
    assert a == b and a.startswith(b"##fileformat")
    assert "subsample:" in open(str(outs["cv_with"] / "candidate_generator.log")).read()
    assert "subsample:" in open(str(outs["cv_with"] / "training.log")).read()


@pytest.fixture(scope="module")
def labelled(tmp_path_factory):
    fx = TC.labelled_fixture(tmp_path_factory.mktemp("subsample_train_bam"))
    prime = dict(fx, bam=SC.subsampled(fx["bam"], F, 7))
    return fx, prime


@pytest.mark.parametrize("inflate_device", [None, "gpu"])
def test_resident_records_from_x_with_the_option_hold_the_blob_of_x_prime(labelled, inflate_device):
    from dl4vc_amd.chunk_loader import ResidentRecords
    fx, prime = labelled
    locs = TC.locations(fx, "train")
    kw = dict(capacity_bytes=1 << 30, slab_bytes=1 << 20, round_locations=16, inflate_device=inflate_device)
    with ResidentRecords.from_bam(fx["bam"], fx["fasta"], locs, 100, 8, subsample=(F, 7), **kw) as got, \
            ResidentRecords.from_bam(prime["bam"], fx["fasta"], locs, 100, 8, **kw) as want, \
            ResidentRecords.from_bam(fx["bam"], fx["fasta"], locs, 100, 8, **kw) as plain:
        assert len(got) == len(want) > 30 and got.blob.tobytes() == want.blob.tobytes()
        for i in range(len(want)):
            assert got.store.record(i) == want.store.record(i), i
        assert got.blob.tobytes() != plain.blob.tobytes()      # (num_reads of the deep sites)
        assert got.stage["gpu"] > plain.stage["gpu"]          # the 1 100-track site is encoded on the GPU at half its depth


def test_one_train_bam_run_gives_the_losses_and_checkpoint_of_x_prime(labelled):
    import torch
    from tests.test_train_bam_gpu import run_main
    from tests.test_train_loader_device_gpu import loss_lines
    fx, prime = labelled
    flags = ["--subsample", str(F), "--subsample-seed", "7"]
    (ra, da), (rb, db) = run_main(fx, "sub_with", "bam", extra=flags), run_main(prime, "sub_prime", "bam")
    la, lb = loss_lines(ra.stdout), loss_lines(rb.stdout)
    assert len(la) >= 5 and la == lb
    for epoch in (1, 2):
        va, vb = (open(os.path.join(x, "epoch%d_model_test.vcf" % epoch), "rb").read() for x in (da, db))
        assert va == vb and len(va.splitlines()) > 15
        sa, sb = (torch.load(os.path.join(x, "model.pth_epoch%d.tar" % epoch), map_location="cpu", weights_only=False) for x in (da, db))
        assert sorted(sa["state_dict"]) == sorted(sb["state_dict"]) and len(sa["state_dict"]) > 20
        for k, v in sa["state_dict"].items():
            assert torch.equal(v, sb["state_dict"][k]), (epoch, k)

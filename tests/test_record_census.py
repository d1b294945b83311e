"""The host side of ``--record-census gpu`` and of ``tools/candidate_generator.py --gpus N`` without a GPU: the shard plan
against a brute-force enumeration, the side-file exchange, the refusals, the merge of candidate parts."""
import os
import sys
import threading
import time

import numpy as np
import pytest

from conftest import ROOT
from dl4vc_amd import candidates as C
from dl4vc_amd.shard import census_path, part_path, plan_bam_shard, remove_census, shard_range, wait_census, write_census


# ---- plan_bam_shard --------------------------------------------------------------------------------------------------------
def _enumerate(flags, held, limit):
    """(location, record index) of the selected records, the slow way."""
    pairs, k = [], 0
    for i, f in enumerate(flags):
        if f:
            if held is None or held[i]:
                pairs.append((i, k))
            k += 1
    return pairs[:limit] if limit > 0 else pairs


def _walk(flags, runs):
    """The (location, record index) pairs scoring the runs gives, and the locations it visits."""
    pairs, visited = [], []
    for lo, hi, first in runs:
        assert 0 <= lo < hi <= len(flags)
        k = first
        for i in range(lo, hi):
            visited.append(i)
            if flags[i]:
                pairs.append((i, k))
                k += 1
    return pairs, visited


@pytest.mark.parametrize("n", [0, 1, 7, 64, 1000])
def test_plan_bam_shard_equals_the_enumeration(n):
    rng = np.random.default_rng(n)
    arrays = [np.zeros(n, np.uint8), np.ones(n, np.uint8)] + [(rng.random(n) < p).astype(np.uint8) for p in (0.5, 0.9, 0.1, 0.02)]
    masks = [None, np.ones(n, bool), np.zeros(n, bool), rng.random(n) < 0.5, np.arange(n) >= n // 2, np.arange(n) % 10 < 3]
    for flags in arrays:
        records = int(flags.sum())
        for held in masks:
            for limit in (0, 1, 5, max(1, records // 2), records + 3):
                want = _enumerate(flags, held, limit)
                for count in (1, 2, 3, 8):
                    got, visited = [], []
                    for g in range(count):
                        runs = plan_bam_shard(flags, held, limit, g, count)
                        pairs, seen = _walk(flags, runs)
                        a, b = shard_range(len(want), g, count)
                        assert pairs == want[a:b], (n, limit, g, count)         # also where count exceeds the record count
                        assert all(held is None or held[i] for i, _k in pairs)
                        got += pairs
                        visited += seen
                    assert got == want
                    assert visited == sorted(set(visited))                       # no location twice, in order
                    if held is None and limit == 0 and records:
                        assert visited == list(range(n))                         # every empty location's flag is checked too


def test_plan_bam_shard_refuses_a_mask_of_another_length_and_a_bad_shard():
    with pytest.raises(ValueError, match="held_out"):
        plan_bam_shard(np.ones(4, np.uint8), np.ones(3, bool))
    with pytest.raises(ValueError):
        plan_bam_shard(np.ones(4, np.uint8), None, 0, 2, 2)


# ---- the side files ----------------------------------------------------------------------------------------------------------
def test_census_side_files_are_atomic_and_a_missing_one_is_named(tmp_path):
    out = str(tmp_path / "epoch1_model_test.vcf")
    assert census_path(out, 1) == part_path(out, 1) + ".census"
    a, b = (np.arange(300_000) % 3 == 0).astype(np.uint8), np.ones(5, np.uint8)
    got = {}

    def reader():
        got["flags"] = wait_census(out, 2, [len(a), len(b)], timeout_s=30.0, poll_s=0.001)

    t = threading.Thread(target=reader)
    t.start()                                                # the reader is first: it sees a file only when it is whole
    write_census(census_path(out, 1), b)
    names = []
    real_replace = os.replace

    def watched(src, dst):
        names.append((os.path.basename(src), os.path.getsize(src), os.path.exists(dst)))
        real_replace(src, dst)

    os.replace = watched
    try:
        write_census(census_path(out, 0), a)
    finally:
        os.replace = real_replace
    t.join(30.0)
    assert not t.is_alive() and np.array_equal(got["flags"], np.concatenate([a, b]))
    # written under another name in full, then renamed: the final name never held a part of it
    assert names == [("epoch1_model_test.vcf.part0.census.tmp%d" % os.getpid(), len(a), False)]
    assert sorted(os.listdir(str(tmp_path))) == ["epoch1_model_test.vcf.part0.census", "epoch1_model_test.vcf.part1.census"]
    with pytest.raises(RuntimeError, match="shard 0/2 holds 300000 flags for 7 locations"):
        wait_census(out, 2, [7, 5], timeout_s=1.0)
    os.remove(census_path(out, 1))
    t0 = time.monotonic()
    with pytest.raises(RuntimeError, match=r"shard 1/2 did not arrive within 0\.3 s .*part1\.census is missing"):
        wait_census(out, 2, [len(a), 5], timeout_s=0.3, poll_s=0.01)
    assert time.monotonic() - t0 < 5.0
    remove_census(out, 2)
    remove_census(out, 2)                                    # (nothing left is no error)
    assert os.listdir(str(tmp_path)) == []


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_main_refuses_the_flag_without_test_bam_and_another_value():
    sys.path.insert(0, ROOT)
    import main as cli
    base = ["--modelload", "c.pt", "--model_pool_combine_dimension", "0", "--sample_vcf", "c.vcf", "--test_fasta", "r.fa"]
    with pytest.raises(SystemExit, match="--record-census gpu is an option of --test_bam"):
        cli.main(base + ["--test_file", "x.hdf", "--record-census", "gpu"])
    with pytest.raises(SystemExit, match="--record-census must be gpu"):
        cli.main(base + ["--test_bam", "x.bam", "--record-census", "cpu"])
    # without the flag the refusals stand, and now name it
    for extra, text in ((["--gpus", "2"], "--test_bam runs on one GPU"), (["--shard", "0/2"], "--test_bam runs on one GPU"),
                        (["--test_holdout_chromosomes", "chr20"], "test_holdout_chromosomes is not supported")):
        with pytest.raises(SystemExit) as e:
            cli.main(base + ["--test_bam", "x.bam"] + extra)
        assert text in str(e.value) and str(e.value).endswith("--record-census gpu"), str(e.value)
    assert cli.GPUS_WITH_BAM.endswith("--record-census gpu")
    # with it they pass the check
    from arguments import parse_args
    cli.check_bam_arguments(parse_args(base + ["--test_bam", "x.bam", "--record-census", "gpu", "--gpus", "2", "--test_holdout_chromosomes",
                                               "chr20"]))
    cli.check_bam_arguments(parse_args(base + ["--test_bam", "x.bam", "--record-census", "gpu", "--shard", "1/3"]))
    args = parse_args(base + ["--test_bam", "x.bam", "--record-census", "gpu"])
    assert args.record_census == "gpu" and args.census_timeout == 600.0
    assert parse_args(base + ["--test_bam", "x.bam"]).record_census is None


def test_candidate_generator_takes_the_two_flags_and_refuses_a_bad_shard():
    import subprocess
    tool = os.path.join(ROOT, "tools", "candidate_generator.py")
    r = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--gpus" in r.stdout and "--shard" in r.stdout
    for bad in (["--shard", "2/2"], ["--gpus", "0"]):
        r = subprocess.run([sys.executable, tool, "--input", "x.bam"] + bad, capture_output=True, text=True)
        assert r.returncode == 2, (bad, r.stderr[-500:])


def test_both_tools_share_the_child_process_helpers():
    sys.path.insert(0, ROOT)
    import main as cli
    from dl4vc_amd import procs
    assert cli.child_devices is procs.child_devices and cli.wait_children is procs.wait_children
    assert procs.child_env("3", X="1")["HIP_VISIBLE_DEVICES"] == "3" and "CUDA_VISIBLE_DEVICES" not in procs.child_env("3")


# ---- merge of candidate parts ------------------------------------------------------------------------------------------------
def test_merge_parts_equals_sort_lines_of_the_whole(tmp_path):
    rng = np.random.default_rng(5)
    lines = []
    for _ in range(500):
        chrom = ["chr1", "chr10", "chr2", "chrX", "1"][rng.integers(5)]
        pos0 = int(rng.integers(0, 300))                     # (few positions: ties down to the whole line)
        ref, alt = "ACGT"[rng.integers(4)], ["A", "C", "GT", "TTA"][rng.integers(4)]
        lines.append(C.record_line(chrom, pos0, ref, alt, int(rng.integers(1, 90)), float(rng.random())))
    lines += lines[:20]                                      # (and whole lines twice, as on a subregion boundary)
    header = C.header_lines(["chr1", "chr2"], [1000, 2000])
    want = "\n".join(header + C.sort_lines(lines)) + "\n"
    for cuts in ([], [0], [len(lines)], [100], [7, 7, 300], sorted(rng.integers(0, len(lines), 7).tolist())):
        out = str(tmp_path / "candidates.vcf")
        edges = [0] + list(cuts) + [len(lines)]
        for g in range(len(edges) - 1):
            C.write_part(out, g, lines[edges[g]:edges[g + 1]], header,
                         {"reads": 10 * (g + 1), "total_ms": 1.5, "regions": 2, "groups": 3, "records": edges[g + 1] - edges[g]})
        count = len(edges) - 1
        stats = C.merge_parts(out, count)
        assert open(out).read() == want, cuts
        assert stats == {"reads": 10 * count * (count + 1) // 2, "total_ms": 1.5 * count, "regions": 2, "groups": 3 * count,
                         "records": len(lines)}
        assert os.listdir(str(tmp_path)) == ["candidates.vcf"]
    # no record at all: the header alone, as one process writes it
    C.write_part(out, 0, [], header, {})
    C.merge_parts(out, 1)
    assert open(out).read() == "\n".join(header) + "\n"


# ---- main.py's census, exchange and plan around stand-ins for the two GPU calls ------------------------------------------------
def test_shards_exchange_their_census_and_score_what_one_process_scores(tmp_path, monkeypatch):
    """``main.score_bam_census`` with ``census_bam`` and ``score_bam`` replaced (flag = POS not divisible by 3; a line = name,
    seed index): two sibling shards in two threads, a lone ``--shard``, holdout and limit against one process."""
    import argparse
    sys.path.insert(0, ROOT)
    import main as cli
    from dl4vc_amd import inference
    vcf = str(tmp_path / "c.vcf")
    with open(vcf, "w") as f:
        f.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\n")
        for c, n in (("chrA", 23), ("chrB", 18)):
            f.write("".join("%s\t%d\t.\tA\tC\n" % (c, 100 + 7 * i) for i in range(n)))
    censused = []

    def fake_census(bam, fasta, locations, inflate_device=None, stage=None, log=None):
        censused.append(len(locations))
        stage["census_ms"] = 1.0
        return np.array([l.pos % 3 != 0 for l in locations], np.uint8)

    def fake_score(net, bam, fasta, locations, write, first_record=0, census=None, **kw):
        assert len(census) == len(locations) and kw["reads_seed"] == 5
        k = 0
        for l, f in zip(locations, census):
            assert f == (l.pos % 3 != 0)
            if f:
                write("%s\t%d\n" % (l.name, first_record + k))
                k += 1
        kw["encoder_counts"]["locations"] = kw["encoder_counts"].get("locations", 0) + len(locations)
        return k

    monkeypatch.setattr(inference, "census_bam", fake_census)
    monkeypatch.setattr(inference, "score_bam", fake_score)
    out_final = str(tmp_path / "epoch1_model_test.vcf")

    def run(shard_i, shard_n, holdout=(), limit=0, shard=""):
        args = argparse.Namespace(sample_vcf=vcf, test_bam="x.bam", test_fasta="r.fa", inflate_device=None, census_timeout=20.0,
                                  sites_per_launch=16, reads_seed=5, use_var_type_threshold=False, shard=shard)
        target, st = str(tmp_path / ("t%d_%d" % (shard_i, shard_n))), {}
        n = cli.score_bam_census(args, None, target, out_final, shard_i, shard_n, holdout, limit, None, {}, st)
        lines = open(target).read().splitlines()
        assert n == len(lines) and st["census_records"] <= st["census_locations"] and st["census_ms"] == 1.0
        return lines, st

    whole, st = run(0, 1)
    on_a = sum((100 + 7 * i) % 3 != 0 for i in range(23))
    records = on_a + sum((100 + 7 * i) % 3 != 0 for i in range(18))
    assert len(whole) == records and [l.split("\t")[1] for l in whole] == [str(i) for i in range(records)]
    assert st["census_locations"] == 41 and st["census_records"] == records
    # a lone --shard censuses everything itself
    censused.clear()
    alone = [run(g, 3, shard="%d/3" % g)[0] for g in range(3)]
    assert sum(alone, []) == whole and censused == [41, 41, 41] and not [f for f in os.listdir(str(tmp_path)) if "census" in f]
    # siblings census a slice each and exchange side files
    monkeypatch.setenv(cli.CENSUS_SIBLINGS, "2")
    censused.clear()
    got = {}
    threads = [threading.Thread(target=lambda g=g: got.__setitem__(g, run(g, 2, shard="%d/2" % g))) for g in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(30.0)
    assert got[0][0] + got[1][0] == whole and sorted(censused) == [20, 21]
    assert [len(got[g][0]) for g in (0, 1)] == [int(np.diff(shard_range(records, g, 2))[0]) for g in (0, 1)]
    assert got[1][1]["census_wait_s"] >= 0
    assert sorted(f for f in os.listdir(str(tmp_path)) if "census" in f) == ["epoch1_model_test.vcf.part%d.census" % g for g in (0, 1)]
    remove_census(out_final, 2)
    with pytest.raises(SystemExit, match="DL4VC_CENSUS_SIBLINGS=2 but --shard 0/3"):
        run(0, 3, shard="0/3")
    monkeypatch.delenv(cli.CENSUS_SIBLINGS)
    # holdout keeps the index among all records; the limit cuts the selection before the split
    held = [l for l in whole if l.startswith("chrB:")]
    assert run(0, 1, holdout=("chrB",))[0] == held and held[0].split("\t")[1] == str(on_a)
    assert sum((run(g, 2, holdout=("chrB",), limit=7, shard="%d/2" % g)[0] for g in (0, 1)), []) == held[:7]
    assert sum((run(g, 3, limit=20, shard="%d/3" % g)[0] for g in range(3)), []) == whole[:20]

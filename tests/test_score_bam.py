"""Scoring straight from a BAM, the parts that need no GPU: the host definition of the site assembly
(``site_assembly.plan_sites`` + ``assemble_host``: what ``pg_assemble_device`` is held to in tests/test_score_bam_gpu.py) against
``dataset.assemble_batch`` over the records of the same locations, the ABI of the new entry, and what ``main.py --test_bam``
refuses."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from dl4vc_amd import loader, pileup_gpu
from dl4vc_amd import pileup_encoder as PE
from dl4vc_amd.dataset import assemble_batch
from dl4vc_amd.site_assembly import assemble_host, plan_sites, stored_vcfrec
from tests.test_pileup_native import _big_case

HEADER = os.path.join(ROOT, "include", "dl4vc_pileup_gpu.h")
needs_loader = pytest.mark.skipif(not loader.available(), reason="libdl4vc_loader.so not built")


def vcf_line(ref, p, kind=0, pad=0):
    """A candidate record at 1-based ``p``: SNP, 1-base deletion or 2-base insertion; ``pad`` lengthens INFO."""
    r = ref[p - 1]
    alt = "A" if r != "A" else "C"
    a, b = [(r, alt), (ref[p - 1:p + 1], r), (r, r + "TT")][kind]
    return "chr20\t%d\t.\t%s\t%s\t50\t.\tDP=40;AF=0.5%s\tGT\t0/1" % (p, a, b, ";X=" + "y" * pad if pad else "")


@needs_loader
@pytest.mark.parametrize("R,seed", [(115, 0), (120, 4000000000)])
def test_host_assembly_equals_assemble_batch_on_the_records(tmp_path, R, seed):
    """~46x reads over 6 kb (100 to 131 rows per location), S = 200 stored rows, R below the deepest pileup (seeded subsets), locations without a read at
    both ends and in the middle of the list (compaction), a record text longer than the stored 128 bytes."""
    bam, fa, ref = _big_case(tmp_path, n_reads=2400, length=6000, seed=3)
    pos = [5995] + list(range(300, 2900, 173)) + [5996] + list(range(2950, 5700, 211)) + [5997]
    locs = [PE.Location("chr20", p, "chr20:%d" % p, 2, vcf_line(ref, p, i % 3, 150 if i == 4 else 0)) for i, p in enumerate(pos)]
    locs.insert(7, PE.Location("chrX", 100, "chrX:100", 2, "chrX\t100\t.\tA\tC"))
    opt = PE.EncoderOptions(window_size=100, max_reads=200, max_insert_length=10, max_insert_length_variant=50)
    recs, errors = PE.encode_locations(bam, fa, locs, opt, native=True)
    with loader.NativePileupEncoder(bam, fa, 100, 200, 10, 50) as e:
        reads, qual, strand, rf, num, status = e.encode([l.contig for l in locs], [l.pos for l in locs], 2)
    assert not (status == 2).any(), "the fixture is meant to be pe_encode's own"
    assert errors == int((status == 0).sum()) >= 4 and status[0] == 0 and status[-1] == 0 and status[7] == 0
    assert num.max() > R and (num[status == 1] <= R).any()
    plan = plan_sites(status, num, rf, [l.vcf_string for l in locs], R, 200, seed)
    assert len(plan) == len(recs) and not plan.first_rows.all() and plan.first_rows.any()
    for use_q, use_strand in ((True, True), (False, True), (True, False)):
        want = assemble_batch(recs, R, seed=seed, use_q=use_q, use_strand=use_strand)
        got = assemble_host(reads, qual, strand, plan, use_q, use_strand)
        for g, w, name in zip(got, want.arrays(), ("reads", "qual", "strand", "ref", "ref_mask", "var_mask")):
            assert g.dtype == np.uint8 and g.shape == w.shape and np.array_equal(g, w), name
        assert plan.vcfrec == want.vcfrec and np.array_equal(plan.num_reads, want.num_reads)
    assert max(len(v.encode()) for v in plan.vcfrec) == 128 and stored_vcfrec("a\tb") == "a\tb"
    # the seed follows the ABSOLUTE record index: the second half planned on its own equals the second half of the whole
    k = len(plan) // 2
    cut = int(plan.slots[k])
    tail = plan_sites(status[cut:], num[cut:], rf[cut:], [l.vcf_string for l in locs[cut:]], R, 200, seed, first_record=k)
    assert np.array_equal(tail.rows, plan.rows[k:]) and np.array_equal(tail.slots + cut, plan.slots[k:])


@needs_loader
def test_plan_refuses_what_it_cannot_assemble():
    one = np.ones(1, np.int8)
    with pytest.raises(ValueError, match="stores only"):
        plan_sites(one, np.array([5]), np.zeros((1, 201), np.uint8), ["chr20\t5\t.\tA\tC"], 300, 200, 0)
    with pytest.raises(ValueError, match="201-column"):
        plan_sites(one, np.array([5]), np.zeros((1, 61), np.uint8), ["chr20\t5\t.\tA\tC"], 100, 200, 0)


def test_header_export_and_binding_agree_on_the_assembly_entry():
    if not pileup_gpu.available():
        import __graft_entry__ as g
        g.build()
    lib = pileup_gpu.load_library()
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decl = re.search(r"int pg_assemble_device\((.*?)\);", text, flags=re.S)
    assert decl and "pg_assemble_device" in pileup_gpu.SYMBOLS
    params = [p.strip() for p in decl.group(1).split(",")]
    assert len(params) == len(lib.pg_assemble_device.argtypes) == 24
    # pointers bind as void*, int64_t / int32_t as themselves, in the header's order
    import ctypes as C
    for p, t in zip(params, lib.pg_assemble_device.argtypes):
        want = C.c_void_p if "*" in p else C.c_int64 if p.startswith("int64_t") else C.c_int32
        assert t is want, p
    out = subprocess.run(["nm", "-D", "--defined-only", pileup_gpu.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "pg_assemble_device" in {l.split()[-1] for l in out.splitlines() if l.split()}


def test_main_refuses_two_sources_several_gpus_and_holdout():
    import sys
    sys.path.insert(0, ROOT)
    import main as cli
    base = ["--modelload", "c.pt", "--model_pool_combine_dimension", "0", "--sample_vcf", "c.vcf", "--test_fasta", "r.fa"]
    with pytest.raises(SystemExit, match="exactly one"):
        cli.main(base + ["--test_file", "x.hdf", "--test_bam", "x.bam"])
    with pytest.raises(SystemExit) as e:
        cli.main(base + ["--test_bam", "x.bam", "--gpus", "2"])
    assert str(e.value) == cli.GPUS_WITH_BAM and "--test_bam runs on one GPU" in cli.GPUS_WITH_BAM
    with pytest.raises(SystemExit, match="one GPU"):
        cli.main(base + ["--test_bam", "x.bam", "--shard", "0/2"])
    with pytest.raises(SystemExit, match="test_holdout_chromosomes is not supported"):
        cli.main(base + ["--test_bam", "x.bam", "--test_holdout_chromosomes", "chr20"])
    with pytest.raises(SystemExit, match="needs --test_fasta"):
        cli.main(["--modelload", "c.pt", "--test_bam", "x.bam", "--sample_vcf", "c.vcf"])
    with pytest.raises(SystemExit, match="inference input"):
        cli.main(base + ["--test_bam", "x.bam", "--train_file", "t.hdf"])
    # without --test_bam the reference's parser is unchanged: --test_file stays required
    with pytest.raises(SystemExit):
        cli.main(["--modelload", "c.pt"])


def test_converter_takes_the_pileup_device_flag(tmp_path):
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "convert_bam_single_reads.py"), "--input", "x.bam", "--pileup-device",
                        "tpu"], capture_output=True, text=True)
    assert r.returncode == 2 and "--pileup-device" in r.stderr and "gpu" in r.stderr

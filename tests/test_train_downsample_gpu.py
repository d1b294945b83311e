"""Dynamic read down-sampling on the MI355X: the three device gathers (``cl_assemble_device``, ``cl_store_assemble_device`` in both
record formats, ``pg_assemble_device``) and a store filled from the BAM follow plans whose entries carry the zero-reads bit
(csrc/plan_entry.h) and give the host path's planes and centre counts byte for byte; whole runs of ``main.py`` with
``--reads-dynamic-downsample-rate 0.3 --reads-dynamic-downsample-prob 0.5`` train the same through every loader."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from dl4vc_amd import hdf5io, pileup_gpu
from dl4vc_amd.chunk_loader import DeviceChunkLoader, ResidentRecords, center_counts_host
from dl4vc_amd.hdf5_schema import record_dtype
from dl4vc_amd.site_assembly import ZERO_READS, plan_records
from dl4vc_amd.train_data import assemble_training_batch, read_indices
from tests import train_bam_cases as TC
from tests.test_cli_gpu import MODEL_FLAGS, TRAIN_FLAGS
from tests.test_train_bam_gpu import assert_same_runs, with_files
from tests.test_train_loader_device_gpu import SMALL, loss_lines
from tests.train_loader_device_cases import PLANES

pytestmark = pytest.mark.gpu
N, STORED, W = 24, 200, 201
NUM_READS = (0, 3, 40, 100, 101, 199, 200, 260)
RATE, PROB = 0.3, 0.5
DOWN = ["--reads-dynamic-downsample-rate", str(RATE), "--reads-dynamic-downsample-prob", str(PROB)]


def _records():
    """24 records of 200 stored rows x 201 columns: every stored row of a site's reads non-zero in all three planes (tokens and
    strands below 16, so the compact format takes them), the rows behind them zero."""
    from dl4vc_amd.synth import make_labelled_records
    wide = make_labelled_records(N, 100, 901)
    recs = np.zeros(N, record_dtype(STORED, W))
    for name in recs.dtype.names:
        if name not in ("single_reads", "q-scores", "strand"):
            recs[name] = wide[name]
    rng = np.random.default_rng(4)
    for i in range(N):
        n = NUM_READS[i % len(NUM_READS)]
        k = min(n, STORED)
        recs[i]["num_reads"] = n
        recs[i]["single_reads"][:k] = rng.integers(1, 10, (k, W))
        recs[i]["q-scores"][:k] = rng.integers(1, 61, (k, W))
        recs[i]["strand"][:k] = rng.integers(1, 3, (k, W))
    return recs


@pytest.fixture(scope="module")
def train_file(tmp_path_factory):
    recs = _records()
    path = str(tmp_path_factory.mktemp("downsample_gpu") / "train.hdf")
    hdf5io.write_candidates(path, recs)
    return path, recs


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    return TC.labelled_fixture(tmp_path_factory.mktemp("downsample_bam"))


def _outs(torch, m, R):
    dev = torch.device("cuda", 0)
    return [torch.full((m, R, W), 0xAB, dtype=torch.uint8, device=dev) for _ in range(3)] + \
           [torch.full((m, W), 0xAB, dtype=torch.uint8, device=dev) for _ in range(3)]


def _same(torch, name, outs, counts, want_planes, want_counts, m):
    torch.cuda.synchronize()
    for plane, t, w in zip(PLANES, outs, want_planes):
        assert t[:m].cpu().numpy().tobytes() == np.ascontiguousarray(w).tobytes(), (name, plane)
    if counts is not None:
        assert np.array_equal(counts, want_counts), name


LISTS = [np.array([5, 13, 21, 3, 11, 19, 7, 15], np.int64),               # 199- and 100-deep and 260-deep sites
         np.random.RandomState(3).permutation(N).astype(np.int64)[:8],
         np.arange(N - 1, N - 9, -1, dtype=np.int64), np.array([8, 0, 16], np.int64)]     # ..., the sites without a read


@pytest.mark.parametrize("R", [100, 64])
def test_device_gathers_equal_the_host_path(train_file, fx, R):
    """The same (seed, epoch, indices) through ``assemble_training_batch`` and through the file's device loader, the resident
    store in both formats and ``pg_assemble_device`` over the records' planes; with prob 1 and with prob 0 (no entry flagged),
    and a plan that flags every row."""
    import torch
    path, recs = train_file
    planes = [np.ascontiguousarray(recs[f]) for f in ("single_reads", "q-scores", "strand")]
    stored = [torch.from_numpy(p).cuda() for p in planes]
    texts = [bytes(v).rstrip(b"\x00").decode() for v in recs["vcfrec"]]
    s = torch.cuda.Stream()
    with hdf5io.CandidateFile(path) as src, DeviceChunkLoader(path, R, 8, shuffled=1) as dl, \
            ResidentRecords(path, R, 8, capacity_bytes=1 << 30, slab_bytes=1 << 22) as store_rows, \
            ResidentRecords(path, R, 8, capacity_bytes=1 << 30, slab_bytes=1 << 22, record_format="compact") as store_compact, \
            pileup_gpu.GpuPileupEncoder(fx["bam"], fx["fasta"], 100, 200, 10, 50) as enc:
        assert store_compact.stage["store_compact_records"] > 0
        flagged = plain = 0
        for epoch, (rate, prob) in ((1, (RATE, 1.0)), (2, (RATE, PROB)), (3, (RATE, 0.0))):
            seed = 7 + epoch * N
            for idx in LISTS:
                m = len(idx)
                want = assemble_training_batch(read_indices(src, idx), idx, max_reads=R, seed=seed, downsample_rate=rate, downsample_prob=prob)
                want_counts = center_counts_host(want.sites.reads)
                for name, ld in (("cl_assemble_device", dl), ("store rows", store_rows), ("store compact", store_compact)):
                    outs = _outs(torch, 8, R)
                    ptrs = [t.data_ptr() for t in outs]
                    got = ld.load_indices(idx, seed, ptrs, s.cuda_stream, rate, prob) if ld is dl else \
                        ld.assemble_list(idx, seed, ptrs, s.cuda_stream, rate, prob)
                    s.synchronize()
                    _same(torch, name, outs, got.counts, want.planes(), want_counts, m)
                    assert np.array_equal(got.plan.sampled, want.sampled), name
                    assert all(t[m:].eq(0xAB).all() for t in outs), name          # nothing written behind the batch's sites
                plan = plan_records(idx.astype(np.int32), idx, recs["num_reads"].reshape(-1), recs["ref_bases"], texts, R, STORED, seed, rate, prob)
                flagged += int((plan.rows & ZERO_READS).any())
                plain += int(not (plan.rows & ZERO_READS).any())
                outs = _outs(torch, m, R)
                enc.assemble_device([t.data_ptr() for t in stored], N, plan, [t.data_ptr() for t in outs], stream=s.cuda_stream,
                                    stored_rows=STORED, window=W)
                s.synchronize()
                _same(torch, "pg_assemble_device", outs, None, want.planes(), None, m)
        assert flagged and plain
        # a plan that flags every row of every site: quality and strand of the named rows under an all-zero reads plane
        idx = LISTS[0]
        plan = plan_records(idx.astype(np.int32), idx, recs["num_reads"].reshape(-1), recs["ref_bases"], texts, R, STORED, 7)
        plan.rows[:] = np.arange(STORED - R, STORED, dtype=np.int16) | ZERO_READS
        plan.first_rows[:] = 0
        from dl4vc_amd.site_assembly import assemble_host
        want = assemble_host(*planes, plan)
        assert not want[0].any() and want[1].any()
        lines = (plan.ref, plan.ref_mask, plan.var_mask)
        for name, st in (("store rows", store_rows), ("store compact", store_compact)):
            outs = _outs(torch, len(idx), R)
            st.store.assemble_device(plan.slots, plan.rows, plan.first_rows, R, lines, True, True, [t.data_ptr() for t in outs], s.cuda_stream)
            s.synchronize()
            _same(torch, name + ", every row flagged", outs, None, want, None, len(idx))
        outs = _outs(torch, len(idx), R)
        enc.assemble_device([t.data_ptr() for t in stored], N, plan, [t.data_ptr() for t in outs], stream=s.cuda_stream, stored_rows=STORED,
                            window=W)
        s.synchronize()
        _same(torch, "pg_assemble_device, every row flagged", outs, None, want, None, len(idx))
        dl.inflate_lists([idx], s.cuda_stream)
        chunk = dl.file.chunk
        chunks = np.unique(idx // chunk)
        plan.slots = (np.searchsorted(chunks, idx // chunk) * chunk + idx % chunk).astype(np.int32)
        outs = _outs(torch, len(idx), R)
        dl.assemble(plan, [t.data_ptr() for t in outs], s.cuda_stream)
        s.synchronize()
        _same(torch, "cl_assemble_device, every row flagged", outs, None, want, None, len(idx))


def test_store_filled_from_the_bam_equals_its_host_twin(fx):
    """``ResidentRecords.from_bam`` on the device against the host filler and the CPU twin of the gather, flags on."""
    import torch
    locs, R = TC.locations(fx, "train"), 100
    n = TC.TRAIN_RECORDS
    perm = np.random.RandomState(5).permutation(n).astype(np.int64)
    s = torch.cuda.Stream()
    with ResidentRecords.from_bam(fx["bam"], fx["fasta"], locs, R, 8, device=-1, capacity_bytes=1 << 30, slab_bytes=1 << 20,
                                  round_locations=16) as host, \
            ResidentRecords.from_bam(fx["bam"], fx["fasta"], locs, R, 8, capacity_bytes=1 << 30, slab_bytes=1 << 20, round_locations=16) as dev:
        hit = 0
        for epoch in (1, 2):
            seed = 7 + epoch * n
            for k in range(0, n, 8):
                idx = perm[k:k + 8]
                w = [np.zeros((8, R, W), np.uint8) for _ in range(3)] + [np.zeros((8, W), np.uint8) for _ in range(3)]
                want = host.assemble_list(idx, seed, w, 0, RATE, PROB)
                outs = _outs(torch, 8, R)
                got = dev.assemble_list(idx, seed, [t.data_ptr() for t in outs], s.cuda_stream, RATE, PROB)
                s.synchronize()
                _same(torch, "from_bam", outs, got.counts, [a[:len(idx)] for a in w], want.counts, len(idx))
                assert np.array_equal(got.plan.rows, want.plan.rows)
                hit += int((got.plan.rows & ZERO_READS).any())
        assert hit


# ---- main.py ---------------------------------------------------------------------------------------------------------------
def run_main(fx, tag, source, extra):
    out = os.path.join(fx["dir"], tag)
    os.makedirs(out, exist_ok=True)
    cmd = [sys.executable, os.path.join(ROOT, "main.py")] + source + \
          ["--modelsave", os.path.join(out, "model.pth.tar"), "--sample_vcf", fx["sample"], "--save_vcf_records", "--save_vcf_records_file",
           os.path.join(out, "model_test.vcf"), "--gpus", "1", "--reads-seed", "7"] + MODEL_FLAGS + TRAIN_FLAGS + SMALL + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    return r, out


def test_main_py_trains_the_same_through_every_loader(fx):
    """Two epochs, 40 training records in batches of 8, both flags on: loader worker processes, the in-process host path,
    ``--train-loader-device gpu``, the resident store in both formats and ``--train_bam`` give the same loss lines, scored VCFs
    and checkpoints; the run without the flags does not; the evaluation is the flagless one."""
    with_files(fx)
    files = ["--train_file", fx["train_hdf"], "--test_file", fx["test_hdf"]]
    bam = ["--train_bam", fx["bam"], "--train_fasta", fx["fasta"], "--train_tp_vcf", fx["train_tp"], "--train_tp_full_vcf", fx["train_full"],
           "--train_fp_vcf", fx["train_fp"], "--test_bam", fx["bam"], "--test_fasta", fx["fasta"], "--test_tp_vcf", fx["test_tp"],
           "--test_tp_full_vcf", fx["test_full"], "--test_fp_vcf", fx["test_fp"]]
    device, cache = ["--train-loader-device", "gpu"], ["--train-loader-device", "gpu", "--train-cache-device", "gpu"]
    want = run_main(fx, "workers", files, DOWN + ["--num-data-workers", "2"])
    arms = [("inprocess", files, ["--num-data-workers", "0"]), ("device", files, device), ("resident", files, cache),
            ("compact", files, cache + ["--train-cache-format", "compact"]), ("bam", bam, cache)]
    for tag, source, extra in arms:
        assert_same_runs(run_main(fx, tag, source, DOWN + extra), want, TC.TEST_RECORDS, 5)
    line = [l for l in want[0].stdout.replace("\r", "\n").splitlines() if l.startswith("dynamic read down-sampling")]
    assert len(line) == 2 and "rate 0.3, prob 0.5" in line[0] and " of 40 sites down-sampled, mean kept fraction 0." in line[0]
    assert int(line[0].split(": ")[1].split(" of ")[0]) > 0
    off = run_main(fx, "off", files, cache)
    assert "dynamic read down-sampling" not in off[0].stdout
    assert loss_lines(off[0].stdout) != loss_lines(want[0].stdout)              # the flags reach the step
    # evaluation is untouched: the epoch's checkpoint scores the test file the same in a run that has no flags at all
    again = os.path.join(fx["dir"], "again")
    os.makedirs(again, exist_ok=True)
    cmd = [sys.executable, os.path.join(ROOT, "main.py"), "--test_file", fx["test_hdf"], "--modelload", os.path.join(want[1], "model.pth_epoch2.tar"),
           "--sample_vcf", fx["sample"], "--save_vcf_records", "--save_vcf_records_file", os.path.join(again, "model_test.vcf"),
           "--compute-empty-rows", "--reads-seed", "7"] + MODEL_FLAGS + SMALL[2:]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(os.path.join(again, "epoch1_model_test.vcf")).read() == open(os.path.join(want[1], "epoch2_model_test.vcf")).read()

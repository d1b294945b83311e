"""Training straight from the BAM on the MI355X (``main.py --train_bam``): ``cl_store_append_planes_device`` against its CPU
definition with the source planes at three alignments, the device filler (``ResidentRecords.from_bam``) against the host filler on a
labelled BAM, batches from a BAM-filled prefetcher with the BAM gone, and whole runs of ``main.py --train_bam --test_bam`` against
converter + ``--train_file --test_file --train-loader-device gpu --train-cache-device gpu``, bit for bit."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from dl4vc_amd.chunk_loader import BamSource, RecordStore, ResidentRecords, StoreFull
from tests import train_bam_cases as TC
from tests.test_cli_gpu import MODEL_FLAGS, TRAIN_FLAGS
from tests.test_train_loader_device_gpu import SMALL, loss_lines
from tests.train_loader_device_cases import PLANES

pytestmark = pytest.mark.gpu
READS = 100
SHIFTS = (0, 1, 9)                               # bytes into their allocations at which the reads, qual and strand arrays start
CACHE = ["--train-loader-device", "gpu", "--train-cache-device", "gpu"]


# ---- the kernels with the planar source ------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,W", TC.SHAPES)
def test_append_planes_device_equals_the_cpu_definition(S, W):
    """The shapes and records of the CPU test (35-byte slots: every source alignment; 48-byte; 40 200-byte: two alignments), the
    three arrays 0, 1 and 9 bytes into their allocations, slots out of order with gaps in two appends, slabs of two of the largest
    records (a second and a third slab), the budget exactly enough.  Every record's table entry and bytes equal the CPU
    definition's, every other byte of the slabs' allocations keeps its 0xAB, and the source planes are unchanged."""
    import torch
    planes, want = TC.planes_and_kept(S, W)
    n = TC.N_SLOTS * S * W
    bufs = [torch.full((sh + n + 64,), 0xCD, dtype=torch.uint8, device="cuda") for sh in SHIFTS]
    views = [b[sh:sh + n] for b, sh in zip(bufs, SHIFTS)]
    for v, p in zip(views, planes):
        v.copy_(torch.from_numpy(p.reshape(-1)))
    before = [b.cpu().numpy().copy() for b in bufs]
    need = int(TC.span(want[TC.TAKEN], W).sum())
    slab = 2 * int(TC.span(S, W))
    records = np.arange(len(TC.TAKEN), dtype=np.int32)
    ptrs = [v.data_ptr() for v in views]
    assert [p % 16 for p in ptrs] == list(SHIFTS)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with RecordStore(W, S, len(TC.TAKEN), need, slab, device=-1) as twin, RecordStore(W, S, len(TC.TAKEN), need, slab, device=0) as st, \
            RecordStore(W, S, len(TC.TAKEN), need - 1, slab, device=0) as tight:
        twin.pack_planes_host(*planes, TC.TAKEN, records)
        # refusals first: nothing is enqueued, nothing allocated
        with pytest.raises(StoreFull, match="capacity of %d bytes would be exceeded" % (need - 1)):
            tight.append_planes_device(ptrs, TC.N_SLOTS, TC.TAKEN, records, side.cuda_stream)
        assert (tight.stats().records, tight.stats().slabs) == (0, 0)
        bad = TC.TAKEN.copy()
        bad[5] = TC.N_SLOTS
        with pytest.raises(ValueError, match="entry 5 names slot %d of %d" % (TC.N_SLOTS, TC.N_SLOTS)):
            st.append_planes_device(ptrs, TC.N_SLOTS, bad, records, side.cuda_stream)
        with pytest.raises(ValueError, match="null argument"):
            st.append_planes_device([ptrs[0], 0, ptrs[2]], TC.N_SLOTS, TC.TAKEN, records)
        assert (st.stats().records, st.stats().slabs) == (0, 0)
        st.debug_fill(0xAB)
        kept = np.concatenate([st.append_planes_device(ptrs, TC.N_SLOTS, TC.TAKEN[:4], records[:4], side.cuda_stream),
                               st.append_planes_device(ptrs, TC.N_SLOTS, TC.TAKEN[4:], records[4:])])
        assert (kept == want[TC.TAKEN]).all()
        s, t = st.stats(), twin.stats()
        assert s.slabs == t.slabs >= 3 and s.stored_bytes == t.stored_bytes == need and s.records == len(TC.TAKEN)
        assert s.inflated_bytes == t.inflated_bytes and s.extent_ms > 0 and s.pack_ms > 0
        for i in records:
            assert st.record(i) == twin.record(i), i           # (slab, offset, kept) from the device's table
        for k in range(s.slabs):
            buf, off, used, cap = st.slab(k)
            w, _o, w_used, w_cap = twin.slab(k)
            assert (off, used, cap) == (256, w_used, w_cap)
            assert buf[off:off + used].tobytes() == w[:used].tobytes(), k
            assert (buf[:off] == 0xAB).all() and (buf[off + used:] == 0xAB).all(), k
    torch.cuda.synchronize()
    for b, was in zip(bufs, before):
        assert b.cpu().numpy().tobytes() == was.tobytes()      # the three source arrays are read only


# ---- the filler ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    return TC.labelled_fixture(tmp_path_factory.mktemp("train_bam_gpu"))


@pytest.fixture(scope="module")
def host_records(fx):
    """The CPU definition: the host filler over the training locations (rounds of 16, slabs of 1 MiB)."""
    rr = ResidentRecords.from_bam(fx["bam"], fx["fasta"], TC.locations(fx, "train"), READS, 8, device=-1, capacity_bytes=1 << 30,
                                  slab_bytes=1 << 20, round_locations=16)
    assert len(rr) == TC.TRAIN_RECORDS
    yield rr
    rr.close()


@pytest.mark.parametrize("inflate_device", [None, "gpu"])
def test_the_device_filler_equals_the_host_filler(fx, host_records, inflate_device):
    want = host_records
    with ResidentRecords.from_bam(fx["bam"], fx["fasta"], TC.locations(fx, "train"), READS, 8, capacity_bytes=1 << 30, slab_bytes=1 << 20,
                                  round_locations=16, debug_fill=0xAB, inflate_device=inflate_device) as rr:
        assert len(rr) == len(want) == TC.TRAIN_RECORDS and rr.blob.tobytes() == want.blob.tobytes()
        for i in range(len(want)):
            assert rr.store.record(i) == want.store.record(i), i
        s, t = rr.store.stats(), want.store.stats()
        assert s.slabs == t.slabs >= 3 and s.stored_bytes == t.stored_bytes and s.inflated_bytes == t.inflated_bytes
        for k in range(s.slabs):
            buf, off, used, _cap = rr.store.slab(k)
            w, _o, w_used, _c = want.store.slab(k)
            assert used == w_used and buf[off:off + used].tobytes() == w[:used].tobytes(), k
            assert (buf[:off] == 0xAB).all() and (buf[off + used:] == 0xAB).all(), k
        c = rr.stage
        print("encoders: %s" % {k: c[k] for k in ("locations", "gpu", "native", "python", "no_record")})
        assert (c["locations"], c["no_record"]) == (43, 3) and c["gpu"] + c["native"] + c["python"] == TC.TRAIN_RECORDS
        assert c["native"] >= 1 and c["python"] >= 1 and c["gpu"] >= 30           # (the 1 100-track site; the twin pair)
        assert c["store_records"] == TC.TRAIN_RECORDS and c["store_bytes"] == want.stage["store_bytes"]
        assert c["fill_ms"] > 0 and c["encode_ms"] > 0 and c["extent_ms"] > 0 and c["pack_ms"] > 0


def test_the_device_filler_refuses_a_budget_too_small(fx):
    with pytest.raises(StoreFull, match=r"do not fit the record store: \d+ records \(of the first 16 of its 43 locations\) fit, in \d+ bytes "
                                        r"of the budget of 300000 bytes"):
        ResidentRecords.from_bam(fx["bam"], fx["fasta"], TC.locations(fx, "train"), READS, 8, capacity_bytes=300000, round_locations=16)


def test_bam_filled_prefetcher_batches_equal_the_host_definition_with_the_bam_gone(fx, host_records):
    """Two shuffled epochs with different seeds and a sequential pass from a prefetcher whose BAM, index and FASTA are REMOVED
    once it is filled.  The budget is asked for as a function, after the staging planes are allocated."""
    import torch
    from dl4vc_amd.train_data import DeviceBatchPrefetcher, targets_from_counts
    gone = os.path.join(fx["dir"], "gone")
    os.makedirs(gone)
    for path in (fx["bam"], fx["bam"] + ".bai", fx["fasta"]):
        shutil.copy(path, gone)
    bam, fasta = os.path.join(gone, os.path.basename(fx["bam"])), os.path.join(gone, os.path.basename(fx["fasta"]))
    asked = []

    def budget():
        asked.append(torch.cuda.memory_allocated())
        return 1 << 30

    n = TC.TRAIN_RECORDS
    perm = np.random.RandomState(5).permutation(n).astype(np.int64)
    shuffled = [perm[k:k + 8] for k in range(0, n, 8)]
    sequential = [np.arange(k, min(n, k + 8), dtype=np.int64) for k in range(0, n, 8)]
    with pytest.raises(ValueError, match="there is no non-resident form"):
        DeviceBatchPrefetcher(BamSource(bam, fasta, TC.locations(fx, "train")), READS, 8)
    with DeviceBatchPrefetcher(BamSource(bam, fasta, TC.locations(fx, "train")), READS, 8, wait_s=60.0, resident=True, cache_bytes=budget,
                               slab_bytes=1 << 20) as pf:
        shutil.rmtree(gone)
        assert len(asked) == 1 and asked[0] >= 3 * 43 * 200 * 201 and len(pf) == n          # (the staging planes were allocated first)
        stage = dict(pf.stage)
        assert stage["store_records"] == n and stage["locations"] == 43
        for lists, seed in ((shuffled, 7 + n), (shuffled[::-1], 7 + 2 * n), (sequential, 7)):
            seen = 0
            for k, batch in enumerate(pf.batches(iter(lists), max_reads=READS, seed=seed, non_snp_train_weight=2.0, keep_candidate_af=True)):
                idx = lists[k]
                outs = [np.zeros((8, READS, 201), np.uint8) for _ in range(3)] + [np.zeros((8, 201), np.uint8) for _ in range(3)]
                want = host_records.assemble_list(idx, seed, outs)
                targets = targets_from_counts(want.plan, want.label, want.counts, 2.0, True, None)
                batch.event.synchronize()
                for name, t, w in zip(PLANES, batch.planes(), outs):
                    assert t.is_cuda and t.cpu().numpy().tobytes() == w[:len(idx)].tobytes(), (name, k)
                assert sorted(batch.targets) == sorted(targets)
                for key, v in targets.items():
                    assert batch.targets[key].dtype == v.dtype and batch.targets[key].tobytes() == v.tobytes(), (key, k)
                assert batch.vcfrec == list(want.plan.vcfrec) and (batch.index == idx).all()
                assert (batch.blacklist == np.array(want.plan.blacklist, bool)).all()
                batch.release()
                seen += 1
            assert seen == len(lists)
        for k in ("store_bytes", "fill_ms", "encode_ms", "locations", "gpu"):
            assert pf.stage[k] == stage[k], k                  # after the fill nothing is encoded


# ---- main.py ---------------------------------------------------------------------------------------------------------------
def run_main(fx, tag, route, gpus=1, extra=(), ok=True):
    out = os.path.join(fx["dir"], tag)
    os.makedirs(out, exist_ok=True)
    env = dict(os.environ)
    if gpus == 2:
        env.update(DL4VC_FORCE_DEVICE0="1", DL4VC_DIST_BACKEND="gloo")
    if route == "file":
        source = ["--train_file", fx["train_hdf"], "--test_file", fx["test_hdf"]]
    else:
        source = ["--train_bam", fx["bam"], "--train_fasta", fx["fasta"], "--train_tp_vcf", fx["train_tp"], "--train_tp_full_vcf",
                  fx["train_full"], "--train_fp_vcf", fx["train_fp"], "--test_bam", fx["bam"], "--test_fasta", fx["fasta"], "--test_tp_vcf",
                  fx["test_tp"], "--test_tp_full_vcf", fx["test_full"], "--test_fp_vcf", fx["test_fp"]]
    cmd = [sys.executable, os.path.join(ROOT, "main.py")] + source + CACHE + \
          ["--modelsave", os.path.join(out, "model.pth.tar"), "--sample_vcf", fx["sample"], "--save_vcf_records", "--save_vcf_records_file",
           os.path.join(out, "model_test.vcf"), "--gpus", str(gpus), "--reads-seed", "7"] + MODEL_FLAGS + TRAIN_FLAGS + SMALL + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert (r.returncode == 0) == ok, (r.stdout[-1500:], r.stderr[-3000:])
    return r, out


def with_files(fx):
    """The file route's inputs: what the converter writes from the same BAM and VCFs."""
    if "train_hdf" not in fx:
        fx["train_hdf"] = TC.convert(fx, "train", os.path.join(fx["dir"], "train.hdf"))
        fx["test_hdf"] = TC.convert(fx, "test", os.path.join(fx["dir"], "test.hdf"))
    return fx


def assert_same_runs(a, b, n_eval, steps):
    """``assert_same_training`` of tests/test_train_loader_device_gpu.py for this fixture's counts: the loss lines, both epochs'
    scored VCFs, every tensor of both checkpoints and of Adam's moments."""
    import torch
    (ra, da), (rb, db) = a, b
    la, lb = loss_lines(ra.stdout), loss_lines(rb.stdout)
    assert len(la) >= steps + 2 + 2 and la == lb             # (the second epoch may keep fewer: the sampler drops easy examples)
    for epoch in (1, 2):
        va, vb = (open(os.path.join(d, "epoch%d_model_test.vcf" % epoch)).read() for d in (da, db))
        assert va == vb and len([l for l in va.splitlines() if not l.startswith("#")]) == n_eval
        sa, sb = (torch.load(os.path.join(d, "model.pth_epoch%d.tar" % epoch), map_location="cpu", weights_only=False) for d in (da, db))
        assert sorted(sa["state_dict"]) == sorted(sb["state_dict"]) and len(sa["state_dict"]) > 20
        for k, v in sa["state_dict"].items():
            assert torch.equal(v, sb["state_dict"][k]), (epoch, k)
        oa, ob = sa["optimizer"]["state"], sb["optimizer"]["state"]
        assert sorted(oa) == sorted(ob) and len(oa) > 10
        for i in oa:
            assert oa[i]["step"] == ob[i]["step"] and steps * (epoch - 1) < oa[i]["step"] <= steps * epoch
            assert torch.equal(oa[i]["exp_avg"], ob[i]["exp_avg"]) and torch.equal(oa[i]["exp_avg_sq"], ob[i]["exp_avg_sq"]), (epoch, i)


FILL = r"--train-cache-device gpu: \S*reads\.bam: (\d+) records resident in \d+ bytes .* filled in [\d.]+ s; (\d+) locations: (\d+) on the " \
       r"GPU, (\d+) by pe_encode, (\d+) by the Python builder, (\d+) without a record"


def test_main_py_trains_the_same_from_the_bam_as_from_the_converters_files(fx):
    """Two epochs, 40 training records in batches of 8 (five steps an epoch) and 23 evaluation records in batches of 6, on one GPU:
    ``--train_bam --test_bam`` against converter + ``--train_file --test_file``, both resident."""
    with_files(fx)
    want = run_main(fx, "file1", "file")
    got = run_main(fx, "bam1", "bam", extra=["--inflate-device", "gpu"])
    assert_same_runs(got, want, TC.TEST_RECORDS, 5)
    fills = [tuple(map(int, m)) for m in re.findall(FILL, got[0].stdout)]
    assert fills[0][:2] == (TC.TRAIN_RECORDS, 43) and fills[1][:2] == (TC.TEST_RECORDS, 26), got[0].stdout[-3000:]
    for records, locs, gpu, native, py, none in fills:
        assert gpu + native + py == records and records + none == locs and native >= 1 and py >= 1
    assert not [f for f in os.listdir(got[1]) if f.endswith(".hdf")]
    assert len(re.findall(FILL, want[0].stdout)) == 0 and "records resident" in want[0].stdout


def test_main_py_trains_the_same_on_two_ranks_with_chromosomes_held_out(tmp_path_factory):
    """Two ranks on device 0 over gloo, a store each, on the two-contig fixture (86 training and 52 evaluation locations) with
    chr21 held out of training and evaluation restricted to it: the easy-example sampler and the evaluation take their indices
    from the resident records' text by ``select_sites``' rule, so the order -- and with it every loss line, scored VCF and
    checkpoint tensor -- is the file route's."""
    fx2 = with_files(TC.labelled_fixture(tmp_path_factory.mktemp("train_bam_two"), contigs=2))
    held = ["--train_holdout_chromosomes", "chr21", "--test_holdout_chromosomes", "chr21"]
    want = run_main(fx2, "file2", "file", gpus=2, extra=held)
    got = run_main(fx2, "bam2", "bam", gpus=2, extra=held)
    assert_same_runs(got, want, TC.TEST_RECORDS, 5)
    fills = [tuple(map(int, m)) for m in re.findall(FILL, got[0].stdout)]
    assert sorted(f[:2] for f in fills) == sorted([(2 * TC.TRAIN_RECORDS, 86), (2 * TC.TEST_RECORDS, 52)] * 2)      # every rank fills its own copy
    assert not [f for f in os.listdir(got[1]) if f.endswith(".hdf")]


def test_main_py_ends_with_the_refusal_when_the_budget_is_too_small(fx):
    r, _ = run_main(fx, "bam_small", "bam", extra=["--train-cache-bytes", "100000"], ok=False)
    assert "--train-cache-device gpu: the records of " in r.stderr and "do not fit the record store: " in r.stderr
    assert re.search(r"\d+ records \(of the first 43 of its 43 locations\) fit, in \d+ bytes of the budget of 100000 bytes; raise "
                     r"--train-cache-bytes", r.stderr) and "Traceback" not in r.stderr

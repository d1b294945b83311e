"""Training batches assembled on the MI355X (``main.py --train_file T --test_file V --train-loader-device gpu``):
``DeviceChunkLoader.load_indices`` against its host definition (tests/train_loader_device_cases.py), the centre-token counts kernel
against ``cl_center_counts_host``, ``dan_train_backward_begin_device`` against the host entry bit for bit, and whole runs of
``main.py`` with the flag against runs with ``--num-data-workers 0``."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from dl4vc_amd import hdf5io
from tests.loader_device_cases import chunk_written, write_chunks
from tests.test_cli_gpu import MODEL_FLAGS, TRAIN_FLAGS
from tests.train_loader_device_cases import (N, PLANES, READS, STORED, draw_seed, host_definition, index_lists, labelled_records)

pytestmark = pytest.mark.gpu

B = 8                                            # sites per batch: the longest index list


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("train_loader_device")
    recs = labelled_records()
    hdf5io.write_candidates(str(d / "gzip4.hdf"), recs)
    chunk_written(str(d / "fixed.hdf"), recs, "fixed")
    w = write_chunks(str(d / "raw.hdf"), recs, raw=(2,))
    assert w.stored_chunks == 1
    write_chunks(str(d / "damaged.hdf"), recs, damage=(2,))
    return {"libhdf5 gzip 4": str(d / "gzip4.hdf"), "ChunkWriter fixed": str(d / "fixed.hdf"), "a raw chunk": str(d / "raw.hdf"),
            "damaged": str(d / "damaged.hdf"), "dir": str(d)}


def fresh_planes(torch, n=B, reads=READS):
    dev = torch.device("cuda", 0)
    return [torch.full((n, reads, 201), 0xAB, dtype=torch.uint8, device=dev) for _ in range(3)] + \
           [torch.full((n, 201), 0xAB, dtype=torch.uint8, device=dev) for _ in range(3)]


@pytest.mark.parametrize("kind", ["libhdf5 gzip 4", "ChunkWriter fixed", "a raw chunk"])
def test_load_indices_equals_the_host_definition(files, kind):
    """Every index list, at the seeds of evaluation and of the first epoch, into 0xAB-filled device tensors: the six planes, the
    targets bitwise, blacklist and record text; the sites behind the last one are not written."""
    import torch
    from dl4vc_amd.chunk_loader import DeviceChunkLoader
    from dl4vc_amd.train_data import targets_from_counts
    side = torch.cuda.Stream()
    with DeviceChunkLoader(files[kind], READS, batch_sites=B, shuffled=True) as dl:
        assert len(dl) == N and dl.stored_rows == STORED
        for epoch in (0, 1):
            seed = draw_seed(epoch)
            for idx in index_lists():
                outs = fresh_planes(torch)
                torch.cuda.synchronize()
                got = dl.load_indices(idx, seed, [t.data_ptr() for t in outs], side.cuda_stream)
                planes, targets, blacklist, vcfrec = host_definition(files[kind], idx, seed)
                m = len(idx)
                for name, t, want in zip(PLANES, outs, planes):
                    h = t.cpu().numpy()
                    assert h[:m].tobytes() == want.tobytes(), (name, idx)
                    assert (h[m:] == 0xAB).all(), (name, idx)
                mine = targets_from_counts(got.plan, got.label, got.counts, 2.0, True)
                assert sorted(mine) == sorted(targets)
                for k, v in targets.items():
                    assert mine[k].dtype == v.dtype and mine[k].tobytes() == v.tobytes(), (k, idx)
                assert (np.array(got.plan.blacklist, bool) == blacklist).all() and list(got.plan.vcfrec) == vcfrec
        # chunk 2 (records 16..23) is read for the lists that name one of its records, once per list
        assert dl.stage["raw_chunks"] == (2 * sum(1 for idx in index_lists() if ((idx // 8) == 2).any()) if kind == "a raw chunk" else 0)
        assert dl.stage["records"] == 2 * sum(len(i) for i in index_lists()) and dl.stage["inflate_ms"] > 0
        with pytest.raises(ValueError, match="at most %d per call" % B):
            dl.load_indices(np.arange(B + 1), 0, [t.data_ptr() for t in outs])
        with pytest.raises(ValueError, match="outside the file's %d records" % N):
            dl.load_indices(np.array([0, N]), 0, [t.data_ptr() for t in outs])


def test_a_handle_not_opened_for_shuffled_records_refuses_too_many_chunks(files):
    import torch
    from dl4vc_amd.chunk_loader import DeviceChunkLoader
    outs = fresh_planes(torch)
    with DeviceChunkLoader(files["ChunkWriter fixed"], READS, batch_sites=B) as dl:
        with pytest.raises(ValueError, match=r"opened for 0 at a time \(shuffled=\)"):
            dl.load_indices(np.array([0, 8, 16, 24, 32, 40]), 0, [t.data_ptr() for t in outs])


def test_a_damaged_chunk_is_named_only_when_an_index_falls_in_it(files):
    import torch
    from dl4vc_amd.chunk_loader import DamagedChunk, DeviceChunkLoader
    outs = fresh_planes(torch)
    ptrs = [t.data_ptr() for t in outs]
    with DeviceChunkLoader(files["damaged"], READS, batch_sites=B, shuffled=True) as dl:
        idx = np.array([44, 3, 15, 24, 9], np.int64)                       # chunks 5, 0, 1, 3, 1: not the damaged one
        dl.load_indices(idx, draw_seed(1), ptrs)
        want = host_definition(files["ChunkWriter fixed"], idx, draw_seed(1))[0]
        assert outs[0].cpu().numpy()[:len(idx)].tobytes() == want[0].tobytes()
        with pytest.raises(DamagedChunk, match="chunk at record 16: "):
            dl.load_indices(np.array([3, 23, 40], np.int64), draw_seed(1), ptrs)
        dl.load_indices(np.array([40], np.int64), draw_seed(1), ptrs)         # the handle goes on


@pytest.mark.parametrize("m", [1, 37])
def test_counts_kernel_equals_its_host_definition(files, m):
    """R = 1, 12, 64, 65, 100 and 128 rows (below, at and past the 64 lanes of the wave); the output lies inside a 0xAB-filled
    array of which no byte outside [m][2][16] changes."""
    import torch
    from dl4vc_amd.chunk_loader import DeviceChunkLoader, center_counts_host
    rng = np.random.default_rng(41 + m)
    pool = np.array(list(range(10)) + [10, 15, 16, 17, 128, 255], np.uint8)
    guard = 64                                                               # int32 words in front of and behind the output
    with DeviceChunkLoader(files["ChunkWriter fixed"], READS, batch_sites=B, shuffled=True) as dl:
        for R in (1, 12, 64, 65, 100, 128):
            reads = rng.integers(0, 10, (m, R, 201)).astype(np.uint8)
            reads[:, :, 100:102] = pool[rng.integers(0, len(pool), (m, R, 2))]
            reads[0, 0, 100] = 255                                            # (a byte above 15 is there to be ignored)
            d_reads = torch.from_numpy(reads).cuda()
            out = torch.full(((guard + m * 32 + guard) * 4,), 0xAB, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            rc = dl.lib.cl_center_counts_device(dl._h, C.c_void_p(d_reads.data_ptr()), m, R, 201, C.c_void_p(out.data_ptr() + guard * 4), None)
            assert rc == 0, dl.lib.cl_last_error(dl._h)
            torch.cuda.synchronize()
            h = out.cpu().numpy()
            assert (h[:guard * 4] == 0xAB).all() and (h[(guard + m * 32) * 4:] == 0xAB).all(), R
            got = h[guard * 4:(guard + m * 32) * 4].view(np.int32).reshape(m, 2, 16)
            want = center_counts_host(reads)
            assert (got == want).all(), R
            assert want.sum() < 2 * m * R
        assert dl.lib.cl_center_counts_device(dl._h, None, 1, 4, 201, C.c_void_p(out.data_ptr()), None) == -1
        assert b"null argument" in dl.lib.cl_last_error(dl._h)
        assert dl.lib.cl_center_counts_device(dl._h, C.c_void_p(d_reads.data_ptr()), 1, 0, 201, C.c_void_p(out.data_ptr()), None) == -1


# ---- the prefetcher: plane sets recycled, record buffer overwritten by the next launch -----------------------------------------
def many_lists():
    """16 index lists: the ten of ``index_lists`` and a second permutation in batches of 8 -- more than ``2 * ahead`` for every
    ``ahead`` below, so plane sets come back and later launches overwrite the record buffer while batches are held."""
    perm = np.random.RandomState(18).permutation(N).astype(np.int64)
    return index_lists() + [perm[k:k + 8] for k in range(0, N, 8)]


@pytest.mark.parametrize("ahead,release", [(1, True), (2, True), (4, True), (1, False), (2, False)])
def test_prefetcher_batches_equal_the_host_definition_while_held(files, ahead, release):
    """``DeviceBatchPrefetcher.batches`` over 16 lists with 2, 4 and 8 plane sets.  The consumer holds every batch until it has
    taken the next one and only then compares its planes (byte for byte) and targets (bitwise) with the host definition, so a
    plane set handed back too early, a launch that overwrote records still to be assembled, or a plan still pointing into the
    overwritten pinned copy would show.  ``release=False``: the consumer never releases; the generator's own rule does."""
    import torch
    from dl4vc_amd.train_data import DeviceBatchPrefetcher
    path, seed, lists = files["libhdf5 gzip 4"], draw_seed(1), many_lists()
    assert len(lists) > 2 * ahead + 2

    def check(batch, idx):
        planes, targets, blacklist, vcfrec = host_definition(path, idx, seed)
        batch.event.synchronize()
        for name, t, want in zip(PLANES, batch.planes(), planes):
            assert t.is_cuda and t.cpu().numpy().tobytes() == want.tobytes(), (name, idx)
        assert sorted(batch.targets) == sorted(targets)
        for k, v in targets.items():
            assert batch.targets[k].dtype == v.dtype and batch.targets[k].tobytes() == v.tobytes(), (k, idx)
        assert (batch.blacklist == blacklist).all() and batch.vcfrec == vcfrec and (batch.index == idx).all()

    with DeviceBatchPrefetcher(path, READS, B, ahead=ahead, wait_s=60.0) as pf:
        assert len(pf.sets) == 2 * ahead
        for _epoch in range(2):                                           # (a second call: the handle and the sets are reused)
            held, seen = None, 0
            for k, batch in enumerate(pf.batches(iter(lists), max_reads=READS, seed=seed, non_snp_train_weight=2.0,
                                                 keep_candidate_af=True)):
                torch.cuda.synchronize()
                if held is not None:
                    check(held, lists[k - 1])
                    if release:
                        held.release()
                held, seen = batch, seen + 1
            check(held, lists[-1])
            held.release()
            assert seen == len(lists)
        assert pf.stage["records"] == 2 * sum(len(i) for i in lists)
        # sized by what the lists touch: never more chunks than the file has
        assert pf.loader.max_chunks <= 6


def test_prefetcher_hands_a_damaged_chunk_to_the_consumer(files):
    from dl4vc_amd.train_data import BatchError, DeviceBatchPrefetcher
    with DeviceBatchPrefetcher(files["damaged"], READS, B, ahead=2, wait_s=60.0) as pf:
        got = []
        with pytest.raises(BatchError, match="chunk at record 16: "):
            for batch in pf.batches([np.array([0, 40]), np.array([9]), np.array([41, 17]), np.array([3])], max_reads=READS, seed=5):
                got.append(batch.index.tolist())
                batch.release()
        assert got == [[0, 40], [9]]                                      # (the launch of lists 0 and 1 held no index of chunk 2)
        with pytest.raises(ValueError, match="needs the seed"):
            next(pf.batches([np.array([0])], max_reads=READS))


# ---- the training ABI ------------------------------------------------------------------------------------------------------
def small_trainers():
    from dl4vc_amd.config import DanConfig
    from dl4vc_amd.train import DanTrainer, TrainHyper
    from oracle.dan_oracle import random_state_dict
    cfg = DanConfig(reads=READS, c_init=16, c_final=16, bottleneck=4, fc_sizes=(8, 8))
    sd = random_state_dict(cfg, seed=5)
    for k in ("fcHidden2BinTarget", "fcHidden2VT", "fcHidden2AF", "fcHidden2Coverage", "fcHidden2VB", "fcHidden2VR"):
        sd[k + ".weight"] = (sd[k + ".weight"] * np.float32(0.15)).astype(np.float32)
    return cfg, [DanTrainer(cfg, TrainHyper(), max_batch=B).load_state_dict(sd) for _ in range(2)]


def test_begin_device_equals_begin_on_the_same_bytes(files):
    """Two consecutive steps: one trainer takes the planes the loader left in device memory (behind the loader's event), a second
    one the same bytes from host arrays; losses, close flags and the flat gradient buffer after each backward, bit for bit."""
    import torch
    from dl4vc_amd.chunk_loader import DeviceChunkLoader
    from dl4vc_amd.train_data import targets_from_counts
    _cfg, (dev_tr, host_tr) = small_trainers()
    side = torch.cuda.Stream()
    lists = index_lists()
    with DeviceChunkLoader(files["libhdf5 gzip 4"], READS, batch_sites=B, shuffled=True) as dl:
        for step, idx in enumerate((lists[0], lists[5])):                    # 8 sites, then the 5 of the last batch
            outs = fresh_planes(torch)
            torch.cuda.synchronize()
            got = dl.load_indices(idx, draw_seed(1), [t.data_ptr() for t in outs], side.cuda_stream)
            targets = targets_from_counts(got.plan, got.label, got.counts, 2.0, True)
            event = torch.cuda.Event()
            event.record(side)
            planes = [t[:len(idx)] for t in outs]
            dev_tr.backward_begin(planes, targets, seed=77, event=event)
            a = dev_tr.backward_end()
            host_tr.backward_begin([t.cpu().numpy() for t in planes], targets, seed=77)
            b = host_tr.backward_end()
            for k in ("loss", "bin", "vt", "af", "cov", "vb", "vr"):
                assert np.float32(a[k]).tobytes() == np.float32(b[k]).tobytes(), (step, k, a[k], b[k])
            assert np.isfinite(a["loss"]) and a["loss"] != 0
            assert (a["vt_close"] == b["vt_close"]).all() and (a["bin_close"] == b["bin_close"]).all()
            ga, gb = dev_tr.grad_tensor(), host_tr.grad_tensor()
            assert torch.equal(ga, gb) and bool(ga.abs().sum() > 0), step
            assert dev_tr.apply() == host_tr.apply()
    dev_tr.close()
    host_tr.close()


def test_begin_device_has_the_entry_checks_of_begin(files):
    import torch
    from dl4vc_amd.train import _CTargets
    _cfg, (tr, other) = small_trainers()
    other.close()
    outs = fresh_planes(torch, n=B + 1)
    tg = {"label": np.zeros(B + 1, np.uint8), "var_type": np.zeros(B + 1, np.uint8), "allele_freq": np.zeros(B + 1, np.float32),
          "coverage": np.ones(B + 1, np.float32), "var_base_enum": np.ones(B + 1, np.uint8), "var_ref_enum": np.ones(B + 1, np.uint8),
          "weight": np.ones(B + 1, np.float32)}
    with pytest.raises(RuntimeError, match=r"a training batch holds 1\.\.%d sites, got %d" % (B, B + 1)):
        tr.backward_begin(outs, tg)
    with pytest.raises(RuntimeError, match=r"a training batch holds 1\.\.%d sites, got 0" % B):
        tr.backward_begin([t[:0] for t in outs], {k: v[:0] for k, v in tg.items()})
    ct = _CTargets(**{k: v.ctypes.data for k, v in tg.items()})
    ptrs = [C.c_void_p(t.data_ptr()) for t in outs]
    for null in (0, 3, 5):
        args = list(ptrs)
        args[null] = None
        assert tr.lib.dan_train_backward_begin_device(tr._h, *args, 4, C.byref(ct), None, 0, None) < 0
        assert b"null input plane" in tr.lib.dan_train_last_error(tr._h)
    assert tr.lib.dan_train_backward_begin_device(tr._h, *ptrs, 4, None, None, 0, None) < 0
    assert b"null target array" in tr.lib.dan_train_last_error(tr._h)
    with pytest.raises(ValueError, match="contiguous uint8 tensor in device memory"):
        tr.backward_begin([t.cpu() for t in outs], tg)
    tr.close()


# ---- main.py ---------------------------------------------------------------------------------------------------------------
SMALL = ["--epochs", "2", "--model-init-conv-channels", "16", "--model-final-conv-channels", "16", "--model-bottleneck-size", "4"]


@pytest.fixture(scope="module")
def train_files(files):
    """17 training records in batches of 8 (the last batch holds ONE site), 16 test records in batches of 6; two sites deeper
    than the model's 100 rows, so each epoch's draw seed matters."""
    from dl4vc_amd.synth import make_labelled_records
    recs = make_labelled_records(17, 100, 900)
    rng = np.random.default_rng(2)
    for i in (3, 12):
        recs[i]["num_reads"] = 150
        for f in ("single_reads", "q-scores", "strand"):
            recs[i][f][100:150] = recs[i][f][rng.integers(0, 100, 50)]
    d = files["dir"]
    hdf5io.write_candidates(os.path.join(d, "train.hdf"), recs)
    hdf5io.write_candidates(os.path.join(d, "test.hdf"), recs[:16])
    write_chunks(os.path.join(d, "train_damaged.hdf"), recs, damage=(1,))
    sample = os.path.join(d, "candidates.vcf")
    open(sample, "w").write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tCALLED\n")
    return d, sample


def run_training(train_files, tag, extra, gpus=1, train="train.hdf", ok=True):
    d, sample = train_files
    out = os.path.join(d, tag)
    os.makedirs(out, exist_ok=True)
    env = dict(os.environ)
    if gpus == 2:
        env.update(DL4VC_FORCE_DEVICE0="1", DL4VC_DIST_BACKEND="gloo")
    cmd = [sys.executable, os.path.join(ROOT, "main.py"), "--train_file", os.path.join(d, train), "--test_file", os.path.join(d, "test.hdf"),
           "--modelsave", os.path.join(out, "model.pth.tar"), "--sample_vcf", sample, "--save_vcf_records", "--save_vcf_records_file",
           os.path.join(out, "model_test.vcf"), "--gpus", str(gpus), "--reads-seed", "7"] + MODEL_FLAGS + TRAIN_FLAGS + SMALL + extra
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert (r.returncode == 0) == ok, (r.stdout[-1500:], r.stderr[-3000:])
    return r, out


def loss_lines(stdout):
    """The progress and evaluation lines, without the wall-clock field."""
    lines = [l.strip() for l in re.split(r"[\r\n]+", stdout) if "Loss:" in l or "Average loss" in l or "close matches" in l]
    return [re.sub(r"Elapsed \([^)]*\)", "", l) for l in lines]


def assert_same_training(a, b):
    import torch
    (ra, da), (rb, db) = a, b
    la, lb = loss_lines(ra.stdout), loss_lines(rb.stdout)
    assert len(la) >= 2 * 3 + 2 + 2 and la == lb
    for epoch in (1, 2):
        va, vb = (open(os.path.join(d, "epoch%d_model_test.vcf" % epoch)).read() for d in (da, db))
        assert va == vb and len([l for l in va.splitlines() if not l.startswith("#")]) == 16
        sa, sb = (torch.load(os.path.join(d, "model.pth_epoch%d.tar" % epoch), map_location="cpu", weights_only=False) for d in (da, db))
        assert sorted(sa["state_dict"]) == sorted(sb["state_dict"]) and len(sa["state_dict"]) > 20
        for k, v in sa["state_dict"].items():
            assert torch.equal(v, sb["state_dict"][k]), (epoch, k)
        oa, ob = sa["optimizer"]["state"], sb["optimizer"]["state"]
        assert sorted(oa) == sorted(ob) and len(oa) > 10
        for i in oa:
            assert oa[i]["step"] == ob[i]["step"] == 3 * epoch
            assert torch.equal(oa[i]["exp_avg"], ob[i]["exp_avg"]) and torch.equal(oa[i]["exp_avg_sq"], ob[i]["exp_avg_sq"]), (epoch, i)


@pytest.mark.parametrize("gpus", [1, 2])
def test_main_py_trains_the_same_with_the_flag(train_files, gpus):
    """Two epochs (the easy-example sampler and the second epoch's draw seed act), the flag against ``--num-data-workers 0``: the
    loss lines, both epochs' scored evaluation VCFs, and every tensor of ``state_dict`` and of Adam's moments in both epochs'
    checkpoints.  gpus = 2: two ranks on device 0 over gloo; rank 1 sits out the one-site last batch."""
    host = run_training(train_files, "host%d" % gpus, ["--num-data-workers", "0"], gpus)
    dev = run_training(train_files, "device%d" % gpus, ["--train-loader-device", "gpu", "--num-data-workers", "5"], gpus)
    assert "--num-data-workers 5 starts no worker process" in dev[0].stdout and "starts no worker process" not in host[0].stdout
    assert_same_training(dev, host)


def test_main_py_names_the_damaged_chunk(train_files):
    r, _ = run_training(train_files, "damaged", ["--train-loader-device", "gpu"], train="train_damaged.hdf", ok=False)
    assert "chunk at record 8: " in r.stderr and "Traceback" not in r.stderr

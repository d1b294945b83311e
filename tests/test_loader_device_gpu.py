"""The candidate file loaded on the MI355X (``chunk_loader.DeviceChunkLoader``, ``main.py --test_file F --loader-device gpu``): the
file's chunks are inflated on the device (``zi_inflate_kernel``) and its sites assembled there (``cl_assemble_device``).  The
reference is the host path: ``loader.NativeLoader``'s planes byte for byte, and the scored VCF of the run without the flag."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from dl4vc_amd import hdf5io
from tests.loader_device_cases import N, RAW_CHUNK, SEED, chunk_written, create_dataset, make_records, write_chunks
from tests.test_cli_gpu import MODEL_FLAGS

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """name -> (path, stored rows, reads of the model)"""
    d = tmp_path_factory.mktemp("loader_device")
    small, prod = make_records(20, 10), make_records(200, 100)
    out = {}
    hdf5io.write_candidates(str(d / "gzip4.hdf"), small)
    out["libhdf5 gzip 4"] = (str(d / "gzip4.hdf"), 20, 10)
    chunk_written(str(d / "fixed.hdf"), small, "fixed")
    out["ChunkWriter fixed"] = (str(d / "fixed.hdf"), 20, 10)
    chunk_written(str(d / "dynamic.hdf"), small, "dynamic")
    out["ChunkWriter dynamic"] = (str(d / "dynamic.hdf"), 20, 10)
    w = write_chunks(str(d / "raw.hdf"), small, raw=(RAW_CHUNK,))
    assert w.stored_chunks == 1
    out["a raw chunk"] = (str(d / "raw.hdf"), 20, 10)
    hdf5io.write_candidates(str(d / "prod.hdf"), prod)
    out["production layout"] = (str(d / "prod.hdf"), 200, 100)
    out["dir"] = str(d)
    out["prod records"] = prod
    return out


FILES = ["libhdf5 gzip 4", "ChunkWriter fixed", "ChunkWriter dynamic", "a raw chunk", "production layout"]


@pytest.mark.parametrize("name", FILES)
def test_planes_equal_the_native_loaders(files, name):
    """The six planes, vcfrec, num_reads and blacklist of [0, n) and of [3, n - 2) in batches of 16, written into 0xAB-filled
    outputs; the raw-chunk file really holds a chunk the filter mask skips."""
    from dl4vc_amd.chunk_loader import DeviceChunkLoader
    from dl4vc_amd.loader import NativeLoader
    path, stored, reads = files[name]
    with DeviceChunkLoader(path, reads, batch_sites=16, seed=SEED) as dl:
        assert len(dl) == N and dl.stored_rows == stored
        for lo, hi in ((0, N), (3, N - 2)):
            with NativeLoader(path, reads, batch_sites=16, lo=lo, hi=hi, seed=SEED, threads=2) as nl:
                want = list(nl)
            got = list(dl.batches(lo, hi))
            assert [len(p) for p, _ in got] == [len(b) for b in want] and sum(len(b) for b in want) == hi - lo
            for (plan, outs), b in zip(got, want):
                for t, ref in zip(outs, (b.reads, b.qual, b.strand, b.ref, b.ref_mask, b.var_mask)):
                    assert (t.cpu().numpy() == ref).all()
                assert plan.vcfrec == list(b.vcfrec)
                assert (plan.num_reads == b.num_reads).all() and (plan.blacklist == b.blacklist).all()
        # (records 16..23 lie in one batch of [0, 45) -- [16, 32) -- and in two of [3, 43): [3, 19) and [19, 35))
        assert dl.stage["raw_chunks"] == (3 if name == "a raw chunk" else 0)
        assert dl.stage["chunks"] > 0 and dl.stage["inflate_ms"] > 0 and dl.stage["records"] == N + N - 5
    if name == "production layout":
        assert dl.stage["inflated_bytes"] % (8 * 123965) == 0


def test_blacklist_and_deep_sites_are_in_the_fixture(files):
    from dl4vc_amd.loader import NativeLoader
    path, _stored, reads = files["libhdf5 gzip 4"]
    with NativeLoader(path, reads, batch_sites=64, seed=SEED, threads=1) as nl:
        b = next(iter(nl))
    assert b.blacklist[7] and b.blacklist.sum() < 10
    assert (b.num_reads > reads).sum() == 5 and (b.num_reads == reads).sum() >= 2 and (b.num_reads == 0).sum() == 1


def test_slots_and_rows_out_of_range_are_refused_before_a_launch(files):
    import torch
    from dl4vc_amd.chunk_loader import DeviceChunkLoader
    path, stored, reads = files["ChunkWriter fixed"]
    with DeviceChunkLoader(path, reads, batch_sites=16, seed=SEED) as dl:
        plan, outs = next(dl.batches(0, 16))
        for t in outs:
            t.fill_(0xAB)
        ptrs = [t.data_ptr() for t in outs]
        bad = plan.slice(0, 4)
        bad.slots = bad.slots.copy()
        bad.slots[2] = 16                                         # the two chunks of the last load hold slots 0..15
        with pytest.raises(RuntimeError, match="names slot 16 of 16"):
            dl.assemble(bad, ptrs)
        bad = plan.slice(0, 4)
        bad.rows, bad.first_rows = bad.rows.copy(), np.zeros(4, np.uint8)
        bad.rows[1, 3] = stored
        with pytest.raises(RuntimeError, match="names stored row %d of %d" % (stored, stored)):
            dl.assemble(bad, ptrs)
        bad.rows[1, 3] = -1
        with pytest.raises(RuntimeError, match="names stored row -1"):
            dl.assemble(bad, ptrs)
        torch.cuda.synchronize()
        assert all(bool((t == 0xAB).all()) for t in outs)
        with pytest.raises(ValueError, match="at most 16"):
            dl.load(0, 17, ptrs)
    with pytest.raises(ValueError, match="stores only 20"):
        DeviceChunkLoader(path, 21)


def test_contiguous_and_shuffled_datasets_are_refused_with_the_reason(files):
    from dl4vc_amd.chunk_loader import DeviceChunkLoader
    recs = make_records(20, 10)[:16]
    flat, shuf, plain = (os.path.join(files["dir"], n) for n in ("contiguous.hdf", "shuffle.hdf", "chunked_plain.hdf"))
    create_dataset(flat, recs, chunked=False, shuffle=False)
    with pytest.raises(ValueError, match="is not chunked"):
        DeviceChunkLoader(flat, 10)
    create_dataset(shuf, recs, chunked=True, shuffle=True)
    with pytest.raises(ValueError, match=r"filters \[2, 1\], not deflate alone"):
        DeviceChunkLoader(shuf, 10)
    create_dataset(plain, recs, chunked=True, shuffle=False)
    with pytest.raises(ValueError, match=r"filters \[\], not deflate alone"):
        DeviceChunkLoader(plain, 10)


# ---- main.py and call_variants.sh -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(files):
    import torch
    from dl4vc_amd.config import DanConfig
    from oracle.dan_oracle import random_state_dict
    sd = random_state_dict(DanConfig(), seed=12)
    ck = os.path.join(files["dir"], "ckpt.pth.tar")
    torch.save({"epoch": 3, "best_loss": 0.0, "optimizer": {}, "state_dict": {"module." + k: torch.from_numpy(v) for k, v in sd.items()}}, ck)
    sample = os.path.join(files["dir"], "candidates.vcf")
    open(sample, "w").write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tCALLED\n")
    return ck, sample


def run_main(files, model, hdf, tag, extra, ok=True):
    ck, sample = model
    d = os.path.join(files["dir"], tag)
    os.makedirs(d, exist_ok=True)
    out = os.path.join(d, "model_test.vcf")
    cmd = [sys.executable, os.path.join(ROOT, "main.py"), "--test_file", hdf, "--modelload", ck, "--sample_vcf", sample, "--save_vcf_records",
           "--save_vcf_records_file", out, "--reads-seed", str(SEED), "--sites-per-launch", "16"] + MODEL_FLAGS + extra
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert (r.returncode == 0) == ok, (r.stdout[-1500:], r.stderr[-2500:])
    return r, os.path.join(d, "epoch1_model_test.vcf")


@pytest.fixture(scope="module")
def host_vcf(files, model):
    """The scored VCF of the run without the flag (fp32, production layout)."""
    _r, path = run_main(files, model, files["production layout"][0], "host", [])
    text = open(path).read()
    assert len([l for l in text.splitlines() if not l.startswith("#")]) == N
    return text


def test_main_py_writes_the_same_scored_vcf(files, model, host_vcf):
    r, path = run_main(files, model, files["production layout"][0], "device", ["--loader-device", "gpu"])
    assert open(path).read() == host_vcf
    assert "device loader:" in r.stdout and "inflate_ms" in r.stdout and "HDF5 raw chunks + device inflate" in r.stdout


def test_two_shards_concatenate_to_the_same_scored_vcf(files, model, host_vcf):
    parts = []
    for i in range(2):
        _r, path = run_main(files, model, files["production layout"][0], "shards", ["--loader-device", "gpu", "--shard", "%d/2" % i])
        parts.append(open(path + ".part%d" % i).read())
    assert [len(p.splitlines()) for p in parts] == [22, 23]                  # (a shard boundary inside a chunk)
    body = "".join(l + "\n" for l in host_vcf.splitlines() if not l.startswith("#"))
    assert "".join(parts) == body


def test_holdout_chromosomes_select_the_same_sites(files, model):
    flags = ["--test_holdout_chromosomes", "chr21"]
    _r, host = run_main(files, model, files["production layout"][0], "holdout_host", flags)
    _r, dev = run_main(files, model, files["production layout"][0], "holdout_device", flags + ["--loader-device", "gpu"])
    text = open(dev).read()
    assert text == open(host).read()
    body = [l for l in text.splitlines() if not l.startswith("#")]
    assert len(body) == N - 30 and all(l.startswith("chr21\t") for l in body)


def test_a_damaged_chunk_ends_the_run_with_its_record_and_status(files, model):
    """Chunk 2's stream with one byte flipped in its middle, written past the filter: the run ends with ``chunk at record 16``."""
    path = os.path.join(files["dir"], "damaged.hdf")
    write_chunks(path, files["prod records"], damage=(2,))
    r, _ = run_main(files, model, path, "damaged", ["--loader-device", "gpu"], ok=False)
    from dl4vc_amd import zinflate
    assert "chunk at record 16: " in r.stderr
    text = r.stderr.split("chunk at record 16: ", 1)[1].splitlines()[0].strip()
    assert text in {zinflate.status_text(c) for c in zinflate.STATUS.values() if c} and "Traceback" not in r.stderr


def test_call_variants_sh_with_l_equals_the_script_without_it(files, model):
    """From an OUTDIR that already holds candidates.hdf and candidates.vcf: -l changes no byte of the scored and called files."""
    import shutil
    ck, sample = model
    outs = []
    for tag, flags in (("cv_host", []), ("cv_device", ["-l"])):
        d = os.path.join(files["dir"], tag)
        os.makedirs(d, exist_ok=True)
        shutil.copy(files["production layout"][0], os.path.join(d, "candidates.hdf"))
        shutil.copy(sample, os.path.join(d, "candidates.vcf"))
        r = subprocess.run(["bash", os.path.join(ROOT, "call_variants.sh"), "-m", ck, "-o", d] + flags, capture_output=True, text=True)
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:], open(os.path.join(d, "training.log")).read()[-2000:])
        log = open(os.path.join(d, "training.log")).read()
        assert ("device loader:" in log) == bool(flags)
        outs.append([open(os.path.join(d, n)).read() for n in ("epoch1_model_test.vcf", "model_test_sorted_thres-join.vcf")])
    assert outs[0] == outs[1] and len(outs[0][0].splitlines()) == N + 2

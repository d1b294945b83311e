"""Dynamic Huffman codes on the GPU: ``zd_deflate_dyn_kernel`` against its CPU twin byte for byte (one definition, deterministic,
independent of the launch order, nothing written outside the streams), its streams through the device inflate,
``compress_records(compress_codes="dynamic")`` against the packed image the host builds and against fixed mode's sizes, and the
converter with ``--compress-codes dynamic`` against the converter without the device compressor, down to the scored VCF."""
import json
import os
import re
import sys
import zlib

import numpy as np
import pytest

from conftest import ROOT
from dl4vc_amd import candgen, hdf5io, pileup_gpu
from dl4vc_amd import pileup_encoder as PE
from dl4vc_amd.hdf5_schema import blob_dtype, record_dtype
from tests import zdeflate_cases as ZC
from tests import zdeflate_dynamic_cases as DC
from tests.test_cli_gpu import MODEL_FLAGS
from tests.test_compress_gpu import OPT, _device_streams, _images, _locations, inputs        # noqa: F401  (inputs: a fixture)
from tests.test_score_bam_gpu import FIXTURE_EMPTY, FIXTURE_LOCATIONS, _run

pytestmark = pytest.mark.gpu
DYN = pileup_gpu.ZD_DYNAMIC


def twin(data, seg):
    return pileup_gpu.zd_deflate_host(data, seg, codes="dynamic")


def check(name, datas, seg, flags=DYN):
    """One launch over equal-length chunks: every stream is the CPU twin's, with its flag and Adler-32, and inflates."""
    got, store, adlers = _device_streams(datas, seg, flags)
    for k, data in enumerate(datas):
        want, adler, st = twin(data, seg)
        assert got[k] == want, (name, k)
        assert bool(store[k]) == st and int(adlers[k]) == adler == zlib.adler32(data), (name, k)
        assert zlib.decompress(got[k]) == data, (name, k)
    return got


def sixty_six_segments():
    """65 * 1024 + 1 bytes at segment 1 024: a full workgroup and one of two lanes, the last segment a single byte; pileup-like
    rows, a stretch no code shortens, zeros and text, so that the lanes of one wave take all three kinds of segment."""
    rng = np.random.default_rng(66)
    data = ZC.pileup_like(40 * 1024) + rng.integers(0, 256, 9 * 1024, dtype=np.uint8).tobytes() + bytes(6 * 1024) + \
        (b"the quick brown fox jumps over the lazy dog, " * 240)[:10 * 1024] + b"\x07"
    assert len(data) == 65 * 1024 + 1
    return data


def test_kernel_streams_equal_the_cpu_twin():
    smaller = 0
    for name, seg, data in [c for c in ZC.grid() if c[1] == ZC.SEGMENT] + DC.special_cases():
        got = check(name, [data], seg)
        smaller += len(got[0]) < len(pileup_gpu.zd_deflate_host(data, seg)[0])
    assert smaller > 10
    check("66 segments", [sixty_six_segments()], 1024)
    p = ZC.pileup_like(49153)
    check("three chunks", [p, p[::-1], p[20000:] + p[:20000]], 16384)


def test_same_bytes_twice_reversed_and_raw_on_store():
    seg = ZC.SEGMENT
    n = 3 * seg + 1
    datas = [d for _name, d in ZC.contents(n, seg)] * 23          # 138 chunks x 4 segments: 9 workgroups, the last one partly filled
    want = [twin(d, seg)[0] for _name, d in ZC.contents(n, seg)] * 23
    first, st1, _ = _device_streams(datas, seg, DYN)
    again, st2, _ = _device_streams(datas, seg, DYN)
    rev, st3, _ = _device_streams(datas, seg, DYN | pileup_gpu.ZD_REVERSED)
    assert first == want and again == want and rev == want
    assert st1.tolist() == st2.tolist() == st3.tolist() and 0 < st1.sum() < len(st1)
    raw, st4, _ = _device_streams(datas, seg, DYN | pileup_gpu.ZD_RAW_ON_STORE)
    assert st4.tolist() == st1.tolist()
    assert all(r == (d if s else w) for r, d, s, w in zip(raw, datas, st4, want))
    random = dict(ZC.contents(n, seg))["random"]
    out, st, _ = _device_streams([random], seg, DYN | pileup_gpu.ZD_RAW_ON_STORE)
    assert st[0] and out[0] == random
    # the 66 segments, whose lanes diverge, in both launch orders
    data = sixty_six_segments()
    assert _device_streams([data], 1024, DYN)[0] == _device_streams([data], 1024, DYN | pileup_gpu.ZD_REVERSED)[0]


def test_device_stream_through_the_device_inflate():
    data = ZC.pileup_like(49153)
    stream = check("pileup-like", [data], 16384)[0]
    assert stream[2] & 6 == 4                                     # the first block is a dynamic one
    block = DC.bgzf_block(data, stream)
    out = np.zeros(len(data) + 8, np.uint8)
    assert candgen.inflate_blocks(block, [0], out, [0], device=0) == [0]          # (0: CRC-32 and ISIZE agree)
    assert out[:len(data)].tobytes() == data and not out[len(data):].any()
    assert zlib.crc32(out[:len(data)].tobytes()) == int.from_bytes(block[-8:-4], "little")


def test_compress_records_in_dynamic_codes(inputs):          # noqa: F811
    """The 42 fixture locations of tests/test_compress_gpu.py::test_packed_image_equals_the_host_records, built the same way: 37
    records, 5 chunks, the last one padded."""
    import torch
    d, bam, fa, vcf, pos, ck = inputs
    keep = set(pos[:35]) | {2000, 2990, 3800, 5520, 6215, 8000, 8500}
    locs = _locations(vcf, pos, keep)
    assert len(locs) == 42
    recs, errors = PE.encode_locations(bam, fa, locs, OPT, device="gpu", threads=2)
    m = len(recs)
    assert errors == 5 and m == 37
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(3)
    n_slots = m + 9
    slots = rng.permutation(n_slots)[:m].astype(np.int32)
    planes = []
    for name in ("single_reads", "q-scores", "strand"):
        host = rng.integers(0, 256, (n_slots, 200, 201), dtype=np.uint8)
        host[slots] = recs[name]
        planes.append(torch.from_numpy(host).to(dev))
    bdt = blob_dtype(201)
    blob = np.zeros(m, bdt)
    for name in bdt.names:
        blob[name] = recs[name]
    out = {}
    for codes in ("fixed", "dynamic"):
        with pileup_gpu.GpuPileupEncoder(bam, fa, 100, 200, 10, 50, compress_codes=codes) as enc:
            out[codes] = (enc.compress_records(planes, slots, blob, 8), enc.stats())
    with pytest.raises(ValueError, match="codes"):
        pileup_gpu.GpuPileupEncoder(bam, fa, 100, 200, 10, 50, compress_codes="best")
    item = record_dtype(200, 201).itemsize
    host_image = np.ascontiguousarray(recs).tobytes() + bytes(3 * item)
    chunks, st = out["dynamic"]
    assert len(chunks) == 5 and not chunks.store.any()
    assert _images(chunks, 8 * item) == host_image
    for c in range(5):
        assert chunks.chunk(c) == pileup_gpu.zd_deflate_host(host_image[c * 8 * item:(c + 1) * 8 * item], codes="dynamic")[0]
    n_segs = 5 * -(-8 * item // pileup_gpu.ZD_DEFAULT_SEGMENT)
    assert st["fixed_segments"] + st["dynamic_segments"] + st["stored_segments"] == n_segs and st["dynamic_segments"] > 0
    assert st["chunks"] == 5 and st["chunk_bytes_out"] == len(chunks.data) and st["deflate_ms"] > 0
    fixed, fst = out["fixed"]
    assert _images(fixed, 8 * item) == host_image
    assert fst["fixed_segments"] == fst["dynamic_segments"] == fst["stored_segments"] == 0        # counted in dynamic mode only
    print("5 chunks of %d bytes: fixed %d, dynamic %d (%s)" % (8 * item, len(fixed.data), len(chunks.data),
                                                              {k: st[k] for k in ("fixed_segments", "dynamic_segments", "stored_segments")}))
    assert len(chunks.data) < len(fixed.data)
    assert all(int(a) <= int(b) for a, b in zip(chunks.sizes, fixed.sizes))


def test_converter_with_dynamic_codes_writes_the_same_records_and_scores(inputs):          # noqa: F811
    d, bam, fa, vcf, pos, ck = inputs
    out = d / "conv_dynamic"
    out.mkdir()
    conv = [sys.executable, os.path.join(ROOT, "tools", "convert_bam_single_reads.py"), "--input", bam, "--fp_vcf", vcf, "--fasta-input", fa,
            "--max-reads", "200", "--num-processes", "2", "--max-insert-length", "10", "--max-insert-length-variant", "50", "--save-q-scores",
            "--save-strand", "--locations-process-step", "33"]            # two steps: 33 + 32 locations
    _run(conv + ["--output", str(out / "plain.hdf")])
    r = _run(conv + ["--output", str(out / "dynamic.hdf"), "--pileup-device", "gpu", "--compress-device", "gpu", "--compress-codes", "dynamic"])
    st = json.loads(re.search(r"compress-device gpu stages: (\{.*\})", r.stdout).group(1))
    assert st["dynamic_segments"] > 0
    assert st["fixed_segments"] + st["dynamic_segments"] + st["stored_segments"] == 61 * st["chunks_from_device"] > 0
    files = []
    for name in ("plain.hdf", "dynamic.hdf"):
        with hdf5io.CandidateFile(str(out / name)) as f:
            files.append(f.read(0, len(f)))
    assert len(files[0]) == FIXTURE_LOCATIONS - FIXTURE_EMPTY and files[0].tobytes() == files[1].tobytes()
    assert hdf5io.dataset_layout(str(out / "plain.hdf")) == hdf5io.dataset_layout(str(out / "dynamic.hdf"))
    print("file sizes: gzip-4 %d, dynamic codes on the device %d" % tuple(os.path.getsize(str(out / n)) for n in ("plain.hdf", "dynamic.hdf")))
    common = ["--modelload", ck, "--sample_vcf", vcf, "--save_vcf_records", "--reads-seed", "5", "--sites-per-launch", "16"] + MODEL_FLAGS
    for name in ("plain", "dynamic"):
        _run([sys.executable, os.path.join(ROOT, "main.py"), "--test_file", str(out / (name + ".hdf")), "--save_vcf_records_file",
              str(out / (name + ".vcf"))] + common)
    a, b = (open(str(out / ("epoch1_%s.vcf" % n)), "rb").read() for n in ("plain", "dynamic"))
    assert a == b and len([l for l in a.decode().splitlines() if not l.startswith("#")]) == FIXTURE_LOCATIONS - FIXTURE_EMPTY

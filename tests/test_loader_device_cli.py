"""``--loader-device gpu`` where no device is needed: what the command line refuses, the ``cl_*`` header against the exports and the
ctypes binding, and the host half of the device loader -- the raw chunks of a file (``hdf5io.RawChunkFile``) through the CPU twin
of the inflate kernel give the file's records, and ``site_assembly.plan_sites`` on them gives ``NativeLoader``'s planes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from dl4vc_amd import chunk_loader, hdf5io, pileup_gpu, zinflate
from dl4vc_amd.site_assembly import assemble_host, plan_sites
from tests.loader_device_cases import N, RAW_CHUNK, SEED, chunk_written, create_dataset, make_records, write_chunks

HEADER = os.path.join(ROOT, "include", "dl4vc_chunks.h")


@pytest.fixture(scope="module", autouse=True)
def lib():
    if not pileup_gpu.available():
        import __graft_entry__ as g
        g.build()
    return chunk_loader.load_library()


def _main(argv):
    import sys
    sys.path.insert(0, ROOT)
    import main as cli
    with pytest.raises(SystemExit) as e:
        cli.main(argv)
    return str(e.value)


def test_loader_device_refusals_name_their_reason():
    base = ["--modelload", "c.pt", "--model_pool_combine_dimension", "0", "--sample_vcf", "c.vcf"]
    assert "--loader-device must be gpu" in _main(base + ["--test_file", "x.hdf", "--loader-device", "cpu"])
    assert "--loader-device must be gpu" in _main(base + ["--test_file", "x.hdf", "--loader-device", ""])
    why = _main(base + ["--test_bam", "x.bam", "--test_fasta", "r.fa", "--loader-device", "gpu"])
    assert "option of --test_file" in why and "--inflate-device gpu" in why
    why = _main(base + ["--test_file", "x.hdf", "--train_file", "t.hdf", "--loader-device", "gpu"])
    assert "training and its evaluation keep the host loaders" in why
    # the BAM option stays what it was
    assert "--inflate-device gpu is an option of --test_bam" in _main(base + ["--test_file", "x.hdf", "--inflate-device", "gpu"])


def test_call_variants_l_is_refused_with_d(tmp_path):
    r = subprocess.run(["bash", os.path.join(ROOT, "call_variants.sh"), "-m", "model", "-o", str(tmp_path / "none"), "-l", "-d"],
                       capture_output=True, text=True)
    assert r.returncode == 1 and "-l loads candidates.hdf on the GPU and -d reads no candidates.hdf" in r.stdout
    text = open(os.path.join(ROOT, "call_variants.sh")).read()
    assert '${LOADER:+--loader-device "$LOADER"}' in text and "[-l]" in text


def test_run_shard_refuses_another_loader_device(tmp_path):
    from dl4vc_amd.inference import run_shard
    with pytest.raises(ValueError, match="loader_device"):
        run_shard(None, "x.hdf", str(tmp_path / "out"), loader_device="cpu")


def test_header_exports_and_binding_agree_on_the_loader(lib):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(cl_[a-z_]+)\s*\(", text))
    assert declared == set(chunk_loader.CL_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", pileup_gpu.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.split() and l.split()[-1].startswith("cl_")}
    assert exported == declared
    body = re.search(r"typedef struct \{([^}]*)\} cl_stats;", text, flags=re.S).group(1)
    fields = []
    for decl in re.findall(r"(double|int64_t)\s+([a-z_, ]+);", body):
        fields += [(n.strip(), decl[0]) for n in decl[1].split(",")]
    assert fields == [(n, "double" if t is C.c_double else "int64_t") for n, t in chunk_loader.Stats._fields_]
    for fn, n_params in (("cl_open", 8), ("cl_inflate_chunks_device", 10), ("cl_assemble_device", 18), ("cl_get_stats", 2)):
        decl = re.search(r"int %s\((.*?)\);" % fn, text, flags=re.S).group(1)
        params = [p.strip() for p in decl.split(",")]
        argtypes = getattr(lib, fn).argtypes
        assert len(params) == len(argtypes) == n_params, fn
        for p, t in zip(params, argtypes):
            if "**" in p:
                assert t is C.POINTER(C.c_void_p), p
            elif "cl_stats*" in p:
                assert t is C.POINTER(chunk_loader.Stats), p
            else:
                assert t is (C.c_void_p if "*" in p else C.c_uint64 if p.startswith("uint64_t") else C.c_int64 if p.startswith("int64_t")
                             else C.c_int32), p
    # a handle that cannot be opened says why, without a device: the planes are not where the candidate record has them
    h = C.c_void_p()
    assert lib.cl_open(15425, 8, 201, 20, (C.c_int64 * 3)(3031, 7385, 11400), 16, 0, C.byref(h)) == -1 and not h
    assert b"not the candidate record's layout" in lib.cl_last_error(None)


@pytest.mark.parametrize("kind", ["libhdf5 gzip 4", "ChunkWriter fixed", "ChunkWriter dynamic", "a raw chunk"])
def test_raw_chunks_through_the_cpu_twin_give_the_native_loaders_planes(tmp_path, kind):
    """What the device loader does, with the host twin of its kernel and the numpy statement of its assembly."""
    from dl4vc_amd.loader import NativeLoader
    stored, reads = 20, 10
    recs = make_records(stored, reads)
    path = str(tmp_path / "c.hdf")
    if kind == "libhdf5 gzip 4":
        hdf5io.write_candidates(path, recs)
    elif kind == "a raw chunk":
        write_chunks(path, recs, raw=(RAW_CHUNK,))
    else:
        chunk_written(path, recs, kind.split()[-1])
    with hdf5io.RawChunkFile(path) as f:
        assert len(f) == N and f.chunk == 8 and f.itemsize == recs.dtype.itemsize and f.offsets["strand"] == recs.dtype.fields["strand"][1]
        nc = -(-N // f.chunk)
        sizes = [f.stored_size(c) for c in range(nc)]
        offs = np.concatenate(([0], np.cumsum(sizes)[:-1]))
        buf = np.zeros(sum(sizes), np.uint8)
        raw = [f.read_chunk(c, buf.ctypes.data + int(offs[c])) & 1 for c in range(nc)]
        assert raw == [int(kind == "a raw chunk" and c == RAW_CHUNK) for c in range(nc)]
        out = np.full(nc * f.chunk_bytes, 0xAB, np.uint8)
        status = zinflate.inflate_streams(buf, offs, sizes, out, [c * f.chunk_bytes for c in range(nc)], [f.chunk_bytes] * nc, raw)
    assert (status == 0).all()
    slots = out.view(recs.dtype)
    assert slots[:N].tobytes() == recs.tobytes() and not slots[N:].tobytes().strip(b"\x00")      # (the edge chunk's padding)
    for lo, hi in ((0, N), (3, N - 2)):
        with NativeLoader(path, reads, batch_sites=16, lo=lo, hi=hi, seed=SEED, threads=2) as nl:
            want = list(nl)
        for b0, b in zip(range(lo, hi, 16), want):
            b1 = min(hi, b0 + 16)
            c0, c1 = b0 // 8, -(-b1 // 8)
            part = slots[c0 * 8:c1 * 8]
            inside = np.zeros(len(part), np.int8)
            inside[b0 - c0 * 8:b1 - c0 * 8] = 1
            plan = plan_sites(inside, part["num_reads"], part["ref_bases"], [bytes(v).decode() for v in part["vcfrec"]], reads, stored, SEED,
                              first_record=b0)
            got = assemble_host(part["single_reads"], part["q-scores"], part["strand"], plan)
            for x, y in zip(got, (b.reads, b.qual, b.strand, b.ref, b.ref_mask, b.var_mask)):
                assert (x == y).all()
            assert plan.vcfrec == list(b.vcfrec) and (plan.num_reads == b.num_reads).all() and (plan.blacklist == b.blacklist).all()


def test_files_the_loader_cannot_take_are_refused_with_the_reason(tmp_path):
    recs = make_records(20, 10)[:16]
    create_dataset(str(tmp_path / "flat.hdf"), recs, chunked=False, shuffle=False)
    with pytest.raises(ValueError, match="is not chunked"):
        hdf5io.RawChunkFile(str(tmp_path / "flat.hdf"))
    create_dataset(str(tmp_path / "shuffle.hdf"), recs, chunked=True, shuffle=True)
    with pytest.raises(ValueError, match=r"filters \[2, 1\], not deflate alone"):
        hdf5io.RawChunkFile(str(tmp_path / "shuffle.hdf"))
    with pytest.raises(FileNotFoundError):
        hdf5io.RawChunkFile(str(tmp_path / "absent.hdf"))

"""Input files of the native loader library's failure-path tests (tests/test_loader_shell.py) and of its stand-alone sanitizer
pass (tools/asan_loader.sh, which runs this module as a plain python child: ``python tests/loader_shell_cases.py DIR``):
candidate files of 24 records in chunks of 8 whose chunk 1 is damaged in the ways the loader must refuse, record types whose
fields do not fit the record, and the damaged BAM records of tests/test_pileup_native.py plus one with ``l_read_name`` 0."""
import ctypes as C
import os
import struct
import sys
import zlib

import numpy as np

if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from dl4vc_amd import hdf5io, pileup_gpu, synth
from dl4vc_amd.bamio import BamWriter, pack_record
from dl4vc_amd.hdf5_schema import record_dtype

N, CHUNK, READS, STORED = 24, 8, 10, 20
# what chunk 1 (records 8..15) of each file is; every other chunk is the zlib stream of its 8 records
CHUNK_CASES = ("intact", "short_inflate", "truncated", "too_long", "short_raw")
LAYOUT_CASES = ("strand_past_record", "ref_bases_in_front")
BAM_CASES = ("l_seq_beyond_record", "negative_l_seq", "negative_block_size", "tiny_block_size", "cigar_count_beyond_record",
             "truncated_record", "l_read_name_zero")
BAM_QUERY = (["ref"] * 6, [110, 115, 120, 125, 130, 135])


def make_records():
    """24 records of ``itemsize`` 15 425, every one different: none deeper than ``READS``, so no seed is needed."""
    recs = hdf5io.records_from_sites(synth.make_sites(N, reads=READS, seed=41), store_reads=STORED)
    assert recs.dtype.itemsize == 15425
    return recs


def write_chunk_case(path, recs, case):
    """The file written chunk by chunk past the filter (``ChunkWriter.write_chunks``), chunk 1 as ``case`` says: a stream that
    inflates to its first record only, a stream cut in half, a stream of the chunk and 100 bytes more, or (written with
    ``H5Dwrite_chunk`` itself: the writer refuses it) the bytes of its first record with the filter mask set."""
    size = recs.dtype.itemsize
    pieces = []
    for c in range(N // CHUNK):
        image = np.ascontiguousarray(recs[c * CHUNK:(c + 1) * CHUNK]).tobytes()
        if c == 1 and case == "short_inflate":
            image = image[:size]
        if c == 1 and case == "too_long":
            image += bytes(100)
        piece = zlib.compress(image, 4)
        if c == 1 and case == "truncated":
            piece = piece[:len(piece) // 2]
        pieces.append(piece)
    sizes = np.array([len(s) for s in pieces], np.uint64)
    offs = np.concatenate(([0], np.cumsum(sizes)[:-1])).astype(np.uint64)
    chunks = pileup_gpu.CompressedChunks(N, np.frombuffer(b"".join(pieces), np.uint8), offs, sizes, np.zeros(len(pieces), np.uint32),
                                         np.zeros(len(pieces), np.uint8))
    with hdf5io.ChunkWriter(path, recs.dtype, chunk=CHUNK) as w:
        w.write_chunks(chunks)
        if case == "short_raw":
            raw = np.frombuffer(np.ascontiguousarray(recs[CHUNK:CHUNK + 1]).tobytes(), np.uint8)
            rc = w._lib.H5Dwrite_chunk(w._did, 0, 1, (hdf5io.hsize_t * 1)(CHUNK), raw.size, raw.ctypes.data_as(C.c_void_p))
            if rc < 0:
                raise OSError("H5Dwrite_chunk refuses a short unfiltered chunk")
    return path


def write_layout_case(path, recs, case):
    """The same records under a record type the loader must refuse: ``strand`` holding half the rows of the other planes, so that
    the extent the loader copies by runs past the record, or ``ref_bases`` in front of ``single_reads``."""
    dt = record_dtype(STORED, 201)
    fields = [(n, dt.fields[n][0]) for n in dt.names]
    if case == "strand_past_record":
        fields[-1] = ("strand", np.uint8, (STORED // 2, 201))
    else:
        i, j = dt.names.index("single_reads"), dt.names.index("ref_bases")
        fields[i], fields[j] = fields[j], fields[i]
    out = np.zeros(len(recs), np.dtype(fields))
    for n in dt.names:
        out[n] = recs[n][:, :STORED // 2] if (n == "strand" and case == "strand_past_record") else recs[n]
    hdf5io.write_candidates(path, out, chunk=CHUNK)
    return path


def damaged_record(case):
    """One raw BAM record, length prefix included, damaged behind intact BGZF framing (``"good"``: as it was packed)."""
    body = bytearray(pack_record(0, 120, "bad", 0, 60, [(0, 50)], "ACGT" * 12 + "AC", [30] * 50)[4:])
    if case == "l_seq_beyond_record":
        body[16:20] = struct.pack("<i", 100000)
    elif case == "negative_l_seq":
        body[16:20] = struct.pack("<i", -5)
    elif case == "negative_block_size":
        return struct.pack("<i", -1) + bytes(body)
    elif case == "tiny_block_size":
        return struct.pack("<i", 8) + bytes(body[:8])
    elif case == "cigar_count_beyond_record":
        body[12:14] = struct.pack("<H", 60000)
    elif case == "truncated_record":
        return struct.pack("<i", len(body)) + bytes(body[:40])        # the file ends inside the record
    elif case == "l_read_name_zero":
        body[8] = 0
    return struct.pack("<i", len(body)) + bytes(body)


def write_bam_case(directory, case):
    """A FASTA and a BAM of three good reads and then the damaged record -> (bam, fasta)."""
    ref = "ACGT" * 200
    fa, bam = os.path.join(directory, "%s.fa" % case), os.path.join(directory, "%s.bam" % case)
    with open(fa, "w") as f:
        f.write(">ref\n%s\n" % ref)
    with BamWriter(bam, [("ref", len(ref))]) as w:
        for i in range(3):
            w.write(0, 100 + i, "r%d" % i, 0, 60, [(0, 50)], ref[100 + i:150 + i], [30] * 50)
        w.w.write(damaged_record(case))
    return bam, fa


def write_all(directory):
    recs = make_records()
    for case in CHUNK_CASES:
        write_chunk_case(os.path.join(directory, case + ".hdf"), recs, case)
    for case in LAYOUT_CASES:
        write_layout_case(os.path.join(directory, case + ".hdf"), recs, case)
    for case in BAM_CASES + ("good",):
        write_bam_case(directory, case)


if __name__ == "__main__":
    write_all(sys.argv[1])
